"""sgan_gauss_down_fwd / _bwd and sgan_gauss_down_multi_fwd / _multi_bwd on their own, fed known inputs, against the float64
reference of tests/resample_ref.py (pinned on the CPU by tests/test_resample_ref_host.py).  The taps differ on every channel and
have no symmetry, so a kernel that swaps ky and kx, convolves instead of correlating, or reads another channel's taps is caught.

Bounds, per element, derived and not tuned (u = 2^-24, T = sum |terms| from the reference's companion):
    forward   |kernel - fp64| <= (k k + 1) u T                  k k products, k k - 1 additions, any order, FMA or not
    backward  |kernel - fp64| <= (n + 2) u T, n = sum over the jobs of ceil(k / s)^2 (+ 1 for the base under accumulate)
over the whole output and again over the border ring (the first and last ceil(pad / s) + 1 rows and columns), where a wrong row
cannot hide behind the interior.  pad_norm_ref.within_yardstick is called as well (4 x the distance of the float32 restatement).
Padding channels: the inputs hold a non-zero constant there, the outputs come back exactly 0.0 (their base, bit for bit, under
accumulate).  Rows and columns no output reads get a gradient of exactly 0.  Outputs live in NaN-filled storage (hip_utils.Guarded):
outside the written view every bit is unchanged, inside everything is finite.  The multi-job kernels are compared with the
reference, and bit for bit with the single-job forward.

Figures of the run on an MI355X (pytest -s prints them per case), worst over all cases of the table:
    kernel                      worst |kernel - fp64| / bound     largest deviation: kernel | fp32 yardstick
    sgan_gauss_down_fwd         0.449 of (k k + 1) u T            7.82e-06 | 6.87e-06
    sgan_gauss_down_bwd         0.445 of (n + 2) u T              1.17e-06 | 1.28e-06
    sgan_gauss_down_multi_fwd   0.406                             7.82e-06 | 6.87e-06   (bit-equal to the single-job forward)
    sgan_gauss_down_multi_bwd   0.445                             1.22e-06 | 8.15e-07
    Worst kernel / yardstick ratio of a single case 3.63 (k13s6-3x6-c4r3-dense-sliced forward, 3.74e-07 | 1.03e-07: Ho = Wo = 1, nine
    numbers), 2.10 in the backward (4jobs-37x41-c8r5-dense-sliced, 1.16e-06 | 5.54e-07).  Adjoint identity <= 4.8e-08 (bound 1e-5).
    The grid-stride cases: forward 0.45, backward 0.34, multi forward 0.41, multi backward 0.34 of their bounds.  No kernel needed a fix.
"""
import numpy as np
import pytest
import torch

import pad_norm_ref as P
import resample_cases as K
import resample_ref as R
from hip_utils import Guarded

pytestmark = pytest.mark.gpu
WORST = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import _lib, ops
    _lib.lib()
    return ops


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()


def _taps(case):
    if case.dense:
        w, gcs = K.dense_weight(case.taps)
        return _dev(w), gcs
    return _dev(case.taps.reshape(-1)), case.k * case.k


def _held(got, ref64, ref32, bound, T, ring, key, what):
    """The derived bound over everything and over the ring alone; the yardstick; returns the worst ratio to the bound."""
    err = np.abs(got.astype(np.float64) - ref64)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    rring = float((err[ring] / np.maximum(bound[ring], 1e-300)).max())
    print(f"{what}: worst |kernel - fp64| / bound = {ratio:.3f} (ring {rring:.3f})")
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    dev, yard = P.within_yardstick(got, ref32, ref64, what)
    P.within_yardstick(got, ref32, ref64, what + ", border ring", sel=ring)
    WORST[key + " dev"] = max(WORST.get(key + " dev", (0.0, 0.0)), (dev, yard))
    assert (err <= bound).all(), f"{what}: {ratio:.3f} of the bound"
    assert (err[ring] <= bound[ring]).all()
    return ratio


def _fwd_refs(case):
    Cr = case.Creal
    a = (case.x[..., :Cr], case.taps, case.k, case.pad, case.s)
    return (K.ref("gf64", case, R.gauss_down, a), K.ref("gf32", case, R.gauss_down, a + (np.float32,)),
            K.ref("gfT", case, R.gauss_down_terms, a))


def _bwd_refs(case, acc):
    Cr = case.Creal
    base = case.base[..., :Cr] if acc else None
    a = (case.R[..., :Cr], case.taps, case.k, case.pad, case.s, case.H, case.W, base)
    return (K.ref("gb64", case, R.gauss_down_adj, a, acc), K.ref("gb32", case, R.gauss_down_adj, a + (np.float32,), acc),
            K.ref("gbT", case, R.gauss_down_adj_terms, a, acc))


def _check_fwd(case, x, out, what):
    assert out.outside_intact() and out.finite_inside() and x.untouched()
    got = out.numpy()
    assert not got[..., case.Creal:].any(), "padding channels of the output must be exactly 0.0"
    r64, r32, T = _fwd_refs(case)
    _held(got[..., :case.Creal], r64, r32, R.bound_gauss_fwd(case.k, T), T, R.gauss_ring(case.Ho, case.Wo, case.pad, case.s), what, f"{case.name} {what}")
    return got


def _check_bwd(case, acc, dout, din, what, ks=None):
    assert din.outside_intact() and din.finite_inside() and dout.untouched()
    got = din.numpy()
    if acc:
        assert np.array_equal(got[..., case.Creal:].view(np.int32), case.base[..., case.Creal:].view(np.int32)), "padding channels must keep their base"
    else:
        assert not got[..., case.Creal:].any(), "padding channels of the gradient must be exactly 0.0"
    r64, r32, T = _bwd_refs(case, acc)
    _held(got[..., :case.Creal], r64, r32, R.bound_gauss_bwd([(case.k, case.s)], T, acc), T,
          R.gauss_ring(case.H, case.W, case.pad, case.s), what, f"{case.name} {what}")
    if case.pad == 0 and not acc:
        hr, wr = case.s * (case.Ho - 1) + case.k, case.s * (case.Wo - 1) + case.k
        assert not got[hr:].any() and not got[:, wr:].any(), "rows / columns no output reads must get exactly 0"
    return got


def _run_single(ops, case):
    g, gcs = _taps(case)
    x, out = Guarded(case.H, case.W, case.C, case.sliced, case.x), Guarded(case.Ho, case.Wo, case.C, case.sliced)
    ops.gauss_down_fwd(x.t, case.Creal, g, gcs, case.k, case.pad, case.s, out.t)
    torch.cuda.synchronize()
    got = _check_fwd(case, x, out, "fwd")
    dout = Guarded(case.Ho, case.Wo, case.C, case.sliced, case.R)
    din = Guarded(case.H, case.W, case.C, case.sliced, case.base if case.acc else None)
    ops.gauss_down_bwd(dout.t, case.Creal, g, gcs, case.k, case.pad, case.s, din.t, accumulate=case.acc)
    torch.cuda.synchronize()
    gin = _check_bwd(case, case.acc, dout, din, "bwd")
    if case.pad == 0 and case.acc:      # the unread rows / columns keep their base bit for bit: exactly 0 was added
        hr, wr = case.s * (case.Ho - 1) + case.k, case.s * (case.Wo - 1) + case.k
        assert np.array_equal(gin[hr:].view(np.int32), case.base[hr:].view(np.int32))
        assert np.array_equal(gin[:, wr:].view(np.int32), case.base[:, wr:].view(np.int32))
    # adjoint identity with the kernels' own outputs, in float64 on the host
    Cr = case.Creal
    o64, r64 = got[..., :Cr].astype(np.float64), case.R[..., :Cr].astype(np.float64)
    d64 = gin[..., :Cr].astype(np.float64) - (case.base[..., :Cr].astype(np.float64) if case.acc else 0.0)
    lhs, rhs = float((o64 * r64).sum()), float((case.x[..., :Cr].astype(np.float64) * d64).sum())
    scale = float((np.abs(o64) * np.abs(r64)).sum()) + (float(np.abs(case.x[..., :Cr] * case.base[..., :Cr]).sum()) if case.acc else 0.0)
    print(f"{case.name} adjoint: |<out, R> - <x, din>| / scale = {abs(lhs - rhs) / scale:.3e} (bound 1e-5)")
    assert abs(lhs - rhs) <= 1e-5 * scale
    return g, gcs, x, out, dout


@pytest.mark.parametrize("case", K.GAUSS, ids=[c.name for c in K.GAUSS])
def test_gauss(ops, case):
    """Single-job forward and backward; for k <= 3 s also the multi-job kernels with this one job."""
    g, gcs, x, out, dout = _run_single(ops, case)
    if case not in K.GAUSS_MULTI_OK:
        return
    out2 = Guarded(case.Ho, case.Wo, case.C, case.sliced)
    ops.gauss_down_multi_fwd([(x.t, out2.t, g, gcs, case.k, case.pad, case.s)], case.Creal)
    torch.cuda.synchronize()
    _check_fwd(case, x, out2, "multi fwd")
    assert torch.equal(out2.t.view(torch.int32), out.t.view(torch.int32)), "multi forward differs from the single-job forward"
    din = Guarded(case.H, case.W, case.C, case.sliced, case.base if case.acc else None)
    ops.gauss_down_multi_bwd([(din.t, dout.t, g, gcs, case.k, case.pad, case.s)], case.Creal, accumulate=case.acc)
    torch.cuda.synchronize()
    _check_bwd(case, case.acc, dout, din, "multi bwd")


@pytest.mark.parametrize("m", K.MULTI, ids=[m.name for m in K.MULTI])
def test_gauss_multi_sets(ops, m):
    """1 .. 5 jobs with different (k, pad, s) and different taps on one image, against the reference: every forward output, and the
    backward as the sum of the jobs' adjoints -- into a NaN-filled gradient without accumulate, onto a base with it.  Five jobs go
    out as 4 + 1, the second launch accumulating."""
    Cr = m.Creal
    x = Guarded(m.H, m.W, m.C, m.sliced, m.x)
    gs = [_taps(j) for j in m.jobs]
    outs = [Guarded(j.Ho, j.Wo, m.C, m.sliced) for j in m.jobs]
    ops.gauss_down_multi_fwd([(x.t, o.t, g, gcs, j.k, j.pad, j.s) for j, o, (g, gcs) in zip(m.jobs, outs, gs)], Cr)
    torch.cuda.synchronize()
    for i, (j, o, (g, gcs)) in enumerate(zip(m.jobs, outs, gs)):
        _check_fwd(j, x, o, "multi fwd")
        single = Guarded(j.Ho, j.Wo, m.C, m.sliced)
        ops.gauss_down_fwd(x.t, Cr, g, gcs, j.k, j.pad, j.s, single.t)
        torch.cuda.synchronize()
        assert torch.equal(single.t.view(torch.int32), o.t.view(torch.int32)), f"job {i}: multi forward differs from the single-job forward"
    douts = [Guarded(j.Ho, j.Wo, m.C, m.sliced, j.R) for j in m.jobs]
    ring = np.zeros((m.H, m.W), dtype=bool)
    for j in m.jobs:
        ring |= R.gauss_ring(m.H, m.W, j.pad, j.s)
    parts64 = [_bwd_refs(j, False) for j in m.jobs]
    for acc in (False, True):
        din = Guarded(m.H, m.W, m.C, m.sliced, m.base if acc else None)
        ops.gauss_down_multi_bwd([(din.t, d.t, g, gcs, j.k, j.pad, j.s) for j, d, (g, gcs) in zip(m.jobs, douts, gs)], Cr, accumulate=acc)
        torch.cuda.synchronize()
        assert din.outside_intact() and din.finite_inside() and all(d.untouched() for d in douts)
        got = din.numpy()
        if acc:
            assert np.array_equal(got[..., Cr:].view(np.int32), m.base[..., Cr:].view(np.int32))
        else:
            assert not got[..., Cr:].any()
        r64, T = sum(p[0] for p in parts64), sum(p[2] for p in parts64)
        r32 = m.base[..., :Cr].copy() if acc else np.zeros((m.H, m.W, Cr), dtype=np.float32)
        for p in parts64:
            r32 = r32 + p[1]
        if acc:
            r64, T = r64 + m.base[..., :Cr].astype(np.float64), T + np.abs(m.base[..., :Cr].astype(np.float64))
        assert r32.dtype == np.float32
        _held(got[..., :Cr], r64, r32, R.bound_gauss_bwd([(j.k, j.s) for j in m.jobs], T, acc), T, ring, "multi bwd",
              f"{m.name} multi bwd" + (" acc" if acc else ""))


def test_gauss_grid_stride(ops):
    """Every capped grid takes its second stride (the caps and the shapes: tests/resample_cases.py): single forward and backward and
    the multi backward at 64 x 65 x 1024, the multi forward at 32 x 65 x 1024.  The only large Gaussian cases."""
    case = K.GAUSS_GRID
    g, gcs, x, out, dout = _run_single(ops, case)
    din = Guarded(case.H, case.W, case.C, False, case.base)
    ops.gauss_down_multi_bwd([(din.t, dout.t, g, gcs, case.k, case.pad, case.s)], case.Creal, accumulate=True)
    torch.cuda.synchronize()
    _check_bwd(case, True, dout, din, "multi bwd")
    del x, out, dout, din
    case = K.GAUSS_GRID_MULTI_FWD
    g, gcs = _taps(case)
    x, out = Guarded(case.H, case.W, case.C, False, case.x), Guarded(case.Ho, case.Wo, case.C, False)
    ops.gauss_down_multi_fwd([(x.t, out.t, g, gcs, case.k, case.pad, case.s)], case.Creal)
    torch.cuda.synchronize()
    _check_fwd(case, x, out, "multi fwd")


# ---- refusals: a negative status as SganError, and the NaN-filled output bit-unchanged ------------------------------------------------
def _refused(call, *guards):
    from supervised_gan_amd._lib import SganError
    with pytest.raises(SganError):
        call()
    torch.cuda.synchronize()
    assert all(g.untouched() for g in guards)


def test_multi_backward_refuses_k_above_three_strides(ops):
    k, pad, s, H, W = 9, 4, 2, 20, 20
    Ho = R.gauss_out_size(H, k, pad, s)
    g = _dev(np.ones(4 * k * k))
    dout, din = Guarded(Ho, Ho, 4, data=np.ones((Ho, Ho, 4))), Guarded(H, W, 4)
    _refused(lambda: ops.gauss_down_multi_bwd([(din.t, dout.t, g, k * k, k, pad, s)], 4), din)
    ops.gauss_down_bwd(dout.t, 4, g, k * k, k, pad, s, din.t)      # the single-job kernel takes it
    torch.cuda.synchronize()
    assert din.finite_inside() and din.outside_intact()


def test_multi_backward_refuses_jobs_that_do_not_share_the_image(ops):
    k, pad, s, H, W = 5, 2, 2, 20, 20
    Ho = R.gauss_out_size(H, k, pad, s)
    g = _dev(np.ones(4 * k * k))
    dout, din, other = Guarded(Ho, Ho, 4, data=np.ones((Ho, Ho, 4))), Guarded(H, W, 4), Guarded(H, W, 4)
    _refused(lambda: ops.gauss_down_multi_bwd([(din.t, dout.t, g, k * k, k, pad, s), (other.t, dout.t, g, k * k, k, pad, s)], 4), din, other)


def test_worst_ratios_are_reported():
    """Runs last (file order): prints what the module docstring records."""
    for key in sorted(WORST):
        print(f"gauss {key}: {WORST[key]}")

"""sgan_pad_reflect_fwd / sgan_pad_reflect_bwd (and the residual tail sgan_add_act_fwd / sgan_tanh_bwd) on their own, fed known
inputs, against the float64 reference of tests/pad_norm_ref.py (pinned on the CPU by tests/test_pad_norm_ref_host.py).

Bounds.  A pure gather (no norm, no activation, no mask) is bit-equal to F.pad(mode="reflect").  A pure fold is held per element
to 8 * 2^-24 * sum |terms| (an fp32 sum of at most 9 terms in any order) and, with the forward kernel's own output, to the
adjoint identity <out, R> == <x, din>.  Everything that carries a norm is held to the YARDSTICK: max |kernel - fp64| <=
4 x max |fp32 restatement - fp64| on the same inputs and elements (pad_norm_ref.within_yardstick), the border ring on its own as
well, so that a wrong mirror cannot hide behind a good interior.  The fp64 channel sums get a floor of H W 2^-53 (|base| +
sum |terms|) on top (the order of the fp64 atomics, which no restatement fixes).  Outputs live in NaN-filled storage
(hip_utils.Guarded): outside the written view every bit is unchanged, inside everything is finite.

Figures of the run on an MI355X, kernel deviation from fp64 | fp32 yardstick (pytest -s prints them per test):
    case                        out               ring              din               s1                s2                dx
    copy3-none-none             0.0e+00 0.0e+00  0.0e+00 0.0e+00     -       -         -       -         -       -         -       -
    copy3-none-none-sliced      0.0e+00 0.0e+00  0.0e+00 0.0e+00     -       -         -       -         -       -         -       -
    copy3-none-none-mask        0.0e+00 0.0e+00  0.0e+00 0.0e+00     -       -         -       -         -       -         -       -
    copy3-relu_only-relu        0.0e+00 0.0e+00  0.0e+00 0.0e+00  1.7e-07 2.4e-07  3.2e-07 7.2e-07  3.8e-07 1.5e-06     -       -
    min1-none-none              0.0e+00 0.0e+00  0.0e+00 0.0e+00     -       -         -       -         -       -         -       -
    min1-in-relu                1.2e-07 1.2e-07  1.2e-07 1.2e-07  1.2e-07 1.2e-07  1.7e-07 1.7e-07  4.9e-07 4.9e-07  2.2e-07 2.2e-07
    min1-bn-lrelu-mask-sliced   3.3e-07 5.6e-07  1.8e-07 5.6e-07  3.9e-07 4.1e-07  3.9e-07 5.0e-07  4.2e-07 6.6e-07  5.1e-07 5.1e-07
    min1-relu_only-relu         0.0e+00 0.0e+00  0.0e+00 0.0e+00  1.9e-07 1.9e-07  1.5e-07 2.4e-07  3.5e-07 3.5e-07     -       -
    min1-in-none-sliced         1.6e-07 1.6e-07  1.6e-07 1.6e-07  4.0e-07 3.6e-07  5.2e-07 5.2e-07  5.6e-07 7.4e-07  4.2e-07 4.2e-07
    min3-none-none              0.0e+00 0.0e+00  0.0e+00 0.0e+00     -       -         -       -         -       -         -       -
    min3-none-none-mask-sliced  0.0e+00 0.0e+00  0.0e+00 0.0e+00     -       -         -       -         -       -         -       -
    min3-in-relu                1.7e-07 2.3e-07  1.7e-07 2.3e-07  5.4e-07 5.4e-07  1.3e-06 5.8e-07  1.6e-06 8.6e-07  6.3e-07 6.3e-07
    min3-bn-lrelu-mask          4.0e-07 5.3e-07  4.0e-07 5.3e-07  1.1e-06 8.2e-07  8.8e-07 1.8e-06  2.4e-06 3.2e-06  1.3e-06 1.3e-06
    min3-bn-none-sliced         2.0e-07 2.6e-07  2.0e-07 2.6e-07  4.6e-07 3.6e-07  1.2e-06 8.9e-07  1.7e-06 1.3e-06  7.2e-07 7.2e-07
    min3-relu_only-relu-mask    0.0e+00 0.0e+00  0.0e+00 0.0e+00  7.5e-07 5.4e-07  1.2e-06 7.6e-07  1.7e-06 1.7e-06     -       -
    fwdonly-none-none           0.0e+00 0.0e+00  0.0e+00 0.0e+00     -       -         -       -         -       -         -       -
    fwdonly-in-relu-mask        3.2e-07 3.7e-07  3.2e-07 3.7e-07     -       -         -       -         -       -         -       -
    fwdonly-bn-lrelu-sliced     1.3e-07 1.4e-07  1.3e-07 1.4e-07     -       -         -       -         -       -         -       -
    pad0-none-none              0.0e+00 0.0e+00     -       -         -       -         -       -         -       -         -       -
    pad0-in-relu                1.8e-07 2.6e-07     -       -      0.0e+00 0.0e+00  0.0e+00 0.0e+00  3.1e-07 3.1e-07  2.7e-07 2.7e-07
    pad0-bn-none-mask-sliced    3.6e-07 5.1e-07     -       -      0.0e+00 0.0e+00  0.0e+00 0.0e+00  7.9e-07 7.9e-07  3.7e-07 4.0e-07
    wideC-none-none             0.0e+00 0.0e+00  0.0e+00 0.0e+00     -       -         -       -         -       -         -       -
    wideC-in-relu               2.0e-07 2.2e-07  1.5e-07 2.2e-07  5.2e-07 4.2e-07  6.1e-07 5.4e-07  1.7e-06 1.2e-06  4.7e-07 4.5e-07
    wideC-bn-lrelu-mask-sliced  6.3e-07 6.8e-07  6.3e-07 6.3e-07  9.2e-07 9.5e-07  1.1e-06 1.1e-06  1.4e-06 1.2e-06  1.5e-06 1.5e-06
    grid-none-none              0.0e+00 0.0e+00  0.0e+00 0.0e+00     -       -         -       -         -       -         -       -
    grid-in-relu                1.9e-07 2.9e-07  1.9e-07 2.5e-07  2.4e-07 2.4e-07  5.9e-07 9.1e-07  1.9e-06 2.0e-06  3.5e-07 3.5e-07
    grid-bn-lrelu-mask-sliced   7.5e-07 7.6e-07  4.1e-07 7.6e-07  8.3e-07 8.3e-07  1.8e-06 1.3e-06  2.4e-06 2.2e-06  9.4e-07 7.6e-07
    grid-bn-relu                3.6e-07 4.1e-07  2.8e-07 3.5e-07  3.0e-07 2.8e-07  6.1e-07 5.8e-07  9.6e-07 9.3e-07  8.2e-07 8.2e-07
    grid-relu_only-relu-sliced  0.0e+00 0.0e+00  0.0e+00 0.0e+00  5.5e-07 3.0e-07  1.2e-06 9.4e-07  2.7e-06 2.0e-06     -       -
    grid-in-none-mask           4.6e-07 5.7e-07  4.2e-07 5.1e-07  8.0e-07 1.1e-06  2.3e-06 2.4e-06  3.9e-06 3.4e-06  1.1e-06 8.3e-07
    block-none-none-mask        0.0e+00 0.0e+00  0.0e+00 0.0e+00     -       -         -       -         -       -         -       -
    block-in-relu-mask          3.5e-07 6.5e-07  3.1e-07 5.1e-07  4.6e-07 6.6e-07  7.2e-07 5.5e-07  1.3e-06 1.5e-06  5.3e-07 7.1e-07
    block-bn-relu-mask-sliced   5.8e-07 6.5e-07  5.8e-07 4.2e-07  4.8e-07 3.0e-07  6.6e-07 5.4e-07  3.6e-06 3.6e-06  4.9e-07 6.5e-07
    block-bn-lrelu              3.0e-07 3.3e-07  1.7e-07 2.6e-07  4.2e-07 3.4e-07  5.8e-07 4.3e-07  9.2e-07 1.0e-06  4.0e-07 5.3e-07
    block-in-lrelu-mask-sliced  3.0e-07 4.1e-07  3.0e-07 3.0e-07  7.2e-07 3.9e-07  6.4e-07 5.3e-07  1.4e-06 1.4e-06  5.3e-07 5.3e-07
    block-relu_only-relu-mask   0.0e+00 0.0e+00  0.0e+00 0.0e+00  4.8e-07 4.8e-07  7.6e-07 7.0e-07  1.4e-06 1.4e-06     -       -
    (each pair: kernel | yardstick; 0 | 0 = exact on both sides.  dgamma / dbeta of the BN cases: kernel 3.4e-7 .. 5.3e-6 beside
    yardsticks 7.8e-7 .. 5.3e-6, worst ratio 2.0 (grid-bn-lrelu-mask-sliced dbeta 3.0e-6 | 1.5e-6).  Worst ratio overall 2.2
    (min3-in-relu s1).  Pure folds: worst |din - fp64| = 3.1 x 2^-24 sum |terms| (bound 8); adjoint identity <= 5.6e-9 (bound 1e-5).
    tanh(a + b): 7.1e-8 | 7.2e-8 (n = 1028), 1.5e-8 | 5.2e-8 (n = 4); its backward 2.4e-7 | 3.2e-7, 2.7e-8 | 3.5e-8.)
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pad_norm_cases as K
import pad_norm_ref as R
from hip_utils import Guarded

pytestmark = pytest.mark.gpu

IDS = [c.name for c in K.CASES]
BWD_CASES = [c for c in K.CASES if 2 * c.pad < min(c.H, c.W)]
U32 = R.U32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import _lib, ops
    _lib.lib()
    return ops


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


class Arena:
    """2 C doubles (sums, then squares) as the kernels address them: plain, or the middle third of a 3 C wide arena under
    sq_stride = 3 C.  The rest of a sliced arena holds `other` (NaN for statistics that are only read; 1.0 for sums that are added
    to, so that a stray add shows)."""

    def __init__(self, C, sliced, values, other):
        self.C, self.width, self.off = C, (3 * C if sliced else C), (C if sliced else 0)
        host = np.full(2 * self.width, other, dtype=np.float64)
        self.own = np.zeros(2 * self.width, dtype=bool)
        for half in (0, 1):
            lo = half * self.width + self.off
            host[lo: lo + C] = values[half * C: (half + 1) * C]
            self.own[lo: lo + C] = True
        self.host0 = host
        self.full = torch.from_numpy(host.copy()).cuda()
        self.view = self.full[self.off:]
        self.sq = self.width if sliced else 0

    def read(self):
        """(own values [2 C], were the others left alone bit for bit)."""
        now = self.full.cpu().numpy()
        same = np.array_equal(now[~self.own].view(np.int64), self.host0[~self.own].view(np.int64))
        return now[self.own], same


def _act_id(ops, act):
    return {"none": ops.ACT_NONE, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU}[act]


def _desc(ops, case):
    """(norm_desc, the statistics arena, gamma, beta on the device) of a case; None for a plain read."""
    st = Arena(case.C, case.sliced, case.stats, np.nan) if case.stats is not None else None
    g, b = _dev(case.gamma), _dev(case.beta)
    nd = ops.norm_desc(None if st is None else st.view, g, b, case.count, K.EPS, _act_id(ops, case.act), K.SLOPE, 0 if st is None else st.sq)
    return nd, st, g, b


def _forward(ops, case):
    x, out = Guarded(case.H, case.W, case.C, case.sliced, case.x), Guarded(case.H + 2 * case.pad, case.W + 2 * case.pad, case.C, case.sliced)
    nd, st, g, b = _desc(ops, case)
    ops.pad_reflect_fwd(x.t, nd, case.pad, out.t, _dev(case.m))
    torch.cuda.synchronize()
    assert out.outside_intact() and out.finite_inside() and x.untouched()
    return x, out


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_forward(ops, case):
    x, out = _forward(ops, case)
    got = out.numpy()
    ref64 = R.pad_reflect_fwd(case.x, case.pad, **K.norm_args(case, np.float64))
    ref32 = R.pad_reflect_fwd(case.x, case.pad, **K.norm_args(case, np.float32))
    if case.norm == "none" and case.m is None:       # a pure gather
        p = case.pad
        want = F.pad(torch.from_numpy(case.x).permute(2, 0, 1).unsqueeze(0), (p, p, p, p), mode="reflect")[0].permute(1, 2, 0) if p \
            else torch.from_numpy(case.x)
        assert torch.equal(out.t.cpu(), want.contiguous())
    R.within_yardstick(got, ref32, ref64, f"{case.name} out")
    if case.pad:
        R.within_yardstick(got, ref32, ref64, f"{case.name} out, border ring", sel=R.ring(case.H, case.W, case.pad))
    if case.Cl < case.C:
        assert np.isfinite(got[..., case.Cl:]).all() and (case.stats is not None or not got[..., case.Cl:].any())


@pytest.mark.parametrize("case", BWD_CASES, ids=[c.name for c in BWD_CASES])
def test_backward(ops, case):
    """din, the channel sums on top of a non-zero `bwd_sums`, and sgan_norm_bwd_apply on top of both (the gradient of x, gamma, beta)."""
    H, W, C, pad = case.H, case.W, case.C, case.pad
    dout, din = Guarded(H + 2 * pad, W + 2 * pad, C, case.sliced, case.R), Guarded(H, W, C, case.sliced)
    with_x = case.norm != "none"
    x = Guarded(H, W, C, case.sliced, case.x) if with_x else None
    nd, st, g, b = _desc(ops, case)
    base = np.concatenate([3.0 + 0.01 * np.arange(C), -2.0 - 0.01 * np.arange(C)])
    sums = Arena(C, case.sliced, base, 1.0) if with_x else None
    ops.pad_reflect_bwd(dout.t, pad, din.t, x.t if with_x else None, nd, _dev(case.m), sums.view if with_x else None, sums.sq if with_x else 0)
    torch.cuda.synchronize()
    assert din.outside_intact() and din.finite_inside() and dout.untouched() and (x is None or x.untouched())
    got = din.numpy()
    kw64, kw32 = K.norm_args(case, np.float64), K.norm_args(case, np.float32)
    d64, s1, s2, terms = R.pad_reflect_bwd(case.R, pad, case.x if with_x else None, **kw64)
    d32, t1, t2, _ = R.pad_reflect_bwd(case.R, pad, case.x if with_x else None, **kw32)
    if not with_x:      # pure fold (times the mask, an exact factor 0 or 2)
        bound = 8 * U32 * terms * (np.abs(case.m.astype(np.float64)) if case.m is not None else 1.0)
        err = np.abs(got.astype(np.float64) - d64)
        print(f"{case.name} fold: worst |din - fp64| / (2^-24 sum |terms|) = {float((err / np.maximum(U32 * terms, 1e-300)).max()):.3f} (bound 8)")
        assert (err <= bound).all()
    if case.norm in ("none", "relu_only"):      # linear, or act(x) = x act'(x): the forward kernel's own output is the adjoint's other side
        _, out = _forward(ops, case)
        o64, r64 = out.numpy().astype(np.float64), case.R.astype(np.float64)
        lhs, rhs = float((o64 * r64).sum()), float((case.x.astype(np.float64) * got).sum())
        scale = float((np.abs(o64) * np.abs(r64)).sum())
        print(f"{case.name} adjoint: |<out, R> - <x, din>| / <|out|, |R|> = {abs(lhs - rhs) / scale:.3e} (bound 1e-5)")
        assert abs(lhs - rhs) <= 1e-5 * scale
    if not with_x:
        return
    R.within_yardstick(got, d32, d64, f"{case.name} din")
    now, others_same = sums.read()
    assert others_same, "a channel sum was added outside the slice"
    # the products in fp32, the additions in fp64 atomics: their order is free, hence the floor
    d64a = np.abs(d64)
    xhat64, _ = R.xhat_y(case.x.astype(np.float64), C, case.stats, case.gamma, case.beta, case.count, K.EPS, 0, 0, 1, np.float64)
    for name, lo, s64, s32, mag in (("s1", 0, s1, t1, d64a.sum((0, 1))), ("s2", C, s2, t2, (d64a * np.abs(xhat64)).sum((0, 1)))):
        bs = base[lo: lo + C]
        floor = float(H * W * 2.0 ** -53 * (np.abs(bs) + mag).max())
        dev, yard = R.within_yardstick(now[lo: lo + C], bs + s32, bs + s64, f"{case.name} {name}", floor=floor)
        allowed = R.YARDSTICK_FACTOR * yard + floor
        assert float(np.abs(s64).max()) > 4 * allowed      # the sums are large enough for the two checks below to mean something
        assert R.deviation(now[lo: lo + C], bs + 2 * s64) > allowed and R.deviation(now[lo: lo + C], s64) > allowed
    if case.norm not in ("in", "bn"):
        return
    # norm backward on top of the kernel's own din and sums (without the base)
    plain = Arena(C, case.sliced, now - base, 1.0)
    gb = np.concatenate([0.5 + 0.25 * np.arange(C), -1.0 + 0.125 * np.arange(C)]).astype(np.float32)
    dgam, dbet = (_dev(gb[:C]), _dev(gb[C:])) if case.norm == "bn" else (None, None)
    ops.norm_bwd_apply(din.t, x.t, nd, plain.view, dgam, dbet, plain.sq)
    torch.cuda.synchronize()
    assert din.outside_intact() and din.finite_inside() and x.untouched() and np.array_equal(plain.read()[0], now - base)
    x64, dg64, db64 = R.norm_bwd(d64, case.x, case.stats, case.gamma, case.count, K.EPS, s1, s2)
    x32, dg32, db32 = R.norm_bwd(d32, case.x, case.stats, case.gamma, case.count, K.EPS, t1, t2, dtype=np.float32)
    R.within_yardstick(din.numpy(), x32, x64, f"{case.name} dx")
    if case.norm == "bn":
        R.within_yardstick(dgam.cpu().numpy(), gb[:C] + dg32, gb[:C].astype(np.float64) + dg64, f"{case.name} dgamma")
        R.within_yardstick(dbet.cpu().numpy(), gb[C:] + db32, gb[C:].astype(np.float64) + db64, f"{case.name} dbeta")


# ---- error paths: SganError, and the NaN-filled output untouched ---------------------------------------------------------------------
def _refused(ops, call, *guards):
    from supervised_gan_amd._lib import SganError
    with pytest.raises(SganError):
        call()
    torch.cuda.synchronize()
    assert all(g.untouched() for g in guards)


def test_forward_refuses_pad_not_below_the_map(ops):
    for H, W in ((3, 9), (9, 3)):
        x, out = Guarded(H, W, 8, data=np.ones((H, W, 8))), Guarded(H + 6, W + 6, 8)
        _refused(ops, lambda: ops.pad_reflect_fwd(x.t, None, 3, out.t), out)


def test_backward_refuses_pad_not_below_half_the_map(ops):
    """Today's contract (case fwdonly): a forward with pad < H succeeds, its backward needs 2 pad < H and 2 pad < W."""
    for H, W in ((4, 9), (6, 9), (9, 6), (9, 4)):
        x, out = Guarded(H, W, 8, data=np.ones((H, W, 8))), Guarded(H + 6, W + 6, 8)
        ops.pad_reflect_fwd(x.t, None, 3, out.t)
        torch.cuda.synchronize()
        assert out.finite_inside() and out.outside_intact()
        dout, din = Guarded(H + 6, W + 6, 8, data=np.ones((H + 6, W + 6, 8))), Guarded(H, W, 8)
        _refused(ops, lambda: ops.pad_reflect_bwd(dout.t, 3, din.t), din)


def test_backward_refuses_sums_without_x(ops):
    dout, din = Guarded(9, 10, 8, data=np.ones((9, 10, 8))), Guarded(7, 8, 8)
    sums = torch.full((16,), 2.5, dtype=torch.float64, device="cuda")
    _refused(ops, lambda: ops.pad_reflect_bwd(dout.t, 1, din.t, bwd_sums=sums), din)
    assert bool((sums == 2.5).all())


def test_refuses_channels_not_a_multiple_of_four(ops):
    x, out = Guarded(5, 6, 6, data=np.ones((5, 6, 6))), Guarded(7, 8, 6)
    _refused(ops, lambda: ops.pad_reflect_fwd(x.t, None, 1, out.t), out)
    dout, din = Guarded(7, 8, 6, data=np.ones((7, 8, 6))), Guarded(5, 6, 6)
    _refused(ops, lambda: ops.pad_reflect_bwd(dout.t, 1, din.t), din)


def test_refuses_a_pixel_stride_below_the_channel_count(ops):
    x, out = Guarded(5, 6, 8, data=np.ones((5, 6, 8))), Guarded(7, 8, 8)
    narrow = torch.as_strided(x.store, (5, 6, 8), (24, 4, 1))          # pixel stride 4 < C = 8
    _refused(ops, lambda: ops.pad_reflect_fwd(narrow, None, 1, out.t), out)
    narrow_out = torch.as_strided(out.store, (7, 8, 8), (32, 4, 1))
    _refused(ops, lambda: ops.pad_reflect_fwd(x.t, None, 1, narrow_out), out)
    dout, din = Guarded(7, 8, 8, data=np.ones((7, 8, 8))), Guarded(5, 6, 8)
    narrow_din = torch.as_strided(din.store, (5, 6, 8), (24, 4, 1))
    _refused(ops, lambda: ops.pad_reflect_bwd(dout.t, 1, narrow_din), din)
    xin = Guarded(5, 6, 8, data=np.ones((5, 6, 8)))
    narrow_x = torch.as_strided(xin.store, (5, 6, 8), (24, 4, 1))
    _refused(ops, lambda: ops.pad_reflect_bwd(dout.t, 1, din.t, narrow_x, ops.norm_desc(None, act=ops.ACT_RELU)), din)


# ---- the --use_residual tail ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1028, 4])
def test_residual_tail(ops, n):
    """out = act(a + b): ACT_NONE bit-equal to a + b, tanh within the yardstick; sgan_tanh_bwd of that output is the one gradient
    that serves both addends (d tanh(a + b) / da == d / db)."""
    rng = np.random.default_rng(n)
    a, b, dy = ((rng.standard_normal(n) * s).astype(np.float32) for s in (1.5, 1.0, 1.0))
    ga, gb, gd = (Guarded(1, n // 4, 4, data=v) for v in (a, b, dy))
    out = Guarded(1, n // 4, 4)
    ops.add_act_fwd(ga.t, gb.t, out.t, ops.ACT_NONE)
    torch.cuda.synchronize()
    assert out.outside_intact() and np.array_equal(out.numpy().reshape(-1), a + b)
    out = Guarded(1, n // 4, 4)
    ops.add_act_fwd(ga.t, gb.t, out.t, ops.ACT_TANH)
    torch.cuda.synchronize()
    assert out.outside_intact() and ga.untouched() and gb.untouched()
    y = out.numpy().reshape(-1)
    y64, y32 = R.add_act(a, b, True), R.add_act(a, b, True, np.float32)
    assert y32.dtype == np.float32
    R.within_yardstick(y, y32, y64, f"tanh(a + b), n = {n}")
    dx = Guarded(1, n // 4, 4)
    ops.tanh_bwd(gd.t, out.t, dx.t)
    torch.cuda.synchronize()
    assert dx.outside_intact() and out.outside_intact()
    R.within_yardstick(dx.numpy().reshape(-1), R.tanh_bwd(dy, y32, np.float32), R.tanh_bwd(dy, y64), f"tanh backward, n = {n}")


def test_residual_tail_refuses_a_ragged_length(ops):
    a = torch.ones(6, device="cuda")
    out = torch.full((6 + 64,), float("nan"), device="cuda")
    snap = out.view(torch.int32).clone()
    from supervised_gan_amd._lib import SganError
    for call in (lambda: ops.add_act_fwd(a, a, out[:6], ops.ACT_TANH), lambda: ops.add_act_fwd(a, a, out[:6], ops.ACT_NONE),
                 lambda: ops.tanh_bwd(a, a, out[:6])):
        with pytest.raises(SganError):
            call()
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), snap)

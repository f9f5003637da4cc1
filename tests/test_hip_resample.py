"""sgan_bilinear_up2_fwd / _bwd and sgan_avgpool_pyramid_fwd / _bwd on their own, fed known inputs, against the float64 reference
of tests/resample_ref.py (pinned on the CPU by tests/test_resample_ref_host.py); the Gaussian kernels: tests/test_hip_resample_gauss.py.

Bounds, per element, derived and not tuned (u = 2^-24, T = sum |terms| from the reference's companion):
    bilinear forward   8 u T           four products and three sums, with or without FMA contraction
    bilinear backward  20 u T          16 terms
    pyramid forward    3 (s + 1) u T   level s, a tree of 2 x 2 sums; the scalings by 1/4 are exact
    pyramid backward   8 u T           six levels and the base; the scalings by 4^-(s+1) are exact
over the whole output and again over the outermost rows and columns alone.  pad_norm_ref.within_yardstick is called as well; for
the bilinear kernels with a floor of 2 u max |input|: where a clamp folds two taps into one the restatement multiplies by a weight
of exactly 1 and is exact, while the kernel adds 0.75 a + 0.25 a and rounds.  The pyramid forward on one-hot labels is bit-equal
to the reference.  The statistics the bilinear forward adds are compared with the float64 sums of its own output read back, to
N 2^-53 sum |v| (N output pixels: the order of the fp64 atomics), on top of non-zero sums, plain and inside a wider arena whose
other entries must not move.  Outputs live in NaN-filled storage (hip_utils.Guarded): outside the written view every bit is
unchanged, inside everything is finite.

Figures of the run on an MI355X (pytest -s prints them per case), worst over all cases of the table:
    kernel                      worst |kernel - fp64| / bound     largest deviation: kernel | fp32 yardstick
    sgan_bilinear_up2_fwd       0.244 of 8 u T                    3.91e-07 | 6.67e-07
    sgan_bilinear_up2_bwd       0.155 of 20 u T                   1.10e-06 | 8.66e-07   (worst ratio of a case 1.99, 5x7-c64)
    its statistics              0.461 of N 2^-53 sum |v|
    sgan_avgpool_pyramid_fwd    level 0 .. 5: 0.581, 0.245, 0.114, 0.048, 0.036, 0.022 of 3 (s + 1) u T;
                                2.09e-07 | 2.09e-07 at level 0 .. 2.89e-08 | 2.89e-08 at level 5: bit-equal to the tree of 2 x 2 means
    sgan_avgpool_pyramid_bwd    0.504 of 8 u T                    4.00e-07 | 4.00e-07   (bit-equal to the restatement)
    Adjoint identities <= 4.8e-08 (bound 1e-5).  No kernel needed a fix.
"""
import numpy as np
import pytest
import torch

import pad_norm_ref as P
import resample_cases as K
import resample_ref as R
from hip_utils import Guarded

pytestmark = pytest.mark.gpu
U32 = R.U32
WORST = {}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import _lib, ops
    _lib.lib()
    return ops


class Arena:
    """2 C doubles (sums, then squares) as the kernel addresses them: plain, or the middle third of a 3 C wide arena under
    stats_sq = 3 C whose other entries hold 1.0, so that a stray add shows (the Arena of tests/test_hip_pad_reflect.py)."""

    def __init__(self, C, sliced, values):
        self.C, self.width, self.off = C, (3 * C if sliced else C), (C if sliced else 0)
        host = np.full(2 * self.width, 1.0, dtype=np.float64)
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
        now = self.full.cpu().numpy()
        same = np.array_equal(now[~self.own].view(np.int64), self.host0[~self.own].view(np.int64))
        return now[self.own], same


def _held(got, ref64, ref32, bound, ring, key, what, floor=0.0):
    err = np.abs(got.astype(np.float64) - ref64)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    rring = float((err[ring] / np.maximum(bound[ring], 1e-300)).max())
    print(f"{what}: worst |kernel - fp64| / bound = {ratio:.3f} (ring {rring:.3f})")
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    dev, yard = P.within_yardstick(got, ref32, ref64, what, floor=floor)
    P.within_yardstick(got, ref32, ref64, what + ", border ring", sel=ring, floor=floor)
    WORST[key + " dev"] = max(WORST.get(key + " dev", (0.0, 0.0)), (dev, yard))
    assert (err <= bound).all(), f"{what}: {ratio:.3f} of the bound"
    assert (err[ring] <= bound[ring]).all()


# ---- bilinear ------------------------------------------------------------------------------------------------------------------------
def _bil_forward(ops, case):
    H, W, C = case.H, case.W, case.C
    x, out = Guarded(H, W, C, case.sliced, case.x), Guarded(2 * H, 2 * W, C, case.sliced)
    st = Arena(C, case.stats == "sliced", case.stats0) if case.stats != "none" else None
    if st is None:
        ops.bilinear_up2_fwd(x.t, out.t)
    else:
        ops.bilinear_up2_fwd(x.t, out.t, st.view, st.sq)
    torch.cuda.synchronize()
    assert out.outside_intact() and out.finite_inside() and x.untouched()
    got = out.numpy()
    a = (case.x,)
    r64, r32, T = K.ref("bf64", case, R.bilinear_up2, a), K.ref("bf32", case, R.bilinear_up2, a + (np.float32,)), K.ref("bfT", case, R.bilinear_up2_terms, a)
    _held(got, r64, r32, R.bound_bilinear_fwd(T), R.ring1(2 * H, 2 * W), "bilinear fwd", f"{case.name} fwd",
          floor=2 * U32 * float(np.abs(case.x).max()))
    if st is not None:
        now, others_same = st.read()
        assert others_same, "a statistic was added outside the slice"
        v = got.astype(np.float64)
        N = 4 * H * W
        for name, lo, add, mag in (("sum", 0, v.sum((0, 1)), np.abs(v).sum((0, 1))), ("sum of squares", C, (v * v).sum((0, 1)), (v * v).sum((0, 1)))):
            inc = now[lo: lo + C] - case.stats0[lo: lo + C]
            err = np.abs(inc - add)
            r = float((err / (N * 2.0 ** -53 * mag)).max())
            print(f"{case.name} {name}: worst |increment - fp64 sum of the output| / (N 2^-53 sum |v|) = {r:.3f}")
            WORST["bilinear stats"] = max(WORST.get("bilinear stats", 0.0), r)
            assert (err <= N * 2.0 ** -53 * mag).all(), f"{case.name} {name}: {r:.3f} of the bound"
            assert (np.abs(inc) > 0).all()
    return got


def _bil_backward(ops, case):
    H, W, C = case.H, case.W, case.C
    dout, din = Guarded(2 * H, 2 * W, C, case.sliced, case.R), Guarded(H, W, C, case.sliced)
    ops.bilinear_up2_bwd(dout.t, din.t)
    torch.cuda.synchronize()
    assert din.outside_intact() and din.finite_inside() and dout.untouched()
    got = din.numpy()
    a = (case.R,)
    r64, r32, T = K.ref("bb64", case, R.bilinear_up2_adj, a), K.ref("bb32", case, R.bilinear_up2_adj, a + (np.float32,)), K.ref("bbT", case, R.bilinear_up2_adj_terms, a)
    _held(got, r64, r32, R.bound_bilinear_bwd(T), R.ring1(H, W), "bilinear bwd", f"{case.name} bwd", floor=2 * U32 * float(np.abs(case.R).max()))
    return got


@pytest.mark.parametrize("case", K.BIL, ids=[c.name for c in K.BIL])
def test_bilinear_forward(ops, case):
    _bil_forward(ops, case)


@pytest.mark.parametrize("case", K.BIL_BWD, ids=[c.name for c in K.BIL_BWD])
def test_bilinear_backward(ops, case):
    din = _bil_backward(ops, case)
    if case.C % 4 or 256 % (case.C // 4):
        return
    # adjoint identity with the forward kernel's own output
    out = Guarded(2 * case.H, 2 * case.W, case.C)
    ops.bilinear_up2_fwd(Guarded(case.H, case.W, case.C, data=case.x).t, out.t)
    torch.cuda.synchronize()
    o64, r64 = out.numpy().astype(np.float64), case.R.astype(np.float64)
    lhs, rhs = float((o64 * r64).sum()), float((case.x.astype(np.float64) * din).sum())
    scale = float((np.abs(o64) * np.abs(r64)).sum())
    print(f"{case.name} adjoint: |<out, R> - <x, din>| / <|out|, |R|> = {abs(lhs - rhs) / scale:.3e} (bound 1e-5)")
    assert abs(lhs - rhs) <= 1e-5 * scale


def test_bilinear_grid_stride(ops):
    """The capped grids take their second stride (tests/resample_cases.py): forward with statistics at 32 x 65 x 1024, backward at
    64 x 65 x 1024.  The only large bilinear cases."""
    _bil_forward(ops, K.BIL_GRID_FWD)
    torch.cuda.empty_cache()
    _bil_backward(ops, K.BIL_GRID_BWD)


# ---- pyramid -------------------------------------------------------------------------------------------------------------------------
def _label(case, data):
    return Guarded(case.H, case.W, 4, data=data, ld=12, off=4) if case.sliced else Guarded(case.H, case.W, 4, data=data)


def _levels(case, data=None):
    return [Guarded(case.H >> (s + 1), case.W >> (s + 1), 4, data=None if data is None else data[s], ld=K.LEVEL_LD[s], off=K.LEVEL_OFF[s])
            for s in range(R.LEVELS)]


def _pyr_forward(ops, case):
    lab, lv = _label(case, case.x), _levels(case)
    ops.avgpool_pyramid_fwd(lab.t, [g.t for g in lv])
    torch.cuda.synchronize()
    assert lab.untouched() and all(g.outside_intact() and g.finite_inside() for g in lv)
    a = (case.x,)
    r64, T = K.ref("pf64", case, R.avgpool_pyramid, a), K.ref("pfT", case, R.avgpool_pyramid_terms, a)
    r32 = K.ref("pf32", case, R.avgpool_pyramid, a + (np.float32, False))      # the tree of 2 x 2 means, every step rounded to float32
    got = [g.numpy() for g in lv]
    for s in range(R.LEVELS):
        _held(got[s], r64[s], r32[s], R.bound_pyramid_fwd(s, T[s]), R.ring1(*got[s].shape[:2]), f"pyramid fwd level {s}", f"{case.name} level {s}")
        if case.onehot:
            assert np.array_equal(got[s].view(np.int32), r64[s].astype(np.float32).view(np.int32)), f"level {s} of one-hot labels must be exact"
    return got


@pytest.mark.parametrize("case", K.PYR, ids=[c.name for c in K.PYR])
def test_pyramid_forward(ops, case):
    _pyr_forward(ops, case)


def _pyr_backward(ops, case, present, acc):
    dl = K.pyr_levels(case, present)
    lv = _levels(case, case.dl)
    dlab = _label(case, case.base if acc else None)
    ops.avgpool_pyramid_bwd([lv[s].t if s in present else None for s in range(R.LEVELS)], dlab.t, accumulate=acc)
    torch.cuda.synchronize()
    assert dlab.outside_intact() and dlab.finite_inside() and all(g.untouched() for g in lv)
    got = dlab.numpy()
    base = case.base if acc else None
    a, extra = (dl, case.H, case.W, base), (present, acc)
    r64, T = K.ref("pb64", case, R.avgpool_pyramid_adj, a, extra), K.ref("pbT", case, R.avgpool_pyramid_adj_terms, a, extra)
    r32 = K.ref("pb32", case, R.avgpool_pyramid_adj, a + (np.float32,), extra)
    _held(got, r64, r32, R.bound_pyramid_bwd(T), R.ring1(case.H, case.W), "pyramid bwd", f"{case.name} bwd {present} acc={acc}")
    return got


@pytest.mark.parametrize("which", list(K.PYR_BWD))
@pytest.mark.parametrize("case", K.PYR[::2], ids=[c.name for c in K.PYR[::2]])
def test_pyramid_backward(ops, case, which):
    """All six levels; [None] * 5 + [d5] with accumulate onto a non-zero base (what generators.py launches); a middle subset; into
    NaN without accumulate."""
    present, acc = K.PYR_BWD[which]
    got = _pyr_backward(ops, case, present, acc)
    if which != "all6-nan":
        return
    fw = _pyr_forward(ops, case)      # adjoint identity with the forward kernel's own levels
    lhs = sum(float((fw[s].astype(np.float64) * case.dl[s].astype(np.float64)).sum()) for s in range(R.LEVELS))
    scale = sum(float((np.abs(fw[s]).astype(np.float64) * np.abs(case.dl[s]).astype(np.float64)).sum()) for s in range(R.LEVELS))
    rhs = float((case.x.astype(np.float64) * got).sum())
    print(f"{case.name} adjoint: |<levels, R> - <x, dlabel>| / scale = {abs(lhs - rhs) / scale:.3e} (bound 1e-5)")
    assert abs(lhs - rhs) <= 1e-5 * scale


@pytest.mark.parametrize("case", K.PYR[1::2], ids=[c.name for c in K.PYR[1::2]])
def test_pyramid_backward_sliced_label(ops, case):
    for which in ("only5-acc", "all6-nan"):
        _pyr_backward(ops, case, *K.PYR_BWD[which])


def test_pyramid_backward_grid_stride(ops):
    """sgan_avgpool_pyramid_bwd caps its grid at 4096 workgroups: 1024 x 1088 pixels take the second stride.  The only large case."""
    _pyr_backward(ops, K.PYR_GRID_BWD, *K.PYR_BWD["only5-acc"])
    _pyr_backward(ops, K.PYR_GRID_BWD, *K.PYR_BWD["all6-nan"])


# ---- refusals: SganError, and the NaN-filled output bit-unchanged --------------------------------------------------------------------
def _refused(call, *guards):
    from supervised_gan_amd._lib import SganError
    with pytest.raises(SganError):
        call()
    torch.cuda.synchronize()
    assert all(g.untouched() for g in guards)


def test_bilinear_forward_refuses_twelve_channels(ops):
    x, out = Guarded(3, 4, 12, data=np.ones((3, 4, 12))), Guarded(6, 8, 12)
    _refused(lambda: ops.bilinear_up2_fwd(x.t, out.t), out)


def test_bilinear_refuses_an_output_of_the_wrong_size(ops):
    x = Guarded(3, 4, 8, data=np.ones((3, 4, 8)))
    for shape in ((6, 7, 8), (8, 6, 8), (6, 8, 4)):
        out = Guarded(*shape)
        _refused(lambda: ops.bilinear_up2_fwd(x.t, out.t), out)
    din = Guarded(3, 4, 8)
    for shape in ((6, 7, 8), (8, 6, 8), (6, 8, 4)):
        dout = Guarded(*shape, data=np.ones(shape))
        _refused(lambda: ops.bilinear_up2_bwd(dout.t, din.t), din)


def test_pyramid_refuses_a_side_of_96(ops):
    H, W = 96, 64
    lab = Guarded(H, W, 4, data=np.ones((H, W, 4)))
    lv = [Guarded(H >> (s + 1), W >> (s + 1), 4) for s in range(R.LEVELS)]
    _refused(lambda: ops.avgpool_pyramid_fwd(lab.t, [g.t for g in lv]), *lv)
    dlab = Guarded(H, W, 4)
    dl = [Guarded(H >> (s + 1), W >> (s + 1), 4, data=np.ones((H >> (s + 1), W >> (s + 1), 4))) for s in range(R.LEVELS)]
    _refused(lambda: ops.avgpool_pyramid_bwd([g.t for g in dl], dlab.t), dlab)


def test_pyramid_refuses_a_level_of_the_wrong_size(ops):
    H, W = 64, 128
    lab = Guarded(H, W, 4, data=np.ones((H, W, 4)))
    lv = [Guarded(H >> (s + 1), W >> (s + 1), 4) for s in range(R.LEVELS)]
    lv[5] = Guarded(1, 1, 4)          # level 5 of 64 x 128 is 1 x 2: the kernel would write past it
    _refused(lambda: ops.avgpool_pyramid_fwd(lab.t, [g.t for g in lv]), *lv)
    dlab = Guarded(H, W, 4)
    d5 = Guarded(1, 1, 4, data=np.ones((1, 1, 4)))
    _refused(lambda: ops.avgpool_pyramid_bwd([None] * 5 + [d5.t], dlab.t, accumulate=True), dlab)


def test_worst_ratios_are_reported():
    """Runs last (file order): prints what the module docstring records."""
    for key in sorted(WORST):
        print(f"{key}: {WORST[key]}")

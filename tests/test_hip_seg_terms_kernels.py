"""sg_seg_terms_fwd_kernel and sg_seg_terms_bwd_kernel (csrc/sgan_segterms.hip) against the float64 reference of
tests/seg_terms_ref.py, element by element.  No error is normalised by a tensor's largest value (tests/test_hip_seg_terms.py keeps
that rule and is unchanged).  The rules stand in seg_terms_ref's docstring; tests/test_seg_terms_ref_host.py holds the reference side;
DESIGN.md R36 has the budgets beside the kernels' own errors.  Nothing is measured on a kernel.

Every operand lies in an allocation filled with NaN sentinels (inputs: in their padding channels too; labels: 1 << 40 behind the map;
the state: NaN behind its 68 doubles) that ends in a guard band: outputs come back with padding channels exactly 0 and the sentinels
intact, inputs keep every bit.  Every case runs twice on ONE workspace and the second run has the first one's bits in the losses,
the state and dz; the workspace, ticket included, reads back as zero after every forward.

Per case: TP, FP, FN, the focal numerator and norm inside the reference's intervals; D, TI, L_c, G(0), G(1), L_T, L_F within counted
fp64 roundings of the float64 recomputation from the device's OWN sums; both fp32 losses the roundings of L_T, L_F; dz (a) against the
reference backward fed the device's own state and (b) end to end against the reference state; exact zeros where the magnitude is 0;
unlisted state slots exactly 0.  Cases (tests/seg_terms_cases.py): 1, 35, 771 pixels x loss_ref.CE_PAIRS x both modes with the
Tversky sets, gammas, listed classes (none, one, [C-1, 0], [4, 0, 2], eight of sixteen scrambled), class weights (softmax C or none,
sigmoid nw 0 / 1 / C) and upstream gradients (NULLs, 0, 1e-30 among them), each dealt by an index of its own so that none is tied
to a (C, ld) pair, plus for every (C, ld) in both modes its richest class list with both terms on under an ordinary upstream pair
and a focal-only call without a listed class (the host file asserts this coverage); 65 792 pixels (257 workgroups: the last
workgroup's slot loop goes round twice) and 131 406 (past the 512-workgroup cap: the grid-stride second trip, forward and backward)
with C = 3 in rows of 4 and C = 16 in rows of 16; the scalar forms of vector-sized rows (3 channels inside rows of 32, a base one float
into its allocation, target rows of 8 or gradient rows of 8 beside logit rows of 4), bit for bit the dense vector run; an absent
listed class with D == 0 and with 1 - TI == 0; both upstream gradients NULL; loss_ref.GAN_PLANTED logits with the label / target on
and off the planted channel at gamma 0, 0.5, 2, 8 (gamma = 0.5 with 1 - pt == 0 exactly: the header leaves the product with
(1 - pt)^(gamma - 1) out there, the value is 0, which is also the limit, so the reference holds a point); labels -100, C, -1,
2^32 + 1 and -(2^32) + 2 in every softmax map of 16 pixels or more.

That the file can fail: one-line changes to a scratch copy of sgan_segterms.hip, none touching an address or a bound of a buffer, and
the cases that fail with the library built from it, in this file (of 110) and in tests/test_hip_seg_terms.py (of 20):
  * `qv = 1.f - pv` in the sigmoid backward: 28 here (every sigmoid case with a focal or Tversky element near p = 1, the 8 planted
    ones among them) -- 0 there
  * `gamma - 1.f` -> `gamma` in the softmax backward: 37 (the softmax cases with gamma > 0) -- 7
  * `(1.0 - A.beta)` -> `A.beta` in G(1): 66 (every case with a listed class and beta != 0.5) -- 13
  * `fn[c] += 1.0 - pd` moved onto `fp[c]`: 34 (every softmax case with a listed class) -- 7
  * the slot loop's stride 256 -> 512: 50 (the 8 large cases, then every case behind them that finds slots 256 .. 511 of the shared
    workspace not zeroed) -- 1 (test_workspace_is_reused_across_calls)
  * the backward's grid stride dropped: 4 (the four 363 x 362 cases: 334 pixels of dz keep their sentinel) -- 0
  * `om = 1.f - expf(zy - m) * inv` (1 - pt by subtraction) in st_softmax: 0 -- 0.  NOT caught, and not catchable at a budget that is
    honest about `lp`: the kernel forms lp = z_y - (m + logf(sum)) with `sum` rounded to fp32, so near pt = 1, where lp ~ -(1 - pt),
    lp itself carries the absolute error u that the subtraction 1 - pt would carry, in the loss term (1 - pt)^g (-lp) and in both
    terms of the derivative alike; torch's CPU fp32 evaluation of the same composition shows it and the 4 x rule allows it.  The
    others-over-sum form buys nothing observable while lp is formed this way; changing lp would change in-envelope bits and is
    left alone.
"""
import numpy as np
import pytest
import torch

import loss_ref as R
import seg_terms_cases as K
import seg_terms_ref as S
from test_hip_head_kernels import Buf, Labels, Vec, _same_bits, _src      # the sentinel-filled operands of the R33 file, as they are
from test_hip_loss_kernels import SENT, _bits, _scalar

pytestmark = pytest.mark.gpu

STATE_GUARD = 8


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import _lib, ops
    _lib.lib()
    return ops


@pytest.fixture(scope="module")
def work(ops):
    """ONE workspace for the whole module: every forward must leave it all zero for the next."""
    return ops.new_seg_terms_workspace(torch.device("cuda", 0))


def _once(ops, work, c, r, layout):
    """One forward and one backward.  Returns (loss_t, loss_f as fp32, state [68], dz [n, C] fp32)."""
    H, W, C = c.H, c.W, c.C
    view = layout == "view32"
    off = 1 if layout == "off1" else 0
    zld = 32 if view else c.ld
    dense = 4 if view else c.ld
    zb = _src(H, W, zld, r.z, off)
    ins = [zb]
    zt = zb.t[:, :, :C] if view else zb.t
    if c.mode == K.SOFTMAX:
        lab = Labels(r.lt)
        ins.append(lab)
        ltt = lab.t
    else:
        tb = _src(H, W, 8 if layout == "tld8" else zld, r.lt, off)
        ins.append(tb)
        ltt = tb.t[:, :, :C] if view else tb.t
    cw = None
    if c.nw:
        cw = Vec(r.cw[:c.nw])
        ins.append(cw)
    state = torch.full((68 + STATE_GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    lT, lF = _scalar(), _scalar()
    a, b, s, E = r.tv
    ops.seg_terms_forward(zt, C, c.mode, ltt, list(c.classes), a, b, s, E, c.gamma, cw.t if cw else None, state[:68], lT, lF, work)
    dz = Buf(H, W, 8 if layout == "dld8" else dense, off=off)
    g = [None if v is None else _scalar(v) for v in c.gout]
    ops.seg_terms_backward(zt, C, c.mode, ltt, list(c.classes), c.gamma, cw.t if cw else None, state[:68], g[0], g[1], dz.t)
    torch.cuda.synchronize()
    assert not bool(work.view(torch.int64).any()), "the workspace or its ticket is not back at zero"
    st = state.cpu().numpy()
    assert np.isnan(st[68:]).all(), "written behind the state"
    assert int(_bits(lT)[0]) != SENT and int(_bits(lF)[0]) != SENT, "a loss was not written"
    out = (np.float32(float(lT)), np.float32(float(lF)), st[:68].copy(), dz.read(C))
    for x in ins:
        assert x.unchanged(), "an input was written"
    return out


def _twice(ops, work, c, r, layout):
    runs = [_once(ops, work, c, r, layout) for _ in range(2)]
    _same_bits([runs[0][0], runs[0][1], runs[0][3]], [runs[1][0], runs[1][1], runs[1][3]], K.case_id(c))
    assert np.array_equal(runs[0][2].view(np.int64), runs[1][2].view(np.int64)), "the second run's state differs"
    return runs[0]


def _inside(got, lo, hi, what):
    assert np.isfinite(got) and lo <= got <= hi, f"{what}: {got!r} not in [{lo!r}, {hi!r}] (reference-side half-width {R.half_width(lo, hi) if hi > 0 else 0:.2e})"


def _check(c, r, got):
    lT, lF, st, dz = got
    what = K.case_id(c)
    px, n = r.px, len(c.classes)
    bp, bt, _ = K.budgets(K.group_of(c))
    bd = K.grad_budget(c)
    assert np.isfinite(st).all() and np.isfinite(dz).all(), what
    # ---- forward sums
    lo, hi, niv, miv = S.forward_intervals(px, c.classes, c.gamma, r.w, bp, bt)
    for j in range(n):
        for i, name in enumerate(("TP", "FP", "FN")):
            _inside(st[8 * j + i], lo[j, i], hi[j, i], f"{what} class {c.classes[j]} {name}")
    assert not st[8 * n:64].any(), f"{what}: an unlisted slot of the state is not 0"
    _inside(st[64], *niv, what + " focal numerator")
    _inside(st[65], *miv, what + " focal norm")
    # ---- derived state, from the device's own sums
    Sdev = st[:8 * n].reshape(n, 8)[:, :3]
    pw = S.pow_allowance(S.pow_pairs(Sdev, r.tv))
    val, bound, LT, bLT = S.derived(Sdev, r.tv, pw)
    worst = 0.0
    for j in range(n):
        for i, name in enumerate(("D", "TI", "L_c", "G(0)", "G(1)")):
            err = abs(st[8 * j + 3 + i] - val[j, i])
            assert err <= bound[j, i], f"{what} class {c.classes[j]} {name}: {st[8 * j + 3 + i]!r} vs {val[j, i]!r}, off by {err:.3e}, allowed {bound[j, i]:.3e}"
            worst = max(worst, err / bound[j, i]) if bound[j, i] > 0.0 else worst
    assert abs(st[66] - LT) <= bLT, (what, "L_T", st[66], LT, bLT)
    LF = st[64] / st[65] if st[65] > 0.0 else 0.0
    assert abs(st[67] - LF) <= 2.0 * S.EPS * abs(LF), (what, "L_F", st[67], LF)      # one division
    assert lT == np.float32(st[66]) and lF == np.float32(st[67]), (what, "the fp32 losses are the roundings of the state's", lT, lF, st[66:])
    # ---- backward (a): the reference backward fed the device's own state
    g = S.upstream(st, c.classes, c.C, c.gout[0], c.gout[1], r.focal)
    ref, mT, mF = S.backward(px, *g, c.gamma, r.w)
    mag = mT + mF
    ea = R.scaled_ulp_error(dz, ref, mag)
    assert ea.max() <= bd, f"{what} dz from the device's state: {float(ea.max()):.2f} ulp at {np.unravel_index(int(ea.argmax()), ea.shape)}, budget {bd:.2f}"
    zero = mag == 0.0
    assert not (dz[zero].view(np.int32) & 0x7FFFFFFF).any(), f"{what}: an element that is 0 by construction is not exactly 0"
    # ---- backward (b): end to end against the reference state
    dg0, dg1, rel_norm = S.g_slack(lo, hi, r.tv, miv, r.state, c.classes, c.C)
    up = abs(R.f32(c.gout[0])) if c.gout[0] is not None else 0.0
    magb = r.mT + r.mF
    room = S.allowed(bd + 1.0, magb) + S.slack_of(px, dg0, dg1, up, rel_norm, r.mF)      # + 1: the upstream constants are rounded from another state
    eb = np.abs(dz.astype(np.float64) - r.dz)
    assert (eb <= room).all(), f"{what} dz end to end: {int((eb > room).sum())} elements outside, worst {float((eb / room).max()):.2f} of the allowance"
    assert not (dz[magb == 0.0].view(np.int32) & 0x7FFFFFFF).any()
    print(f"{what}: dz {float(ea.max()):.2f} of {bd:.2f} ulp; derived state at most {worst:.2f} of its bound; pow allowance {pw:.2f} fp64 ulp")
    # ---- the exact zeros by name
    assert not (dz[~px.ok].view(np.int32) & 0x7FFFFFFF).any(), f"{what}: a pixel with a label outside [0, C) has a gradient"
    if c.mode == K.SIGMOID and not r.focal:
        unlisted = [k for k in range(c.C) if k not in c.classes]
        assert not (dz[:, unlisted].view(np.int32) & 0x7FFFFFFF).any(), f"{what}: an unlisted sigmoid channel has a gradient"
    if c.gout == (None, None):
        assert not (dz.view(np.int32) & 0x7FFFFFFF).any()
    if c.kind == "absent" and c.tv[2] == 0.0:
        assert st[0] == 0.0 and st[2] == 0.0 and not st[3:8].any(), f"{what}: the D == 0 class"
        if n == 1:
            assert lT == 0.0 and not (dz.view(np.int32) & 0x7FFFFFFF).any()
    if c.kind == "absent" and c.tv[2] == 1.0:
        assert st[4] == 1.0 and not st[5:8].any(), f"{what}: the 1 - TI == 0 class"


@pytest.mark.parametrize("c", K.CASES, ids=K.case_id)
def test_seg_terms_kernels(ops, work, c):
    r = K.ref_of(c)
    got = _twice(ops, work, c, r, c.layout)
    _check(c, r, got)
    if c.layout != "dense":
        # the scalar form of the same values: the dense vector run's bits
        d = _twice(ops, work, c, r, "dense")
        _same_bits([got[0], got[1], got[3]], [d[0], d[1], d[3]], K.case_id(c) + " against the dense run")
        assert np.array_equal(got[2].view(np.int64), d[2].view(np.int64)), "the state differs from the dense run's"


def test_misaligned_operands_that_fit_exactly_are_taken(ops, work):
    """Rows of 4 from a base one float into allocations that end with the last row: the wrapper sizes them by their stride and must
    not refuse them; the scalar form gives the dense run's bits."""
    c = next(k for k in K.CASES if k.layout == "off1" and (k.H, k.W) == (5, 7) and k.mode == K.SIGMOID)
    r = K.ref_of(c)
    n = c.H * c.W

    def exact(data):
        flat = torch.full((1 + n * 4,), float("nan"), device="cuda")
        v = flat[1:].view(c.H, c.W, 4)
        if data is not None:
            v[:, :, :c.C] = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).cuda().view(c.H, c.W, c.C)
        return v

    zt, tt, dz = exact(r.z), exact(r.lt), exact(None)
    state = torch.full((68,), float("nan"), dtype=torch.float64, device="cuda")
    lT, lF = _scalar(), _scalar()
    cw = torch.from_numpy(r.cw[:c.nw]).cuda()
    ops.seg_terms_forward(zt, c.C, c.mode, tt, list(c.classes), *r.tv, c.gamma, cw, state, lT, lF, work)
    ops.seg_terms_backward(zt, c.C, c.mode, tt, list(c.classes), c.gamma, cw, state, _scalar(c.gout[0]), _scalar(c.gout[1]), dz)
    torch.cuda.synchronize()
    d = _once(ops, work, c, r, "dense")
    assert np.array_equal(state.cpu().numpy().view(np.int64), d[2].view(np.int64))
    assert np.array_equal(_bits(dz[:, :, :c.C].contiguous()), d[3].reshape(-1).view(np.int32)) and not bool(dz[:, :, c.C:].any())

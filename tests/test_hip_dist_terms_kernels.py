"""sg_dist_loss_fwd_kernel and sg_dist_loss_bwd_kernel (csrc/sgan_distloss.hip) against the float64 reference of
tests/dist_terms_ref.py, element by element.  No error is normalised by a tensor's largest value (tests/test_hip_dist_terms.py keeps
that rule and is unchanged): every gradient element of this node is weighted by a distance field that spans many orders of magnitude
over a plane, and the pixels next to the contour -- the ones the terms exist to move -- are the small ones.  The rules stand in
dist_terms_ref's docstring; tests/test_dist_terms_kernels_ref_host.py holds the reference side; DESIGN.md R37 has the budgets beside
the kernels' own errors.  Nothing is measured on a kernel.

Every operand lies in an allocation filled with NaN sentinels (inputs: in their padding channels too, and in every sigmoid target
channel but the class's; labels: 1 << 40 behind the map; both signed maps: a sentinel behind them; the state: NaN behind its 5
doubles) that ends in a guard band: outputs come back with padding channels exactly 0 and the sentinels intact, inputs keep every
bit.  Every case runs twice on ONE module-wide workspace and the second run has the first one's bits in both losses, the state and
dz; the workspace, ticket included, reads back as zero after every forward.

Per case: S_B and S_H inside the reference's intervals; state[2] == npix, state[3] and state[4] the float64 quotients of the device's
OWN sums to the bit, both fp32 losses their single roundings, a switched-off term exactly 0; dz within the (mode, alpha) group's
budget in ulps of the element's magnitude (the backward takes no state, so this one measurement is "against the reference backward"
and "end to end" at once); exact zeros where the magnitude is 0.  A form that is not the dense pad4(C) one must give the dense vector
run's bits; a NULL upstream gradient beside a term that is on must give the bits of the call with that term switched off.

Cases (tests/dist_terms_cases.py): 1, 35, 1023 pixels x 22 (C, logit row, gradient row, layout) forms x both modes -- C in 1, 2, 3, 4,
12, 16 in rows of pad4(C), 8, 16; 3 channels inside rows of 32; bases one float into their allocations; gradient rows of 3, 5, 8, 20, 32
(dl_store_row<0>, its trailing loop behind channel 16 included); sigmoid logits in rows of 8 beside gradient rows of 4 -- with alpha in
0.5, 1, 1.5, 2, nextafter(2, 3), 3, 4, the three term switches, the upstream pairs (NULLs, 0, 1e-30 among them), the class, hot and soft
targets and the map geometry each dealt by an index of its own, plus every form with both terms on under an ordinary upstream pair;
64 x 64 blob geometry (a radius-15 disc against an offset radius-11 disc, one-pixel walls against the same walls moved, single inside
pixels: maps from util.signed_edt_sq) and synthetic integer maps with 0, +-1, +-2^30, INT32_MIN and INT32_MAX; 65 792 pixels (257
workgroups: the last workgroup's slot loop goes round twice) and 131 406 (past the 512-workgroup cap: the grid-stride second trip,
forward AND backward) with C = 3 in rows of 4 and C = 16 in rows of 16; loss_ref.GAN_PLANTED logits on pixels whose level set and
field are not zero, the label / target on and off the planted channel; +-40 saturated; one-channel softmax (every dz exactly 0, L_B
the mean of phi); labels -100, C, -1, 2^32 + 1 and -(2^32) + 2 in every softmax map of 16 pixels or more.

That the file can fail: one-line changes to a scratch copy of sgan_distloss.hip, none touching an address or a bound of a buffer,
each built and run once, and the cases that fail with the library built from it, in this file (of 267) and in
tests/test_hip_dist_terms.py (of 25):
  * `dv = Gp * (1.f - pc)` in the sigmoid backward: 82 here (every sigmoid case with an element whose p is near 1, the 8 planted ones
    among them) -- 0 there
  * `Gp * (1.f - pc)` for `Gp * om` in the softmax backward: 66 (the 8 planted and both saturated cases among them) -- 0
  * the `1.0 -` of dl_phi's inside branch dropped: 187 (every case with the boundary term on and an inside pixel) -- 19
  * `pow(a, h)` with `h = alpha`: 167 (every case with the Hausdorff term on at alpha != 2) -- 17
  * `alpha == 2.0` widened to `alpha >= 2.0`: 69 (every case at nextafter(2, 3), 3 and 4) -- 16
  * `yl` narrowed to `int`: 97 (every softmax case of 16 pixels or more: 2^32 + 1 and -(2^32) + 2 read as 1 and 2) -- 0
  * the backward's grid stride dropped (one trip): 4 (the four 363 x 362 cases: 334 pixels of dz keep their sentinel) -- 0
  * the forward's slot-loop stride 256 -> 512: 44 (the 8 large cases, then the cases behind them that find slots 256 .. 511 of the
    shared workspace not zeroed) -- 1 (test_workspace_is_reused_across_calls)
  * the trailing zero loop of dl_store_row<0> removed: 32 (every case with gradient rows of 20 or 32) -- 0
  * `sqrt` -> `sqrtf` of the map cast to float in dl_phi: 9 -- 0.  Caught where p carries no error of its own and nowhere else: the
    nine are one-channel softmax cases (p = 1 / 1 exactly), whose S_B interval is the fp64 accumulation alone.  Everywhere else the
    change sits below the error of p itself (2^-24 of phi against a p budget of tens of ulp) and is not catchable at an honest
    budget, in the sums or in dz.
"""
import numpy as np
import pytest
import torch

import dist_terms_cases as K
import dist_terms_ref as D
import loss_ref as R
from test_hip_head_kernels import Buf, Labels, _same_bits, _src      # the sentinel-filled operands of the R33 file, as they are
from test_hip_loss_kernels import SENT, _bits, _dev, _scalar

pytestmark = pytest.mark.gpu

STATE_WRITTEN, STATE_GUARD = 5, 11
MAP_SENT = 0x5A5A5A5A


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
    return ops.new_dist_loss_workspace(torch.device("cuda", 0))


class Map:
    """An int32 signed map [H, W] with a sentinel behind it."""

    def __init__(self, H, W, m):
        host = np.full(m.size + 64, MAP_SENT, dtype=np.int32)
        host[: m.size] = m
        self.snap, self.flat = host, _dev(host)
        self.t = self.flat[: m.size].view(H, W)

    def unchanged(self):
        return np.array_equal(self.flat.cpu().numpy(), self.snap)


def _once(ops, work, c, r):
    """One forward and one backward of case `c` on the inputs of `r`.  Returns (loss_b, loss_h as fp32, state [5], dz [n, C] fp32)."""
    H, W, C = c.H, c.W, c.C
    view = c.layout == "view32"
    off = 1 if c.layout == "off1" else 0
    zb = _src(H, W, c.ld, r.z, off)
    ins = [zb]
    zt = zb.t[:, :, :C] if view else zb.t
    if c.mode == K.SOFTMAX:
        lab = Labels(r.lt)
        ins.append(lab)
        ltt = lab.t
    else:
        tb = _src(H, W, c.ld, r.lt, off)      # NaN in every channel but the class's, as r.lt holds them
        ins.append(tb)
        ltt = tb.t[:, :, :C] if view else tb.t
    tm = Map(H, W, r.t_s)
    ins.append(tm)
    pm = None
    if c.alpha is not None:
        pm = Map(H, W, r.p_s)
        ins.append(pm)
    state = torch.full((STATE_WRITTEN + STATE_GUARD,), float("nan"), dtype=torch.float64, device="cuda")
    lB, lH = _scalar(), _scalar()
    pmt = pm.t if pm is not None else None
    ops.dist_loss_forward(zt, C, c.mode, ltt, c.cls, tm.t, pmt, c.boundary, c.alpha, state, lB, lH, work)
    dz = Buf(H, W, c.dld, off=off)
    g = [None if v is None else _scalar(v) for v in c.gout]
    ops.dist_loss_backward(zt, C, c.mode, ltt, c.cls, tm.t, pmt, c.boundary, c.alpha, g[0], g[1], dz.t)
    torch.cuda.synchronize()
    assert not bool(work.view(torch.int64).any()), "the workspace or its ticket is not back at zero"
    st = state.cpu().numpy()
    assert np.isnan(st[STATE_WRITTEN:]).all(), "written behind the state"
    assert int(_bits(lB)[0]) != SENT and int(_bits(lH)[0]) != SENT, "a loss was not written"
    out = (np.float32(float(lB)), np.float32(float(lH)), st[:STATE_WRITTEN].copy(), dz.read(C))
    for x in ins:
        assert x.unchanged(), "an input was written"
    return out


def _twice(ops, work, c, r):
    runs = [_once(ops, work, c, r) for _ in range(2)]
    _same_bits([runs[0][0], runs[0][1], runs[0][3]], [runs[1][0], runs[1][1], runs[1][3]], K.case_id(c))
    assert np.array_equal(runs[0][2].view(np.int64), runs[1][2].view(np.int64)), "the second run's state differs"
    return runs[0]


def _inside(got, lo, hi, what):
    assert np.isfinite(got) and lo <= got <= hi, f"{what}: {got!r} not in [{lo!r}, {hi!r}]"


def _nonzero(a):
    return (np.ascontiguousarray(a).view(np.int32) & 0x7FFFFFFF).any()


def _check(c, r, got):
    lB, lH, st, dz = got
    what = K.case_id(c)
    px = r.px
    n = px.npix
    bp, bd = K.p_budget(c.mode), K.grad_budget(K.group_of(c))
    assert np.isfinite(st).all() and np.isfinite(dz).all() and np.isfinite(lB) and np.isfinite(lH), what
    # ---- forward sums
    (blo, bhi), (hlo, hhi) = D.forward_intervals(px, bp, r.pow_ulps)
    _inside(st[0], blo, bhi, what + " S_B")
    _inside(st[1], hlo, hhi, what + " S_H")
    # ---- derived state, from the device's own sums: to the bit
    want, wB, wH = D.derived(st[0], st[1], n, c.boundary, r.hausdorff)
    assert st[2] == n, (what, st[2])
    assert np.array_equal(st.view(np.int64)[3:], want.view(np.int64)[3:]), (what, "L_B, L_H are not the quotients of the device's sums", st, want)
    assert np.array([lB, lH], np.float32).view(np.int32).tolist() == np.array([wB, wH], np.float32).view(np.int32).tolist(), (what, "the fp32 losses are the roundings of the state's", lB, lH, st[3:])
    if not c.boundary:
        assert st[0] == 0.0 and st[3] == 0.0 and lB == 0.0, what
    if not r.hausdorff:
        assert st[1] == 0.0 and st[4] == 0.0 and lH == 0.0, what
    # ---- backward: one measurement (the kernel takes no state)
    e = R.scaled_ulp_error(dz, r.dz, r.mag)
    worst = float(e.max())
    assert worst <= bd, f"{what} dz: {worst:.2f} ulp at {np.unravel_index(int(e.argmax()), e.shape)}, budget {bd:.2f}"
    assert not _nonzero(dz[r.mag == 0.0]), f"{what}: an element that is 0 by construction is not exactly 0"
    # ---- the exact zeros by name
    assert not _nonzero(dz[~px.ok]), f"{what}: a pixel with a label outside [0, C) has a gradient"
    if c.mode == K.SIGMOID:
        assert not _nonzero(np.delete(dz, c.cls, axis=1)), f"{what}: another sigmoid channel has a gradient"
    if c.mode == K.SOFTMAX and c.C == 1:
        assert not _nonzero(dz), f"{what}: one-channel softmax has a gradient"
    if c.gout == (None, None):
        assert not _nonzero(dz), what
    both_zero = (px.tmap == 0) & ((px.pmap == 0) if r.hausdorff else True)
    assert not _nonzero(dz[both_zero]), f"{what}: a pixel with both maps 0 has a gradient"
    hw = R.half_width(hlo, hhi) if hhi > 0 else 0.0
    print(f"{what}: dz {worst:.2f} of {bd:.2f} ulp ({worst / bd:.2f} of the budget); S_H at {(st[1] - r.SH) / (0.5 * (hhi - hlo)) if hhi > hlo else 0:+.2f} of "
          f"its half-width ({hw:.2e}), S_B at {(st[0] - r.SB) / (0.5 * (bhi - blo)) if bhi > blo else 0:+.2f} of its")


@pytest.mark.parametrize("c", K.CASES, ids=K.case_id)
def test_dist_terms_kernels(ops, work, c):
    r = K.ref_of(c)
    got = _twice(ops, work, c, r)
    _check(c, r, got)
    w = K.pad4(c.C)
    if (c.ld, c.dld, c.layout) != (w, w, "dense"):
        # another form of the same values: the dense vector run's bits
        d = _twice(ops, work, c._replace(ld=w, dld=w, layout="dense"), r)
        _same_bits([got[0], got[1], got[3]], [d[0], d[1], d[3]], K.case_id(c) + " against the dense run")
        assert np.array_equal(got[2].view(np.int64), d[2].view(np.int64)), "the state differs from the dense run's"
    if c.boundary and r.hausdorff and (c.gout[0] is None) != (c.gout[1] is None):
        # a term left out by a NULL upstream gradient is the call with that term switched off, bit for bit
        off = c._replace(boundary=False) if c.gout[0] is None else c._replace(alpha=None)
        d = _once(ops, work, off, r)
        _same_bits([got[3]], [d[3]], K.case_id(c) + " against the call with the term switched off")
        assert (d[0], d[2][0], d[2][3]) == (0.0, 0.0, 0.0) if c.gout[0] is None else (d[1], d[2][1], d[2][4]) == (0.0, 0.0, 0.0)
        assert d[1] == got[1] if c.gout[0] is None else d[0] == got[0]      # the term that stays has the joint call's loss

"""The ten entry points of csrc/sgan_seghead.hip and csrc/sgan_factd.hip against the float64 references of tests/loss_ref.py, element
by element: sgan_seg_head, sgan_seg_head_pw, sgan_label_weight_sum, sgan_pixel_weight_sum, sgan_factd_loss_multi_fwd / _bwd,
sgan_sigmoid_nhwc_fwd / _bwd, sgan_bce_weighted_fwd / _bwd, and the wrappers of ops.py / losses.py in front of them.  No error is
normalised by a tensor's largest value (tests/test_hip_seg_head*.py, test_hip_bce_weighted.py and test_hip_factd.py keep that rule).

Every operand lies `off` elements into an allocation filled with a NaN sentinel (inputs: POISON in their padding channels too;
labels: 1 << 40 behind the map) and ending in TAIL more: outputs come back with padding channels exactly 0 and the sentinel intact
around them, inputs keep every bit.  Every case runs twice on the same workspace and the second run has the first one's bits in
full; the seg-head workspaces are all zero after every call, the tickets of the other two read back as zero.

Rules (u = 2^-24; nothing is measured on a kernel; tests/test_head_ref_host.py holds the reference side):
  sigmoid head, sigmoid_nhwc, bce_weighted    intervals of loss_ref.bcew_ref: the float64 formula at p32 + k ulp, k = -3 .. 3, widened by 4
                     roundings per element, by the roundings of the pixel weight (3 nw) and of the scale; the loss is the mean of the
                     intervals.  sgan_sigmoid_nhwc_bwd from a given p is dp p (1 - p): three roundings, bound 4 u.
  softmax head       in fp32 ulps of the magnitude the roundings are relative to (loss_ref.ce_ref): 4 x the largest error of torch's CPU
                     fp32 evaluation on the same inputs, at least 2 ulp.  The weight sums: one rounding of the fp64 sum (and one per
                     pixel of the PW form), loss_ref.weight_sum_ref.
  factored loss      BCE mode: intervals of loss_ref.factd_term, p = q a2 at +- kp ulp and q at +- kq ulp, kp / kq = 4 x the largest
                     deviation of torch's CPU fp32 composition from float64 (3 .. 13 and 3 .. 9 on these inputs), times the sigmoid
                     derivatives' own candidates, widened by 12 (dl2) and 40 (dl1, of the sum of the absolute gathered terms) roundings.
                     MSE modes: ulp budgets as for the softmax head, of the magnitudes loss_ref.factd_term states.
DESIGN.md R33 has the budgets beside the kernels' own errors.

That the file can fail: one arithmetic change each to a scratch copy of the two sources, no address, loop bound, ticket or barrier
touched, and the cases of this file that fail with the library built from it (all pass with the library as it is):
  * sh_total's second trip dropped (`v += b < 256 ? sg_slot_load(&part[b]) : 0.0`): 12 cases -- the 6 large ones (257 and 514
    workgroups) of test_seg_head_softmax and the 6 of test_seg_head_sigmoid
  * the PW weight also given to a pixel with an ignored label (`w = w + A.padd[i]` in sg_seg_head_kernel): 24 -- all 18 of
    test_seg_head_softmax, the 4 of test_seg_head_scalar_forms_of_vector_sized_rows, both upstream-gradient cases
  * the sigmoid head's scale without C (`1.f / (float)A.npix`): 22 -- the 16 cases of test_seg_head_sigmoid with C > 1, the 4 scalar-form
    cases, both upstream-gradient cases
  * `T.pt = dH / 2` (top and bottom remainder swapped): 34 -- 32 of test_factd_one_term, both eight-term cases
  * the mirror test `uy <= T.pt` as `<`: 38 -- 36 of test_factd_one_term, both eight-term cases
  * sg_bcew_weight leaving its last weight out: 20 -- all 16 of test_sigmoid_ss_kernels, both cap cases, 2 of the planted ones
  * the x2 adjoint's outer row taps 0.75 / 0.25 swapped: 30 -- 28 of test_factd_one_term, both eight-term cases
"""
import functools

import numpy as np
import pytest
import torch

import loss_cases as K
import loss_ref as R
from test_hip_loss_kernels import POISON, SENT, TAIL, _bits, _dev, _in, _rel, _scalar

pytestmark = pytest.mark.gpu

U = R.U
LABEL_SENT = 1 << 40


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import _lib, ops
    _lib.lib()
    return ops


class Buf:
    """[H, W, ld] fp32 view `off` elements into an allocation of sentinels that ends in TAIL more.  data [n, c <= ld] (fp32) fills the
    first c channels.  off = 1: a base that is not 16-byte aligned."""

    def __init__(self, H, W, ld, data=None, off=0, fill=SENT):
        self.n, self.ld, self.off = H * W, ld, off
        host = np.full(off + self.n * ld + TAIL, fill, dtype=np.int32)
        if data is not None:
            data = np.ascontiguousarray(data, dtype=np.float32)
            host[off: off + self.n * ld].reshape(self.n, ld)[:, : data.shape[1]] = data.view(np.int32)
        self.snap = host
        self.flat = _dev(host).view(torch.float32)
        self.t = self.flat[off: off + self.n * ld].view(H, W, ld)

    def unchanged(self):
        return np.array_equal(_bits(self.flat), self.snap)

    def read(self, C):
        """[n, C] fp32 as written: channels C .. ld - 1 exactly +0.0, everything in front of and behind the map still the sentinel."""
        torch.cuda.synchronize()
        got = _bits(self.flat)
        a, b = self.off, self.off + self.n * self.ld
        assert (got[:a] == self.snap[:a]).all() and (got[b:] == self.snap[b:]).all(), "written outside the map"
        body = got[a:b].reshape(self.n, self.ld)
        assert not body[:, C:].any(), "a padding channel is not +0.0"
        return np.ascontiguousarray(body[:, :C]).view(np.float32)


def _src(H, W, ld, data, off=0):
    return Buf(H, W, ld, data, off, POISON)


class Labels:
    def __init__(self, lab):
        host = np.full(lab.size + 64, LABEL_SENT, dtype=np.int64)
        host[: lab.size] = lab
        self.snap, self.flat = host, _dev(host)
        self.t = self.flat[: lab.size]

    def unchanged(self):
        return np.array_equal(self.flat.cpu().numpy(), self.snap)


class Vec:
    """A float vector with NaN sentinels behind it."""

    def __init__(self, v):
        host = np.full(v.size + 64, POISON, dtype=np.int32)
        host[: v.size] = np.ascontiguousarray(v, dtype=np.float32).view(np.int32)
        self.snap, self.flat = host, _dev(host).view(torch.float32)
        self.t = self.flat[: v.size]

    def unchanged(self):
        return np.array_equal(_bits(self.flat), self.snap)


def _ulp(got, ref, mag, bud, what):
    e = R.scaled_ulp_error(got, ref, mag)
    assert np.isfinite(np.asarray(got, dtype=np.float64)).all() and e.max() <= bud, f"{what}: {float(e.max()):.2f} ulp at {int(e.argmax())}, budget {bud:.2f}"
    return float(e.max())


def _same_bits(a, b, what):
    for x, y in zip(a, b):
        assert (x is None and y is None) or np.array_equal(np.asarray(x).view(np.int32), np.asarray(y).view(np.int32)), f"{what}: the second run differs"


def _seghead_ws_zero(ops):
    for which in ("head", "norm"):
        assert not bool(ops._seghead_workspace(torch.device("cuda", 0), which).view(torch.int64).any()), f"the {which} workspace is not all zero"


@functools.lru_cache(maxsize=2)
def _head_inputs(H, W, C):
    return R.head_inputs(H, W, C, K.head_seed(H, W, C))


# ---- sgan_seg_head / _pw, sgan_label_weight_sum / sgan_pixel_weight_sum: softmax mode ---------------------------------------------
def _softmax_once(ops, H, W, C, zb, ld, lab, cw, add, want_dz, off):
    """norm through the weight-sum entry point, then the head.  Returns (norm, loss, p, dz) as read."""
    norm, loss = _scalar(), _scalar()
    if add is not None:
        ops.pixel_weight_sum(lab.t, C, cw.t if cw else None, add.t, norm)
    else:
        ops.label_weight_sum(lab.t, C, cw.t if cw else None, norm)
    p, d = Buf(H, W, ld, off=off), Buf(H, W, ld, off=off) if want_dz else None
    assert ops.seg_head(zb.t, C, ops.SEGHEAD_SOFTMAX, lab.t, cw.t if cw else None, C if cw else 0, norm, p.t, d.t if d else None, loss,
                        pixel_add=add.t if add is not None else None)
    out = (np.float32(float(norm)), np.float32(float(loss)), p.read(C), d.read(C) if d else None)
    _seghead_ws_zero(ops)
    return out


def _softmax_case(ops, H, W, C, ld, zld=None, off=0, variants=("u", "w", "pw_u", "pw_w")):
    z, lab, _, _, cw, add = _head_inputs(H, W, C)
    zb = _src(H, W, zld or ld, z, off)
    labd, cwd, addd = Labels(lab), Vec(cw), Vec(add)
    pref = R.softmax_ref(z, C)
    bp = R.budget(K.f32_softmax(z, C), pref)
    ok = (lab >= 0) & (lab < C)
    for i, v in enumerate(variants):
        w, a = (cw if v.endswith("w") else None), (add if v.startswith("pw") else None)
        want_dz = i % 2 == 0 or len(variants) == 1
        runs = [_softmax_once(ops, H, W, C, zb, ld, labd, cwd if w is not None else None, addd if a is not None else None, want_dz, off)
                for _ in range(2)]
        _same_bits(runs[0], runs[1], v)
        norm, loss, p, dz = runs[0]
        s, bound = R.weight_sum_ref(C, lab, w, a)
        assert abs(float(norm) - s) <= bound, (v, "norm", float(norm), s, bound)
        rl, rg, den, lmag, gmag = R.ce_ref(z, C, lab, 0, w, 1.0, pixel_add=a)
        l32, g32 = K.f32_ce(z, C, lab, 0, w, 1.0, a)
        ep = _ulp(p, pref, None, bp, f"{v} p")
        bl = R.budget(l32, rl, lmag)
        el = _ulp(loss, rl, lmag, bl, f"{v} loss")
        msg = f"seg_head softmax {H}x{W} C={C} ld={ld} {v}: p {ep:.2f} of {bp:.2f} ulp, loss {el:.2f} of {bl:.2f}"
        if dz is not None:
            bg = R.budget(g32, rg, gmag)
            eg = _ulp(dz, rg, gmag, bg, f"{v} dz")
            assert not (dz[~ok].view(np.int32) & 0x7FFFFFFF).any(), f"{v}: a pixel with a label outside [0, C) has a gradient"
            msg += f", dz {eg:.2f} of {bg:.2f}"
        print(msg)
    # every label ignored: norm 0, loss 0, dz all zero, p as before
    ign = np.full(H * W, -100, dtype=np.int64)
    ign[::3], ign[1::7] = R.BIG_LABELS[0], C
    ignd = Labels(ign)
    norm, loss, p, dz = _softmax_once(ops, H, W, C, zb, ld, ignd, cwd, addd, True, off)
    assert float(norm) == 0.0 and float(loss) == 0.0 and not (dz.view(np.int32) & 0x7FFFFFFF).any()
    _ulp(p, pref, None, bp, "ignored p")
    for b in (zb, labd, cwd, addd, ignd):
        assert b.unchanged(), "an input was written"


@pytest.mark.parametrize("H,W,C,ld", K.head_shapes(), ids=lambda v: str(v))
def test_seg_head_softmax(ops, H, W, C, ld):
    """The 16-byte row forms 4 / 8 / 12 / 16 and the scalar form (5, 5), at 35, 771, 65 792 (257 workgroups: the slot sum's second trip)
    and 131 406 pixels (past the 512-workgroup cap).  Unweighted, weighted, PW with a non-zero map; dz asked for and not; the first
    image row -100, then C, -1, 2^32 + 1 and -(2^32) + 2; a map with every label ignored."""
    _softmax_case(ops, H, W, C, ld)


# ---- sgan_seg_head: sigmoid mode ----------------------------------------------------------------------------------------------
def _sigmoid_once(ops, H, W, C, zb, tb, ld, cw, nw, want_dz, off):
    loss = _scalar()
    p, d = Buf(H, W, ld, off=off), Buf(H, W, ld, off=off) if want_dz else None
    assert ops.seg_head(zb.t, C, ops.SEGHEAD_SIGMOID, tb.t, cw.t if nw else None, nw, None, p.t, d.t if d else None, loss)
    out = (np.float32(float(loss)), p.read(C), d.read(C) if d else None)
    _seghead_ws_zero(ops)
    return out


def _sigmoid_case(ops, H, W, C, ld, zld=None, off=0, variants=(("0", 0), ("2", 1), ("C", 0), ("C", 1))):
    z, _, hot, soft, cw, _ = _head_inputs(H, W, C)
    zb, cwd = _src(H, W, zld or ld, z, off), Vec(cw)
    p64 = R.sigmoid64(z)
    pc = R.p_candidates(p64)
    plo, phi = pc.min(0), pc.max(0)
    for i, (which, is_soft) in enumerate(variants):
        nw, t = K.nw_of(which, C), (soft if is_soft else hot)
        tb = _src(H, W, ld, t, off)
        want_dz = i % 2 == 0 or len(variants) == 1
        runs = [_sigmoid_once(ops, H, W, C, zb, tb, ld, cwd, nw, want_dz, off) for _ in range(2)]
        _same_bits(runs[0], runs[1], which)
        loss, p, dz = runs[0]
        (llo, lhi), (glo, ghi) = R.bcew_ref(p64, t, C, cw, nw, 1.0, chain=True)
        what = f"seg_head sigmoid {H}x{W} C={C} ld={ld} nw={nw} {'soft' if is_soft else 'hard'}"
        _in(p, plo, phi, what + " p")
        _in(float(loss), llo, lhi, what + " loss")
        if dz is not None:
            _in(dz, glo, ghi, what + " dz")
        assert tb.unchanged()
    assert zb.unchanged() and cwd.unchanged()


@pytest.mark.parametrize("H,W,C,ld", K.head_shapes(), ids=lambda v: str(v))
def test_seg_head_sigmoid(ops, H, W, C, ld):
    """nw = 0, 2 and C, one-hot and soft targets, dz asked for and not, at the shapes of test_seg_head_softmax."""
    _sigmoid_case(ops, H, W, C, ld)


@pytest.mark.parametrize("layout", ["z_of_8_beside_4", "misaligned_base"])
@pytest.mark.parametrize("H,W", K.HEAD_SMALL)
def test_seg_head_scalar_forms_of_vector_sized_rows(ops, H, W, layout):
    """Logits that are the first 3 channels of an 8-channel buffer beside 4-channel outputs, and 4-channel operands whose base is one
    element into a larger allocation: both take the scalar form."""
    zld, off = (8, 0) if layout == "z_of_8_beside_4" else (4, 1)
    _softmax_case(ops, H, W, 3, 4, zld, off, variants=("pw_w",))
    _sigmoid_case(ops, H, W, 3, 4, zld, off, variants=(("C", 1),))


@pytest.mark.parametrize("H,W,C", [(5, 7, 3), (257, 3, 5)])
def test_seg_head_upstream_gradient_through_the_rescale_launch(ops, H, W, C):
    """losses.seg_head with (1.7 loss).backward(): dz is the forward's gradient times 1.7, one more rounding."""
    from supervised_gan_amd import losses
    z, lab, hot, soft, cw, add = _head_inputs(H, W, C)
    ok = (lab >= 0) & (lab < C)

    def nchw(a):
        return _dev(np.ascontiguousarray(a.reshape(H, W, -1).transpose(2, 0, 1)[None]))

    def grad_of(zd):
        return zd.grad[0].permute(1, 2, 0).reshape(H * W, C).cpu().numpy()

    zd = nchw(z).requires_grad_(True)
    p, loss = losses.seg_head(zd, _dev(lab.reshape(1, H, W)), _dev(cw), None, ops.SEGHEAD_SOFTMAX, pixel_add=_dev(add.reshape(H, W)))
    (loss * K.HEAD_GOUT).backward()
    rl, rg, den, lmag, gmag = R.ce_ref(z, C, lab, 0, cw, K.HEAD_GOUT, pixel_add=add)
    l32, g32 = K.f32_ce(z, C, lab, 0, cw, K.HEAD_GOUT, add)
    dz = grad_of(zd)
    _ulp(dz, rg, gmag, R.budget(g32, rg, gmag), "softmax dz * 1.7")
    _ulp(float(loss.detach()), rl, lmag, R.budget(l32, rl, lmag), "softmax loss")
    assert not (dz[~ok].view(np.int32) & 0x7FFFFFFF).any()
    zd = nchw(z).requires_grad_(True)
    p, loss = losses.seg_head(zd, nchw(soft), _dev(cw), None, ops.SEGHEAD_SIGMOID)
    (loss * K.HEAD_GOUT).backward()
    (llo, lhi), (glo, ghi) = R.bcew_ref(R.sigmoid64(z), soft, C, cw, C, K.HEAD_GOUT, chain=True, extra=1)
    _in(grad_of(zd), glo, ghi, "sigmoid dz * 1.7")
    _in(float(loss.detach()), llo, lhi, "sigmoid loss")
    _seghead_ws_zero(ops)


# ---- sgan_sigmoid_nhwc_fwd / _bwd, sgan_bce_weighted_fwd / _bwd ---------------------------------------------------------------------
def _bcew_ticket_zero(ops):
    ws = ops._zeroed_workspace("bce_weighted", torch.device("cuda", 0), ops.BCE_WEIGHTED_WS_BYTES)
    assert not bool(ws[64:].view(torch.int64).any()), "the ticket is not back at zero"


def _sigmoid_ss_case(ops, H, W, C, ld, pld, dpld):
    n = H * W
    z, _, hot, soft, cw, _ = _head_inputs(H, W, C)
    zb, cwd = _src(H, W, ld, z), Vec(cw)
    p64 = R.sigmoid64(z)
    pc = R.p_candidates(p64)
    outs = []
    for _ in range(2):
        p = Buf(H, W, pld)
        ops.sigmoid_nhwc_fwd(zb.t, C, p.t)
        outs.append(p.read(C))
    _same_bits(outs[:1], outs[1:], "sigmoid_nhwc_fwd")
    _in(outs[0], pc.min(0), pc.max(0), "sigmoid_nhwc_fwd p")
    p32 = p64.astype(np.float32)                        # a given p for the other three: the fp32 rounding of the float64 sigmoid
    pb = _src(H, W, pld, p32)
    for which, t in (("0", hot), ("1", soft), ("C", hot)):
        nw = K.nw_of(which, C)
        tb = _src(H, W, ld, t)
        losses = []
        for _ in range(2):
            loss = _scalar()
            ops.bce_weighted_fwd(pb.t, tb.t, C, cwd.t if nw else None, nw, loss)
            losses.append(np.float32(float(loss)))
            _bcew_ticket_zero(ops)
        _same_bits(losses[:1], losses[1:], "bce_weighted_fwd")
        for gout in (1.0, -2.5):
            (llo, lhi), (glo, ghi) = R.bcew_ref(p32, t, C, cw, nw, gout, chain=False)
            _in(float(losses[0]), llo, lhi, f"bce_weighted_fwd nw={nw}")
            dps = []
            for _ in range(2):
                dp = Buf(H, W, dpld)
                ops.bce_weighted_bwd(pb.t, tb.t, C, cwd.t if nw else None, nw, _scalar(gout), dp.t)
                dps.append(dp.read(C))
            _same_bits(dps[:1], dps[1:], "bce_weighted_bwd")
            _in(dps[0], glo, ghi, f"bce_weighted_bwd nw={nw} gout={gout}")
        assert tb.unchanged()
    g = (np.random.default_rng(n + C).standard_normal((n, C)) * 2.0).astype(np.float32)
    gb = _src(H, W, dpld, g)
    dz = Buf(H, W, ld)
    ops.sigmoid_nhwc_bwd(gb.t, pb.t, C, dz.t)
    _rel(dz.read(C), g.astype(np.float64) * p32 * (1.0 - p32.astype(np.float64)), 4, "sigmoid_nhwc_bwd")
    for b in (zb, cwd, pb, gb):
        assert b.unchanged(), "an input was written"


@pytest.mark.parametrize("C,ld,pld,dpld", K.BCEW_PAIRS, ids=lambda v: str(v))
@pytest.mark.parametrize("H,W", K.BCEW_SHAPES, ids=lambda v: str(v))
def test_sigmoid_ss_kernels(ops, H, W, C, ld, pld, dpld):
    """16 383, 16 384, 16 385 and 130 x 127 pixels around the forward's 64-workgroup sweep; ld != pld != dpld; nw = 0, 1, C; soft
    targets; gout 1 and -2.5."""
    _sigmoid_ss_case(ops, H, W, C, ld, pld, dpld)


@pytest.mark.parametrize("npix", [K.BCEW_BWD_CAP_NPIX, K.SIGMOID_CAP_NPIX])
def test_sigmoid_ss_kernels_past_their_workgroup_caps(ops, npix):
    """1025 workgroups' worth for the 1024 cap of sgan_bce_weighted_bwd, 2049 for the 2048 cap of sgan_sigmoid_nhwc_*: C = 1, ld = 4."""
    _sigmoid_ss_case(ops, 1, npix, 1, 4, 4, 4)


@pytest.mark.parametrize("t", [0.0, 1.0, 0.9])
def test_planted_logits_of_the_sigmoid_paths(ops, t):
    """+-17 .. +-120 as a 16-pixel one-channel map through the sigmoid head and the three separate kernels: finite, inside the
    intervals (a denormal p may be flushed to 0, exact 0 and 1 stay candidates), no cap on the widths."""
    z = np.array(R.GAN_PLANTED, dtype=np.float32).reshape(-1, 1)
    tt = np.full_like(z, t)
    cw = np.array([3.0], dtype=np.float32)
    zb, tb, cwd = _src(1, 16, 4, z), _src(1, 16, 4, tt), Vec(cw)
    p64 = R.sigmoid64(z)
    pc = R.p_candidates(p64)
    for nw in (0, 1):
        loss, dz = _sigmoid_once(ops, 1, 16, 1, zb, tb, 4, cwd, nw, True, 0)[::2]
        (llo, lhi), (glo, ghi) = R.bcew_ref(p64, tt, 1, cw, nw, 1.0, chain=True)
        _in(float(loss), llo, lhi, f"head loss nw={nw}")
        _in(dz, glo, ghi, f"head dz nw={nw}")
        p = Buf(1, 16, 4)
        ops.sigmoid_nhwc_fwd(zb.t, 1, p.t)
        got = p.read(1)
        _in(got, pc.min(0), pc.max(0), "sigmoid_nhwc_fwd")
        loss, dp = _scalar(), Buf(1, 16, 4)
        ops.bce_weighted_fwd(p.t, tb.t, 1, cwd.t if nw else None, nw, loss)
        ops.bce_weighted_bwd(p.t, tb.t, 1, cwd.t if nw else None, nw, _scalar(1.0), dp.t)
        _in(float(loss), llo, lhi, f"bce_weighted_fwd nw={nw}")
        _in(dp.read(1), *R.bcew_ref(p64, tt, 1, cw, nw, 1.0, chain=False)[1], f"bce_weighted_bwd nw={nw}")


# ---- sgan_factd_loss_multi_fwd / _bwd ---------------------------------------------------------------------------------------------
def _factd_ticket_zero(ops):
    ws = ops._factd_loss_workspace(torch.device("cuda", 0))
    assert not bool(ws[8 * 16:].view(torch.int64).any()), "the ticket is not back at zero"


def _named(idx, shape, pads):
    """Where element idx of an [h, w] map lies: corners and the rows / columns within the pads of a border by name."""
    h, w = shape
    y, x = divmod(int(idx), w)
    pl, pr, pt, pb = pads
    names = []
    if y in (0, h - 1) and x in (0, w - 1):
        names.append("corner")
    if y <= pt:
        names.append(f"within the top pad ({pt}) of the border")
    if y >= h - 1 - pb:
        names.append(f"within the bottom pad ({pb})")
    if x <= pl:
        names.append(f"within the left pad ({pl})")
    if x >= w - 1 - pr:
        names.append(f"within the right pad ({pr})")
    return f"({y}, {x})" + (": " + ", ".join(names) if names else ": interior")


def _factd_check_grad(got, ref, name, mode, shape, c32, what):
    """Per element of dl1 / dl2; the failure message names the first failing elements by where they lie."""
    h1, w1, up, H2, W2 = shape
    pads = R.factd_pad_split(H2 - h1 * up, W2 - w1 * up)
    if up == 2:
        pads = tuple((v + 1) // 2 for v in pads) if name == "dl1" else pads
    got = np.asarray(got, dtype=np.float64)
    if mode[2]:
        bud = R.budget(c32, ref[name], ref[name + "_mag"])
        e = R.scaled_ulp_error(got.reshape(ref[name].shape), ref[name], ref[name + "_mag"])
        bad, worst = ~(e <= bud), f"worst {float(e.max()):.2f} of {bud:.2f} ulp"
    else:
        lo, hi = ref[name + "_iv"]
        bad, worst = ~R.inside(got.reshape(lo.shape), lo, hi), "outside the interval"
        e = None
    bad |= ~np.isfinite(got.reshape(bad.shape))
    if bad.any():
        where = [_named(i, bad.shape, pads) for i in np.nonzero(bad.reshape(-1))[0][:6]]
        raise AssertionError(f"{what} {name}: {int(bad.sum())} of {bad.size} elements wrong ({worst}), first at " + "; ".join(where))
    return 0.0 if e is None else float(e.max())


def _factd_run(ops, terms, mode, wants, lds, gout=None):
    """One launch of the forward (gout None) or of the second entry point.  terms: [(l1, l2, up, target, weight)].  Returns (each, total,
    [dl1 or None], [dl2 or None]) as read."""
    b1 = [_src(l1.shape[0], l1.shape[1], ld[0], l1.reshape(-1, 1)) for (l1, *_), ld in zip(terms, lds)]
    b2 = [_src(l2.shape[0], l2.shape[1], ld[1], l2.reshape(-1, 1)) for (_, l2, *_), ld in zip(terms, lds)]
    d1 = [Buf(b.t.shape[0], b.t.shape[1], b.ld) if w[0] else None for b, w in zip(b1, wants)]
    d2 = [Buf(b.t.shape[0], b.t.shape[1], b.ld) if w[1] else None for b, w in zip(b2, wants)]
    ups, tgs, wts = [t[2] for t in terms], [t[3] for t in terms], [t[4] for t in terms]
    args = ([b.t for b in b1], [b.t for b in b2], ups, tgs, wts, ops.factd_mode(*mode))
    dls = ([d.t if d else None for d in d1], [d.t if d else None for d in d2])
    if gout is None:
        each, total = torch.full((len(terms),), float("nan"), device="cuda"), _scalar()
        assert ops.factd_loss_multi_fwd(*args, each, total, *dls)
        torch.cuda.synchronize()
        _factd_ticket_zero(ops)
        res = (each.cpu().numpy(), np.float32(float(total)))
    else:
        ops.factd_loss_multi_bwd(*args, _scalar(gout), *dls)
        res = (None, None)
    out = res + ([d.read(1)[:, 0] if d else None for d in d1], [d.read(1)[:, 0] if d else None for d in d2])
    for b in b1 + b2:
        assert b.unchanged(), "an input was written"
    return out


def _factd_check(ops, shapes, mode, targets, weights, wants, lds, seeds, gout=None):
    refs = [K.factd_reference(s, mode, t, w, 1.0 if gout is None else gout, seed) for s, t, w, seed in zip(shapes, targets, weights, seeds)]
    terms = [(r[0], r[1], s[2], t, w) for r, s, t, w in zip(refs, shapes, targets, weights)]
    runs = [_factd_run(ops, terms, mode, wants, lds, gout) for _ in range(2)]
    for a, b in zip(runs[0], runs[1]):
        _same_bits(a if isinstance(a, list) else [a], b if isinstance(b, list) else [b], "factd")
    each, total, d1, d2 = runs[0]
    elo, ehi = np.zeros(len(terms)), np.zeros(len(terms))
    for i, (s, (l1, l2, ref, c32)) in enumerate(zip(shapes, refs)):
        what = f"factd {s} mode {mode} t={targets[i]} w={weights[i]} term {i}"
        if gout is None:
            if mode[2]:
                be = R.budget(c32[0][0], ref["each"], ref["each_mag"])
                ee = _ulp(each[i], ref["each"], ref["each_mag"], be, what + " each")
                elo[i] = ref["each"] - be * 2 * U * ref["each_mag"]
                ehi[i] = ref["each"] + be * 2 * U * ref["each_mag"]
            else:
                elo[i], ehi[i] = ref["each_iv"]
                _in(each[i], elo[i], ehi[i], what + " each")
        for name, d, c in (("dl1", d1[i], c32[2][0]), ("dl2", d2[i], c32[3][0])):
            if d is not None:
                e = _factd_check_grad(d, ref, name, mode, s, c, what)
                if mode[2]:
                    print(f"{what} {name}: {e:.2f} ulp")
    if gout is None:
        _in(float(total), *R.weighted_total_interval(elo, ehi, weights), "total")
        tsum = np.array([R.f32(w) for w in weights]) * each.astype(np.float64)
        assert abs(float(total) - tsum.sum()) <= U * abs(tsum.sum()) + 2.0 ** -45 * np.abs(tsum).sum() + R.MIN_NORMAL


FACTD_WANTS = ((True, True), (True, False), (False, True))
FACTD_LDS = ((1, 1), (4, 1), (1, 4), (4, 4))
FACTD_WEIGHTS = (0.7, -0.6, 0.0)


@pytest.mark.parametrize("mode", R.FACTD_MODES, ids=["sig_sig_bce", "raw_raw_mse", "sig_raw_mse", "raw_sig_mse"])
@pytest.mark.parametrize("si", range(len(R.FACTD_SHAPES)), ids=["%dx%d_up%d_%dx%d" % s for s in R.FACTD_SHAPES])
def test_factd_one_term(ops, si, mode):
    """Every geometry in every mode, targets 0 and 1; over the cases ld 1 and 4 on each side independently, dl1 or dl2 absent,
    weights 0.7, -0.6 and 0; where both gradients are asked for, the second entry point with gout 2.5 as well."""
    shape = R.FACTD_SHAPES[si]
    mi = R.FACTD_MODES.index(mode)
    for ti, target in enumerate((0.0, 1.0)):
        want, ld, w = FACTD_WANTS[(si + mi + 2 * ti) % 3], FACTD_LDS[(si + 2 * mi + ti) % 4], FACTD_WEIGHTS[(si + mi + ti) % 3]
        seed = 100 + shape[0] * shape[3]
        _factd_check(ops, [shape], mode, [target], [w], [want], [ld], [seed])
        if want == (True, True):
            _factd_check(ops, [shape], mode, [target], [w], [want], [ld], [seed], gout=2.5)


@pytest.mark.parametrize("mode", [(1, 1, 0), (0, 0, 1)], ids=["sig_sig_bce", "raw_raw_mse"])
def test_factd_eight_terms_then_three_on_the_same_workspace(ops, mode):
    """Eight mixed geometries in one launch, weights of both signs and 0, gradient buffers for some; a 3-term launch directly behind
    it finds the ticket at zero; then the second entry point on the eight with gout 2.5."""
    sel = (0, 1, 8, 3, 10, 11, 6, 12)
    shapes = [R.FACTD_SHAPES[i] for i in sel]
    targets = [0.0, 0.0, 1.0, 0.0, 1.0, 1.0, 1.0, 0.0]
    weights = [0.25, -0.25, 0.25, 0.0, 0.5, 0.5, -0.6, -0.4]
    wants = [FACTD_WANTS[i % 3] for i in range(8)]
    lds = [FACTD_LDS[i % 4] for i in range(8)]
    seeds = [300 + i for i in range(8)]
    _factd_check(ops, shapes, mode, targets, weights, wants, lds, seeds)
    _factd_check(ops, shapes[5:], mode, targets[5:], weights[5:], wants[5:], lds[5:], seeds[5:])
    _factd_check(ops, shapes, mode, targets, weights, [(True, True)] * 8, lds, seeds, gout=2.5)


# ---- the wrappers refuse what the kernels would read or write out of bounds -------------------------------------------------------
def test_sigmoid_ss_wrappers_refuse_operands_that_do_not_fit(ops):
    """Nothing is launched: every output keeps its sentinel.  The guards must exist before any of these calls is made -- without
    them the calls below would read or write out of bounds on the device."""
    from supervised_gan_amd import _lib
    assert callable(getattr(ops, "_rows_fit", None)) and callable(getattr(ops, "_class_w_fits", None)), \
        "ops._rows_fit / ops._class_w_fits are missing: the calls of this test must not reach the device without them"
    E = _lib.SganError
    H, W, C = 5, 7, 3
    z, _, hot, _, cw, _ = _head_inputs(H, W, C)
    zb, tb, pb = _src(H, W, 4, z), _src(H, W, 4, hot), _src(H, W, 4, R.sigmoid64(z).astype(np.float32))
    cwd = _dev(cw)
    out, other, loss, one = Buf(H, W, 4), Buf(7, 6, 4), _scalar(), _scalar(1.0)
    narrow = Buf(H, W, 2)
    short = torch.zeros(96, device="cuda").as_strided((H, W, 4), (8, 8, 1))      # rows overlap: 35 pixels of stride 8 need 276 elements, 96 are there
    for bad in (other.t, narrow.t, short):        # another pixel count; fewer than Creal channels; too little storage
        with pytest.raises(E):
            ops.sigmoid_nhwc_fwd(zb.t, C, bad)
        with pytest.raises(E):
            ops.sigmoid_nhwc_fwd(bad, C, out.t)
        with pytest.raises(E):
            ops.sigmoid_nhwc_bwd(bad, pb.t, C, out.t)
        with pytest.raises(E):
            ops.sigmoid_nhwc_bwd(zb.t, pb.t, C, bad)
        with pytest.raises(E):
            ops.sigmoid_nhwc_bwd(zb.t, bad, C, out.t)
        with pytest.raises(E):
            ops.bce_weighted_fwd(pb.t, bad, C, cwd, C, loss)
        with pytest.raises(E):
            ops.bce_weighted_fwd(bad, tb.t, C, cwd, C, loss)
        with pytest.raises(E):
            ops.bce_weighted_bwd(pb.t, tb.t, C, cwd, C, one, bad)
        with pytest.raises(E):
            ops.bce_weighted_bwd(pb.t, bad, C, cwd, C, one, out.t)
    wide = _dev(np.repeat(cw, 2))
    for bad in (cwd.double(), wide[::2], cwd[:2], cwd.cpu(), None):      # not fp32; not contiguous; too few; on another device; absent
        with pytest.raises(E):
            ops.bce_weighted_fwd(pb.t, tb.t, C, bad, C, loss)
        with pytest.raises(E):
            ops.bce_weighted_bwd(pb.t, tb.t, C, bad, C, one, out.t)
    torch.cuda.synchronize()
    assert int(_bits(loss)[0]) == SENT
    for b in (out, other, narrow, zb, tb, pb):
        assert b.unchanged()


def test_weighted_bce_refuses_class_weights_on_another_device(ops):
    """ValueError, as cross_entropy_logits raises for a label map on another device."""
    from supervised_gan_amd import losses
    p = torch.full((1, 3, 4, 4), 0.5, device="cuda")
    with pytest.raises(ValueError):
        losses.weighted_bce(p, torch.zeros_like(p), torch.ones(3))

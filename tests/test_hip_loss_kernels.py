"""The loss kernels of csrc/sgan_ew.hip against the plain float64 references of tests/loss_ref.py: sgan_gan_loss_fwd / _bwd,
sgan_gan_loss_multi_fwd / _multi_bwd, sgan_l1w_fwd, sgan_bce01_fwd, sgan_ce_fwd / _bwd, sgan_softmax_fwd / _bwd, and the wrappers of
losses.py / ops.py in front of them.  tests/test_hip_loss_bits.py keeps the bits of these kernels; this file says whether the
bits are right, element by element: no error is normalised by a map's largest value.

Every output lies in storage that starts as a NaN sentinel and ends in TAIL sentinel floats: padding channels (c >= C; c >= 1 of a
logits gradient) come back exactly 0, everything behind the last pixel keeps the sentinel.  Source channels nobody should read hold
another NaN.  Every multi / CE case runs twice on the same workspace and the ticket word reads back as zero; the second run has the
bits of the first, except the CE loss of more than one workgroup (over 256 pixels): sg_ce_fwd_kernel adds its workgroups' fp64 sums
with atomics, in any order, so there the two losses may be fp32 neighbours, as in tests/test_hip_loss_bits.py (the reduction order
is not this file's to change).

Bounds (u = 2^-24, one fp32 rounding; none is measured on a kernel):
  BCE terms (GAN mode 0, bce01)   the interval of loss_ref: the float64 formula at p32 + k ulp, k = -3 .. 3 (and at 0 where p32 is
                     denormal), min and max per element, widened by 4 u |value| + 2^-126; a mean: the mean of the intervals,
                     widened by u |result|; each / total / the fp64 slot partials of the multi kernel likewise, through the weights.
                     On every random map the reference's own half-width of the summed loss is asserted <= 2e-5 of the loss.
  GAN mode 1 (x - t)^2            loss element: 3 roundings (x - t enters the square twice, the product) -> 4 u; a mean one more.
                     Gradient 2 (x - t) scale: x - t, scale = w / npix (single backward: gout / npix), the product -> 3 roundings,
                     bound 4 u |ref|; the multi backward rounds gout * w as well -> 4 roundings, bound 5 u |ref|.
  sgan_l1w_fwd       loss_ref.l1w_ref states the count: gradient (kw + 4) u |w| lam / N with kw = 0 (no weight, explicit map) or
                     3 + nw (label form); loss (kw + 3) u lam / N sum |d| |w| + u |loss|.
  sgan_ce_fwd / _bwd, sgan_softmax_fwd / _bwd   in fp32 ulps (of the reference for the softmax; of the magnitude that the roundings
                     are relative to where the expression cancels, loss_ref.ce_ref / softmax_bwd_ref): 4 x the largest error of
                     torch's CPU fp32 evaluation of the kernel's composition on the same inputs, at least 2 ulp (loss_ref.budget).
                     The CE denominator acc[1]: 1e-12 relative to the float64 sum of the weights.
Budgets as observed (pytest -s prints them beside the kernel's own error), worst over the six (C, ld) pairs and the four label
forms, budget / the kernel's own error in ulp, at 10 x 20, 70 x 66 and 363 x 362 pixels (torch's CPU kernels differ between hosts):
  softmax forward    40.33 / 10.08    52.13 / 13.18    64.03 / 15.41
  softmax backward   10.21 / 2.67     16.90 / 4.23     18.97 / 5.49
  CE gradient        48.19 / 12.05    55.85 / 14.73    65.15 / 16.72
  CE loss            2.00 (the floor) / 0.50    2.00 / 0.49    2.00 / 0.51
tests/test_loss_ref_host.py keeps the 10 x 20 budgets <= 64 ulp (the CE loss: <= 16).

That the file can fail: one arithmetic change each to a scratch copy of sgan_ew.hip (sgan_reduce.h for the clamp), none of which
touches addressing, and the tests of this file that fail with the library built from it (all pass with the library as it is):
  * `/ npix` taken as `/ (npix + 1)` in the multi forward's gradient only (go = J.weight[j] / (float)(np + 1)): the 16 cases of
    test_gan_multi that have a gradient buffer (both modes; every case but "absent"), all 4 of test_gan_multi_planted_logits
  * the `u` unroll reading 3 of 4 strides (both loops of sg_gan_loss_multi_fwd_kernel): all cases of test_gan_multi (22 as the file stands) -- each holds
    the 130 x 127 map, whose fourth stride is not empty (slots, each, total, and the sentinel left in the gradient)
  * the 1e-12 clamp dropped (sg_bce_dden returns (1 - p) p): all 4 of test_gan_single_planted_logits, all 4 of
    test_gan_multi_planted_logits, all 8 of test_image_losses (bce01 at the planted p = 0 and p = 1)
  * `class_w[y]` read as `class_w[0]` in sg_ce_bwd_kernel: 15 of the 18 cases of test_cross_entropy (with C = 1 there is no other class)
  * the softmax backward's `dot` summed over pld instead of C: the 9 cases of test_softmax with pld > C, (C, ld) = (1, 4), (3, 4), (5, 8)
With the library of the parent commit (labels narrowed to int before the range test): the same 15 cases of test_cross_entropy.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases as K
import loss_ref as R

pytestmark = pytest.mark.gpu

U = R.U
SENT = 0x7FC5A5A5          # a quiet NaN with a payload: what every output word holds before the call
POISON = 0x7FC1B2B3        # another: what source channels hold that nobody should read
TAIL = 256                 # sentinel floats behind the last pixel of every output
GOUT = 0.37


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import _lib, ops
    _lib.lib()
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _filled(n, bits):
    return torch.full((n,), bits, dtype=torch.int32, device="cuda").view(torch.float32)


class Out:
    """[H, W, ld] fp32 output and TAIL floats behind it, all SENT."""

    def __init__(self, H, W, ld):
        self.H, self.W, self.ld, self.n = H, W, ld, H * W
        self.flat = _filled(self.n * ld + TAIL, SENT)
        self.t = self.flat[: self.n * ld].view(H, W, ld)

    def read(self, Creal, stored=None):
        """[npix, Creal] fp32 as written: channels Creal .. stored - 1 must be 0 (stored: how many channels the kernel owns, default
        all ld), channels behind `stored` and the TAIL must keep the sentinel."""
        stored = self.ld if stored is None else stored
        torch.cuda.synchronize()
        got = self.flat.cpu().numpy().view(np.int32)
        body = got[: self.n * self.ld].reshape(self.n, self.ld)
        assert (got[self.n * self.ld:] == SENT).all(), "written beyond the last pixel"
        assert (body[:, stored:] == SENT).all(), "written beyond the channels the kernel owns"
        assert not (body[:, Creal:stored] & 0x7FFFFFFF).any(), "a padding channel is not 0"
        return np.ascontiguousarray(body[:, :Creal]).view(np.float32)


def _src(data, ld):
    """[npix, C] host data -> device [1, npix, ld] buffer with POISON in channels C .. ld - 1."""
    data = np.asarray(data, dtype=np.float32)
    n, Cn = data.shape
    host = np.full((n, ld), POISON, dtype=np.int32).view(np.float32)
    host[:, :Cn] = data
    return _dev(host).view(1, n, ld)


def _map(x, ld):
    """[h, w] logits -> device [h, w, ld] map, POISON behind channel 0."""
    h, w = x.shape
    return _src(x.reshape(-1, 1), ld).view(h, w, ld)


def _scalar(v=None):
    if v is None:
        return _filled(1, SENT)[0]
    return torch.full((), v, dtype=torch.float32, device="cuda")


def _bits(t):
    return t.detach().cpu().numpy().reshape(-1).view(np.int32).copy()


def _in(got, lo, hi, what):
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), f"{what}: not finite"
    bad = ~R.inside(got, lo, hi)
    if bad.any():
        i = int(np.argmax(bad.reshape(-1)))
        raise AssertionError(f"{what}: {int(bad.sum())} outside the interval, first at {i}: {got.reshape(-1)[i]!r} not in "
                             f"[{np.asarray(lo).reshape(-1)[i]!r}, {np.asarray(hi).reshape(-1)[i]!r}]")


def _rel(got, ref, k, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bad = ~(np.abs(got - ref) <= k * U * np.abs(ref) + R.MIN_NORMAL)
    assert not bad.any(), f"{what}: {int(bad.sum())} beyond {k} u, first at {int(np.argmax(bad.reshape(-1)))}"


def _loss_elems(x, target, mode):
    lo, hi = R.gan_loss_elem(x, target, mode)
    return R.widen(lo, hi, 4) if mode == 1 else (lo, hi)       # mode 1: three roundings per element (module docstring)


def _check_grad(got, x, target, mode, scale, what, k1=4):
    lo, hi = R.gan_grad_elem(x.reshape(-1), target, mode, scale)
    if mode == 1:
        _rel(got, lo, k1, what)
    else:
        _in(got, lo, hi, what)


# ---- sgan_gan_loss_fwd / _bwd ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld,dld", [(1, 1), (4, 4), (1, 4)])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("h,w,seed", K.SINGLE_MAPS, ids=lambda v: str(v))
def test_gan_single(ops, h, w, seed, mode, ld, dld):
    """1, 1023, 1025 and 67 x 67 pixels around the 1024-thread sweep of the one-workgroup forward; all four targets."""
    x = R.gan_logits(h, w, seed)
    lg = _map(x, ld)
    for target in R.GAN_TARGETS:
        loss, p = _scalar(), Out(h, w, ld)
        ops.gan_loss_fwd(lg, target, mode, loss, p.t if mode == 0 else None)
        lo, hi = _loss_elems(x.reshape(-1), target, mode)
        if mode == 0:
            assert R.gan_half_width(x, target) <= R.GAN_MAX_HALF_WIDTH
            pc = R.p_candidates(R.sigmoid64(x.reshape(-1)))
            _in(p.read(1, 1)[:, 0], pc.min(0), pc.max(0), f"p_out t={target}")      # channel 0 only: the rest keeps the sentinel
        _in(float(loss), *R.mean_interval(lo, hi), f"loss t={target}")
        d = Out(h, w, dld)
        ops.gan_loss_bwd(lg, target, mode, _scalar(GOUT), d.t)
        _check_grad(d.read(1)[:, 0], x, target, mode, R.f32(GOUT) / x.size, f"dlogits t={target}")


@pytest.mark.parametrize("dld", [1, 4])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("h,w,seed", K.BWD_MAPS, ids=lambda v: str(v))
def test_gan_bwd_past_one_sweep(ops, h, w, seed, mode, dld):
    """130 x 127 = 16 510 and 16 384 +- 1 pixels around one sweep of the multi kernel, and 65 537 pixels: 257 workgroups' worth for the
    256-workgroup cap of sgan_gan_loss_bwd, whose grid-stride loop takes the last pixel."""
    x = R.gan_logits(h, w, seed)
    lg = _map(x, 4 if dld == 4 else 1)
    for target in (0.9, 0.0):
        d = Out(h, w, dld)
        ops.gan_loss_bwd(lg, target, mode, _scalar(GOUT), d.t)
        _check_grad(d.read(1)[:, 0], x, target, mode, R.f32(GOUT) / x.size, f"dlogits t={target}")


def _planted_asserts(x, target, loss, grad, weight):
    """What the issue states for a planted logit alone in its 1 x 1 map, beside the interval."""
    assert np.isfinite(loss) and np.isfinite(grad)
    if target in (0.0, 1.0):
        assert loss <= 100.0
    if x == -30.0 and target == 1.0:      # p (1 - p) = 9.4e-14 < 1e-12: the gradient decays as -p (1 - p) / 1e-12 w, far below p - t = -1
        p = float(R.sigmoid64(-30.0))
        want = -p * (1 - p) / R.CLAMP * weight
        assert abs(grad - want) <= 10 * U * abs(want) and abs(grad) < 0.1 * abs(weight)      # 3 ulp of p = 6 u, 4 roundings


@pytest.mark.parametrize("target", R.GAN_TARGETS)
def test_gan_single_planted_logits(ops, target):
    """Each of +-17 .. +-120 alone in a 1 x 1 map: its loss and gradient are observable by themselves."""
    for xv in R.GAN_PLANTED:
        x = np.full((1, 1), xv, dtype=np.float32)
        lg, loss, d = _map(x, 1), _scalar(), Out(1, 1, 1)
        ops.gan_loss_fwd(lg, target, 0, loss)
        ops.gan_loss_bwd(lg, target, 0, _scalar(GOUT), d.t)
        g = float(d.read(1)[0, 0])
        lo, hi = R.gan_loss_elem(x.reshape(-1), target, 0)
        _in(float(loss), *R.mean_interval(lo, hi), f"loss x={xv}")
        _check_grad([g], x, target, 0, R.f32(GOUT), f"dlogits x={xv}")
        _planted_asserts(xv, target, float(loss), g, R.f32(GOUT))


# ---- sgan_gan_loss_multi_fwd / _multi_bwd ---------------------------------------------------------------------------------------
def _gan_ws(ops):
    return ops._zeroed_workspace("gan_loss", torch.device("cuda", 0), ops.GAN_LOSS_WS_BYTES)


def _run_multi(ops, xs, lds, targets, weights, mode, dlds):
    """One forward launch on the shared workspace.  Returns (each, total, slots [n, 16], gradients as read)."""
    n = len(xs)
    ws = _gan_ws(ops)
    lg = [_map(x, ld) for x, ld in zip(xs, lds)]
    outs = [Out(x.shape[0], x.shape[1], dld) if dld else None for x, dld in zip(xs, dlds)]
    each, total = _filled(n, SENT), _scalar()
    ops.gan_loss_multi_fwd(lg, targets, weights, mode, each, total, [o.t if o else None for o in outs] if any(dlds) else None)
    torch.cuda.synchronize()
    w64 = ws.cpu().numpy()
    assert not w64[8 * R.GAN_BLOCKS:].view(np.int64).any(), "the ticket is not back at zero"
    grads = [o.read(1)[:, 0] if o else None for o in outs]
    return each.cpu().numpy(), float(total), w64[: n * R.GAN_BLOCKS].reshape(n, R.GAN_BLOCKS).copy(), grads, lg


def _check_multi(ops, xs, lds, targets, weights, mode, dlds, planted=False):
    n = len(xs)
    first = _run_multi(ops, xs, lds, targets, weights, mode, dlds)
    second = _run_multi(ops, xs, lds, targets, weights, mode, dlds)
    for a, b in zip(first[:3], second[:3]):
        assert np.array_equal(np.asarray(a).view(np.int32 if np.asarray(a).dtype == np.float32 else np.int64),
                              np.asarray(b).view(np.int32 if np.asarray(b).dtype == np.float32 else np.int64)), "the second run differs"
    for a, b in zip(first[3], second[3]):
        assert (a is None and b is None) or np.array_equal(a.view(np.int32), b.view(np.int32)), "the second run's gradient differs"
    each, total, slots, grads, lg = first
    elo, ehi = np.zeros(n), np.zeros(n)
    for i, x in enumerate(xs):
        lo, hi = _loss_elems(x.reshape(-1), targets[i], mode)
        if mode == 0 and not planted:
            assert R.gan_half_width(x, targets[i]) <= R.GAN_MAX_HALF_WIDTH
        _in(slots[i], *R.gan_slot_intervals(lo, hi), f"slots of term {i}")
        elo[i], ehi[i] = R.mean_interval(lo, hi)
        _in(each[i], elo[i], ehi[i], f"each[{i}]")
        if grads[i] is not None:
            _check_grad(grads[i], x, targets[i], mode, R.f32(weights[i]) / x.size, f"dlogits of term {i}")
    _in(total, *R.weighted_total_interval(elo, ehi, weights), "total")
    terms = np.array([R.f32(w) for w in weights]) * each.astype(np.float64)      # the total is the fp64 sum of w_i each_i, rounded once
    assert abs(total - terms.sum()) <= U * abs(terms.sum()) + 2.0 ** -45 * np.abs(terms).sum() + R.MIN_NORMAL
    return each, total, grads, lg


MULTI_GRADS = {"absent": lambda i: 0, "dld1": lambda i: 1, "dld4": lambda i: 4, "some": lambda i: (0, 4, 1)[i % 3]}


@pytest.mark.parametrize("n,grads", [(n, g) for n in (1, 3, 8) for g in MULTI_GRADS if (n, g) != (1, "some")])      # one term: "some" is "absent"
@pytest.mark.parametrize("mode", [0, 1])
def test_gan_multi(ops, mode, n, grads):
    """n = 1, 3, 8 terms of mixed sizes (130 x 127 past one 16 * 256 * 4 sweep), mixed ld, targets 1 / 0 / 0.9 / 0.1, weights with a
    negative one and 0; gradient buffers absent, dld 1, dld 4, present for some terms only.  Where every term has a buffer, the
    backward entry point with an upstream gradient of 0.37 is held to the same reference through scale = 0.37 w / npix."""
    first = {1: 2, 3: 0, 8: 0}[n]                    # n = 1: the 130 x 127 map alone
    sel = list(range(first, first + n))
    xs = [R.gan_logits(*K.MULTI_MAPS[i]) for i in sel]
    lds = [K.MULTI_LD[i] for i in sel]
    targets, weights = [K.MULTI_TARGETS[i] for i in sel], [K.MULTI_WEIGHTS[i] for i in sel]
    dlds = [MULTI_GRADS[grads](i) for i in range(n)]
    each, total, g1, lg = _check_multi(ops, xs, lds, targets, weights, mode, dlds)
    if all(dlds):
        outs = [Out(x.shape[0], x.shape[1], dld) for x, dld in zip(xs, dlds)]
        ops.gan_loss_multi_bwd(lg, targets, weights, mode, _scalar(GOUT), [o.t for o in outs])
        for i, (x, o) in enumerate(zip(xs, outs)):
            _check_grad(o.read(1)[:, 0], x, targets[i], mode, R.f32(GOUT) * R.f32(weights[i]) / x.size, f"multi_bwd term {i}", k1=5)


@pytest.mark.parametrize("target", R.GAN_TARGETS)
def test_gan_multi_planted_logits(ops, target):
    """The sixteen planted logits, eight 1 x 1 maps per launch."""
    weights = (0.5, -0.6, 2.0, 1.0, 1.0, 0.125, 3.0, 0.75)
    for k in (0, 8):
        vals = R.GAN_PLANTED[k: k + 8]
        xs = [np.full((1, 1), v, dtype=np.float32) for v in vals]
        each, total, grads, _ = _check_multi(ops, xs, [1, 4] * 4, [target] * 8, weights, 0, [1, 4] * 4, planted=True)
        assert np.isfinite(total)
        for v, e, g, w in zip(vals, each, grads, weights):
            _planted_asserts(v, target, float(e), float(g[0]), R.f32(w))


# ---- sgan_l1w_fwd, sgan_bce01_fwd ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,ld", [(2, 4), (3, 3)])
@pytest.mark.parametrize("H,W", [(10, 10), (1, 255), (1, 257), (257, 256)])
def test_image_losses(ops, H, W, C, ld):
    """100, 255 and 257 pixels; 257 x 256 is past the 256-workgroup cap.  l1w with a three-channel label image and weights, an explicit
    weight map, and no weight, lambda = 10 (sign(0) = 0 at the planted x == y); bce01 with x, t = +-1 planted."""
    x, y, a, wts, wmap = R.image_inputs(H, W, C, ld, 7 + H + W)
    xd, yd = _src(x[:, :C], ld).view(H, W, ld), _src(y[:, :C], ld).view(H, W, ld)
    ad, wd, wm = _src(a[:, :3], 4).view(H, W, 4), _dev(wts), _dev(wmap).view(H, W, 1)
    for name, aa, ww, nw, ha in (("label3", ad, wd, 3, a), ("map", wm, None, 0, wmap), ("plain", None, None, 0, None)):
        loss, g = _scalar(), Out(H, W, ld)
        ops.l1w_fwd(xd, yd, C, aa, ww, nw, 10.0, loss, g.t)
        rl, rg, lb, gb = R.l1w_ref(x, y, C, ha, wts, nw, 10.0)
        got = g.read(C)
        assert np.isfinite(float(loss)) and abs(float(loss) - rl) <= lb, (name, float(loss), rl, lb)
        bad = ~(np.abs(got.astype(np.float64) - rg) <= gb)          # a NaN (the sentinel of an unwritten element) is bad
        assert np.isfinite(got).all() and not bad.any(), f"l1w {name}: {int(bad.sum())} gradient elements beyond the bound"
        assert got[H * W - 1, 0] == 0.0 and rg[H * W - 1, 0] == 0.0
    loss, g = _scalar(), Out(H, W, ld)
    ops.bce01_fwd(xd, yd, C, loss, g.t)
    (llo, lhi), (glo, ghi) = R.bce01_ref(x, y, C)
    assert lhi - llo <= 1e-4 * lhi
    _in(g.read(C), glo, ghi, "bce01 gradient")
    _in(float(loss), llo, lhi, "bce01 loss")


# ---- sgan_ce_fwd / _bwd -------------------------------------------------------------------------------------------------------
def _ce_once(ops, zd, H, W, C, ld, label, const, cw):
    acc = torch.zeros(3, dtype=torch.float64, device="cuda")
    loss, d = _scalar(), Out(H, W, ld)
    out = []
    for _ in range(2):                                # twice on the same scratch: the sums are the caller's to clear, the ticket is not
        acc[:2].zero_()
        ops.ce_fwd(zd, C, label, const, cw, acc, loss)
        torch.cuda.synchronize()
        assert int(acc.view(torch.int64)[2]) == 0, "the ticket is not back at zero"
        out.append((float(loss), float(acc[1])))
    ops.ce_bwd(zd, C, label, const, cw, acc, _scalar(GOUT), d.t)
    return out, d.read(C)


@pytest.mark.parametrize("C,ld", R.CE_PAIRS)
@pytest.mark.parametrize("H,W", R.CE_SHAPES)
def test_cross_entropy(ops, H, W, C, ld):
    """One workgroup, several, and 363 x 362 = 514 workgroups' worth, past the 512-workgroup cap of the forward (the backward's cap of
    1024: test_cross_entropy_past_the_backward_cap); the backward always runs behind that forward.  Labels -100, C, -1, 2^32 + 1 and
    -(2^32) + 2 are skipped; a map that is entirely ignored gives loss 0 and an all-zero gradient; const_label k = 0 and k = C - 1."""
    _ce_case(ops, H, W, C, ld)


def test_cross_entropy_past_the_backward_cap(ops):
    """1 x 262 147 pixels: 1025 workgroups' worth for the 1024-workgroup cap of sgan_ce_bwd; the last three pixels belong to the
    grid-stride loop's second pass."""
    assert R.CE_BWD_CAP_NPIX > 1024 * 256
    _ce_case(ops, 1, R.CE_BWD_CAP_NPIX, 3, 4)


def _ce_case(ops, H, W, C, ld):
    z, lab, cw = R.ce_inputs(H, W, C, ld, 100 + C)
    zd, labd, cwd = _src(z[:, :C], ld).view(H, W, ld), _dev(lab), _dev(cw)
    ignored = np.full(H * W, -100, dtype=np.int64)
    ignored[::3], ignored[1::7] = R.BIG_LABELS[0], C
    forms = [("map_w", lab, 0, cw), ("map_u", lab, 0, None), ("const0_w", None, 0, cw), ("constlast_u", None, C - 1, None),
             ("ignored", ignored, 0, cw)]
    for name, label, const, w in forms:
        runs, grad = _ce_once(ops, zd, H, W, C, ld, _dev(label) if label is not None else None, const, cwd if w is not None else None)
        loss, rg, den, lmag, gmag = R.ce_ref(z, C, label, const, w, GOUT)
        if name == "ignored":
            assert all(r == (0.0, 0.0) for r in runs) and not (grad.view(np.int32) & 0x7FFFFFFF).any()
            continue
        l32, g32 = K.f32_ce(z, C, label, const, w, GOUT)
        bl, bg = R.budget(l32, loss, lmag), R.budget(g32, rg, gmag)
        for got_loss, got_den in runs:
            assert abs(got_den - den) <= 1e-12 * den, (name, got_den, den)
            el = float(R.scaled_ulp_error(got_loss, loss, lmag))
            assert np.isfinite(got_loss) and el <= bl, (name, got_loss, loss, el, bl)
        # several workgroups add their fp64 sums in any order: the two runs agree to an fp32 neighbour, one workgroup bit for bit
        a, b = (np.float32(r[0]).view(np.int32) for r in runs)
        assert abs(int(a) - int(b)) <= (0 if H * W <= 256 else 1)
        eg = R.scaled_ulp_error(grad, rg, gmag)
        print(f"ce {H}x{W} C={C} ld={ld} {name}: loss {el:.2f} of {bl:.2f} ulp, gradient {eg.max():.2f} of {bg:.2f} ulp")
        assert np.isfinite(grad).all() and eg.max() <= bg, (name, int(eg.argmax()), float(eg.max()), bg)
        skipped = ~((np.asarray(label if label is not None else np.full(H * W, const)) >= 0)
                    & (np.asarray(label if label is not None else np.full(H * W, const)) < C))
        assert not (grad[skipped].view(np.int32) & 0x7FFFFFFF).any(), f"{name}: a skipped pixel has a gradient"


# ---- sgan_softmax_fwd / _bwd --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,ld", R.CE_PAIRS)
@pytest.mark.parametrize("H,W", R.CE_SHAPES)
def test_softmax(ops, H, W, C, ld):
    """Forward into a pld = ld buffer; backward from a dp of another pixel stride into dzld = ld.  363 x 362 = 131 406 pixels: 514
    workgroups, under the 2048 cap, as large as the trainers' maps get."""
    z, _, _ = R.ce_inputs(H, W, C, ld, 100 + C)
    zd = _src(z[:, :C], ld).view(H, W, ld)
    p = Out(H, W, ld)
    ops.softmax_fwd(zd, C, p.t)
    got = p.read(C)
    ref = R.softmax_ref(z, C)
    bf = R.budget(K.f32_softmax(z, C), ref)
    ef = R.scaled_ulp_error(got, ref)
    assert np.isfinite(got).all() and ef.max() <= bf, (int(ef.argmax()), float(ef.max()), bf)
    assert np.abs(got.astype(np.float64).sum(1) - 1.0).max() <= (C + bf) * 2 * U
    dp, p32 = K.softmax_bwd_inputs(z, C, 200 + C)
    dz = Out(H, W, ld)
    ops.softmax_bwd(_src(dp, C + 3).view(H, W, C + 3), _src(p32, ld).view(H, W, ld), C, dz.t)
    gb = dz.read(C)
    rb, mag = R.softmax_bwd_ref(dp, p32, C)
    bb = R.budget(K.f32_softmax_bwd(dp, p32, C), rb, mag)
    eb = R.scaled_ulp_error(gb, rb, mag)
    print(f"softmax {H}x{W} C={C} ld={ld}: forward {ef.max():.2f} of {bf:.2f} ulp, backward {eb.max():.2f} of {bb:.2f} ulp")
    assert np.isfinite(gb).all() and eb.max() <= bb, (int(eb.argmax()), float(eb.max()), bb)


# ---- the wrappers in front of the kernels -------------------------------------------------------------------------------------
def _last_kernel():
    from supervised_gan_amd import _lib
    return _lib.lib().sgan_last_kernel().decode()


def test_label_maps_of_other_integer_types(ops):
    """A uint8 and an int32 label map give the int64 result bit for bit (the kernel reads int64: they are converted), loss and
    gradient; the call ends in sg_ce_fwd_kernel."""
    from supervised_gan_amd.losses import cross_entropy_logits
    Cn, H, W = 5, 13, 17
    z, lab, cw = R.ce_inputs(H, W, Cn, Cn, 11)
    lab = np.where((lab >= 0) & (lab < Cn), lab, 2).reshape(1, H, W)
    zt = _dev(np.ascontiguousarray(z.reshape(H, W, Cn).transpose(2, 0, 1)[None]))
    res = {}
    for dt in (torch.int64, torch.uint8, torch.int32):
        zc = zt.clone().requires_grad_(True)
        loss = cross_entropy_logits(zc, _dev(lab).to(dt), 0, _dev(cw))
        assert _last_kernel() == "sg_ce_fwd_kernel"
        loss.backward()
        res[dt] = (_bits(loss), _bits(zc.grad))
    ref = R.ce_ref(z, Cn, lab.reshape(-1), 0, cw)
    assert abs(float(np.frombuffer(res[torch.int64][0].tobytes(), np.float32)[0]) - ref[0]) <= 1e-5 * ref[0]
    for dt in (torch.uint8, torch.int32):
        assert np.array_equal(res[dt][0], res[torch.int64][0]) and np.array_equal(res[dt][1], res[torch.int64][1]), dt


def test_label_map_on_another_device_raises(ops):
    from supervised_gan_amd.losses import cross_entropy_logits
    z = torch.zeros(1, 3, 4, 4, device="cuda")
    with pytest.raises(ValueError):
        cross_entropy_logits(z, torch.zeros(1, 4, 4, dtype=torch.int64), 0, None)


def test_fallbacks_outside_the_envelope_equal_torch(ops):
    """Batch 2, C = 17, fp64 logits, CPU logits: F.cross_entropy(weight=, ignore_index=-100) and F.softmax themselves; inside the
    envelope the same calls end in the HIP kernels."""
    from supervised_gan_amd import _lib
    from supervised_gan_amd.losses import cross_entropy_logits, softmax_channels
    g = torch.Generator().manual_seed(5)
    cases = {"batch": (torch.randn(2, 3, 6, 5, generator=g).cuda(), 3), "C17": (torch.randn(1, 17, 6, 5, generator=g).cuda(), 17),
             "fp64": (torch.randn(1, 3, 6, 5, generator=g, dtype=torch.float64).cuda(), 3), "cpu": (torch.randn(1, 3, 6, 5, generator=g), 3)}
    for name, (z, Cn) in cases.items():
        lab = torch.randint(0, Cn, (z.shape[0], 6, 5), generator=g, dtype=torch.int32)
        lab[:, 0, :2] = -100
        lab[:, 1, 0], lab[:, 1, 1] = Cn, -1                 # skipped like -100 on this path too: F.cross_entropy itself would raise
        ref_lab = torch.where((lab < 0) | (lab >= Cn), torch.full_like(lab, -100), lab).long().to(z.device)
        lab = lab.to(z.device)
        cw = (torch.rand(Cn, generator=g) + 0.5).to(z.device)
        before = _last_kernel()
        zc = z.clone().requires_grad_(True)
        loss = cross_entropy_logits(zc, lab, 0, cw)
        zr = z.clone().requires_grad_(True)
        ref = F.cross_entropy(zr, ref_lab, weight=cw.to(z.dtype), ignore_index=-100)
        loss.backward()
        ref.backward()
        # torch's own 2-d NLL forward adds with atomics on the device: the loss to an fp32 rounding or two, the gradient exactly
        assert torch.allclose(loss, ref, rtol=4 * U, atol=0) and torch.equal(zc.grad, zr.grad), name
        const = cross_entropy_logits(z, None, Cn - 1)
        assert torch.allclose(const, F.cross_entropy(z, torch.full((z.shape[0], 6, 5), Cn - 1, dtype=torch.int64, device=z.device)), rtol=4 * U, atol=0), name
        zi = z.clone().requires_grad_(True)
        none = cross_entropy_logits(zi, None, Cn)             # every pixel skipped: 0 and an all-zero gradient, as on the kernel path
        none.backward()
        assert float(none) == 0.0 and not bool(zi.grad.any()), name
        assert torch.equal(softmax_channels(z), F.softmax(z, dim=1)), name
        assert _last_kernel() == before, name
    z = torch.randn(1, 3, 6, 5, generator=g).cuda()
    softmax_channels(z)
    assert _last_kernel() == "sg_softmax_fwd_kernel"
    cross_entropy_logits(z, None, 2)
    assert _last_kernel() == "sg_ce_fwd_kernel"


def test_gan_loss_fwd_refuses_a_p_out_of_another_stride(ops):
    """The kernel writes p_out[i * ld] with the logits' ld: a tight p_out beside ld = 4 logits would be written out of bounds.  The
    wrapper raises before anything is launched: the loss keeps its sentinel."""
    x = R.gan_logits(5, 7, 1)
    lg, loss = _map(x, 4), _scalar()
    tight = Out(5, 7, 1)
    for bad in (tight.t, torch.zeros(5, 7, 4, dtype=torch.float64, device="cuda"), Out(7, 5, 4).t):
        with pytest.raises(AssertionError):
            ops.gan_loss_fwd(lg, 1.0, 0, loss, bad)
    torch.cuda.synchronize()
    assert int(_bits(loss)[0]) == SENT and (_bits(tight.flat) == SENT).all()

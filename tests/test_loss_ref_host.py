"""tests/loss_ref.py against torch's double autograd on the CPU -- F.binary_cross_entropy(torch.sigmoid(x), t), F.mse_loss,
F.cross_entropy(weight=, ignore_index=-100), F.softmax, the oracle's weighted_l1 -- to 1e-12 where no clamp engages, and the
properties of the input sets that tests/test_hip_loss_kernels.py relies on: every BCE interval contains torch's CPU fp32 result of
the kernels' expression, element by element, for every input set used on the device; the reference's own interval of a summed loss
stays inside GAN_MAX_HALF_WIDTH; the budgets measured on the reference side stay small.  No GPU, no library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases as K
import loss_ref as R
import sgan_oracle as O

TOL = 1e-12


def _close(a, b, tol=TOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool((np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))).all())


def _td(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


@pytest.mark.parametrize("target", R.GAN_TARGETS)
def test_gan_term_formulas_against_double_autograd(target):
    """The two formulas loss_ref evaluates at its candidates, at p = the float64 sigmoid itself: |x| < 20 keeps p (1 - p) above
    1e-12 and both logs above -100."""
    x = R.gan_logits(19, 21, 1).astype(np.float64)
    assert np.abs(x).max() < 20
    xd = _td(x).requires_grad_(True)
    t = R.f32(target)
    ref = F.binary_cross_entropy(torch.sigmoid(xd), torch.full_like(xd, t))
    ref.backward()
    p = R.sigmoid64(x)
    assert _close(R.bce_term(p, t).mean(), ref.item())
    assert _close(R.bce_dterm(p, t) * (p * (1 - p)) * 0.37 / x.size, 0.37 * xd.grad.numpy(), 1e-12)
    xm = _td(x).requires_grad_(True)
    F.mse_loss(xm, torch.full_like(xm, t)).backward()
    lo, hi = R.gan_loss_elem(x.astype(np.float32), target, 1)
    assert lo is hi and _close(lo.mean(), F.mse_loss(_td(x), torch.full_like(xm, t)).item())
    glo, ghi = R.gan_grad_elem(x.astype(np.float32), target, 1, 0.37 / x.size)
    assert glo is ghi and _close(glo, 0.37 * xm.grad.numpy())


def test_clamps_are_torchs():
    """p = 0 and p = 1: the -100 clamp of the logs; p (1 - p) < 1e-12: the clamp of the gradient's denominator (torch's own, as an
    fp32 constant: R.CLAMP is within 5e-9 of 1e-12)."""
    p = torch.tensor([0.0, 1.0, 1e-14, 1.0 - 1e-14], dtype=torch.float64, requires_grad=True)
    for t in (0.0, 1.0, 0.9):
        tt = torch.full_like(p, t)
        ref = F.binary_cross_entropy(p, tt, reduction="none")
        g, = torch.autograd.grad(ref.sum(), p)
        assert _close(R.bce_term(p.detach().numpy(), t), ref.detach().numpy())
        assert _close(R.bce_dterm(p.detach().numpy(), t), g.numpy(), 1e-8)
    assert abs(R.CLAMP - 1e-12) < 5e-21


def test_interval_contains_the_cpu_fp32_result_on_every_gan_input_set():
    for h, w, seed in K.random_gan_maps():
        x = R.gan_logits(h, w, seed)
        for target in R.GAN_TARGETS:
            assert R.gan_half_width(x, target) <= R.GAN_MAX_HALF_WIDTH, (h, w, seed, target)
            for weight in (1.0, -0.6):
                scale = R.f32(weight) / x.size
                l32, d32 = K.f32_gan_elem(x, target, scale)
                assert R.inside(l32, *R.gan_loss_elem(x, target, 0)).all(), (h, w, seed, target)
                assert R.inside(d32, *R.gan_grad_elem(x, target, 0, scale)).all(), (h, w, seed, target, weight)
    x = np.array(R.GAN_PLANTED, dtype=np.float32)
    for target in R.GAN_TARGETS:
        l32, d32 = K.f32_gan_elem(x, target, 2.0)
        lo, hi = R.gan_loss_elem(x, target, 0)
        assert np.isfinite(lo).all() and np.isfinite(hi).all() and R.inside(l32, lo, hi).all(), target
        assert R.inside(d32, *R.gan_grad_elem(x, target, 0, 2.0)).all(), target
        if target in (0.0, 1.0):
            assert hi.max() <= 100.0 * (1 + 4 * R.U) + 1e-30


def test_planted_logits_are_where_the_issue_says():
    """|x| >= 30: p32 is exactly 0 or 1, or a tiny number whose candidates all give the same clamped or well-conditioned value, so the
    loss interval of the saturated side is narrow; x = -30, t = 1: the gradient has decayed below the unclamped p - t."""
    for x in R.GAN_PLANTED:
        p32 = np.float32(R.sigmoid64(x))
        if x >= 30:
            assert p32 == 1.0
        if x <= -104:
            assert p32 == 0.0
        if x in (-30.0, -40.0):
            lo, hi = R.gan_loss_elem(np.float32(x), 1.0, 0)
            assert hi - lo <= 1e-5 * hi, x
    p = float(R.sigmoid64(-30.0))
    glo, ghi = R.gan_grad_elem(np.float32(-30.0), 1.0, 0, 1.0)
    decayed = -p * (1 - p) / R.CLAMP
    assert glo <= decayed <= ghi and abs(decayed) < 0.1 and ghi - glo < 1e-5 * abs(decayed)


@pytest.mark.parametrize("shape", [(10, 10), (1, 255), (1, 257), (257, 256)])       # every image set of the device test
@pytest.mark.parametrize("C,ld", [(2, 4), (3, 3)])
def test_image_losses_against_double(shape, C, ld):
    H, W = shape
    x, y, a, wts, wmap = R.image_inputs(H, W, C, ld, 7 + H + W)
    xd = _td(x[:, :C]).requires_grad_(True)
    yd = _td(y[:, :C])
    for aa, nw in ((a, 3), (wmap, 0), (None, 0)):
        if aa is None:
            wd = None
        elif nw:
            wd = 1.0 + sum((_td(a[:, i: i + 1]) + 1.0) * 0.5 * (float(wts[i]) - 1.0) for i in range(3))
        else:
            wd = _td(wmap)
        xd.grad = None
        ref = 10.0 * O.weighted_l1(xd, yd, wd)
        ref.backward()
        loss, grad, lb, gb = R.l1w_ref(x, y, C, aa, wts, nw, 10.0)
        assert _close(loss, ref.item()) and _close(grad, xd.grad.numpy())
        assert grad[H * W - 1, 0] == 0.0 and lb < 1e-5 * abs(loss) and gb.max() < 1e-5 * np.abs(grad).max()
    # BCE on the rescaled maps: the interval contains the double result, and torch's fp32 evaluation element by element
    xd.grad = None
    ref = F.binary_cross_entropy((xd + 1.0) * 0.5, (yd + 1.0) * 0.5)
    ref.backward()
    (llo, lhi), (glo, ghi) = R.bce01_ref(x, y, C)
    assert llo <= ref.item() <= lhi and lhi - llo <= 1e-4 * lhi
    g = xd.grad.numpy()
    p64 = (x[:, :C].astype(np.float64) + 1.0) * 0.5
    # t' is the fp32 value of (t + 1) / 2, torch's double is not (one rounding of t' through the quotient); the clamp is 1e-12f
    tol = R.U * 0.5 / x[:, :C].size / np.maximum(p64 * (1 - p64), R.CLAMP) + 1e-8 * np.abs(g) + 1e-30
    assert ((g >= glo - tol) & (g <= ghi + tol)).all()
    l32, g32 = K.f32_bce01_elem(x, y, C)
    assert R.inside(g32, glo, ghi).all()
    p = R.p_candidates((x[:, :C].astype(np.float64) + 1.0) * 0.5, True)
    tg = ((y[:, :C] + np.float32(1.0)) * np.float32(0.5)).astype(np.float64)
    v = R.bce_term(p, tg)
    assert R.inside(l32, *R.widen(v.min(0), v.max(0))).all()
    planted = (x[:, :C] == 1.0) | (x[:, :C] == -1.0)
    assert planted.sum() >= 2 and (p.min(0)[planted] == p.max(0)[planted]).all()      # p exactly 0 or 1: the interval is a point
    # why only those are points: an element whose (x + 1) / 2 is exact otherwise carries up to six roundings in its gradient, and
    # torch's fp32 evaluation leaves a point widened by four of them -- on the 257 x 256 set with two channels
    p64 = (x[:, :C].astype(np.float64) + 1.0) * 0.5
    point = R.bce_dterm(p64, tg) * 0.5 / p64.size
    exact = (p64.astype(np.float32).astype(np.float64) == p64) & ~planted & (point != 0.0)
    off = np.abs(g32 - point)[exact] / (R.U * np.abs(point[exact]))
    print(f"bce01 {H}x{W} C={C}: {int(exact.sum())} exact maps, the fp32 gradient up to {off.max():.2f} roundings off its point")
    assert off.max() <= 6.0 and ((H, W, C) != (257, 256, 2) or off.max() > 4.0)


def test_bce01_point_formula_on_exact_maps():
    """x, t multiples of 2^-10: both maps are exact in fp32, and the formulas at the first candidate row, p32 itself, must be torch's
    double result to 1e-12 (p (1 - p) >= 2^-11 there, far above the clamp)."""
    rng = np.random.default_rng(3)
    x = (rng.integers(-1023, 1024, size=(50, 2)) / 1024.0).astype(np.float32)
    t = (rng.integers(-1024, 1025, size=(50, 2)) / 1024.0).astype(np.float32)
    xd = _td(x).requires_grad_(True)
    ref = F.binary_cross_entropy((xd + 1.0) * 0.5, (_td(t) + 1.0) * 0.5)
    ref.backward()
    p = R.p_candidates((x.astype(np.float64) + 1.0) * 0.5, True)
    assert np.array_equal(p[0], (x.astype(np.float64) + 1.0) * 0.5)
    tg = (t.astype(np.float64) + 1.0) * 0.5
    assert _close(R.bce_term(p[0], tg).mean(), ref.item())
    assert _close(R.bce_dterm(p[0], tg) * 0.5 / x.size, xd.grad.numpy())


@pytest.mark.parametrize("C,ld", R.CE_PAIRS)
def test_ce_and_softmax_against_double_autograd(C, ld):
    H, W = 10, 20
    z, lab, cw = R.ce_inputs(H, W, C, ld, 100 + C)
    torch_lab = np.where((lab >= 0) & (lab < C), lab, -100)          # torch raises for anything out of range but its ignore_index
    assert (torch_lab != lab).sum() >= 6
    for label, const, w in ((lab, 0, cw), (lab, 0, None), (None, 0, cw), (None, C - 1, None)):
        zd = _td(z[:, :C]).requires_grad_(True)
        tl = torch.from_numpy(torch_lab if label is not None else np.full(H * W, const, dtype=np.int64))
        ref = F.cross_entropy(zd, tl, weight=_td(w) if w is not None else None, ignore_index=-100)
        (ref * R.f32(0.37)).backward()
        loss, grad, den, lmag, gmag = R.ce_ref(z, C, label, const, w, 0.37)
        assert _close(loss, ref.item()) and _close(grad, zd.grad.numpy())
        want_den = float(_td(w)[tl[tl >= 0]].sum()) if w is not None else float((tl >= 0).sum())
        assert _close(den, want_den) and lmag >= abs(loss) and (gmag >= np.abs(grad) - 1e-18).all()
        l32, g32 = K.f32_ce(z, C, label, const, w, 0.37)
        bl, bg = R.budget(l32, loss, lmag), R.budget(g32, grad, gmag)
        print(f"ce C={C} {'map' if label is not None else 'const'} {'w' if w is not None else 'u'}: loss budget {bl:.2f}, grad budget {bg:.2f} ulp")
        assert bl <= 16.0 and bg <= 64.0
    ignored = np.full(H * W, -100, dtype=np.int64)
    ignored[::3] = R.BIG_LABELS[0]
    loss, grad, den, _, _ = R.ce_ref(z, C, ignored, 0, cw)
    assert loss == 0.0 and den == 0.0 and not grad.any()
    # softmax and its backward
    zd = _td(z[:, :C]).requires_grad_(True)
    p = F.softmax(zd, dim=1)
    dp, p32 = K.softmax_bwd_inputs(z, C, 200 + C)
    (p * _td(dp)).sum().backward()
    assert _close(R.softmax_ref(z, C), p.detach().numpy())
    dz, mag = R.softmax_bwd_ref(dp, p.detach().numpy(), C)
    assert _close(dz, zd.grad.numpy()) and (mag >= np.abs(dz) - 1e-18).all()
    ref_p = R.softmax_ref(z, C)
    dz32, mag32 = R.softmax_bwd_ref(dp, p32, C)
    bf, bb = R.budget(K.f32_softmax(z, C), ref_p), R.budget(K.f32_softmax_bwd(dp, p32, C), dz32, mag32)
    print(f"softmax C={C}: forward budget {bf:.2f}, backward budget {bb:.2f} ulp")
    assert bf <= 64.0 and bb <= 16.0


def test_slot_map_and_mean_interval():
    """Element i of a term goes to slot (i mod 4096) // 256; a mean's interval is the mean of the intervals, one rounding wider."""
    s = R.gan_slot_of(16510)
    assert s[0] == 0 and s[255] == 0 and s[256] == 1 and s[4095] == 15 and s[4096] == 0 and s[16384] == 0 and s[16509] == 0
    lo, hi = np.arange(10.0), np.arange(10.0) + 1
    a, b = R.mean_interval(lo, hi)
    assert a < 4.5 < 5.5 < b and 4.5 - a < 1e-6 and b - 5.5 < 1e-6
    tl, th = R.weighted_total_interval([1.0, 2.0], [1.5, 2.5], [1.0, -1.0])
    assert tl < -1.5 < -0.5 < th and -1.5 - tl < 1e-6

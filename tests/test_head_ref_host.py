"""The head and factored-loss references of tests/loss_ref.py against torch's double autograd on the CPU, to 1e-12, at every shape and
mode tests/test_hip_head_kernels.py uses -- F.softmax + F.cross_entropy(weight=) (times w_p / sum w_p for the pixel-weighted form),
torch.sigmoid + the weight-map loop + F.binary_cross_entropy(weight=), and sigmoid -> F.interpolate(bilinear) -> F.pad(reflect) ->
product -> BCE / MSE -- and the conditions the reference alone must meet so that an interval cannot hide a wrong kernel: on every
random map the half-width of the summed loss stays inside GAN_MAX_HALF_WIDTH and at most GRAD_MAX_WIDE_SHARE of the gradient
elements have an interval wider than 1e-3 of its larger endpoint; every interval contains torch's CPU fp32 result of the kernels'
expression.  No GPU, no library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases as K
import loss_ref as R

TOL = 1e-12


def _close(a, b, tol=TOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool((np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))).all())


def _td(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def _unique_head_maps():
    seen = []
    for H, W, C, _ in K.head_shapes():
        if (H, W, C) not in seen:
            seen.append((H, W, C))
    return seen


@pytest.mark.parametrize("H,W,C", _unique_head_maps())
def test_softmax_head_against_double_autograd(H, W, C):
    z, lab, _, _, cw, add = R.head_inputs(H, W, C, K.head_seed(H, W, C))
    ok = (lab >= 0) & (lab < C)
    assert (~ok).sum() >= 8
    tl = torch.from_numpy(np.where(ok, lab, -100))
    for w, pa in ((None, None), (cw, None), (None, add), (cw, add)):
        zd = _td(z).requires_grad_(True)
        wv = (_td(w) if w is not None else torch.ones(C, dtype=torch.float64))[tl.clamp(min=0)] + (_td(pa) if pa is not None else 0.0)
        wv = torch.where(tl >= 0, wv, torch.zeros_like(wv))
        ref = (F.cross_entropy(zd, tl, reduction="none") * wv).sum() / wv.sum()
        (ref * R.f32(K.HEAD_GOUT)).backward()
        loss, grad, den, lmag, gmag = R.ce_ref(z, C, lab, 0, w, K.HEAD_GOUT, pixel_add=pa)
        assert _close(loss, ref.item()) and _close(grad, zd.grad.numpy()) and _close(den, float(wv.sum()))
        s, bound = R.weight_sum_ref(C, lab, w, pa)
        assert _close(s, den) and bound <= 1e-5 * s
        assert not grad[~ok].any()
        if pa is None:          # and that is F.cross_entropy(weight=) itself
            assert _close(loss, F.cross_entropy(_td(z), tl, weight=_td(w) if w is not None else None).item())
        l32, g32 = K.f32_ce(z, C, lab, 0, w, K.HEAD_GOUT, pa)
        bl, bg = R.budget(l32, loss, lmag), R.budget(g32, grad, gmag)
        print(f"softmax head {H}x{W} C={C} {'w' if w is not None else 'u'}{'+pw' if pa is not None else ''}: loss budget {bl:.2f}, gradient budget {bg:.2f} ulp")
        assert bl <= 16.0 and bg <= 96.0
    assert _close(R.softmax_ref(z, C), F.softmax(_td(z), dim=1).numpy())
    loss, grad, den, _, _ = R.ce_ref(z, C, np.full(H * W, -100), 0, cw, pixel_add=add)
    assert loss == 0.0 and den == 0.0 and not grad.any() and R.weight_sum_ref(C, np.full(H * W, -100), cw, add)[0] == 0.0


def _sigmoid_case(z, t, C, cw, nw, gout, what, random_map=True):
    """bcew_point at the float64 sigmoid against double autograd, both gradients; the intervals against torch's fp32 evaluation."""
    zd = _td(z).requires_grad_(True)
    p = torch.sigmoid(zd)
    p.retain_grad()
    tt = _td(t)
    wm = None
    if nw:
        wm = torch.ones_like(tt[:, :1])
        for i in range(nw):
            wm = wm + tt[:, i: i + 1] * (float(cw[i]) - 1.0)
    ref = F.binary_cross_entropy(p, tt[:, :C], weight=wm)
    (ref * R.f32(gout)).backward()
    p64 = R.sigmoid64(z)
    for chain, want in ((True, zd.grad.numpy()), (False, p.grad.numpy())):
        loss, g = R.bcew_point(p64, t, C, cw, nw, gout, chain)
        assert _close(loss, ref.item()) and _close(g, want), what
        (llo, lhi), (glo, ghi) = R.bcew_ref(p64, t, C, cw, nw, gout, chain)
        assert llo <= loss <= lhi and R.inside(g, glo, ghi).all(), what
        t32, g32 = K.f32_bcew(p64.astype(np.float32), t, C, cw, nw, gout, chain)
        assert R.inside(g32, glo, ghi).all(), (what, chain)
        assert llo <= t32.astype(np.float64).mean() <= lhi, (what, chain)
        if random_map:
            hw, share = R.half_width(llo, lhi), R.wide_share(glo, ghi)
            assert hw <= R.GAN_MAX_HALF_WIDTH and share <= R.GRAD_MAX_WIDE_SHARE, (what, chain, hw, share)
    return hw, share


@pytest.mark.parametrize("H,W,C", _unique_head_maps())
def test_sigmoid_head_against_double_autograd(H, W, C):
    z, _, hot, soft, cw, _ = R.head_inputs(H, W, C, K.head_seed(H, W, C))
    worst = (0.0, 0.0)
    for nw in ("0", "2", "C"):
        for t in (hot, soft):
            r = _sigmoid_case(z, t, C, cw, K.nw_of(nw, C), K.HEAD_GOUT, (H, W, C, nw))
            worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print(f"sigmoid head {H}x{W} C={C}: loss half-width {worst[0]:.2e}, wide gradient intervals {worst[1]:.2e} of the elements")


@pytest.mark.parametrize("npix", [16383, 16384, 16385, 130 * 127, K.BCEW_BWD_CAP_NPIX, K.SIGMOID_CAP_NPIX])
def test_weighted_bce_pieces_against_double_autograd(npix):
    pairs = K.BCEW_PAIRS if npix < 10 ** 5 else K.BCEW_PAIRS[:1]
    for C, _, _, _ in pairs:
        z, _, hot, soft, cw, _ = R.head_inputs(1, npix, C, K.head_seed(1, npix, C))
        for nw in ("0", "1", "C"):
            for gout in (1.0, -2.5):
                _sigmoid_case(z, soft if nw == "1" else hot, C, cw, K.nw_of(nw, C), gout, (npix, C, nw, gout))


@pytest.mark.parametrize("t", [0.0, 1.0, 0.9])
def test_planted_logits_of_the_sigmoid_head(t):
    """+-17 .. +-120: no cap on the widths; every interval is finite and contains torch's fp32 result, the loss stays <= 100 w."""
    z = np.array(R.GAN_PLANTED, dtype=np.float32).reshape(-1, 1)
    tt = np.full_like(z, t)
    cw = np.array([3.0], dtype=np.float32)
    for nw in (0, 1):
        for chain in (True, False):
            (llo, lhi), (glo, ghi) = R.bcew_ref(R.sigmoid64(z), tt, 1, cw, nw, 1.7, chain)
            t32, g32 = K.f32_bcew(K.f32_sigmoid(z).numpy(), tt, 1, cw, nw, 1.7, chain)
            assert np.isfinite([llo, lhi]).all() and np.isfinite(glo).all() and np.isfinite(ghi).all()
            assert R.inside(g32, glo, ghi).all(), (nw, chain, np.nonzero(~R.inside(g32, glo, ghi))[0])
            assert llo <= t32.astype(np.float64).mean() <= lhi


def test_pad_split_and_maps():
    from supervised_gan_amd.losses import factd_pad_split
    for dH in range(8):
        for dW in range(8):
            assert R.factd_pad_split(dH, dW) == factd_pad_split(dH, dW)
    x = np.random.default_rng(0).standard_normal((3, 5))
    My, Mx = R.factd_maps(3, 5, 2, 9, 13)
    want = F.pad(F.interpolate(_td(x)[None, None], scale_factor=2, mode="bilinear", align_corners=False), R.factd_pad_split(3, 3), mode="reflect")
    assert _close(My @ x @ Mx.T, want[0, 0].numpy())
    assert _close(My.sum(1), 1.0) and _close(Mx.sum(1), 1.0)


@pytest.mark.parametrize("mode", R.FACTD_MODES, ids=["sig_sig_bce", "raw_raw_mse", "sig_raw_mse", "raw_sig_mse"])
@pytest.mark.parametrize("shape", R.FACTD_SHAPES, ids=lambda s: "%dx%d_up%d_%dx%d" % s)
def test_factored_term_against_double_autograd(shape, mode):
    """The explicit adjoint My^T G Mx is torch's autograd through interpolate and pad; in BCE mode the intervals contain torch's fp32
    result element by element and meet the two width conditions; in MSE mode the budgets are printed."""
    for target, weight, gout in ((0.0, 0.7, 1.0), (1.0, -0.6, 2.5)):
        l1, l2, ref, c32 = K.factd_reference(shape, mode, target, weight, gout, 100 + shape[0] * shape[3])
        c64 = K.factd_composition([l1], [l2], [shape[2]], [target], [weight], mode, torch.float64, gout)
        assert _close(ref["each"], c64[0][0]) and _close(ref["dl1"], c64[2][0]) and _close(ref["dl2"], c64[3][0]), (shape, mode, target)
        assert _close(ref["p"], c64[4][0]) and _close(ref["q"], c64[5][0])
        assert (ref["dl1_mag"] >= np.abs(ref["dl1"]) * (1 - 1e-12)).all() and (ref["dl2_mag"] >= np.abs(ref["dl2"]) * (1 - 1e-12)).all()
        if not mode[2]:
            lo, hi = ref["each_iv"]
            assert lo <= ref["each"] <= hi and lo <= c32[0][0] <= hi
            hw = R.half_width(lo, hi)
            for name, got in (("dl1", c32[2][0]), ("dl2", c32[3][0])):
                glo, ghi = ref[name + "_iv"]
                assert R.inside(ref[name], glo, ghi).all() and R.inside(got, glo, ghi).all(), (shape, target, name)
            s1, s2 = R.wide_share(*ref["dl1_iv"]), R.wide_share(*ref["dl2_iv"])
            print(f"factd {shape} t={target}: kp {ref['kp']}, kq {ref['kq']}, half-width {hw:.2e}, wide dl1 {s1:.2e}, dl2 {s2:.2e}")
            assert hw <= R.GAN_MAX_HALF_WIDTH and s1 <= R.GRAD_MAX_WIDE_SHARE and s2 <= R.GRAD_MAX_WIDE_SHARE, (shape, target, hw, s1, s2)
        else:
            be = R.budget(c32[0][0], ref["each"], ref["each_mag"])
            b1, b2 = R.budget(c32[2][0], ref["dl1"], ref["dl1_mag"]), R.budget(c32[3][0], ref["dl2"], ref["dl2_mag"])
            print(f"factd {shape} {mode} t={target}: budgets each {be:.2f}, dl1 {b1:.2f}, dl2 {b2:.2f} ulp")
            assert np.isfinite([be, b1, b2]).all()

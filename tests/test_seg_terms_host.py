"""CPU tests of the Tversky (soft Dice, focal-Tversky) and focal loss terms: the host yardstick util.seg_terms_ref against torch
float64 autograd of the plain formulas in both head modes over the corner values of (alpha, beta, smooth, power, gamma), its two
classical special cases, and the C ABI's declarations and refusals (which launch nothing, so they run without a device)."""
import itertools
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NPIX, C = 61, 4


def case(mode, seed, absent=None):
    """fp32 logits [NPIX, C] and the label (softmax: a few -100 among them; `absent`: that class never occurs) or soft target."""
    rng = np.random.default_rng(seed)
    z = (3.0 * rng.standard_normal((NPIX, C))).astype(np.float32)
    if mode == 0:
        y = rng.integers(0, C, NPIX)
        if absent is not None:
            y[y == absent] = (absent + 1) % C
        y[[0, 17]] = -100
        return z, y.astype(np.int64)
    t = rng.random((NPIX, C)).astype(np.float32)
    if absent is not None:
        t[:, absent] = 0.0
    return z, t


def plain_losses(zt, lt, mode, classes, a, b, s, E, gamma, wt):
    """(L_T, L_F) of the logits zt [npix, C] by the plain formulas in torch ops of zt's dtype and device; lt: the int64 label
    tensor or the target tensor; wt: the class weight tensor or None; gamma None / classes empty: that term is 0."""
    npix, Cn = zt.shape
    dtype = zt.dtype
    if mode == 0:
        ok = (lt >= 0) & (lt < Cn)
        ys = torch.where(ok, lt, torch.zeros_like(lt))
        p = torch.softmax(zt, dim=1)
        t = F.one_hot(ys, Cn).to(dtype) * ok[:, None]
        valid = ok.to(dtype)
    else:
        t = lt.to(dtype)
        p = torch.sigmoid(zt)
        valid = torch.ones(npix, dtype=dtype, device=zt.device)
    LT = zt.sum() * 0
    for c in classes:
        TP = (p[:, c] * t[:, c] * valid).sum()
        FP = (p[:, c] * (1 - t[:, c]) * valid).sum()
        FN = ((1 - p[:, c]) * t[:, c] * valid).sum()
        D = TP + a * FP + b * FN + s
        if float(D.detach()) == 0.0:
            continue
        u = 1 - (TP + s) / D
        if float(u.detach()) == 0.0:      # the derivative is defined as 0 there (autograd of u^E gives 0 * inf at E < 1)
            continue
        LT = LT + u ** E
    if classes:
        LT = LT / len(classes)
    LF = zt.sum() * 0
    if gamma is not None:
        if wt is None:
            wt = torch.ones(Cn, dtype=dtype, device=zt.device)
        if mode == 0:
            lp = (zt - torch.logsumexp(zt, dim=1, keepdim=True)).gather(1, ys[:, None])[:, 0]
            pt = lp.exp()
            wy = wt[ys] * ok
            if float(wy.sum()) > 0.0:      # no labelled pixel: 0
                LF = (wy * (1 - pt) ** gamma * -lp).sum() / wy.sum()
        else:
            LF = (wt * (t * (1 - p) ** gamma * F.softplus(-zt) + (1 - t) * p ** gamma * F.softplus(zt))).sum() / (Cn * npix)
    return LT, LF


def torch_terms(z, lt, mode, classes, a, b, s, E, gamma, w, dtype=torch.float64):
    """plain_losses with autograd on the CPU: (L_T, L_F, dL_T/dz, dL_F/dz) as Python floats and float64 arrays.  dtype
    torch.float32: the same composition in fp32, whose error against the float64 run is the e_ref of the GPU tests."""
    zt = torch.tensor(z, dtype=dtype, requires_grad=True)
    wt = None if w is None else torch.tensor(np.asarray(w, np.float32), dtype=dtype)
    LT, LF = plain_losses(zt, torch.tensor(lt), mode, list(classes), a, b, s, E, gamma, wt)
    gT = torch.autograd.grad(LT, zt, retain_graph=True)[0].double().numpy()
    gF = torch.autograd.grad(LF, zt)[0].double().numpy()
    return float(LT.detach()), float(LF.detach()), gT, gF


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / (np.max(np.abs(b)) + 1e-12))


@pytest.mark.parametrize("mode", [0, 1])
def test_ref_equals_torch_float64_autograd_over_the_corners(mode):
    from supervised_gan_amd.util import seg_terms_ref
    w = [1.0, 2.5, 0.5, 1.5]
    z, lt = case(mode, 3 + mode)
    for (a, b), s, E, gamma in itertools.product(((0.5, 0.5), (0.3, 0.7), (0.0, 1.0)), (1.0, 0.0), (1.0, 0.75), (0.0, 0.5, 1.0, 2.0)):
        LT, LF, state, dT, dF = seg_terms_ref(z, lt, mode, [0, 2], a, b, s, E, gamma, w)
        rLT, rLF, rT, rF = torch_terms(z, lt, mode, [0, 2], a, b, s, E, gamma, w)
        assert abs(LT - rLT) <= 1e-12 and abs(LF - rLF) <= 1e-12, (a, b, s, E, gamma, LT, rLT, LF, rLF)
        assert rel(dT, rT) <= 1e-10 and rel(dF, rF) <= 1e-10, (a, b, s, E, gamma, rel(dT, rT), rel(dF, rF))
        assert state[66] == LT and state[67] == LF and abs(state[5] + state[13] - 2 * LT) <= 1e-15
        if mode == 0:
            assert not dT[[0, 17]].any() and not dF[[0, 17]].any()      # labels of -100: exactly nothing
        else:
            assert not dT[:, [1, 3]].any()                               # unlisted sigmoid channels: exactly nothing


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("s", [0.0, 1.0])
def test_absent_class(mode, s):
    """A listed class without a pixel: with smooth = 1 it is an ordinary class (TP = FN = 0); with smooth = 0 and alpha = 0 its
    D is exactly 0 and it takes no part: L_c = 0, no gradient, the mean still over n."""
    from supervised_gan_amd.util import seg_terms_ref
    z, lt = case(mode, 11, absent=1)
    LT, _, state, dT, _ = seg_terms_ref(z, lt, mode, [1, 2], 0.0, 1.0, s, 0.75)
    rLT, _, rT, _ = torch_terms(z, lt, mode, [1, 2], 0.0, 1.0, s, 0.75, None, None)
    assert abs(LT - rLT) <= 1e-12 and rel(dT, rT) <= 1e-10
    assert state[0] == 0.0 and state[2] == 0.0      # TP, FN of the absent class
    if s == 0.0:
        assert state[3] == 0.0 and state[5] == 0.0 and state[6] == 0.0 and state[7] == 0.0
        _, _, st1, d1, _ = seg_terms_ref(z, lt, mode, [2], 0.0, 1.0, s, 0.75)
        assert abs(LT - 0.5 * st1[5]) <= 1e-15      # the mean stays over n = 2
        if mode == 1:
            assert not dT[:, 1].any()
    # alpha > 0: the false positives of the absent class give it a D and a gradient
    LT, _, state, dT, _ = seg_terms_ref(z, lt, mode, [1, 2], 0.5, 0.5, s, 1.0)
    rLT, _, rT, _ = torch_terms(z, lt, mode, [1, 2], 0.5, 0.5, s, 1.0, None, None)
    assert state[3] > 0.0 and abs(LT - rLT) <= 1e-12 and rel(dT, rT) <= 1e-10


def test_gamma_zero_is_the_weighted_cross_entropy():
    from supervised_gan_amd.util import seg_terms_ref
    z, y = case(0, 5)
    for w in (None, [1.0, 2.5, 0.5, 1.5]):
        _, LF, _, _, dF = seg_terms_ref(z, y, 0, (), focal_gamma=0.0, class_weights=w)
        zt = torch.tensor(z.astype(np.float64), requires_grad=True)
        ce = F.cross_entropy(zt, torch.tensor(y), weight=None if w is None else torch.tensor(w, dtype=torch.float64))
        ce.backward()
        assert abs(LF - float(ce)) <= 1e-12 and rel(dF, zt.grad.numpy()) <= 1e-12


@pytest.mark.parametrize("mode", [0, 1])
def test_half_half_is_dice(mode):
    from supervised_gan_amd.util import seg_terms_ref
    z, lt = case(mode, 7)
    z64 = z.astype(np.float64)
    if mode == 0:
        ok = lt >= 0
        p = np.exp(z64 - z64.max(1, keepdims=True))
        p = (p / p.sum(1, keepdims=True))[ok]
        t = np.eye(C)[lt[ok]]
    else:
        p, t = 1 / (1 + np.exp(-z64)), lt.astype(np.float64)
    for s in (0.0, 1.0, 3.5):
        # TP + FP / 2 + FN / 2 + smooth = (sum p + sum t) / 2 + smooth: the Dice loss 1 - (2 TP + s) / (sum p + sum t + s) at smooth = s / 2
        LT, _, state, _, _ = seg_terms_ref(z, lt, mode, [0, 1, 3], 0.5, 0.5, s / 2, 1.0)
        dice = [1 - (2 * (p[:, c] * t[:, c]).sum() + s) / (p[:, c].sum() + t[:, c].sum() + s) for c in (0, 1, 3)]
        assert abs(LT - float(np.mean(dice))) <= 1e-12
        assert all(abs(state[8 * j + 5] - dice[j]) <= 1e-12 for j in range(3))


def test_ref_refuses_bad_classes():
    from supervised_gan_amd.util import seg_terms_ref
    z, y = case(0, 1)
    for bad in ([0, 0], [C], [-1], list(range(9))):
        with pytest.raises(AssertionError):
            seg_terms_ref(z, y, 0, bad)


def test_entry_points_are_declared_bound_and_refuse(built_lib):
    import ctypes
    from supervised_gan_amd import _lib, ops
    from supervised_gan_amd.losses import seg_terms
    header = open(os.path.join(ROOT, "include", "sgan_hip.h")).read()
    assert "Segmentation loss terms" in header
    assert re.search(r"\bint\s+sgan_seg_terms_forward\s*\(\s*const float\* logits,", header)
    assert re.search(r"\bint\s+sgan_seg_terms_backward\s*\(\s*const float\* logits,", header)
    for name, val in (("MAX_CLASSES", ops.SEGTERMS_MAX_CLASSES), ("STATE_BYTES", ops.SEGTERMS_STATE_BYTES), ("WS_BYTES", ops.SEGTERMS_WS_BYTES)):
        assert re.search(r"#define SGAN_SEGTERMS_%s %d\b" % (name, val), header), name
    assert ops.SEGTERMS_STATE_BYTES == 8 * 68 and ops.SEGTERMS_WS_BYTES == 8 * ((3 * 8 + 2) * 512 + 1)
    assert [len(_lib.SIGNATURES[n]) for n in ("sgan_seg_terms_forward", "sgan_seg_terms_backward")] == [22, 19]
    assert "sgan_segterms.hip" in open(os.path.join(ROOT, "supervised-gan_amd", "csrc", "Makefile")).read()
    lib = _lib.lib()
    one, nine, big, twice = (ctypes.c_int32 * 1)(0), (ctypes.c_int32 * 9)(*range(9)), (ctypes.c_int32 * 1)(3), (ctypes.c_int32 * 2)(1, 1)
    x = ctypes.c_void_p(64)      # a non-null pointer nothing dereferences: every call below is refused before a launch

    def fwd(C_=3, classes=one, n=1, focal=1, a=0.5, b=0.5, s=1.0, E=1.0, g=2.0, z=x, lt=x, state=x, lo=x, ws=x):
        return lib.sgan_seg_terms_forward(z, 4, 16, C_, 0, lt, 0, classes, n, a, b, s, E, focal, g, None, 0, state, lo, lo, ws, None)

    def bwd(C_=3, classes=one, n=1, focal=1, g=2.0, z=x, lt=x, state=x, dz=x):
        return lib.sgan_seg_terms_backward(z, 4, 16, C_, 0, lt, 0, classes, n, focal, g, None, 0, state, None, None, dz, 4, None)

    for f in (fwd, bwd):
        for kw, why in ((dict(C_=17), b"not covered: 17 channels"), (dict(n=9, classes=nine), b"not covered: 9 listed"),
                        (dict(n=-1), b"not covered"), (dict(n=0, focal=0), b"both terms are off"), (dict(classes=big), b"not below C"),
                        (dict(classes=twice, n=2), b"repeats"), (dict(z=None), b"null"), (dict(lt=None), b"null"), (dict(state=None), b"null"),
                        (dict(g=8.5), b"gamma"), (dict(g=float("nan")), b"gamma")):
            assert f(**kw) == 1 and why in lib.sgan_last_error(), (f.__name__, kw, lib.sgan_last_error())
    for kw, why in ((dict(lo=None), b"null"), (dict(ws=None), b"null"), (dict(a=0.0, b=0.0), b"alpha + beta"), (dict(E=0.0), b"power"),
                    (dict(E=4.5), b"power"), (dict(s=-1.0), b"smooth"), (dict(a=float("nan")), b"alpha")):
        assert fwd(**kw) == 1 and why in lib.sgan_last_error(), (kw, lib.sgan_last_error())
    assert bwd(dz=None) == 1 and b"null" in lib.sgan_last_error()
    # the Python wrapper refuses off the device: there is no fallback
    with pytest.raises(_lib.SganError):
        seg_terms(torch.randn(1, 3, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), 0, [0])

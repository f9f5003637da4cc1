"""GPU tests of the Tversky / focal loss terms on the logits (sgan_segterms.hip) against the fp64 yardstick util.seg_terms_ref and
torch float64 autograd of the plain formulas, all fed the same fp32 inputs.

Pass rule for losses, state and dz, the project's: max|a - b| / (max|b| + 1e-12) <= max(1e-3, 4 e_ref), e_ref the same statistic of the
fp32 torch composition on the CPU (for the state's derived fields, which that composition does not hand out, the floor 1e-3 alone).

The sums TP, FP, FN hold no transcendental beyond p and have a bound counted from roundings (u = 2^-24, one rounding to fp32;
eps = 2^-53, one to fp64).  The device takes p in fp32 and everything after it in fp64, where p t, p (1 - t) are exact and (1 - p) t
costs eps:
  softmax  z - m is one fp32 subtraction: an absolute error u |z - m| of the argument, a relative error S u of the exponential, S the
           largest max - min of a pixel's logits; expf is good to one ulp (2 u); so every e_c is off by at most (S + 2) u.  Their sum
           adds C - 1 roundings, the reciprocal one, the product one: p is off by at most R u p with R = 2 S + C + 8 (numerator and
           denominator, and 3 u of slack for the second order terms).
  sigmoid  expf (2 u), 1 + e (u), the reciprocal (u), doubled for the second order: R = 8.
  Then |TP - TP_ref| <= R u TP, |FP - FP_ref| <= R u FP, and |FN - FN_ref| <= R u TP because 1 - p moves by what p moves by; plus
  the fp64 accumulation of npix non-negative terms on either side, 2 (npix + 2) eps of the sum.  A sum whose yardstick is 0 and
  whose bound is 0 must be exactly 0 on the device.

Where the yardstick's gradient is zero by construction the device's must be exactly 0, from buffers filled with NaN before the call."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_seg_terms_host import rel, torch_terms      # noqa: E402  the plain formulas in torch, float64 or float32

pytestmark = pytest.mark.gpu

# the shapes of test_hip_seg_head.py plus one pixel: 4- and 12-channel rows dense (8 and 16 through the "wide" layouts below), one
# partial workgroup, several workgroups, pixel counts that are no multiple of 256
SHAPES = ((5, 7, 3), (33, 31, 2), (257, 3, 3), (64, 64, 4), (9, 7, 12), (1, 1, 2))
U, EPS = 2.0 ** -24, 2.0 ** -53
SOFTMAX, SIGMOID = 0, 1
# kind -> (alpha, beta, smooth, power, gamma); gamma < 1 only where 1 - pt is never exactly 0 (torch's pow has no derivative there)
KINDS = {"random": (0.3, 0.7, 1.0, 0.75, 0.5), "saturated": (0.5, 0.5, 1.0, 1.0, 2.0), "absent_s0": (0.0, 1.0, 0.0, 0.75, 1.0),
         "absent_s1": (0.5, 0.5, 1.0, 1.0, 2.0), "full": (0.5, 0.5, 1.0, 0.75, 0.0), "ignored": (0.5, 0.5, 1.0, 1.0, 2.0)}
GT, GF = 0.5, 0.25      # the upstream gradients of the two terms


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")


def inputs(H, W, C, mode, kind, seed=0):
    """(z [npix, C] fp32, label [npix] int64 or target [npix, C] fp32, listed classes, class weights).  Class 1 is the absent /
    class 0 the full one; it is listed first."""
    rng = np.random.default_rng(seed + 7 * H + W)
    npix = H * W
    z = (3.0 * rng.standard_normal((npix, C))).astype(np.float32)
    y = rng.integers(0, C, npix)
    if kind == "saturated":      # +-40: softmax and sigmoid reach exactly 1.0 in fp32; every other pixel with the wrong class on top
        z = np.full((npix, C), -40.0, np.float32)
        top = np.where(np.arange(npix) % 2 == 0, y, (y + 1) % C)
        z[np.arange(npix), top] = 40.0
    if kind in ("absent_s0", "absent_s1"):
        y[y == 1] = 0
    if kind == "full":
        y[:] = 0
    if kind == "ignored":      # labels of -100 at the start of every row
        y.reshape(H, W)[:, 0] = -100
    classes = [1, 0] if kind.startswith("absent") else ([0, C - 1] if C > 1 else [0])
    w = (1.0 + np.arange(C) / 2.0).astype(np.float32)
    if mode == SOFTMAX:
        return z, y.astype(np.int64), classes, w
    t = np.eye(C, dtype=np.float32)[np.maximum(y, 0)]
    if kind == "random":      # soft targets
        t = rng.random((npix, C)).astype(np.float32)
    if kind == "ignored":
        t[y < 0] = 0.0
    return z, t, classes, w


def run_device(H, W, z, lt, mode, classes, par, w, layout="dense", gout=(GT, GF)):
    """One forward and one backward from NaN-filled outputs: (L_T, L_F, state [68], dz [npix, C], the padding of dz, the workspace
    after the calls).  layout: "dense" rows of pad4(C); "wide8" / "wide16" dense rows of 8 / 16; "view" logits and target as a window of rows of 32 (the
    scalar form; the gradient stays dense).  gout: the two upstream gradients, None = NULL.  par = (alpha, beta, smooth, power, gamma), gamma None = focal off."""
    from supervised_gan_amd import ops
    dev = torch.device("cuda", 0)
    npix, C = z.shape
    a, b, s, E, gamma = par

    def buf(src, fill, layout=layout):
        if layout == "view":
            base = torch.full((H, W, 32), fill, dtype=torch.float32, device=dev)
            v = base[:, :, 8:8 + C]
        else:
            cs = {"dense": ops.pad4(C), "wide8": 8, "wide16": 16}[layout]
            assert cs >= C
            base = torch.full((H, W, cs), fill, dtype=torch.float32, device=dev)
            v = base
        if src is not None:
            v[:, :, :C] = torch.from_numpy(src).to(dev).view(H, W, C)
        return v

    nan = float("nan")
    zb = buf(z, nan)      # NaN in the padding channels: they are never used
    if mode == SOFTMAX:
        ltb = torch.from_numpy(lt).to(dev)
    else:
        ltb = buf(lt, nan)
    dz = buf(None, nan, "dense" if layout == "view" else layout)      # a written operand owns its whole rows
    state = torch.full((68,), nan, dtype=torch.float64, device=dev)
    lT, lF = torch.full((), nan, device=dev), torch.full((), nan, device=dev)
    work = ops.new_seg_terms_workspace(dev)
    cw = None if w is None else torch.from_numpy(w).to(dev)
    ops.seg_terms_forward(zb, C, mode, ltb, classes, a, b, s, E, gamma, cw, state, lT, lF, work)
    g = [None if x is None else torch.tensor(x, dtype=torch.float32, device=dev) for x in gout]
    ops.seg_terms_backward(zb, C, mode, ltb, classes, gamma, cw, state, g[0], g[1], dz)
    torch.cuda.synchronize()
    pad = dz[:, :, C:]
    return (float(lT), float(lF), state.cpu().numpy(), dz[:, :, :C].reshape(npix, C).cpu().numpy().astype(np.float64),
            pad.cpu().numpy(), work.cpu().numpy())


def judge(name, got, ref64, ref32):
    e, e_ref = rel(got, ref64), rel(ref32, ref64)
    print(f"{name}: kernel vs fp64 {e:.3e}, fp32 composition vs fp64 {e_ref:.3e}")
    assert e <= max(1e-3, 4 * e_ref), (name, e, e_ref)


@pytest.mark.parametrize("mode", [SOFTMAX, SIGMOID])
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_and_exact_zeros(shape, mode):
    _need_gpu()
    from supervised_gan_amd.util import seg_terms_ref
    H, W, C = shape
    npix = H * W
    for kind, par in KINDS.items():
        a, b, s, E, gamma = par
        z, lt, classes, w = inputs(H, W, C, mode, kind)
        n = len(classes)
        LT, LF, state, dz, pad, work = run_device(H, W, z, lt, mode, classes, par, w)
        rLT, rLF, rstate, rT, rF = seg_terms_ref(z, lt, mode, classes, a, b, s, E, gamma, w)
        rdz = GT * rT + GF * rF
        tag = f"{shape} mode {mode} {kind}"
        # the yardstick, then torch float64 autograd, each with the fp32 composition's own error as e_ref
        t64 = torch_terms(z, lt, mode, classes, a, b, s, E, gamma, w)
        t32 = torch_terms(z, lt, mode, classes, a, b, s, E, gamma, w, dtype=torch.float32)
        d64, d32 = GT * t64[2] + GF * t64[3], GT * t32[2] + GF * t32[3]
        assert np.isfinite(d64).all() and np.isfinite(dz).all() and not work.any(), tag
        judge(tag + " L_T vs ref", [LT], [rLT], [t32[0]])
        judge(tag + " L_F vs ref", [LF], [rLF], [t32[1]])
        judge(tag + " L_T vs torch64", [LT], [t64[0]], [t32[0]])
        judge(tag + " L_F vs torch64", [LF], [t64[1]], [t32[1]])
        judge(tag + " dz vs ref", dz, rdz, d32)
        judge(tag + " dz vs torch64", dz, d64, d32)
        # the state: the sums within the counted bound, the derived fields within the rule's floor
        S = float(np.max(z.max(1) - z.min(1))) if mode == SOFTMAX else 0.0
        R = (2 * S + C + 8) if mode == SOFTMAX else 8.0
        for j in range(n):
            TP, FP, FN = rstate[8 * j:8 * j + 3]
            acc = 2 * (npix + 2) * EPS
            for k, (name, bound) in enumerate((("TP", R * U * TP + acc * TP), ("FP", R * U * FP + acc * FP), ("FN", R * U * TP + acc * FN))):
                err = abs(state[8 * j + k] - rstate[8 * j + k])
                print(f"{tag} class {classes[j]} {name}: |device - fp64| {err:.3e}, counted bound {bound:.3e}")
                assert err <= bound, (tag, j, name, err, bound)
            for k, name in ((3, "D"), (4, "TI"), (5, "L_c")):
                assert rel([state[8 * j + k]], [rstate[8 * j + k]]) <= 1e-3, (tag, j, name, state[8 * j + k], rstate[8 * j + k])
            assert rel(state[8 * j + 6:8 * j + 8], rstate[8 * j + 6:8 * j + 8]) <= 1e-3, (tag, j, "G", state[8 * j:8 * j + 8], rstate[8 * j:8 * j + 8])
        assert not state[8 * n:64].any()
        assert rel(state[64:66], rstate[64:66]) <= 1e-3 and rel([state[66]], [rstate[66]]) <= 1e-3 and rel([state[67]], [rstate[67]]) <= 1e-3
        assert abs(state[66] - LT) <= U * abs(state[66]) and abs(state[67] - LF) <= U * abs(state[67])      # one rounding to fp32
        # exact zeros
        assert pad.size == (ops_pad4(C) - C) * npix and not pad.any(), tag      # padding channels: written, as zeros
        if mode == SOFTMAX and kind == "ignored":
            rows = np.arange(npix).reshape(H, W)[:, 0]
            assert not dz[rows].any() and not rdz[rows].any(), tag
        if kind == "absent_s0":
            assert rstate[3] == 0.0 and state[3] == 0.0 and not state[4:8].any(), tag      # D == 0: TI, L_c, G(0), G(1) all 0
            # the Tversky term alone: the D == 0 class moves nothing -- alone it leaves the whole gradient exactly 0
            only = run_device(H, W, z, lt, mode, [1], (a, b, s, E, None), None)
            assert only[0] == 0.0 and only[1] == 0.0 and not only[3].any() and not only[4].any(), tag
        if mode == SIGMOID:
            tv = run_device(H, W, z, lt, mode, classes, (a, b, s, E, None), None)
            unlisted = [c for c in range(C) if c not in classes]
            assert not tv[3][:, unlisted].any(), tag      # unlisted sigmoid channels
            if kind == "absent_s0":
                assert not tv[3][:, 1].any(), tag


def ops_pad4(c):
    return (c + 3) // 4 * 4


@pytest.mark.parametrize("mode", [SOFTMAX, SIGMOID])
def test_null_upstream_and_one_term_at_a_time(mode):
    _need_gpu()
    H, W, C = 33, 31, 2
    par = KINDS["random"]
    a, b, s, E, gamma = par
    z, lt, classes, w = inputs(H, W, C, mode, "random")
    joint = run_device(H, W, z, lt, mode, classes, par, w)
    none = run_device(H, W, z, lt, mode, classes, par, w, gout=(None, None))
    assert not none[3].any() and not none[4].any()      # both NULL: every element exactly 0
    no_t = run_device(H, W, z, lt, mode, classes, par, w, gout=(None, GF))
    no_f = run_device(H, W, z, lt, mode, classes, par, w, gout=(GT, None))
    dice = run_device(H, W, z, lt, mode, classes, (a, b, s, E, None), None, gout=(GT, None))
    focal = run_device(H, W, z, lt, mode, [], par, w, gout=(None, GF))
    # a term left out by a NULL gradient is the call with that term switched off, bit for bit
    assert np.array_equal(no_t[3], focal[3]) and np.array_equal(no_f[3], dice[3])
    assert dice[0] == joint[0] and focal[1] == joint[1] and dice[1] == 0.0 and focal[0] == 0.0
    # the joint call adds the two parts in fp32: within two roundings of the sum (a fused multiply-add may round once less)
    err = np.abs(joint[3] - (dice[3] + focal[3]))
    bound = 2 * U * (np.abs(dice[3]) + np.abs(focal[3])) + 1e-44
    print(f"mode {mode}: max |joint - (dice + focal)| {err.max():.3e}, largest bound {bound.max():.3e}")
    assert (err <= bound).all()


def test_focal_gamma_zero_is_the_seg_head_gradient():
    _need_gpu()
    from supervised_gan_amd import ops
    from supervised_gan_amd.util import seg_terms_ref
    dev = torch.device("cuda", 0)
    for H, W, C in ((64, 64, 4), (33, 31, 2), (9, 7, 12)):
        z, y, _, w = inputs(H, W, C, SOFTMAX, "ignored")
        got = run_device(H, W, z, y, SOFTMAX, [], (0.5, 0.5, 1.0, 1.0, 0.0), w, gout=(None, 1.0))
        zb = torch.zeros((H, W, ops.pad4(C)), device=dev)
        zb[:, :, :C] = torch.from_numpy(z).to(dev).view(H, W, C)
        yb, cw = torch.from_numpy(y).to(dev), torch.from_numpy(w).to(dev)
        norm, loss = torch.zeros((), device=dev), torch.zeros((), device=dev)
        p, dh = torch.empty_like(zb), torch.empty_like(zb)
        ops.label_weight_sum(yb, C, cw, norm)
        assert ops.seg_head(zb, C, ops.SEGHEAD_SOFTMAX, yb, cw, C, norm, p, dh, loss)
        head = dh[:, :, :C].reshape(H * W, C).cpu().numpy().astype(np.float64)
        _, rLF, _, _, rF = seg_terms_ref(z, y, SOFTMAX, (), focal_gamma=0.0, class_weights=w)
        t32 = torch_terms(z, y, SOFTMAX, [], 0.5, 0.5, 1.0, 1.0, 0.0, w, dtype=torch.float32)
        e_ref = rel(t32[3], rF)
        e = rel(got[3], head)
        print(f"{(H, W, C)}: focal(gamma = 0) dz vs sgan_seg_head dz {e:.3e}; fp32 composition vs fp64 {e_ref:.3e}; loss {got[1]:.7g} vs {float(loss):.7g}")
        assert e <= max(1e-3, 4 * e_ref)
        judge(f"{(H, W, C)} loss vs head", [got[1]], [float(loss)], [t32[1]])
        judge(f"{(H, W, C)} dz vs ref", got[3], rF, t32[3])


@pytest.mark.parametrize("mode", [SOFTMAX, SIGMOID])
def test_repeatable_and_layout_independent(mode):
    _need_gpu()
    for H, W, C in ((64, 64, 4), (257, 3, 3), (9, 7, 12), (1, 1, 2)):
        z, lt, classes, w = inputs(H, W, C, mode, "random")
        par = KINDS["random"]
        first = run_device(H, W, z, lt, mode, classes, par, w)
        assert not first[5].any()      # the workspace is all zero again
        layouts = ["dense", "view"] + [l for l, cs in (("wide8", 8), ("wide16", 16)) if cs >= C]
        for layout in layouts:
            again = run_device(H, W, z, lt, mode, classes, par, w, layout=layout)
            assert again[0] == first[0] and again[1] == first[1], (layout, again[:2], first[:2])
            assert np.array_equal(again[2], first[2]) and np.array_equal(again[3], first[3]), layout
            assert not again[4].any() and not again[5].any(), layout


def test_workspace_is_reused_across_calls():
    """One workspace and one state through several forwards of different sizes: each leaves the slots and the ticket at zero."""
    _need_gpu()
    from supervised_gan_amd import ops
    from supervised_gan_amd.util import seg_terms_ref
    dev = torch.device("cuda", 0)
    work, state = ops.new_seg_terms_workspace(dev), ops.new_seg_terms_state(dev)
    lT, lF = torch.zeros((), device=dev), torch.zeros((), device=dev)
    for H, W, C in ((64, 64, 4), (5, 7, 3), (600, 300, 3), (64, 64, 4)):      # 180000 pixels: more workgroups than slots per sum
        z, y, classes, w = inputs(H, W, C, SOFTMAX, "random")
        zb = torch.zeros((H, W, 4), device=dev)
        zb[:, :, :C] = torch.from_numpy(z).to(dev).view(H, W, C)
        ops.seg_terms_forward(zb, C, SOFTMAX, torch.from_numpy(y).to(dev), classes, 0.5, 0.5, 1.0, 1.0, 2.0, None, state, lT, lF, work)
        torch.cuda.synchronize()
        assert not work.cpu().numpy().any()
        rLT, rLF, _, _, _ = seg_terms_ref(z, y, SOFTMAX, classes, 0.5, 0.5, 1.0, 1.0, 2.0)
        assert abs(float(lT) - rLT) <= 1e-5 * abs(rLT) + 1e-7 and abs(float(lF) - rLF) <= 1e-5 * abs(rLF) + 1e-7, (float(lT), rLT, float(lF), rLF)


def test_not_covered_launches_nothing():
    _need_gpu()
    from supervised_gan_amd import _lib, ops
    dev = torch.device("cuda", 0)
    H, W = 8, 8
    nan = float("nan")
    zb = torch.zeros((H, W, 20), device=dev)
    y = torch.zeros(H * W, dtype=torch.int64, device=dev)
    state = torch.full((68,), nan, dtype=torch.float64, device=dev)
    lT, lF = torch.full((), nan, device=dev), torch.full((), nan, device=dev)
    dz = torch.full((H, W, 20), nan, device=dev)
    work = ops.new_seg_terms_workspace(dev)
    one = torch.ones((), device=dev)
    for C, classes, gamma, why in ((17, [0], 2.0, "17 channels"), (3, list(range(9)), 2.0, "9 listed"), (3, [], None, "both terms are off"),
                                   (3, [3], 2.0, "not below C"), (3, [1, 1], None, "repeats"), (3, [0], 9.0, "gamma")):
        with pytest.raises(_lib.SganError, match=why):
            ops.seg_terms_forward(zb, C, SOFTMAX, y, classes, 0.5, 0.5, 1.0, 1.0, gamma, None, state, lT, lF, work)
        assert why.encode() in _lib.lib().sgan_last_error()
        with pytest.raises(_lib.SganError, match=why):
            ops.seg_terms_backward(zb, C, SOFTMAX, y, classes, gamma, None, state, one, one, dz)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    arr = (ctypes.c_int32 * 1)(0)
    lib = _lib.lib()
    assert lib.sgan_seg_terms_forward(P(zb), 20, 64, 3, 0, P(y), 0, arr, 1, 0.5, 0.5, 1.0, 1.0, 1, 2.0, None, 0, P(state), None, P(lF), P(work), None) == 1
    assert b"null" in lib.sgan_last_error()
    assert lib.sgan_seg_terms_backward(P(zb), 20, 64, 3, 0, P(y), 0, arr, 1, 1, 2.0, None, 0, None, P(one), P(one), P(dz), 20, None) == 1
    assert b"null" in lib.sgan_last_error()
    torch.cuda.synchronize()
    # every output is as it was
    assert torch.isnan(state).all() and torch.isnan(lT) and torch.isnan(lF) and torch.isnan(dz).all() and not work.any()


def test_autograd_node():
    """losses.seg_terms: the gradient reaches the logits only, each term's times its own upstream gradient; a term nobody uses is
    left out; the buffers persist."""
    _need_gpu()
    from supervised_gan_amd import ops
    from supervised_gan_amd.losses import SegTermsBuffers, seg_terms
    from supervised_gan_amd.util import seg_terms_ref
    dev = torch.device("cuda", 0)
    H, W, C = 33, 31, 3
    z, y, classes, w = inputs(H, W, C, SOFTMAX, "random")
    bufs = SegTermsBuffers(C, H, W, dev)
    logits = torch.from_numpy(z).to(dev).view(H, W, C).permute(2, 0, 1).unsqueeze(0).contiguous().requires_grad_(True)
    label = torch.from_numpy(y).to(dev).view(1, H, W)
    cw = torch.from_numpy(w).to(dev)
    rLT, rLF, _, rT, rF = seg_terms_ref(z, y, SOFTMAX, classes, 0.3, 0.7, 1.0, 0.75, 2.0, w)
    to_np = lambda g: g[0].permute(1, 2, 0).reshape(H * W, C).cpu().numpy().astype(np.float64)      # noqa: E731
    for lam_t, lam_f in ((0.5, 0.25), (0.5, 0.0), (0.0, 2.0)):
        logits.grad = None
        LT, LF = seg_terms(logits, label, ops.SEGHEAD_SOFTMAX, classes, 0.3, 0.7, 1.0, 0.75, 2.0, cw, buffers=bufs)
        assert LT.data_ptr() == bufs.loss_t.data_ptr() and LF.data_ptr() == bufs.loss_f.data_ptr()
        loss = (lam_t * LT if lam_t else 0) + (lam_f * LF if lam_f else 0)
        loss.backward()
        assert abs(float(LT.detach()) - rLT) <= 1e-5 and abs(float(LF.detach()) - rLF) <= 1e-5
        want = lam_t * rT + lam_f * rF
        assert rel(to_np(logits.grad), want) <= 1e-3, (lam_t, lam_f, rel(to_np(logits.grad), want))
    with pytest.raises(Exception):
        seg_terms(logits, label, ops.SEGHEAD_SOFTMAX, (), focal_gamma=None, buffers=bufs)      # both terms off

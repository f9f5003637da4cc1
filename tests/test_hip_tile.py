"""GPU tests of the kernels of whole-image inference (csrc/sgan_tile.hip) against the host yardsticks of util.py.

image_prep_tile: bit-equal to ops.image_prep for windows inside the image and to util.prep_tile_ref for windows that reach outside.

tile_blend + tile_finish against util.blend_tiles_ref (float64).  Per pixel, with n passes reaching it with a non-zero weight and
u = 2^-24:  |P - P_ref| <= gamma_{n+2} + e_p,  gamma_k = k u / (1 - k u).  Every term w p of the sum is positive, the integer weight w
is exact, so the n fused multiply-adds of the running sum cost n roundings relative to a partial sum that is at most the total; the
integer n_tta Wy Wx converts exactly (util.tile_plan keeps it below 2^24) and the division is one more; one spare covers the product
where the compiler does not fuse it.  The total over the weight sum is a weighted mean of values in [0, 1], so the relative bound is
an absolute one.  e_p is the per-element bound the softmax / sigmoid kernel tests of this project use: 1e-6 absolute for sgan_softmax_fwd
(tests/test_hip_ops.py:1036), 1e-6 relative to a maximum below 1 for the sigmoid (tests/test_hip_ops.py:346); tile_blend evaluates the same
expressions, and a weighted mean of elements within e_p is within e_p.  The one-tile plan (16, 0, 1, 16) on a 16 x 16 canvas has w = 1 and
a weight sum of 1: there P must be the pass's own p -- ops.softmax_fwd / ops.sigmoid_nhwc_fwd of the same logits -- bit for bit, which
separates an arithmetic error from a geometry error.

logp against float64 log of the device's own P: no accuracy table of the device math library is installed beside the compiler, so the
margin is capped at 4 ulp of the result (a chosen cap, DESIGN.md R21 says so); the measured maximum is printed (run with -s)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from supervised_gan_amd import util  # noqa: E402

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
E_P = 1e-6                       # tests/test_hip_ops.py:1036 (softmax), :346 (sigmoid)
LOGF_ULP_CAP = 4.0
H0, W0, T, MARGIN = 37, 53, 16, 5
D4 = [(f, r) for f in (0, 1) for r in range(4)]
FLT_MIN = float(np.finfo(np.float32).tiny)


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def source(h=H0, w=W0, seed=3):
    img = np.random.RandomState(seed).randint(0, 256, size=(h, w, 3), dtype=np.uint8)
    img.setflags(write=False)
    return img


@pytest.fixture(scope="module")
def ops(built_lib):
    _dev()
    from supervised_gan_amd import ops
    return ops


def _chw(buf):
    assert not buf[..., 3].any()                          # the padding channel is written, as zero
    return buf[..., :3].permute(2, 0, 1).cpu().numpy()


@pytest.mark.parametrize("flip,rot", D4)
def test_image_prep_tile_inside_the_image_is_image_prep(ops, flip, rot):
    img = torch.from_numpy(source().copy()).to(_dev())
    for y0, x0 in [(0, 0), (H0 - T, W0 - T), (0, W0 - T), (H0 - T, 0), (7, 19)]:
        got = ops.image_prep_tile(img, x0, y0, T, T, flip, rot)
        want = ops.image_prep(img, x0, y0, T, flip, rot)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (y0, x0)


BORDER_ORIGINS = [(-MARGIN, -MARGIN), (-MARGIN, W0 + MARGIN - T), (H0 + MARGIN - T, -MARGIN), (H0 + MARGIN - T, W0 + MARGIN - T),
                  (-MARGIN, 20), (H0 + MARGIN - T, 20), (10, -MARGIN), (10, W0 + MARGIN - T)]      # the corners, and one on each edge


@pytest.mark.parametrize("flip,rot", D4)
def test_image_prep_tile_at_the_borders_is_the_reflected_yardstick(ops, flip, rot):
    img = torch.from_numpy(source().copy()).to(_dev())
    for y0, x0 in BORDER_ORIGINS:
        got = _chw(ops.image_prep_tile(img, x0, y0, T, T, flip, rot))
        want = util.prep_tile_ref(source(), y0, x0, T, T, flip, rot)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (y0, x0)


def test_image_prep_tile_rectangular(ops):
    from supervised_gan_amd import _lib as L
    img = torch.from_numpy(source().copy()).to(_dev())
    for flip in (0, 1):
        got = ops.image_prep_tile(img, 0, 0, H0, W0, flip, 0)
        assert tuple(got.shape) == (H0, W0, 4)
        assert np.array_equal(_chw(got).view(np.int32), util.prep_tile_ref(source(), 0, 0, H0, W0, flip, 0).view(np.int32))
    got = _chw(ops.image_prep_tile(img, -3, -2, 20, 31, 1, 0))           # a rectangle over two borders
    assert np.array_equal(got.view(np.int32), util.prep_tile_ref(source(), -2, -3, 20, 31, 1, 0).view(np.int32))
    # the scalar store path: a 3-channel destination
    out3 = torch.full((T, T, 3), float("nan"), device=_dev())
    ops.image_prep_tile(img, -MARGIN, -MARGIN, T, T, 1, 3, out=out3)
    assert np.array_equal(out3.permute(2, 0, 1).cpu().numpy().view(np.int32), util.prep_tile_ref(source(), -MARGIN, -MARGIN, T, T, 1, 3).view(np.int32))
    out = torch.zeros((H0, W0, 4), device=_dev())
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    lib = L.lib()
    assert lib.sgan_image_prep_tile(P(img), H0, W0, 0, 0, H0, W0, 0, 1, P(out), 4, 4, None) != 0      # a rotated rectangle
    assert b"rectangular" in lib.sgan_last_error()
    assert lib.sgan_image_prep_tile(P(img), H0, W0, 0, -H0, T, T, 0, 0, P(out), 4, 4, None) != 0      # beyond one reflection
    assert lib.sgan_image_prep_tile(P(img), H0, W0, 2 * W0 - T, 0, T, T, 0, 0, P(out), 4, 4, None) != 0
    assert lib.sgan_image_prep_tile(None, H0, W0, 0, 0, T, T, 0, 0, P(out), 4, 4, None) != 0
    torch.cuda.synchronize()
    assert not out.any()


# ---- blend + finish --------------------------------------------------------------------------------------------------------------
CANVAS = (40, 56)
BLEND_PLANS = [(16, 3, 4, 6), (16, 0, 1, 16)]                            # (T, M, R, S)
HEADS = [(2, False), (3, False), (1, True), (2, True)]                   # (C, sigmoid)


@functools.lru_cache(maxsize=None)
def pass_logits(H, W, plan, C, tta):
    """Independent uniform logits in +-8 per pass, [passes, C, T, T] float32; made once per case and never written."""
    t, m, r, s = plan
    oy, ox, _, _ = util.tile_plan(H, W, t, m, r, s)
    n = len(util.tile_passes(oy, ox, tta))
    z = np.random.RandomState(1000 * C + 10 * m + tta).uniform(-8.0, 8.0, size=(n, C, t, t)).astype(np.float32)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def reference(H, W, plan, C, sigmoid, tta):
    t, m, r, s = plan
    return util.blend_tiles_ref(pass_logits(H, W, plan, C, tta), H, W, t, m, r, s, tta=tta, sigmoid=sigmoid, return_count=True)


def run_device(ops, H, W, plan, C, sigmoid, tta):
    """The pass sequence on the device -> (P, logp) as [C, H, W] float32 numpy, and the padding channels of both."""
    t, m, r, s = plan
    dev = _dev()
    oy, ox, Wy, Wx = util.tile_plan(H, W, t, m, r, s)
    z = pass_logits(H, W, plan, C, tta)
    zb = torch.zeros((z.shape[0], t, t, 4), device=dev)
    zb[..., :C] = torch.from_numpy(z.copy()).to(dev).permute(0, 2, 3, 1)
    zb[..., C:] = 77.0                                                  # padding channels of the logits are not read into the result
    canvas = torch.zeros((H, W, 4), device=dev)
    mode = ops.SEGHEAD_SIGMOID if sigmoid else ops.SEGHEAD_SOFTMAX
    for k, (y0, x0, flip, rot) in enumerate(util.tile_passes(oy, ox, tta)):
        ops.tile_blend(zb[k], C, mode, x0, y0, m, r, flip, rot, canvas)
    prob = torch.full((H, W, 4), float("nan"), device=dev)
    logp = torch.full((H, W, 4), float("nan"), device=dev)
    ops.tile_finish(canvas, C, torch.tensor(Wy, dtype=torch.int32, device=dev), torch.tensor(Wx, dtype=torch.int32, device=dev),
                    8 if tta else 1, prob, logp)
    assert not prob[..., C:].any() and not logp[..., C:].any()
    return prob[..., :C].permute(2, 0, 1).cpu().numpy(), logp[..., :C].permute(2, 0, 1).cpu().numpy()


@pytest.mark.parametrize("tta", [False, True])
@pytest.mark.parametrize("C,sigmoid", HEADS)
@pytest.mark.parametrize("plan", BLEND_PLANS)
def test_blend_and_finish_against_the_float64_yardstick(ops, plan, C, sigmoid, tta):
    H, W = CANVAS
    P_ref, n = reference(H, W, plan, C, sigmoid, tta)
    P, logp = run_device(ops, H, W, plan, C, sigmoid, tta)
    k = (n + 2).astype(np.float64)
    bound = k * U32 / (1.0 - k * U32) + E_P
    err = np.abs(P.astype(np.float64) - P_ref)
    print("blend %s C %d %s tta %d: max |P - P_ref| %.3e, bound there %.3e, worst err / bound %.3f (n up to %d)"
          % (plan, C, "sigmoid" if sigmoid else "softmax", tta, err.max(), float(np.broadcast_to(bound, err.shape).ravel()[err.argmax()]),
             float((err / bound).max()), n.max()))
    assert (err <= bound).all()
    # logp = logf(max(P, FLT_MIN)) of the device's own P
    want = np.log(np.maximum(P.astype(np.float64), FLT_MIN))
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    lerr = np.abs(logp.astype(np.float64) - want) / ulp
    print("logp: worst error %.3f ulp of the result (cap %.1f)" % (lerr.max(), LOGF_ULP_CAP + 0.5))
    assert (lerr <= LOGF_ULP_CAP + 0.5).all()                           # the cap, plus the rounding of the float64 logarithm to fp32
    if C > 1:
        assert np.array_equal(logp.argmax(axis=0), P.argmax(axis=0))
    # the same pass sequence again: the same bits
    P2, logp2 = run_device(ops, H, W, plan, C, sigmoid, tta)
    assert np.array_equal(P.view(np.int32), P2.view(np.int32)) and np.array_equal(logp.view(np.int32), logp2.view(np.int32))


@pytest.mark.parametrize("C,sigmoid", HEADS)
def test_one_tile_of_weight_one_returns_the_bits_of_the_head_kernels(ops, C, sigmoid):
    plan = (16, 0, 1, 16)
    P, _ = run_device(ops, 16, 16, plan, C, sigmoid, False)
    z = pass_logits(16, 16, plan, C, False)
    assert z.shape[0] == 1
    zb = torch.zeros((16, 16, 4), device=_dev())
    zb[..., :C] = torch.from_numpy(z[0].copy()).to(_dev()).permute(1, 2, 0)
    pb = torch.empty_like(zb)
    (ops.sigmoid_nhwc_fwd if sigmoid else ops.softmax_fwd)(zb, C, pb)
    want = pb[..., :C].permute(2, 0, 1).cpu().numpy()
    assert np.array_equal(P.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("flip,rot", D4)
def test_one_rotated_tile_is_the_rotated_head_output(ops, flip, rot):
    """One tile, weight 1, every D4 element: P is the head kernel's output moved through d4_inverse, bit for bit (geometry alone)."""
    dev = _dev()
    z = np.random.RandomState(flip * 4 + rot).uniform(-8, 8, size=(3, 16, 16)).astype(np.float32)
    zb = torch.zeros((16, 16, 4), device=dev)
    zb[..., :3] = torch.from_numpy(z).to(dev).permute(1, 2, 0)
    pb = torch.empty_like(zb)
    ops.softmax_fwd(zb, 3, pb)
    canvas = torch.zeros((16, 16, 4), device=dev)
    ops.tile_blend(zb, 3, ops.SEGHEAD_SOFTMAX, 0, 0, 0, 1, flip, rot, canvas)
    want = util.d4_inverse(pb[..., :3].permute(2, 0, 1).cpu().numpy(), flip, rot)
    assert np.array_equal(canvas[..., :3].permute(2, 0, 1).cpu().numpy().view(np.int32), np.ascontiguousarray(want).view(np.int32))


def test_bad_arguments_return_a_status_and_launch_nothing(ops):
    from supervised_gan_amd import _lib as L
    lib, dev = L.lib(), _dev()
    H, W = CANVAS
    z = torch.zeros((16, 16, 8), device=dev)
    canvas = torch.zeros((H, W, 4), device=dev)
    small = torch.zeros((12, 12, 4), device=dev)
    prob, logp = torch.zeros((H, W, 4), device=dev), torch.zeros((H, W, 4), device=dev)
    wy, wx = torch.ones(H, dtype=torch.int32, device=dev), torch.ones(W, dtype=torch.int32, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    blend = lambda **k: lib.sgan_tile_blend(*[k.get(n, d) for n, d in (      # noqa: E731
        ("logits", P(z)), ("ld", 8), ("C", 2), ("mode", 0), ("x0", -3), ("y0", -3), ("T", 16), ("M", 3), ("R", 4), ("flip", 0), ("rot", 0),
        ("canvas", P(canvas)), ("canvas_ld", 4), ("H", H), ("W", W), ("stream", None))])
    assert blend() == 0
    torch.cuda.synchronize()
    canvas.zero_()
    for bad in (dict(C=5), dict(C=0), dict(R=0), dict(R=65), dict(mode=2), dict(rot=4), dict(M=8), dict(M=-1), dict(logits=None),
                dict(canvas=None), dict(x0=-4), dict(y0=H + 3 - 16 + 1), dict(ld=6), dict(canvas_ld=3),
                dict(canvas=P(small), H=12, W=12, M=1, x0=-1, y0=-1),          # T > H + 2 M
                dict(canvas=P(small), H=3, W=12, M=3, T=8, x0=-3, y0=-3)):     # M > H - 1
        assert blend(**bad) != 0, bad
        assert lib.sgan_last_error()
    finish = lambda **k: lib.sgan_tile_finish(*[k.get(n, d) for n, d in (      # noqa: E731
        ("canvas", P(canvas)), ("canvas_ld", 4), ("H", H), ("W", W), ("C", 2), ("Wy", P(wy)), ("Wx", P(wx)), ("n_tta", 1), ("prob", P(prob)),
        ("prob_ld", 4), ("logp", P(logp)), ("logp_ld", 4), ("stream", None))])
    for bad in (dict(C=5), dict(n_tta=2), dict(Wy=None), dict(prob=None), dict(logp=None), dict(canvas=None), dict(H=0), dict(prob_ld=3)):
        assert finish(**bad) != 0, bad
    torch.cuda.synchronize()
    assert not canvas.any() and not prob.any() and not logp.any()      # nothing was launched; the process lives
    assert finish() == 0
    torch.cuda.synchronize()

"""GPU tests of the boundary / Hausdorff loss node on the logits (sgan_distloss.hip) against the fp64 yardstick util.dist_terms_ref fed
the same fp32 inputs.  Both signed maps come from the host yardstick util.signed_edt_sq -- the prediction's from a GIVEN mask -- so no
threshold tie can separate device and host.

Pass rule for losses and dz, the project's (stated at the top of tests/test_hip_seg_terms.py): max|a - b| / (max|b| + 1e-12) <=
max(1e-3, 4 e_ref), e_ref the same statistic of the fp32 torch composition of the plain formulas on the CPU.  The state's two sums
are the losses times N and take the losses' bound.

Where the yardstick is zero by construction the device's value must be exactly 0, from buffers filled with NaN before the call."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_dist_terms_ref_host import rel, torch_dist_terms      # noqa: E402  the plain formulas in torch, float64 or float32

pytestmark = pytest.mark.gpu

# the shapes of tests/test_hip_seg_terms.py plus the two planes of tests/test_hip_signed_edt.py with 3 classes
SHAPES = ((5, 7, 3), (33, 31, 2), (257, 3, 3), (64, 64, 4), (9, 7, 12), (1, 1, 2), (31, 33, 3), (65, 5, 3))
KINDS = ("random", "saturated", "absent", "full", "ignored")
ALPHAS = (2.0, 1.0, 3.0)
SOFTMAX, SIGMOID = 0, 1
CLS = 0
GB, GH = 0.5, 0.25      # the upstream gradients of the two terms
U = 2.0 ** -24


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")


@functools.lru_cache(maxsize=None)
def inputs(H, W, C, mode, kind):
    """(z [npix, C] fp32, label [npix] int64 or target [npix, C] fp32, t_sdsq [npix] int32, p_sdsq [npix] int32) for class 0.  The
    maps are computed once per case and shared, never changed."""
    from supervised_gan_amd.util import signed_edt_sq
    rng = np.random.default_rng(7 * H + W + 1000 * mode)
    npix = H * W
    z = (3.0 * rng.standard_normal((npix, C))).astype(np.float32)
    y = rng.integers(0, C, npix)
    if kind == "saturated":      # +-40: softmax and sigmoid reach exactly 1.0 in fp32; every other pixel with the wrong class on top
        z = np.full((npix, C), -40.0, np.float32)
        top = np.where(np.arange(npix) % 2 == 0, y, (y + 1) % C)
        z[np.arange(npix), top] = 40.0
    if kind == "absent":
        y[y == CLS] = 1
    if kind == "full":
        y[:] = CLS
    truth = (y == CLS).reshape(H, W)
    if kind == "ignored":      # labels of -100 at the start of every row
        y.reshape(H, W)[:, 0] = -100
    pred = np.zeros((H, W), bool) if kind == "absent" else rng.random((H, W)) < 0.4      # absent: both maps are 0 everywhere
    t_s, p_s = signed_edt_sq(truth).reshape(-1), signed_edt_sq(pred).reshape(-1)
    if mode == SOFTMAX:
        lt = y.astype(np.int64)
    else:
        lt = np.eye(C, dtype=np.float32)[np.maximum(y, 0)]
        if kind == "random":      # soft targets
            lt = rng.random((npix, C)).astype(np.float32)
        if kind == "ignored":
            lt[y < 0] = 0.0
    return z, lt, t_s, p_s


def run_device(H, W, z, lt, mode, t_s, p_s, boundary, alpha, layout="dense", gout=(GB, GH), cls=CLS):
    """One forward and one backward from NaN-filled outputs: (L_B, L_H, state [8], dz [npix, C], the padding of dz, the workspace
    after the calls).  layout: "dense" rows of pad4(C); "wide8" / "wide16" dense rows of 8 / 16; "view" logits and target as a window
    of rows of 32 (the scalar form; the gradient stays dense).  gout: the two upstream gradients, None = NULL.  alpha None: the
    Hausdorff term is off and p_sdsq is not handed over."""
    from supervised_gan_amd import ops
    dev = torch.device("cuda", 0)
    npix, C = z.shape

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
    ltb = torch.from_numpy(lt).to(dev) if mode == SOFTMAX else buf(lt, nan)
    dz = buf(None, nan, "dense" if layout == "view" else layout)      # a written operand owns its whole rows
    state = torch.full((8,), nan, dtype=torch.float64, device=dev)
    lB, lH = torch.full((), nan, device=dev), torch.full((), nan, device=dev)
    work = ops.new_dist_loss_workspace(dev)
    tm = torch.from_numpy(t_s).to(dev).view(H, W)
    pm = None if alpha is None else torch.from_numpy(p_s).to(dev).view(H, W)
    ops.dist_loss_forward(zb, C, mode, ltb, cls, tm, pm, boundary, alpha, state, lB, lH, work)
    g = [None if x is None else torch.tensor(x, dtype=torch.float32, device=dev) for x in gout]
    ops.dist_loss_backward(zb, C, mode, ltb, cls, tm, pm, boundary, alpha, g[0], g[1], dz)
    torch.cuda.synchronize()
    pad = dz[:, :, C:]
    return (float(lB), float(lH), state.cpu().numpy(), dz[:, :, :C].reshape(npix, C).cpu().numpy().astype(np.float64),
            pad.cpu().numpy(), work.cpu().numpy())


def judge(name, got, ref64, ref32):
    e, e_ref = rel(got, ref64), rel(ref32, ref64)
    print(f"{name}: kernel vs fp64 {e:.3e}, fp32 composition vs fp64 {e_ref:.3e}")
    assert e <= max(1e-3, 4 * e_ref), (name, e, e_ref)


@pytest.mark.parametrize("mode", [SOFTMAX, SIGMOID])
@pytest.mark.parametrize("shape", SHAPES)
def test_parity_and_exact_zeros(shape, mode):
    _need_gpu()
    from supervised_gan_amd.util import dist_terms_ref
    H, W, C = shape
    npix = H * W
    for kind in KINDS:
        z, lt, t_s, p_s = inputs(H, W, C, mode, kind)
        for alpha in ALPHAS:
            LB, LH, state, dz, pad, work = run_device(H, W, z, lt, mode, t_s, p_s, True, alpha)
            rLB, rLH, rstate, rB, rH = dist_terms_ref(z, lt, mode, CLS, t_s, p_s, True, alpha)
            rdz = GB * rB + GH * rH
            t32 = torch_dist_terms(z, lt, mode, CLS, t_s, p_s, alpha, dtype=torch.float32)
            d32 = GB * t32[2] + GH * t32[3]
            tag = f"{shape} mode {mode} {kind} alpha {alpha}"
            assert np.isfinite(dz).all() and not work.any(), tag
            judge(tag + " L_B", [LB], [rLB], [t32[0]])
            judge(tag + " L_H", [LH], [rLH], [t32[1]])
            judge(tag + " dz", dz, rdz, d32)
            judge(tag + " state sum_B", [state[0]], [rstate[0]], [t32[0] * npix])
            judge(tag + " state sum_H", [state[1]], [rstate[1]], [t32[1] * npix])
            assert state[2] == npix and state[3] == state[0] / npix and state[4] == state[1] / npix, tag
            assert abs(state[3] - LB) <= U * abs(state[3]) and abs(state[4] - LH) <= U * abs(state[4]), tag      # one rounding to fp32
            # exact zeros
            assert pad.size == ((C + 3) // 4 * 4 - C) * npix and not pad.any(), tag      # padding channels: written, as zeros
            if kind in ("absent", "full") or npix == 1:      # the truth's map is 0 everywhere: the boundary term is exactly 0
                assert not t_s.any() and rLB == 0.0 and LB == 0.0 and state[0] == 0.0, tag
            if kind == "absent":      # both maps 0: losses and the whole gradient exactly 0
                assert LH == 0.0 and state[1] == 0.0 and not dz.any() and not rdz.any(), tag
            if mode == SOFTMAX and kind == "ignored":
                rows = np.arange(npix).reshape(H, W)[:, 0]
                assert not dz[rows].any() and not rdz[rows].any(), tag
            if mode == SIGMOID:
                assert not dz[:, 1:].any(), tag      # every channel but the class's


@pytest.mark.parametrize("mode", [SOFTMAX, SIGMOID])
def test_null_upstream_and_one_term_at_a_time(mode):
    _need_gpu()
    from supervised_gan_amd.util import dist_terms_ref
    H, W, C = 33, 31, 2
    z, lt, t_s, p_s = inputs(H, W, C, mode, "random")
    for alpha in ALPHAS:
        joint = run_device(H, W, z, lt, mode, t_s, p_s, True, alpha)
        none = run_device(H, W, z, lt, mode, t_s, p_s, True, alpha, gout=(None, None))
        assert not none[3].any() and not none[4].any()      # both NULL: every element exactly 0
        no_b = run_device(H, W, z, lt, mode, t_s, p_s, True, alpha, gout=(None, GH))
        no_h = run_device(H, W, z, lt, mode, t_s, p_s, True, alpha, gout=(GB, None))
        bnd = run_device(H, W, z, lt, mode, t_s, p_s, True, None, gout=(GB, None))
        hd = run_device(H, W, z, lt, mode, t_s, p_s, False, alpha, gout=(None, GH))
        # a term left out by a NULL gradient is the call with that term switched off, bit for bit
        assert np.array_equal(no_b[3], hd[3]) and np.array_equal(no_h[3], bnd[3])
        assert bnd[0] == joint[0] and hd[1] == joint[1] and bnd[1] == 0.0 and hd[0] == 0.0
        assert bnd[2][1] == 0.0 and bnd[2][4] == 0.0 and hd[2][0] == 0.0 and hd[2][3] == 0.0
        # each alone against the yardstick's own parts
        _, _, _, rB, rH = dist_terms_ref(z, lt, mode, CLS, t_s, p_s, True, alpha)
        t32 = torch_dist_terms(z, lt, mode, CLS, t_s, p_s, alpha, dtype=torch.float32)
        judge(f"mode {mode} alpha {alpha} boundary alone", bnd[3], GB * rB, GB * t32[2])
        judge(f"mode {mode} alpha {alpha} hausdorff alone", hd[3], GH * rH, GH * t32[3])
        judge(f"mode {mode} alpha {alpha} joint", joint[3], GB * rB + GH * rH, GB * t32[2] + GH * t32[3])


def test_another_class():
    """The class is an argument: class C - 1 of a 3-class map, whose maps are the yardstick's of that class."""
    _need_gpu()
    from supervised_gan_amd.util import dist_terms_ref, signed_edt_sq
    H, W, C = 33, 31, 3
    for mode in (SOFTMAX, SIGMOID):
        z, lt, _, p_s = inputs(H, W, C, mode, "random")
        truth = (lt == 2) if mode == SOFTMAX else (lt[:, 2] > 0.5)
        t_s = signed_edt_sq(truth.reshape(H, W)).reshape(-1)
        got = run_device(H, W, z, lt, mode, t_s, p_s, True, 2.0, cls=2)
        rLB, rLH, _, rB, rH = dist_terms_ref(z, lt, mode, 2, t_s, p_s, True, 2.0)
        t32 = torch_dist_terms(z, lt, mode, 2, t_s, p_s, 2.0, dtype=torch.float32)
        judge(f"mode {mode} class 2 L_B", [got[0]], [rLB], [t32[0]])
        judge(f"mode {mode} class 2 L_H", [got[1]], [rLH], [t32[1]])
        judge(f"mode {mode} class 2 dz", got[3], GB * rB + GH * rH, GB * t32[2] + GH * t32[3])


@pytest.mark.parametrize("mode", [SOFTMAX, SIGMOID])
def test_repeatable_and_layout_independent(mode):
    _need_gpu()
    for H, W, C in ((64, 64, 4), (257, 3, 3), (9, 7, 12), (1, 1, 2)):
        z, lt, t_s, p_s = inputs(H, W, C, mode, "random")
        first = run_device(H, W, z, lt, mode, t_s, p_s, True, 3.0)
        assert not first[5].any()      # the workspace is all zero again
        layouts = ["dense", "view"] + [l for l, cs in (("wide8", 8), ("wide16", 16)) if cs >= C]
        for layout in layouts:
            again = run_device(H, W, z, lt, mode, t_s, p_s, True, 3.0, layout=layout)
            assert again[0] == first[0] and again[1] == first[1], (layout, again[:2], first[:2])
            assert np.array_equal(again[2][:5], first[2][:5]) and np.array_equal(again[3], first[3]), layout
            assert not again[4].any() and not again[5].any(), layout


def test_workspace_is_reused_across_calls():
    """One workspace and one state through several forwards of different sizes: each leaves the slots and the ticket at zero.  The
    last size has more workgroups than slots per sum (the grid-stride loop's second trip)."""
    _need_gpu()
    from supervised_gan_amd import ops
    from supervised_gan_amd.util import dist_terms_ref
    dev = torch.device("cuda", 0)
    work, state = ops.new_dist_loss_workspace(dev), ops.new_dist_loss_state(dev)
    lB, lH = torch.zeros((), device=dev), torch.zeros((), device=dev)
    rng = np.random.default_rng(5)
    for H, W, C in ((64, 64, 4), (5, 7, 3), (600, 300, 3), (64, 64, 4)):
        npix = H * W
        z = (3.0 * rng.standard_normal((npix, C))).astype(np.float32)
        y = rng.integers(0, C, npix).astype(np.int64)
        t_s = rng.integers(-50, 50, npix).astype(np.int32)      # the node reads the maps as numbers: any integers will do here
        p_s = rng.integers(-50, 50, npix).astype(np.int32)
        zb = torch.zeros((H, W, 4), device=dev)
        zb[:, :, :C] = torch.from_numpy(z).to(dev).view(H, W, C)
        ops.dist_loss_forward(zb, C, SOFTMAX, torch.from_numpy(y).to(dev), 0, torch.from_numpy(t_s).to(dev), torch.from_numpy(p_s).to(dev),
                              True, 2.0, state, lB, lH, work)
        torch.cuda.synchronize()
        assert not work.cpu().numpy().any()
        rLB, rLH, _, _, _ = dist_terms_ref(z, y, SOFTMAX, 0, t_s, p_s, True, 2.0)
        assert abs(float(lB) - rLB) <= 1e-5 * abs(rLB) + 1e-6 and abs(float(lH) - rLH) <= 1e-5 * abs(rLH) + 1e-6, (float(lB), rLB, float(lH), rLH)


def test_graph_replay_gives_the_eager_bits():
    _need_gpu()
    from supervised_gan_amd import ops
    dev = torch.device("cuda", 0)
    H, W, C = 64, 64, 4
    z, y, t_s, p_s = inputs(H, W, C, SOFTMAX, "random")
    eager = run_device(H, W, z, y, SOFTMAX, t_s, p_s, True, 1.0)
    zb = torch.zeros((H, W, 4), device=dev)
    yb, tm, pm = torch.zeros(H * W, dtype=torch.int64, device=dev), torch.zeros((H, W), dtype=torch.int32, device=dev), torch.zeros((H, W), dtype=torch.int32, device=dev)
    state, work = ops.new_dist_loss_state(dev), ops.new_dist_loss_workspace(dev)
    lB, lH = torch.zeros((), device=dev), torch.zeros((), device=dev)
    dz = torch.empty((H, W, 4), device=dev)
    gb, gh = torch.tensor(GB, device=dev), torch.tensor(GH, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.dist_loss_forward(zb, C, SOFTMAX, yb, CLS, tm, pm, True, 1.0, state, lB, lH, work)
        ops.dist_loss_backward(zb, C, SOFTMAX, yb, CLS, tm, pm, True, 1.0, gb, gh, dz)
    zb[:, :, :C] = torch.from_numpy(z).to(dev).view(H, W, C)
    yb.copy_(torch.from_numpy(y).to(dev))
    tm.copy_(torch.from_numpy(t_s).to(dev).view(H, W))
    pm.copy_(torch.from_numpy(p_s).to(dev).view(H, W))
    for _ in range(2):
        dz.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert float(lB) == eager[0] and float(lH) == eager[1] and np.array_equal(state.cpu().numpy()[:5], eager[2][:5])
        assert np.array_equal(dz.reshape(H * W, 4).cpu().numpy().astype(np.float64), eager[3]) and not work.cpu().numpy().any()


def test_not_covered_launches_nothing():
    _need_gpu()
    from supervised_gan_amd import _lib, ops
    dev = torch.device("cuda", 0)
    H, W = 8, 8
    nan = float("nan")
    zb = torch.zeros((H, W, 20), device=dev)
    y = torch.zeros(H * W, dtype=torch.int64, device=dev)
    maps = torch.zeros((H, W), dtype=torch.int32, device=dev)
    state = torch.full((8,), nan, dtype=torch.float64, device=dev)
    lB, lH = torch.full((), nan, device=dev), torch.full((), nan, device=dev)
    dz = torch.full((H, W, 20), nan, device=dev)
    work = ops.new_dist_loss_workspace(dev)
    one = torch.ones((), device=dev)
    for C, cls, boundary, alpha, why in ((17, 0, True, 2.0, "17 channels"), (3, 3, True, 2.0, "not below C"), (3, -1, True, 2.0, "not below C"),
                                         (3, 0, False, None, "both terms are off"), (3, 0, True, 0.0, "alpha"), (3, 0, True, 4.5, "alpha"),
                                         (3, 0, False, float("nan"), "alpha"), (3, 0, True, -1.0, "alpha")):
        with pytest.raises(_lib.SganError, match=why):
            ops.dist_loss_forward(zb, C, SOFTMAX, y, cls, maps, maps, boundary, alpha, state, lB, lH, work)
        assert why.encode() in _lib.lib().sgan_last_error()
        with pytest.raises(_lib.SganError, match=why):
            ops.dist_loss_backward(zb, C, SOFTMAX, y, cls, maps, maps, boundary, alpha, one, one, dz)
    with pytest.raises(_lib.SganError, match="p_sdsq is required"):
        ops.dist_loss_forward(zb, 3, SOFTMAX, y, 0, maps, None, True, 2.0, state, lB, lH, work)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    lib = _lib.lib()
    # NULL: the Hausdorff term's map, a loss scalar, the gradient
    assert lib.sgan_dist_loss_forward(P(zb), 20, 64, 3, 0, P(y), 0, 0, P(maps), None, 1, 1, 2.0, P(state), P(lB), P(lH), P(work), None) == 1
    assert b"null" in lib.sgan_last_error()
    assert lib.sgan_dist_loss_forward(P(zb), 20, 64, 3, 0, P(y), 0, 0, P(maps), None, 1, 0, 2.0, P(state), None, P(lH), P(work), None) == 1
    assert b"null" in lib.sgan_last_error()
    assert lib.sgan_dist_loss_backward(P(zb), 20, 64, 3, 0, P(y), 0, 0, P(maps), P(maps), 1, 1, 2.0, P(one), P(one), None, 20, None) == 1
    assert b"null" in lib.sgan_last_error()
    assert lib.sgan_dist_loss_backward(P(zb), 20, 64, 3, 0, P(y), 0, 0, P(maps), P(maps), 1, 1, 2.0, P(one), P(one), P(dz), 2, None) == 1
    assert b"gradient rows" in lib.sgan_last_error()
    torch.cuda.synchronize()
    # every output is as it was
    assert torch.isnan(state).all() and torch.isnan(lB) and torch.isnan(lH) and torch.isnan(dz).all() and not work.any()


def test_autograd_node():
    """losses.dist_terms: the gradient reaches the logits only, each term's times its own upstream gradient; a term nobody uses is
    left out; the buffers persist."""
    _need_gpu()
    from supervised_gan_amd import ops
    from supervised_gan_amd.losses import DistLossBuffers, dist_terms
    from supervised_gan_amd.util import dist_terms_ref
    dev = torch.device("cuda", 0)
    H, W, C = 33, 31, 3
    z, y, t_s, p_s = inputs(H, W, C, SOFTMAX, "random")
    bufs = DistLossBuffers(C, H, W, dev)
    logits = torch.from_numpy(z).to(dev).view(H, W, C).permute(2, 0, 1).unsqueeze(0).contiguous().requires_grad_(True)
    label = torch.from_numpy(y).to(dev).view(1, H, W)
    tm, pm = torch.from_numpy(t_s).to(dev).view(H, W), torch.from_numpy(p_s).to(dev).view(H, W)
    rLB, rLH, _, rB, rH = dist_terms_ref(z, y, SOFTMAX, CLS, t_s, p_s, True, 1.0)
    to_np = lambda g: g[0].permute(1, 2, 0).reshape(H * W, C).cpu().numpy().astype(np.float64)      # noqa: E731
    for lam_b, lam_h in ((0.5, 0.25), (0.5, 0.0), (0.0, 2.0)):
        logits.grad = None
        LB, LH = dist_terms(logits, label, ops.SEGHEAD_SOFTMAX, CLS, tm, pm, True, 1.0, buffers=bufs)
        assert LB.data_ptr() == bufs.loss_b.data_ptr() and LH.data_ptr() == bufs.loss_h.data_ptr()
        loss = (lam_b * LB if lam_b else 0) + (lam_h * LH if lam_h else 0)
        loss.backward()
        assert abs(float(LB.detach()) - rLB) <= 1e-5 * max(1.0, abs(rLB)) and abs(float(LH.detach()) - rLH) <= 1e-5 * max(1.0, abs(rLH))
        want = lam_b * rB + lam_h * rH
        assert rel(to_np(logits.grad), want) <= 1e-3, (lam_b, lam_h, rel(to_np(logits.grad), want))
    LB, LH = dist_terms(logits, label, ops.SEGHEAD_SOFTMAX, CLS, tm, None, True, None, buffers=bufs)      # the Hausdorff term off
    assert float(LH) == 0.0 and abs(float(LB) - rLB) <= 1e-5 * max(1.0, abs(rLB))
    with pytest.raises(Exception):
        dist_terms(logits, label, ops.SEGHEAD_SOFTMAX, CLS, tm, None, False, None, buffers=bufs)      # both terms off
    with pytest.raises(Exception):
        dist_terms(logits.cpu(), label.cpu(), ops.SEGHEAD_SOFTMAX, CLS, tm, None, True, None)         # no fallback off the device

"""CPU tests of the soft-clDice term: the host yardstick util.soft_cldice_ref against torch float64 autograd of the published
formulation (Shit et al., CVPR 2021: max-pool erosion / dilation, relu, the relu(delta - S delta) update), its invariants, the tie
rule, the options, and the C ABI's declarations and refusals."""
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


# ---- the published code, literally (clDice/cldice_loss/pytorch: soft_skeleton.py, cldice.py), on [1, 1, H, W] ---------------------
def soft_erode(img):
    p1 = -F.max_pool2d(-img, (3, 1), (1, 1), (1, 0))
    p2 = -F.max_pool2d(-img, (1, 3), (1, 1), (0, 1))
    return torch.min(p1, p2)


def soft_dilate(img):
    return F.max_pool2d(img, (3, 3), (1, 1), (1, 1))


def soft_open(img):
    return soft_dilate(soft_erode(img))


def soft_skel(img, iter_):
    img1 = soft_open(img)
    skel = F.relu(img - img1)
    for _ in range(iter_):
        img = soft_erode(img)
        img1 = soft_open(img)
        delta = F.relu(img - img1)
        skel = skel + F.relu(delta - skel * delta)
    return skel


def published_soft_cldice(y_true, y_pred, iter_, smooth=1.0):
    skel_pred = soft_skel(y_pred, iter_)
    skel_true = soft_skel(y_true, iter_)
    tprec = (torch.sum(skel_pred * y_true) + smooth) / (torch.sum(skel_pred) + smooth)
    tsens = (torch.sum(skel_true * y_pred) + smooth) / (torch.sum(skel_true) + smooth)
    return 1.0 - 2.0 * (tprec * tsens) / (tprec + tsens)


def distinct_plane(H, W, seed):
    """A permutation of H W distinct fp32 values in [0.2, 0.8], and a random binary truth."""
    rng = np.random.default_rng(seed)
    v = (0.2 + 0.6 * (rng.permutation(H * W).astype(np.float64) + 0.5) / (H * W)).astype(np.float32)
    assert len(np.unique(v)) == H * W
    return v.reshape(H, W), (rng.random((H, W)) < 0.4).astype(np.float32)


@pytest.mark.parametrize("H,W,K", ((17, 23, 3), (40, 33, 6), (1, 9, 2)))
def test_yardstick_against_autograd_of_the_published_code(H, W, K):
    from supervised_gan_amd.util import soft_cldice_ref
    P, T = distinct_plane(H, W, 100 * H + K)
    p = torch.from_numpy(P.astype(np.float64))[None, None].requires_grad_(True)
    t = torch.from_numpy(T.astype(np.float64))[None, None]
    want = published_soft_cldice(t, p, K)
    want.backward()
    L, dP, SP, ST, I, M = soft_cldice_ref(P, T, K)
    assert len(I) == K + 2 and all(i.dtype == np.float32 and i.shape == (H, W) for i in I) and np.array_equal(I[0], P)
    err_l, err_g = abs(L - float(want.detach())), float(np.abs(dP - p.grad[0, 0].numpy()).max())
    print(f"{H} x {W}, K = {K}: loss error {err_l:.2e}, gradient error {err_g:.2e}")
    assert err_l <= 1e-12 and err_g <= 1e-12
    assert np.abs(SP - soft_skel(p.detach(), K)[0, 0].numpy()).max() <= 1e-12
    assert (M >= np.abs(dP)).all()      # the absolute-value run bounds the signed one


def test_invariants():
    from supervised_gan_amd.util import soft_cldice_ref, soft_skeleton_ref
    P, T = distinct_plane(21, 19, 7)
    for X in (P, T, np.zeros((4, 5), np.float32), np.ones((4, 5), np.float32)):
        for K in (1, 4, 16):
            S = soft_skeleton_ref(X, K)[0]
            assert (S >= 0.0).all() and (S <= 1.0).all()
    line = np.zeros((9, 11), np.float32)
    line[4, :] = 1.0      # a one-pixel-wide line from edge to edge
    for K in (1, 5):
        assert np.array_equal(soft_skeleton_ref(line, K)[0], line.astype(np.float64))
        L, dP, SP, ST, _, _ = soft_cldice_ref(line, line, K)
        assert L == 0.0 and np.array_equal(SP, ST)
    with pytest.raises(AssertionError):
        soft_skeleton_ref(line, 0)
    with pytest.raises(AssertionError):
        soft_skeleton_ref(line, 17)


def test_tie_rule():
    """The first pixel in the stated order that attains the extreme takes the whole gradient: centre, up, left, right, down for the
    erosion; centre, then row-major for the dilation."""
    from supervised_gan_amd import util
    ones = np.ones((3, 3))
    flat = np.full((3, 3), 0.5, np.float32)
    for order, pad, pick in ((util.CLDICE_ERODE_ORDER, np.float32(np.inf), np.argmin), (util.CLDICE_DILATE_ORDER, np.float32(-np.inf), np.argmax)):
        val, sel = util._cldice_select(flat, order, pad, pick)
        assert np.array_equal(val, flat) and not sel.any()                                   # every window of a constant plane selects its centre
        assert np.array_equal(util._cldice_scatter(ones, sel, order), ones)                  # ... so a gradient stays where it is
    dot = np.zeros((3, 3), np.float32)
    dot[1, 1] = 1.0
    val, sel = util._cldice_select(dot, util.CLDICE_ERODE_ORDER, np.float32(np.inf), np.argmin)
    assert not val.any() and sel.tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]]              # the centre's four zeros tie: up wins
    assert util._cldice_scatter(ones, sel, util.CLDICE_ERODE_ORDER).tolist() == [[1, 2, 1], [1, 0, 1], [1, 1, 1]]
    val, sel = util._cldice_select(dot, util.CLDICE_DILATE_ORDER, np.float32(-np.inf), np.argmax)
    assert val.tolist() == [[1, 1, 1]] * 3 and util._cldice_scatter(ones, sel, util.CLDICE_DILATE_ORDER).tolist() == [[0, 0, 0], [0, 9, 0], [0, 0, 0]]
    ring = np.ones((3, 3), np.float32)
    ring[1, 1] = 0.0
    _, sel = util._cldice_select(ring, util.CLDICE_DILATE_ORDER, np.float32(-np.inf), np.argmax)
    # the centre's eight ones tie: the first in row-major order, the top-left corner, wins; every other pixel is its own maximum
    assert sel.tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]]
    assert util._cldice_scatter(ones, sel, util.CLDICE_DILATE_ORDER).tolist() == [[2, 1, 1], [1, 0, 1], [1, 1, 1]]
    # a constant plane has delta = 0 everywhere (derivative 0 at 0): what is left is the direct term gC S(T), and it is a gradient
    T = np.zeros((3, 3), np.float32)
    T[1, :] = 1.0
    L, dP, SP, ST, _, M = util.soft_cldice_ref(flat, T, 2)
    gC = util.soft_cldice_sums(SP, T.astype(np.float64), ST, flat.astype(np.float64))[7]
    assert not SP.any() and np.array_equal(ST, T) and gC < 0.0
    assert np.array_equal(dP, gC * ST) and np.array_equal(M, -gC * ST) and np.isfinite(L)


def test_options(tmp_path):
    from supervised_gan_amd.options import TrainOptions, check_cldice_options
    base = ["--name", "t", "--gpu_ids", "-1", "--checkpoints_dir", str(tmp_path), "--model", "segmentation"]
    opt = TrainOptions().parse(base, save=False, verbose=False)
    assert (opt.cldice_weight, opt.cldice_iters, opt.cldice_class) == (0.0, 5, 0)
    off = TrainOptions().parse(base + "--cldice_weight 0 --cldice_iters 99 --cldice_class -3".split(), save=False, verbose=False)
    rest = lambda o: {k: v for k, v in vars(o).items() if k not in ("cldice_iters", "cldice_class")}      # noqa: E731
    assert rest(off) == rest(opt)      # with the weight at 0 nothing is checked and nothing is filled in
    on = TrainOptions().parse(base + "--cldice_weight 0.5 --cldice_iters 16 --cldice_class 1 --which_model_netD None".split(), save=False,
                              verbose=False)
    assert (on.cldice_weight, on.cldice_iters, on.cldice_class) == (0.5, 16, 1)
    TrainOptions().parse(base + "--cldice_weight 0.5 --use_sigmoid_ss".split(), save=False, verbose=False)      # beside discriminators too
    for bad, why in (("--cldice_weight -1", "weight >= 0"), ("--cldice_weight nan", "weight >= 0"), ("--cldice_weight 1 --cldice_iters 0", "1..16"),
                     ("--cldice_weight 1 --cldice_iters 17", "1..16"), ("--cldice_weight 1 --cldice_class -1", "class index")):
        with pytest.raises(AssertionError, match=why):
            TrainOptions().parse(base + bad.split(), save=False, verbose=False)
    with pytest.raises(AssertionError, match="--model segmentation"):
        TrainOptions().parse(["--name", "t", "--gpu_ids", "-1", "--checkpoints_dir", str(tmp_path), "--model", "cgan", "--cldice_weight", "1"],
                             save=False, verbose=False)

    class Bare:
        pass
    check_cldice_options(Bare())      # an options object without the flags passes


def test_entry_points_are_declared_and_bound(built_lib):
    import ctypes
    from supervised_gan_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "sgan_hip.h")).read()
    assert "soft-clDice" in header
    assert re.search(r"\bint64_t\s+sgan_cldice_workspace_bytes\s*\(\s*int32_t H,\s*int32_t W,\s*int32_t iters,\s*int32_t with_backward\s*\)\s*;", header)
    assert re.search(r"\bint\s+sgan_soft_skeleton\s*\(\s*const float\* x,\s*int64_t x_rs,\s*int64_t x_ps,\s*int32_t H,\s*int32_t W,\s*int32_t iters,\s*"
                     r"float\* skel,\s*void\* workspace,\s*int64_t workspace_bytes,\s*void\* stream\s*\)\s*;", header)
    assert re.search(r"\bint\s+sgan_cldice_finish\s*\(\s*const float\* sp,\s*const float\* t,\s*int64_t t_rs,\s*int64_t t_ps,\s*const float\* st,\s*"
                     r"const float\* p,\s*int64_t p_rs,\s*int64_t p_ps,\s*int32_t H,\s*int32_t W,\s*double\* state,\s*float\* loss_out,\s*"
                     r"void\* stream\s*\)\s*;", header)
    assert re.search(r"\bint\s+sgan_cldice_backward\s*\(\s*const float\* t,\s*int64_t t_rs,\s*int64_t t_ps,\s*const float\* st,\s*const double\* state,\s*"
                     r"const float\* gout,\s*int32_t H,\s*int32_t W,\s*int32_t iters,\s*float\* dp,\s*void\* workspace,\s*int64_t workspace_bytes,\s*"
                     r"void\* stream\s*\)\s*;", header)
    macros = dict(re.findall(r"#define (SGAN_CLDICE_[A-Z0-9_]+) (\d+)", header))
    assert macros == {"SGAN_CLDICE_MAX_ITERS": "16", "SGAN_CLDICE_STATE_BYTES": "4096"}
    assert ops.CLDICE_MAX_ITERS == 16 and ops.CLDICE_STATE_BYTES == 4096 and len(ops.CLDICE_STATE) == 8
    names = ("sgan_cldice_workspace_bytes", "sgan_soft_skeleton", "sgan_cldice_finish", "sgan_cldice_backward")
    assert all(n in _lib.SIGNATURES for n in names) and _lib.RESTYPES["sgan_cldice_workspace_bytes"] is ctypes.c_int64
    assert [len(_lib.SIGNATURES[n]) for n in names] == [4, 10, 13, 13]
    lib = _lib.lib()
    # the workspace entry needs no device: K + 2 planes for the forward, 2 K + 5 with the backward
    for H, W, K in ((5, 7, 1), (512, 512, 5), (33, 47, 16)):
        assert lib.sgan_cldice_workspace_bytes(H, W, K, 0) == 4 * H * W * (K + 2)
        assert lib.sgan_cldice_workspace_bytes(H, W, K, 1) == 4 * H * W * (2 * K + 5)
    for K in (0, 17, -1):
        assert lib.sgan_cldice_workspace_bytes(64, 64, K, 1) < 0 and b"not covered" in lib.sgan_last_error()
        # refused before anything else is looked at: return 1, nothing launched
        assert lib.sgan_soft_skeleton(None, 64, 1, 64, 64, K, None, None, 0, None) == 1 and b"not covered" in lib.sgan_last_error()
        assert lib.sgan_cldice_backward(None, 64, 1, None, None, None, 64, 64, K, None, None, 0, None) == 1
        assert b"not covered" in lib.sgan_last_error()
    for H, W in ((0, 4), (4, 0), (1, 32769), (32768, 32768)):
        assert lib.sgan_cldice_workspace_bytes(H, W, 5, 0) < 0
    assert lib.sgan_soft_skeleton(None, 64, 1, 64, 64, 5, None, None, 0, None) == 1 and b"null" in lib.sgan_last_error()
    assert lib.sgan_cldice_finish(None, None, 64, 1, None, None, 64, 1, 64, 64, None, None, None) == 1 and b"null" in lib.sgan_last_error()
    assert lib.sgan_cldice_backward(None, 64, 1, None, None, None, 64, 64, 5, None, None, 0, None) == 1 and b"null" in lib.sgan_last_error()

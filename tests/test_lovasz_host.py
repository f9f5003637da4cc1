"""CPU tests of the Lovasz-softmax term: the host yardstick util.lovasz_ref against a brute-force Lovasz extension of the Jaccard
set function, exact rational weights and torch float64 autograd of the published algorithm (Berman, Triki, Blaschko, CVPR 2018),
its invariants, the options, and the C ABI's declarations and refusals."""
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def jaccard_loss_of_set(fg, wrong):
    """The set function whose Lovasz extension the loss is: the Jaccard loss of a prediction that is wrong exactly on `wrong`."""
    hit = sum(1 for i in range(len(fg)) if fg[i] and i not in wrong)             # foreground still found
    union = sum(fg) + sum(1 for i in wrong if not fg[i])                         # foreground and false positives
    return Fraction(0) if union == 0 else 1 - Fraction(hit, union)


def choquet(e, fg):
    """The Lovasz extension as the Choquet integral over the level sets of e: sum over the distinct values v_1 > v_2 > ... of
    (v_j - v_{j+1}) F({e >= v_j}), v_last+1 = 0.  Exact rationals; no order among ties enters."""
    vals = sorted({Fraction(float(x)) for x in e if x > 0}, reverse=True) + [Fraction(0)]
    total = Fraction(0)
    for a, b in zip(vals[:-1], vals[1:]):
        total += (a - b) * jaccard_loss_of_set(fg, {i for i in range(len(e)) if Fraction(float(e[i])) >= a})
    return total


def small_case(N, seed, quantised):
    rng = np.random.default_rng(seed)
    C = 3
    P = rng.random((C, 1, N)).astype(np.float32)
    if quantised:
        P = (np.round(P * 4) / 4).astype(np.float32)
    label = rng.integers(0, C, (1, N))
    return P, label


@pytest.mark.parametrize("quantised", (False, True))
def test_yardstick_against_the_brute_force_extension(quantised):
    from supervised_gan_amd.util import lovasz_ref
    for N in (1, 2, 3, 5, 8, 11):
        for seed in range(6):
            P, label = small_case(N, 100 * N + seed, quantised)
            classes = [2, 0, 1][:1 + seed % 3]
            L, dP, perm, g, Lc, M = lovasz_ref(P, label, classes)
            present = 0
            for a, c in enumerate(classes):
                fg = [bool(v) for v in (label.reshape(-1) == c)]
                e = np.abs(np.asarray(fg, np.float32) - P[c].reshape(-1))
                # pi is the stated total order
                order = sorted(range(N), key=lambda i: (-float(e[i]), i))
                assert perm[a].tolist() == order
                if not any(fg):
                    assert Lc[a] == 0.0 and not g[a].any() and not dP[c].any()
                    continue
                present += 1
                assert abs(Lc[a] - float(choquet(e, fg))) <= 1e-14
                # the weights are the differences of the set function along pi, exactly rounded
                prev = Fraction(0)
                for k in range(N):
                    now = jaccard_loss_of_set(fg, set(order[:k + 1]))
                    assert abs(Fraction(float(g[a, k])) - (now - prev)) <= 2 * Fraction(1, 2 ** 53) * (now - prev), (N, seed, a, k)
                    prev = now
                assert prev == 1 and g[a].min() >= 0.0 and abs(g[a].sum() - 1.0) <= 1e-15 * N
                p64 = P[c].reshape(-1).astype(np.float64)
                want = np.zeros(N)
                want[order] = np.sign(p64 - np.asarray(fg, np.float64))[order] * g[a]
                m = sum(1 for cc in classes if (label == cc).any())
                assert np.allclose(dP[c].reshape(-1) * m, want, rtol=4e-16, atol=0.0)
            m = present
            assert abs(L - (Lc.sum() / m if m else 0.0)) <= 1e-15
            assert np.array_equal(M, np.abs(dP))
            for c in range(3):
                if c not in classes:
                    assert not dP[c].any()


def published_lovasz_softmax(p64, e32, label, classes):
    """The published algorithm (lovasz_losses.py: lovasz_grad, lovasz_softmax_flat with classes = 'present' restricted to a list) in
    torch float64, the errors taking the fp32 values e32 and the gradient of |fg - p|."""
    losses = []
    for c in classes:
        fg = (label == c).double()
        if fg.sum() == 0:
            continue
        exact = (fg - p64[c]).abs()
        errors = e32[c].double() + (exact - exact.detach())
        errors_sorted, perm = torch.sort(errors, dim=0, descending=True, stable=True)
        gt = fg[perm]
        gts = gt.sum()
        inter = gts - gt.cumsum(0)
        union = gts + (1.0 - gt).cumsum(0)
        jac = 1.0 - inter / union
        jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
        losses.append(torch.dot(errors_sorted, jac.detach()))
    return torch.stack(losses).mean() if losses else p64.sum() * 0.0


@pytest.mark.parametrize("H,W,classes", ((17, 23, (0,)), (40, 33, (0, 1)), (1, 9, (2, 1, 0)), (64, 65, (1,))))
def test_yardstick_against_autograd_of_the_published_algorithm(H, W, classes):
    from supervised_gan_amd.util import lovasz_ref
    rng = np.random.default_rng(H * W)
    C, N = 3, H * W
    P = np.stack([(0.031 + 0.917 * (rng.permutation(N) + 0.5) / N) for _ in range(C)]).astype(np.float32).reshape(C, H, W)
    label = rng.integers(0, C, (H, W))
    p32 = torch.from_numpy(P).reshape(C, N)
    lab = torch.from_numpy(label).reshape(N)
    e32 = torch.stack([((lab == c).float() - p32[c]).abs() for c in range(C)])
    assert all(len(np.unique(e32[c].numpy())) == N for c in classes), "tie-free by construction"
    p64 = p32.double().requires_grad_(True)
    want = published_lovasz_softmax(p64, e32, lab, classes)
    want.backward()
    L, dP, perm, g, Lc, M = lovasz_ref(P, label, classes)
    err_l, err_g = abs(L - float(want.detach())), float(np.abs(dP.reshape(C, N) - p64.grad.numpy()).max())
    print(f"{H} x {W}, classes {classes}: loss error {err_l:.2e}, gradient error {err_g:.2e}")
    assert err_l <= 1e-12 and err_g <= 1e-12
    assert np.abs(g.sum(1) - 1.0).max() <= 1e-12 and g.min() >= 0.0
    assert perm.dtype == np.int32 and all(sorted(perm[a].tolist()) == list(range(N)) for a in range(len(classes)))


def test_absent_classes_take_no_part():
    from supervised_gan_amd.util import lovasz_ref
    rng = np.random.default_rng(3)
    P = rng.random((3, 6, 7)).astype(np.float32)
    label = rng.integers(0, 2, (6, 7))      # class 2 never occurs
    one = lovasz_ref(P, label, [0, 1])
    with_absent = lovasz_ref(P, label, [0, 2, 1])
    assert with_absent[0] == one[0] and np.array_equal(with_absent[1], one[1])
    assert with_absent[4][1] == 0.0 and not with_absent[3][1].any() and not with_absent[1][2].any()
    none = lovasz_ref(P, np.full((6, 7), 2), [0, 1])
    assert none[0] == 0.0 and not none[1].any() and not none[3].any() and not none[5].any()
    every = lovasz_ref(P, np.zeros((6, 7), int), [0])      # the class covers every pixel: I U-form never used, g_k = 1 / N
    assert np.array_equal(every[3][0], np.full(42, 1.0 / 42)) and abs(every[0] - float(np.mean((np.float32(1.0) - P[0]).astype(np.float64)))) <= 1e-15
    with pytest.raises(AssertionError):
        lovasz_ref(P, label, [0, 0])
    with pytest.raises(AssertionError):
        lovasz_ref(P, label, [3])


def test_options(tmp_path):
    from supervised_gan_amd.options import TrainOptions, check_lovasz_options
    base = ["--name", "t", "--gpu_ids", "-1", "--checkpoints_dir", str(tmp_path), "--model", "segmentation"]
    opt = TrainOptions().parse(base, save=False, verbose=False)
    assert (opt.lovasz_weight, opt.lovasz_classes) == (0.0, [0])
    off = TrainOptions().parse(base + "--lovasz_weight 0 --lovasz_classes -3 -3".split(), save=False, verbose=False)
    rest = lambda o: {k: v for k, v in vars(o).items() if k != "lovasz_classes"}      # noqa: E731
    assert rest(off) == rest(opt)      # with the weight at 0 nothing is checked and nothing is filled in
    on = TrainOptions().parse(base + "--lovasz_weight 0.5 --lovasz_classes 1 0 --which_model_netD None".split(), save=False, verbose=False)
    assert (on.lovasz_weight, on.lovasz_classes) == (0.5, [1, 0])
    TrainOptions().parse(base + "--lovasz_weight 0.5 --use_sigmoid_ss --cldice_weight 0.25".split(), save=False, verbose=False)
    for bad, why in (("--lovasz_weight -1", "weight >= 0"), ("--lovasz_weight nan", "weight >= 0"),
                     ("--lovasz_weight 1 --lovasz_classes 0 1 2 3 4 5 6 7 8", "1..8 classes"), ("--lovasz_weight 1 --lovasz_classes -1", "class indices"),
                     ("--lovasz_weight 1 --lovasz_classes 1 1", "distinct")):
        with pytest.raises(AssertionError, match=why):
            TrainOptions().parse(base + bad.split(), save=False, verbose=False)
    with pytest.raises(AssertionError, match="--model segmentation"):
        TrainOptions().parse(["--name", "t", "--gpu_ids", "-1", "--checkpoints_dir", str(tmp_path), "--model", "cgan", "--lovasz_weight", "1"],
                             save=False, verbose=False)

    class Bare:
        pass
    check_lovasz_options(Bare())      # an options object without the flags passes


def test_entry_points_are_declared_and_bound(built_lib):
    import ctypes
    from supervised_gan_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "sgan_hip.h")).read()
    assert "Lovasz-softmax" in header
    assert re.search(r"\bint64_t\s+sgan_lovasz_workspace_bytes\s*\(\s*int32_t H,\s*int32_t W,\s*int32_t n\s*\)\s*;", header)
    assert re.search(r"\bint\s+sgan_lovasz_forward\s*\(\s*const float\* p,\s*int64_t p_cs,\s*int64_t p_rs,\s*int64_t p_ps,\s*const int64_t\* label,\s*"
                     r"const int32_t\* classes,\s*int32_t n,\s*int32_t C,\s*int32_t H,\s*int32_t W,\s*float\* loss_out,\s*void\* workspace,\s*"
                     r"int64_t workspace_bytes,\s*void\* stream\s*\)\s*;", header)
    assert re.search(r"\bint\s+sgan_lovasz_backward\s*\(\s*const float\* p,\s*int64_t p_cs,\s*int64_t p_rs,\s*int64_t p_ps,\s*const int32_t\* classes,\s*"
                     r"int32_t n,\s*int32_t C,\s*int32_t H,\s*int32_t W,\s*const float\* gout,\s*float\* dp,\s*const void\* workspace,\s*"
                     r"int64_t workspace_bytes,\s*void\* stream\s*\)\s*;", header)
    assert ops.LOVASZ_MAX_CLASSES == 8 and ops.LOVASZ_MAX_PIXELS == 1 << 20 and ops.LOVASZ_STATE_BYTES == 256
    assert re.search(r"#define SGAN_LOVASZ_MAX_CLASSES 8\b", header) and re.search(r"#define SGAN_LOVASZ_STATE_BYTES 256\b", header)
    names = ("sgan_lovasz_workspace_bytes", "sgan_lovasz_forward", "sgan_lovasz_backward")
    assert all(n in _lib.SIGNATURES for n in names) and _lib.RESTYPES["sgan_lovasz_workspace_bytes"] is ctypes.c_int64
    assert [len(_lib.SIGNATURES[n]) for n in names] == [3, 14, 14]
    lib = _lib.lib()
    for H, W, n in ((1, 1, 1), (5, 7, 3), (64, 65, 2), (512, 512, 1), (1024, 1024, 8)):
        lay = ops.lovasz_layout(H, W, n)      # the header's layout, restated in ops
        assert lib.sgan_lovasz_workspace_bytes(H, W, n) == lay["bytes"] and lay["bytes"] % 8 == 0
        assert lay["P"] >= H * W and lay["P"] & (lay["P"] - 1) == 0 and all(lay[k] % 8 == 0 for k in ("g", "keys", "slots"))
    one = (ctypes.c_int32 * 1)(0)
    for H, W, n in ((0, 4, 1), (4, 0, 1), (1024, 1025, 1), (1, (1 << 20) + 1, 1), (64, 64, 0), (64, 64, 9), (64, 64, -1)):
        assert lib.sgan_lovasz_workspace_bytes(H, W, n) < 0 and b"not covered" in lib.sgan_last_error()
        # refused before anything else is looked at: return 1, nothing launched
        assert lib.sgan_lovasz_forward(None, 1, 1, 1, None, None, n, 3, H, W, None, None, 0, None) == 1 and b"not covered" in lib.sgan_last_error()
        assert lib.sgan_lovasz_backward(None, 1, 1, 1, None, n, 3, H, W, None, None, None, 0, None) == 1 and b"not covered" in lib.sgan_last_error()
    assert lib.sgan_lovasz_forward(None, 4096, 64, 1, None, one, 1, 3, 64, 64, None, None, 0, None) == 1 and b"null" in lib.sgan_last_error()
    assert lib.sgan_lovasz_backward(None, 4096, 64, 1, one, 1, 3, 64, 64, None, None, None, 0, None) == 1 and b"null" in lib.sgan_last_error()
    # the Python wrappers refuse off the device
    from supervised_gan_amd.losses import lovasz_softmax
    with pytest.raises(_lib.SganError):
        lovasz_softmax(torch.rand(1, 3, 4, 4), torch.zeros(4, 4, dtype=torch.int64), [0])
    with pytest.raises(_lib.SganError, match="not covered"):
        ops.new_lovasz_workspace(1024, 1025, 1, torch.device("cpu"))

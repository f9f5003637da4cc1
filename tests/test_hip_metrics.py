"""GPU tests of the segmentation-metric kernels (sgan_metrics.hip): the labelling against scipy, exactly; the four integer sums of
the Rand F-score against their NumPy restatement, exactly, and the score against util.compute_Rand_F_scores and the oracle; the
running accumulators; the confusion matrix against the torch expression of compute_current_accuracy, exactly."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import metrics_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def _label(ops, m, dev):
    return ops.ccl_label(torch.from_numpy(np.ascontiguousarray(m)).to(dev))


@pytest.mark.parametrize("H,W", M.SIZES)
def test_labels_equal_scipy_exactly(H, W):
    from supervised_gan_amd import ops
    dev = _dev()
    for kind, (m, ref) in M.maps_and_labels(H, W).items():
        x = torch.from_numpy(m.copy()).to(dev)
        lab = ops.ccl_label(x)
        again = ops.ccl_label(x)
        got = lab.cpu().numpy()
        ops.check_metric_err(dev)
        assert got.shape == (H, W) and got.dtype == np.int32
        assert np.array_equal(got == 0, m > 0.5), kind
        assert np.array_equal(M.canonical(got), ref), kind                       # scipy's numbering, pixel for pixel
        # canonical form: label - 1 is the smallest raster index of the component
        idx = np.arange(H * W).reshape(H, W)
        first = np.full(int(ref.max()) + 1, H * W)
        np.minimum.at(first, ref.ravel(), idx.ravel())
        assert np.array_equal(got[ref > 0], first[ref[ref > 0]] + 1), kind
        assert torch.equal(lab, again), kind                                    # the same bits on a second run


def _pairs(H, W):
    maps = M.maps_and_labels(H, W)
    kinds = list(maps)
    out = [(kinds[i], kinds[(i + 1) % len(kinds)]) for i in range(len(kinds))] + [("rand25", "rand25"), ("free", "rand60")]
    return [(s, t, maps[s][0], maps[t][0], maps[s][1], maps[t][1]) for s, t in out]


def _score_on_device(ops, s_plane, t_plane, dev):
    sums, f, acc = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev), \
        torch.zeros(2, dtype=torch.float64, device=dev)
    ops.rand_f_accumulate(ops.ccl_label(t_plane), ops.ccl_label(s_plane), acc, sums_out=sums, f_out=f)
    return tuple(int(v) for v in sums.cpu()), float(f.cpu()), acc.cpu().numpy()


@pytest.mark.parametrize("H,W", M.SIZES)
def test_rand_sums_exact_and_score(H, W):
    """(prediction, truth) pairs of the label tests' maps: the integers exactly, F within 1e-9 (fp64 rounding over at most H W squared
    terms is ~6e-11 at 512 x 512) of the host function and, where its loops are affordable, of the oracle; NaN where the host gives NaN."""
    import rand_score as R
    from supervised_gan_amd import ops
    from supervised_gan_amd.util import compute_Rand_F_scores
    dev = _dev()
    for sk, tk, s, t, s_lab, t_lab in _pairs(H, W):
        want = M.rand_sums(t_lab, s_lab)
        sums, f, acc = _score_on_device(ops, torch.from_numpy(s.copy()).to(dev), torch.from_numpy(t.copy()).to(dev), dev)
        ops.check_metric_err(dev)
        assert sums == want, (sk, tk, sums, want)
        with np.errstate(all="ignore"):
            host = float(compute_Rand_F_scores(s, t)[0])
        print(f"{H}x{W} {sk}/{tk}: F {f!r} host {host!r} diff {abs(f - host):.3e}")
        if np.isnan(host):
            assert np.isnan(f) and np.isnan(acc[0]) and acc[1] == 1, (sk, tk, f)
            continue
        assert abs(f - host) < 1e-9 and acc[0] == f and acc[1] == 1, (sk, tk, f, host)
        if H * W <= 96 * 80:
            assert abs(f - R.rand_f_score(s, t)) < 1e-9, (sk, tk)


def test_rand_score_hand_built_cases_and_strided_planes():
    """The merged / split / diagonal cases of tests/test_host_logic.py at 24 x 24, read as channel 0 of a 2-channel and of a 4-wide
    padded NHWC buffer where they lie (pixel stride 2 and 4)."""
    import rand_score as R
    from supervised_gan_amd import ops
    from supervised_gan_amd.util import compute_Rand_F_scores
    dev = _dev()
    t = np.zeros((24, 24), np.float32)
    t[:, 8] = t[:, 16] = t[12, :] = 1
    merged, split, diag = t.copy(), t.copy(), np.zeros((24, 24), np.float32)
    merged[:, 8] = 0
    merged[12, :] = 1
    split[6, :] = 1
    diag[np.arange(24), np.arange(24)] = 1
    rng = np.random.default_rng(5)
    for name, s in (("same", t), ("merged", merged), ("split", split), ("diag", diag)):
        for Cs in (1, 2, 4):
            def plane(m):
                buf = torch.from_numpy(rng.random((24, 24, Cs)).astype(np.float32)).to(dev)      # the other channels hold anything
                buf[:, :, 0] = torch.from_numpy(m).to(dev)
                return buf[:, :, 0]
            sp, tp = plane(s), plane(t)
            assert sp.stride() == (24 * Cs, Cs)
            sums, f, _ = _score_on_device(ops, sp, tp, dev)
            ops.check_metric_err(dev)
            from supervised_gan_amd.util import _label_false_regions
            assert sums == M.rand_sums(_label_false_regions(t > 0.5), _label_false_regions(s > 0.5)), (name, Cs)
            assert abs(f - compute_Rand_F_scores(s, t)[0]) < 1e-9 and abs(f - R.rand_f_score(s, t)) < 1e-9, (name, Cs, f)
            assert (f == 1.0) if name == "same" else (0 < f < 1), (name, f)


def test_running_accumulators_without_a_host_read():
    from supervised_gan_amd import ops
    from supervised_gan_amd.util import compute_Rand_F_scores
    dev = _dev()
    maps = M.maps_and_labels(130, 70)
    pairs = [("rand25", "rand40"), ("serpentine", "rand25"), ("rand50", "spiral")]
    acc = torch.zeros(2, dtype=torch.float64, device=dev)
    planes = [(torch.from_numpy(maps[s][0].copy()).to(dev), torch.from_numpy(maps[t][0].copy()).to(dev)) for s, t in pairs]
    labels = torch.empty((2, 130, 70), dtype=torch.int32, device=dev)
    for sp, tp in planes:                     # enqueue only
        ops.ccl_label(tp, labels[0])
        ops.ccl_label(sp, labels[1])
        ops.rand_f_accumulate(labels[0], labels[1], acc)
    got = acc.cpu().numpy()
    ops.check_metric_err(dev)
    want = sum(float(compute_Rand_F_scores(maps[s][0], maps[t][0])[0]) for s, t in pairs)
    assert got[1] == 3 and abs(got[0] - want) < 3e-9, (got, want)


def _torch_confusion(x, C, label=None, y=None, bg=False):
    """compute_current_accuracy's expression (segm_model.py of the parent commit) on logical [1, C, H, W] tensors."""
    if bg:
        f = lambda t: torch.cat([t, 1.0 - torch.clamp(t.sum(dim=1, keepdim=True), max=1)], 1).argmax(dim=1)      # noqa: E731
        labels, pred, k = (label if label is not None else f(y)), f(x), C + 1
    else:
        labels, pred, k = (label if label is not None else y.argmax(dim=1)), x.argmax(dim=1), C
    return torch.bincount(labels.reshape(-1) * k + pred.reshape(-1), minlength=k * k).reshape(k, k)


def _channel_maps(C, H, W, seed, dev):
    """Padded NHWC buffer [H, W, pad4(C)] of multiples of 1/64 in [0, 1/2] (sums exact in fp32 in any order), with planted ties: equal
    maxima in two channels, and a background value 1 - sum that equals the largest channel."""
    from supervised_gan_amd import ops
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 33, size=(H, W, C)).astype(np.float32) / 64.0
    v[::3, ::2, C - 1] = v[::3, ::2].max(axis=-1)                     # tie between an earlier maximum and the last channel
    v[1::5, :, :] = 0
    v[1::5, :, 0] = 0.5                                               # background 1 - 0.5 ties with channel 0: channel 0 wins
    if C >= 2:
        v[2::7, 1::2, :] = 0
        v[2::7, 1::2, 1] = 0.25                                       # background 0.75 beats everything
    buf = torch.zeros((H, W, ops.pad4(C)), dtype=torch.float32, device=dev)
    buf[:, :, :C] = torch.from_numpy(v).to(dev)
    if ops.pad4(C) > C:
        buf[:, :, C:] = 9.0                                           # padding channels must not be read
    return buf


@pytest.mark.parametrize("C", [2, 3, 16])
@pytest.mark.parametrize("bg", [False, True])
def test_confusion_equals_torch_exactly(C, bg):
    from supervised_gan_amd import ops
    dev = _dev()
    for H, W in ((37, 53), (300, 450)):         # neither a multiple of a workgroup's 256 pixels; the larger wraps the grid-stride loop
        k = C + int(bg)
        xb, yb = _channel_maps(C, H, W, 1, dev), _channel_maps(C, H, W, 2, dev)
        x, y = ops.logical_view(xb, C), ops.logical_view(yb, C)
        label = torch.from_numpy(np.random.default_rng(3).integers(0, k, size=(1, H, W))).to(dev)
        total = torch.zeros((k, k), dtype=torch.int64, device=dev)
        # channel-map form
        conf = torch.zeros((k, k), dtype=torch.int64, device=dev)
        ops.confusion_accumulate(xb, C, conf, y=yb, add_background=bg)
        want = _torch_confusion(x, C, y=y, bg=bg)
        assert torch.equal(conf, want), (C, bg, H, W)
        total += want
        # label-map form: labels in [0, k), the prediction with or without the appended class
        conf2 = torch.zeros((k, k), dtype=torch.int64, device=dev)
        ops.confusion_accumulate(xb, C, conf2, label=label.reshape(-1), add_background=bg)
        want2 = _torch_confusion(x, C, label=label, bg=bg)
        assert torch.equal(conf2, want2), (C, bg, H, W)
        assert not bg or int(conf2[C].sum()) > 0          # the background label is among the truths
        # further accumulations into one matrix equal the sum
        ops.confusion_accumulate(xb, C, conf, label=label.reshape(-1), add_background=bg)
        total += want2
        ops.confusion_accumulate(yb, C, conf, y=xb, add_background=bg)
        total += _torch_confusion(y, C, y=x, bg=bg)
        assert torch.equal(conf, total) and int(conf.sum()) == 3 * H * W
        ops.check_metric_err(dev)


def test_confusion_on_generic_floats():
    """Random floats (a softmax output and uniform maps), C = 2: fp32 addition of two numbers has one order."""
    from supervised_gan_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    H, W, C = 130, 70, 2
    for make in (lambda: torch.rand(H, W, 4, generator=g), lambda: torch.softmax(torch.randn(H, W, 4, generator=g) * 3, dim=-1)):
        xb, yb = make().to(dev), make().to(dev)
        for bg in (False, True):
            conf = torch.zeros((C + int(bg),) * 2, dtype=torch.int64, device=dev)
            ops.confusion_accumulate(xb, C, conf, y=yb, add_background=bg)
            assert torch.equal(conf, _torch_confusion(ops.logical_view(xb, C), C, y=ops.logical_view(yb, C), bg=bg)), bg
    ops.check_metric_err(dev)


def test_short_workspace_is_refused_before_any_launch():
    from supervised_gan_amd import _lib, ops
    dev = _dev()
    l = _lib.lib()
    H, W = 37, 53
    need = l.sgan_rand_f_workspace(H, W)
    ws = torch.full((need // 8 + 1,), 7, dtype=torch.int64, device=dev)
    lab = torch.zeros((H, W), dtype=torch.int32, device=dev)
    acc = torch.zeros(2, dtype=torch.float64, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    rc = l.sgan_rand_f_accumulate(P(lab), P(lab), H, W, P(ws), need - 16, P(acc), None, None, P(ops.metric_err(dev)), None)
    assert rc < 0 and b"workspace" in l.sgan_last_error() and b"nothing was launched" in l.sgan_last_error()
    torch.cuda.synchronize()
    assert bool((ws == 7).all()) and acc.cpu().tolist() == [0.0, 0.0]         # untouched
    with pytest.raises(_lib.SganError, match="workspace"):
        ops.rand_f_accumulate(lab, lab, acc, workspace=ws[:8])

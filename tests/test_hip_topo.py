"""GPU tests of ops.topo_accumulate (sgan_topo.hip) against the host yardstick util.topo_counts: all twelve integers equal, on every
shape / window / stride of topo_ref.CASES and every pair of topo_ref.PAIRS (noise at three densities, a cell map with punched walls,
all wall, all free, a serpentine, a checkerboard, nested rings, diagonals); strided planes, counts_out, pooling, repeatability, null
thinned planes, refusals, and a captured call replayed on other inputs.  Everything is an exact integer: no tolerance.

The thinned planes handed to both sides are ops.thin's (tests/test_hip_thin.py pins those to util.thin)."""
import os
import sys

import numpy as np
import pytest
import torch

import topo_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def _zeros(dev):
    return torch.zeros(12, dtype=torch.int64, device=dev)


def _run(s, t, window, stride, dev, thinned=True):
    """(counts_out of one call as a list, the thinned planes on the host)"""
    from supervised_gan_amd import ops
    s_d, t_d = torch.from_numpy(np.array(s)).to(dev), torch.from_numpy(np.array(t)).to(dev)
    s_thin, t_thin = (ops.thin(s_d), ops.thin(t_d)) if thinned else (None, None)
    acc, out = _zeros(dev), _zeros(dev)
    out.fill_(-7)                                                  # counts_out is written, whatever it held
    ops.topo_accumulate(t_d, s_d, acc, t_thin=t_thin, s_thin=s_thin, window=window, stride=stride, counts_out=out)
    ops.check_metric_err(dev)
    assert torch.equal(acc, out)
    return out.cpu().tolist(), (None if s_thin is None else s_thin.cpu().numpy(), None if t_thin is None else t_thin.cpu().numpy())


@pytest.mark.parametrize("H,W,window,stride", R.CASES)
def test_counts_equal_the_yardstick(H, W, window, stride):
    from supervised_gan_amd import ops, util
    dev = _dev()
    p = R.planes(H, W)
    for s_name, t_name in R.PAIRS:
        got, (s_thin, t_thin) = _run(p[s_name], p[t_name], window, stride, dev)
        want = R.want_betti(H, W, window, stride, s_name, t_name)
        print(H, W, window, stride, s_name, t_name, got, want)
        assert got[:7] == want, (s_name, t_name)
        full = util.topo_counts(p[s_name], p[t_name], window, stride, s_thin=s_thin, t_thin=t_thin)
        assert full[:7].tolist() == want and got == full.tolist(), (s_name, t_name)
    assert int(ops.metric_err(dev).item()) == 0


def test_the_worst_cases_at_window_64():
    """One full-size window: the serpentine is one wall component 2047 + 32 pixels long, the checkerboard 2048 free components."""
    from supervised_gan_amd import util
    dev = _dev()
    p = R.planes(64, 64)
    got, _ = _run(p["serpentine"], p["checkerboard"], 64, 64, dev, thinned=False)
    named = dict(zip(util.TOPO_COUNTS, got))
    assert (named["windows"], named["b0_s"], named["b1_s"], named["b0_t"]) == (1, 1, 0, 1)
    assert named["b1_t"] == 2048 - 126 and named["abs_d0"] == 0 and named["abs_d1"] == 2048 - 126      # 126 of the 252 edge pixels are free
    inverse = (p["serpentine"] < 0.5).astype(np.float32)            # 32 wall bars; the serpentine is now the free space, and touches the edge
    got, _ = _run(inverse, p["all_wall"], 64, 64, dev, thinned=False)
    assert got[:7] == [1, 31, 0, 32, 1, 0, 0]


def test_a_strided_prediction_equals_the_contiguous_one():
    from supervised_gan_amd import ops
    dev = _dev()
    H, W, window, stride = 33, 47, 16, 8
    p = R.planes(H, W)
    want, _ = _run(p["cells_punched"], p["cells"], window, stride, dev)
    nhwc = torch.full((H, W, 4), 0.75, dtype=torch.float32, device=dev)      # the other channels are wall everywhere: a wrong stride shows
    nhwc[:, :, 0] = torch.from_numpy(np.array(p["cells_punched"])).to(dev)
    s_view = nhwc[:, :, 0]
    assert not s_view.is_contiguous() and s_view.stride() == (4 * W, 4)
    t_wide = torch.full((H, W, 2), 0.75, dtype=torch.float32, device=dev)
    t_wide[:, :, 0] = torch.from_numpy(np.array(p["cells"])).to(dev)
    acc = _zeros(dev)
    ops.topo_accumulate(t_wide[:, :, 0], s_view, acc, t_thin=ops.thin(t_wide[:, :, 0]), s_thin=ops.thin(s_view), window=window, stride=stride)
    ops.check_metric_err(dev)
    assert acc.cpu().tolist() == want and nhwc.data_ptr() == s_view.data_ptr()


def test_pooling_counts_out_and_repeatability():
    from supervised_gan_amd import ops
    dev = _dev()
    H, W, window, stride = 96, 80, 33, 17
    p = R.planes(H, W)
    pairs = (("noise30", "noise50"), ("cells_punched", "cells"))
    singles = [_run(p[a], p[b], window, stride, dev)[0] for a, b in pairs]
    acc, out = _zeros(dev), _zeros(dev)
    acc[:] = torch.arange(12, device=dev) * 1000                    # counts_out is the difference, whatever the accumulator held
    for k, (a, b) in enumerate(pairs):
        s_d, t_d = (torch.from_numpy(np.array(p[n])).to(dev) for n in (a, b))
        before = acc.clone()
        ops.topo_accumulate(t_d, s_d, acc, t_thin=ops.thin(t_d), s_thin=ops.thin(s_d), window=window, stride=stride, counts_out=out)
        assert torch.equal(acc - before, out) and out.cpu().tolist() == singles[k]
        again = _zeros(dev)
        ops.topo_accumulate(t_d, s_d, _zeros(dev), t_thin=ops.thin(t_d), s_thin=ops.thin(s_d), window=window, stride=stride, counts_out=again)
        assert torch.equal(again, out)                               # two runs, identical bits
    total = [1000 * i + x + y for i, (x, y) in enumerate(zip(*singles))]
    assert acc.cpu().tolist() == total and total[0] == 2 * 12 + 0 and total[11] == 11000 + 2
    ops.check_metric_err(dev)


def test_null_thinned_planes_leave_the_skeleton_counters_alone():
    from supervised_gan_amd import ops
    dev = _dev()
    H, W, window, stride = 33, 47, 16, 8
    p = R.planes(H, W)
    s_d, t_d = (torch.from_numpy(np.array(p[n])).to(dev) for n in ("cells_punched", "cells"))
    full, _ = _run(p["cells_punched"], p["cells"], window, stride, dev)
    assert min(full[7:11]) > 0
    for t_thin, s_thin, moved in ((None, None, ()), (None, ops.thin(s_d), (7, 8)), (ops.thin(t_d), None, (9, 10))):
        acc = torch.full((12,), 5, dtype=torch.int64, device=dev)
        out = _zeros(dev)
        ops.topo_accumulate(t_d, s_d, acc, t_thin=t_thin, s_thin=s_thin, window=window, stride=stride, counts_out=out)
        got = acc.cpu().tolist()
        assert got == [5 + (full[k] if k < 7 or k == 11 or k in moved else 0) for k in range(12)], (moved, got)
        assert out.cpu().tolist() == [full[k] if k < 7 or k == 11 or k in moved else 0 for k in range(12)]
    ops.check_metric_err(dev)


def test_what_is_not_covered_is_refused():
    from supervised_gan_amd import _lib, ops
    dev = _dev()
    s_d = torch.zeros((64, 64), dtype=torch.float32, device=dev)
    acc = _zeros(dev)
    for window, stride in ((7, None), (65, None), (16, 0), (16, 17)):
        with pytest.raises(_lib.SganError, match="not covered"):
            ops.topo_accumulate(s_d, s_d, acc, window=window, stride=stride)
        with pytest.raises(_lib.SganError, match="not covered"):
            ops.topo_workspace(64, 64, window, window if stride is None else stride, dev)
    torch.cuda.synchronize()
    assert not acc.any()                                             # nothing was launched
    with pytest.raises(_lib.SganError, match="workspace"):
        ops.topo_accumulate(s_d, s_d, acc, window=8, stride=8, workspace=torch.zeros(4, dtype=torch.int64, device=dev))
    assert not acc.any()


def test_a_captured_call_replays_on_other_inputs():
    from supervised_gan_amd import ops, util
    dev = _dev()
    H, W, window, stride = 128, 128, 64, 32
    p = R.planes(H, W)
    s_d, t_d = torch.zeros((H, W), dtype=torch.float32, device=dev), torch.zeros((H, W), dtype=torch.float32, device=dev)
    s_thin, t_thin = torch.zeros_like(s_d), torch.zeros_like(t_d)
    acc, out = _zeros(dev), _zeros(dev)

    def call():
        ops.thin(s_d, out=s_thin)
        ops.thin(t_d, out=t_thin)
        ops.topo_accumulate(t_d, s_d, acc, t_thin=t_thin, s_thin=s_thin, window=window, stride=stride, counts_out=out)

    call()                                                           # the cached workspaces and dev_err exist before the capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            call()
    torch.cuda.current_stream().wait_stream(side)
    acc.zero_()
    total = np.zeros(12, dtype=np.int64)
    for s_name, t_name in (("cells_punched", "cells"), ("serpentine", "checkerboard"), ("cells_punched", "cells")):
        s_d.copy_(torch.from_numpy(np.array(p[s_name])))
        t_d.copy_(torch.from_numpy(np.array(p[t_name])))
        out.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        eager, _ = _run(p[s_name], p[t_name], window, stride, dev)
        assert out.cpu().tolist() == eager, (s_name, t_name)
        assert eager[:7] == R.want_betti(H, W, window, stride, s_name, t_name)
        assert eager == util.topo_counts(p[s_name], p[t_name], window, stride, s_thin=s_thin.cpu().numpy(), t_thin=t_thin.cpu().numpy()).tolist()
        total += np.array(eager)
    assert acc.cpu().tolist() == total.tolist()
    ops.check_metric_err(dev)

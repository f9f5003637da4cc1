"""GPU tests of the thinning kernel (sgan_thin in sgan_metrics.hip) against the host rule util.thin, bit for bit.

The kernel's tile is a 32 x 32 core with a 16-pixel halo (8 iterations per launch).  The random shapes cover: smaller than a tile
(7 x 5), one pixel past a tile in each direction (33 x 70, 65 x 129), several tiles with ragged edges (97 x 131, 130 x 67).  The
all-ones 64 x 64 erodes for 32 iterations -- four launches and a fifth that finds nothing -- across the tile corner at (32, 32), so
erosion crosses every tile border with more iterations than one launch performs; seed 6 does the same on a ragged grid."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import thin_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
CASES = list(R.RANDOM) + ["ones64", "ones17x130", "band40x200", "frame20", "band7x9", "line", "dot"]


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def _mask(name):
    return R.fixed(name) if name in R.FIXED else R.random_mask(name)


def _plane(mask, dev):
    return torch.from_numpy(mask.astype(np.float32)).to(dev)


def _run(ops, plane, dev, max_num_iter=None, **kw):
    it = torch.full((1,), -7, dtype=torch.int32, device=dev)
    out = ops.thin(plane, max_num_iter=max_num_iter, iters_out=it, **kw)
    return out, it


@pytest.mark.parametrize("name", CASES)
def test_equals_the_host_rule_bit_for_bit(name):
    from supervised_gan_amd import ops
    dev = _dev()
    m = _mask(name)
    want, n = R.host_thin(name)
    assert n + 1 <= min(m.shape) // 2 + 2                      # inside the documented budget
    x = _plane(m, dev)
    out, it = _run(ops, x, dev)
    again, it2 = _run(ops, x, dev)
    got = out.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == m.shape and set(np.unique(got).tolist()) <= {0.0, 1.0}
    print("%s: kept %d of %d, %d changing iterations (host %d, %d)" % (name, int(got.sum()), int(m.sum()), int(it.item()), int(want.sum()), n))
    assert np.array_equal(got == 1.0, want), (name, int((got == 1.0).sum()), int(want.sum()))
    assert int(it.item()) == n
    assert torch.equal(out, again) and int(it2.item()) == n    # the same bits on a second run
    assert int(ops.metric_err(dev).item()) == 0
    assert torch.equal(x, _plane(m, dev))                      # the input is left alone


@pytest.mark.parametrize("seed", [s for s in R.RANDOM if R.RANDOM[s][6] is not None])
def test_max_num_iter_gives_the_partial_results(seed):
    from supervised_gan_amd import ops
    dev = _dev()
    x = _plane(R.random_mask(seed), dev)
    for k, kept in zip((1, 2, 3), R.RANDOM[seed][6]):
        want, n = R.host_thin(seed, k)
        out, it = _run(ops, x, dev, max_num_iter=k)
        got = out.cpu().numpy() == 1.0
        assert np.array_equal(got, want) and int(got.sum()) == kept and int(it.item()) == n == k, (seed, k)
    want, n = R.host_thin(seed)
    out, it = _run(ops, x, dev, max_num_iter=1000)             # beyond the budget: the converged result, and no shortfall reported
    assert np.array_equal(out.cpu().numpy() == 1.0, want) and int(it.item()) == n
    assert int(ops.metric_err(dev).item()) == 0


def test_channel_0_of_a_padded_buffer_with_nan_and_one_half():
    from supervised_gan_amd import ops
    dev = _dev()
    m = R.random_mask(2).copy()
    H, W = m.shape
    vals = np.where(m, 0.75, 0.25).astype(np.float32)
    vals[5, 7], vals[20, 33], vals[0, 0], vals[H - 1, W - 1] = np.nan, np.nan, 0.5, 0.5      # not wall, whatever the mask said
    vals[10, 10], vals[11, 40] = np.inf, 0.5000001                                           # wall
    m[5, 7] = m[20, 33] = m[0, 0] = m[H - 1, W - 1] = False
    m[10, 10] = m[11, 40] = True
    from supervised_gan_amd.util import thin
    want, n = thin(m)
    buf = torch.from_numpy(np.random.default_rng(0).random((H, W, 4)).astype(np.float32) * 2).to(dev)      # the other channels hold anything
    buf[:, :, 0] = torch.from_numpy(vals).to(dev)
    plane = buf[:, :, 0]
    assert plane.stride() == (4 * W, 4)
    keep = buf.clone()
    out, it = _run(ops, plane, dev)
    assert np.array_equal(out.cpu().numpy() == 1.0, want) and int(it.item()) == n
    assert torch.equal(torch.nan_to_num(buf, nan=-3.0), torch.nan_to_num(keep, nan=-3.0))
    labels = ops.ccl_label(out)                                # the output is a plane sgan_ccl_label takes as it is
    assert np.array_equal(labels.cpu().numpy() == 0, want)
    ops.check_metric_err(dev)


def test_one_workspace_serves_every_shape():
    """A workspace sized for the largest shape, filled with ones, serves all of them in turn; `out` is written in place."""
    from supervised_gan_amd import _lib, ops
    dev = _dev()
    need = max(_lib.lib().sgan_thin_workspace(*_mask(c).shape) for c in CASES)
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    for name in (4, "ones64", 1, 6, "line", 2):
        ws.fill_(0x0101010101010101)
        m = _mask(name)
        want, n = R.host_thin(name)
        dst = torch.full(m.shape, 5.0, dtype=torch.float32, device=dev)
        out, it = _run(ops, _plane(m, dev), dev, out=dst, workspace=ws)
        assert out is dst and np.array_equal(dst.cpu().numpy() == 1.0, want) and int(it.item()) == n, name
    assert int(ops.metric_err(dev).item()) == 0


def test_a_captured_call_replays_on_data_that_needs_more_iterations():
    """Captured on a one-pixel line (0 changing iterations: every tile launch but the first returns at once), then replayed on the
    all-ones 64 x 64 (32 changing iterations) and on seed 2 (33 x 70, 12): the launch sequence depends on the shape alone.  A graph
    holds one shape, so the three inputs lie in one 64 x 70 plane, zeros elsewhere -- outside the image counts as 0, so the thinned
    rectangle is util.thin of the input itself."""
    from supervised_gan_amd import ops
    dev = _dev()
    H, W = 64, 70
    inputs = []
    for name in ("line", "ones64", 2, "line"):
        m = _mask(name)
        assert m.shape[0] <= H and m.shape[1] <= W
        inputs.append((name, m, np.pad(m, ((0, H - m.shape[0]), (0, W - m.shape[1])))))
    x = _plane(inputs[0][2], dev)
    out = torch.zeros((H, W), dtype=torch.float32, device=dev)
    it = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.thin(x, out=out, iters_out=it)                         # the cached workspace and dev_err exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.thin(x, out=out, iters_out=it)
    for name, m, padded in inputs:
        want, n = R.host_thin(name)
        x.copy_(_plane(padded, dev))
        out.fill_(3.0)
        it.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy() == 1.0
        assert np.array_equal(got[:m.shape[0], :m.shape[1]], want) and int(got.sum()) == int(want.sum()), name
        assert int(it.item()) == n, (name, int(it.item()), n)
    assert R.host_thin("line")[1] == 0 and R.host_thin("ones64")[1] == 32 and R.host_thin(2)[1] == 12
    assert int(ops.metric_err(dev).item()) == 0


def test_malformed_calls_are_refused_before_any_launch():
    from supervised_gan_amd import _lib, ops
    dev = _dev()
    l = _lib.lib()
    H, W = 37, 53
    need = l.sgan_thin_workspace(H, W)
    assert need > 0 and need % 16 == 0 and need >= 2 * H * W + 4 * (min(H, W) // 2 + 2)
    ws = torch.full((need // 8 + 1,), 7, dtype=torch.int64, device=dev)
    x = torch.ones((H, W), dtype=torch.float32, device=dev)
    out = torch.full((H, W), 5.0, dtype=torch.float32, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    err = P(ops.metric_err(dev))
    assert l.sgan_thin(P(x), 1, H, W, P(out), 0, P(ws), need - 16, None, err, None) < 0
    assert b"workspace" in l.sgan_last_error() and b"nothing was launched" in l.sgan_last_error()
    assert l.sgan_thin(P(x), 0, H, W, P(out), 0, P(ws), need, None, err, None) < 0 and b"bad shape" in l.sgan_last_error()
    assert l.sgan_thin(P(x), 1, 0, W, P(out), 0, P(ws), need, None, err, None) < 0 and b"bad shape" in l.sgan_last_error()
    assert l.sgan_thin(P(x), 1, H, W, None, 0, P(ws), need, None, err, None) < 0 and b"null pointer" in l.sgan_last_error()
    assert l.sgan_thin_workspace(0, 5) < 0
    torch.cuda.synchronize()
    assert bool((ws == 7).all()) and bool((out == 5.0).all())                  # untouched
    with pytest.raises(_lib.SganError, match="workspace"):
        ops.thin(x, workspace=ws[:8])

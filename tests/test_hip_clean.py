"""GPU tests of the cleaning stage (sgan_clean_wall in sgan_clean.hip) against the host yardstick util.clean_wall: every plane with
torch.equal, every count with ==, no tolerance anywhere.

Shapes: where tiles, segments and waves end (clean_ref.SHAPES) and one plane of 257 x 255.  Inputs: noise at wall densities 0.05,
0.3 and 0.6; the cell map (Voronoi walls two pixels thick, gaps punched in, specks added) at the shapes that have room for cells
(both sides >= 33: in a row of pixels a two-pixel wall with a hole in it is one pixel, which nothing closes); an empty, an all-wall
and a NaN / 0.5 / just-above-0.5 plane; channel 0 of an NCHW and of an NHWC tensor.  Parameters: clean_ref.cases.

So that a no-op cannot pass, every noise and cell-map case first asserts ON THE YARDSTICK that each enabled stage changed at least
one pixel, wherever the stage can: a closing cannot change a single pixel (1 x 1), and a threshold of exactly a component's area A
removes something only if a smaller component exists (at density 0.05 the free pixels are one component), in which case A + 1, which
always does, carries the condition.  clean_ref.cases marks these."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import clean_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
SPECIAL_PARAMS = tuple((r, 0, 0) for r in R.RSQS) + ((0, 2, 0), (0, 0, 2), (2, 4, 10), (0, 0, 0))


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def _want(name, H, W, params):
    mask, counts = R.want(name, H, W, *params, R.seed_of(name, H, W))
    return torch.from_numpy(mask.astype(np.float32)), counts


def _params_of(name, H, W):
    """[(params, yardstick-checked)]: the cases of a noise / cell-map plane with the no-op condition asserted, the fixed list else."""
    if name in R.SPECIAL:
        return list(SPECIAL_PARAMS)
    out = []
    for params, must in R.cases(name, H, W, R.seed_of(name, H, W)):
        changed = R.stages_changed(R.want(name, H, W, *params, R.seed_of(name, H, W))[1])
        assert all(c for m, c in zip(must, changed) if m), (name, H, W, params, must, changed)      # the yardstick, before the device
        out.append(params)
    return out + [(0, 0, 0)]


def _clean_checked(dev, H, W, name, params, ws, view=None):
    """One case: two calls on the same buffers into a workspace of 0xFF bytes, planes and counts against the yardstick."""
    from supervised_gan_amd import ops
    host = torch.from_numpy(np.array(R.plane(name, H, W, R.seed_of(name, H, W))))
    plane = host.to(dev) if view is None else view(host, dev)
    want, counts = _want(name, H, W, params)
    acc = torch.zeros(6, dtype=torch.int64, device=dev)
    out = torch.full((H, W), 7.0, dtype=torch.float32, device=dev)
    ws.fill_(-1)
    ops.clean_wall(plane, *params, out=out, acc=acc, workspace=ws)
    first, first_acc = out.cpu(), acc.cpu().tolist()
    ops.clean_wall(plane, *params, out=out, acc=acc, workspace=ws)      # what the first call left in the workspace is garbage too
    second, second_acc = out.cpu(), acc.cpu().tolist()
    where = (H, W, name, params)
    assert torch.equal(first, want), (where, int((first != want).sum()), (first != want).nonzero()[:4].tolist())
    assert torch.equal(second, first), where
    assert first_acc == counts and second_acc == [2 * c for c in counts], (where, first_acc, second_acc, counts)


@pytest.mark.parametrize("H,W", R.SHAPES + (R.BIG,))
def test_clean_equals_the_host_yardstick(H, W):
    from supervised_gan_amd import ops
    dev = _dev()
    ws = ops.clean_workspace(H, W, dev).clone()
    names = R.inputs(H, W) if (H, W) != R.BIG else ("noise30", "cell_map")
    for name in names:
        for params in _params_of(name, H, W):
            _clean_checked(dev, H, W, name, params, ws)
    ops.check_metric_err(dev)


def _nchw(host, dev):
    t = torch.full((1, 2) + tuple(host.shape), 0.75, dtype=torch.float32, device=dev)
    t[0, 0] = host.to(dev)
    return t[0, 0]


def _nhwc(host, dev):
    buf = torch.full(tuple(host.shape) + (4,), 0.75, dtype=torch.float32, device=dev)      # the other channels are all wall
    buf[:, :, 0] = host.to(dev)
    return buf[:, :, 0]


@pytest.mark.parametrize("view", (_nchw, _nhwc), ids=("nchw", "nhwc"))
def test_channel_0_is_read_where_it_lies(view):
    """The pixel-stride path: stride 1 inside an NCHW tensor, stride 4 inside an NHWC buffer; every first launch of the three-stage,
    closing-only, specks-only (copy pass) and cells-only (labelling reads the plane itself) sequences reads it."""
    from supervised_gan_amd import ops
    dev = _dev()
    for H, W in ((33, 65), (97, 131)):
        ws = ops.clean_workspace(H, W, dev).clone()
        assert view(torch.zeros(H, W), dev).stride(1) == (1 if view is _nchw else 4)
        for name in ("noise30", "cell_map", "edge_values"):
            params = _params_of(name, H, W)
            for p in (params[1], params[5], params[7], params[-2], (0, 0, 0)) if name not in R.SPECIAL else params:
                _clean_checked(dev, H, W, name, p, ws, view=view)
    ops.check_metric_err(dev)


def test_capture_replays_on_other_planes():
    """One three-stage call captured and replayed on three planes of the same shape, an empty one among them: no launch count
    depends on the data."""
    from supervised_gan_amd import ops
    dev = _dev()
    H, W = 97, 131
    params = (2, 4, 10)
    plane = torch.from_numpy(np.array(R.plane("noise60", H, W))).to(dev)
    out = torch.empty((H, W), dtype=torch.float32, device=dev)
    acc = torch.zeros(6, dtype=torch.int64, device=dev)
    ops.clean_wall(plane, *params, out=out, acc=acc)               # the workspace and dev_err exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.clean_wall(plane, *params, out=out, acc=acc)
    total = [0] * 6
    for name in ("noise30", "cell_map", "empty"):
        want, counts = _want(name, H, W, params)
        plane.copy_(torch.from_numpy(np.array(R.plane(name, H, W))))
        acc.zero_()
        out.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want), name
        assert acc.cpu().tolist() == counts, (name, acc.cpu().tolist(), counts)
        total = [a + b for a, b in zip(total, counts)]
    assert total[5] == 3 and all(R.stages_changed(total)), total      # over the three planes every stage changed something
    ops.check_metric_err(dev)


def test_malformed_calls_are_refused_before_any_launch():
    from supervised_gan_amd import _lib, ops
    dev = _dev()
    l = _lib.lib()
    H, W = 37, 53
    need = l.sgan_clean_workspace(H, W)
    assert need > 0
    ws = torch.full((need // 8 + 1,), 7, dtype=torch.int64, device=dev)
    plane = torch.ones((H, W), dtype=torch.float32, device=dev)
    out = torch.full((H, W), 7.0, dtype=torch.float32, device=dev)
    acc = torch.zeros(6, dtype=torch.int64, device=dev)
    err = ops.metric_err(dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    ok = (1, H, W, 2, 4, 10)
    for args, message in (((None,) + ok + (P(out), P(acc), P(ws), need, P(err), None), b"null pointer"),
                          ((P(plane),) + ok + (None, P(acc), P(ws), need, P(err), None), b"null pointer"),
                          ((P(plane),) + ok + (P(out), P(acc), None, need, P(err), None), b"null pointer"),
                          ((P(plane),) + ok + (P(out), P(acc), P(ws), need, None, None), b"null pointer"),
                          ((P(plane), 1, 0, W, 2, 4, 10, P(out), P(acc), P(ws), need, P(err), None), b"bad shape"),
                          ((P(plane), 1, H, -1, 2, 4, 10, P(out), P(acc), P(ws), need, P(err), None), b"bad shape"),
                          ((P(plane), 1, 32768, 32768, 2, 4, 10, P(out), P(acc), P(ws), 1 << 40, P(err), None), b"bad shape"),      # H W = 2^30
                          ((P(plane), 0, H, W, 2, 4, 10, P(out), P(acc), P(ws), need, P(err), None), b"pixel stride"),
                          ((P(plane), 1, H, W, -1, 4, 10, P(out), P(acc), P(ws), need, P(err), None), b"bad parameter"),
                          ((P(plane), 1, H, W, 2, -4, 10, P(out), P(acc), P(ws), need, P(err), None), b"bad parameter"),
                          ((P(plane), 1, H, W, 2, 4, -10, P(out), P(acc), P(ws), need, P(err), None), b"bad parameter"),
                          ((P(plane), 1, H, W, 4097, 4, 10, P(out), P(acc), P(ws), need, P(err), None), b"bad parameter"),
                          ((P(out),) + ok + (P(out), P(acc), P(ws), need, P(err), None), b"aliases"),
                          ((P(plane),) + ok + (P(out), P(acc), P(ws), need - 16, P(err), None), b"nothing was launched")):
        assert l.sgan_clean_wall(*args) == 1 and message in l.sgan_last_error(), (message, l.sgan_last_error())
    torch.cuda.synchronize()
    assert bool((ws == 7).all()) and bool((out == 7.0).all()) and acc.cpu().tolist() == [0] * 6      # untouched
    assert l.sgan_clean_workspace(0, 5) < 0 and l.sgan_clean_workspace(32768, 32768) < 0
    with pytest.raises(_lib.SganError, match="workspace"):
        ops.clean_wall(plane, 2, 4, 10, workspace=ws[:4])
    assert l.sgan_clean_wall(P(plane), 1, H, W, 4096, 0, 0, P(out), None, P(ws), need, P(err), None) == 0      # the largest radius, no acc
    torch.cuda.synchronize()
    assert bool((out == 1.0).all())
    ops.check_metric_err(dev)

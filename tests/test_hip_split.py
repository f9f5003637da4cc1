"""GPU tests of the cell-splitting stage (sgan_split_cells in sgan_split.hip) against the host yardstick util.split_cells: every plane
with torch.equal, every count with ==, no tolerance anywhere.

Shapes: where the flood's 48 x 32 tiles, its halo, the labelling's tiles and the waves end (split_ref.SHAPES).  Inputs: noise at wall
densities 0.05, 0.3 and 0.6; clean_ref's punched cell map where both sides are >= 33; an empty, an all-wall and a NaN / 0.5 /
just-above-0.5 plane; channel 0 of an NCHW and of an NHWC tensor; a spiral corridor that crosses every tile of its plane and needs
some 2700 rounds; two lobes whose neck lies on the corner of four tiles.  split_rsq in {1, 2, 9, 25}, max_rounds in {1, 8, 9, 64}, and
budgets the spiral exhausts.  Every case makes two calls into a workspace of 0xFF bytes.

So that a no-op cannot pass, every noise and cell-map plane first asserts ON THE YARDSTICK that at least one of its split_rsq values
cuts a pixel -- at every shape that can be cut at all: a single row or column has one core per free run (split_ref.cuttable)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import split_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
BUDGET_BIT = 64


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def _split_checked(dev, H, W, name, rsq, rounds, ws, view=None):
    """One case: two calls on the same buffers into a workspace of 0xFF bytes; planes, counts and the budget bit against the
    yardstick.  Returns the yardstick's counts."""
    from supervised_gan_amd import ops
    host = torch.from_numpy(np.array(R.plane(name, H, W)))
    plane = host.to(dev) if view is None else view(host, dev)
    mask, counts = R.want(name, H, W, rsq, rounds)
    want = torch.from_numpy(mask.astype(np.float32))
    acc = torch.zeros(6, dtype=torch.int64, device=dev)
    out = torch.full((H, W), 7.0, dtype=torch.float32, device=dev)
    err = ops.metric_err(dev)
    assert int(err.item()) == 0
    ws.fill_(-1)
    ops.split_cells(plane, rsq, rounds, out=out, acc=acc, workspace=ws)
    first, first_acc, first_err = out.cpu(), acc.cpu().tolist(), int(err.item())
    ops.split_cells(plane, rsq, rounds, out=out, acc=acc, workspace=ws)      # what the first call left in the workspace is garbage too
    second, second_acc = out.cpu(), acc.cpu().tolist()
    where = (H, W, name, rsq, rounds)
    assert torch.equal(first, want), (where, int((first != want).sum()), (first != want).nonzero()[:4].tolist())
    assert torch.equal(second, first), where
    assert first_acc == counts and second_acc == [2 * c for c in counts], (where, first_acc, second_acc, counts)
    assert first_err == (BUDGET_BIT if counts[4] else 0) and int(err.item()) == first_err, (where, first_err)
    err.zero_()
    return counts


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_split_equals_the_host_yardstick(H, W):
    from supervised_gan_amd import ops
    dev = _dev()
    ws = ops.split_workspace(H, W, dev).clone()
    for name in R.inputs(H, W):
        if name not in R.SPECIAL and R.cuttable(H, W):
            assert any(R.want(name, H, W, rsq, 64)[1][1] > 0 for rsq in R.RSQS), (name, H, W)      # the yardstick, before the device
        full = name in ("noise30", "cell_map")
        for rsq in R.RSQS:
            for rounds in R.ROUNDS if full or rsq == 2 else (64,):
                _split_checked(dev, H, W, name, rsq, rounds, ws)
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
    """The pixel-stride path: stride 1 inside an NCHW tensor, stride 4 inside an NHWC buffer; the transform is the one launch that
    reads the plane."""
    from supervised_gan_amd import ops
    dev = _dev()
    for H, W in ((33, 31), (97, 130)):
        ws = ops.split_workspace(H, W, dev).clone()
        assert view(torch.zeros(H, W), dev).stride(1) == (1 if view is _nchw else 4)
        cut = 0
        for name in ("noise30", "edge_values") + (("cell_map",) if H >= 33 and W >= 33 else ()):
            for rsq in (2, 9):
                cut += _split_checked(dev, H, W, name, rsq, 64, ws, view=view)[1]
        assert cut > 0
    ops.check_metric_err(dev)


def test_the_spiral_needs_many_launches_and_exhausts_a_short_budget():
    """One core in the room at the corridor's mouth, some 2700 rounds to its end, through every tile of the plane.  Budgets of 9, 64
    and 200 rounds are exhausted: the budget bit and counts[4] are set and the plane still equals the yardstick's (nothing is cut,
    there is one core).  4096 rounds finish it, most of the 512 flood launches returning at once."""
    from supervised_gan_amd import ops
    dev = _dev()
    H, W = 97, 130
    ws = ops.split_workspace(H, W, dev).clone()
    for rounds in (9, 64, 200):
        counts = _split_checked(dev, H, W, "spiral", 9, rounds, ws)
        assert counts[0] == 1 and counts[3] == rounds and counts[4] == 1, counts
    counts = _split_checked(dev, H, W, "spiral", 9, 4096, ws)
    free = int((np.array(R.plane("spiral", H, W)) < 0.5).sum())
    assert counts[0] == 1 and 64 < counts[3] < 4096 and counts[4] == 0 and counts[2] == free, counts
    ops.check_metric_err(dev)


def test_a_neck_on_a_tile_corner_is_cut():
    """Two lobes that meet diagonally at (32, 48), where four 48 x 32 tile cores meet: the two floods arrive through the halos."""
    from supervised_gan_amd import ops
    dev = _dev()
    H, W = 96, 112
    ws = ops.split_workspace(H, W, dev).clone()
    for rsq in R.RSQS:
        for rounds in R.ROUNDS:
            counts = _split_checked(dev, H, W, "lobes", rsq, rounds, ws)
            if rsq >= 9 and rounds == 64:
                assert counts[0] == 2 and counts[1] == 3, counts
    ops.check_metric_err(dev)


def test_capture_replays_on_planes_that_need_other_numbers_of_rounds():
    """One call captured on the cell map and replayed on the spiral, which needs all 64 rounds and more, on the lobes, and on an empty
    plane, which needs none: no launch count depends on the data."""
    from supervised_gan_amd import ops
    dev = _dev()
    H, W = 97, 130
    rsq, rounds = 9, 64
    plane = torch.from_numpy(np.array(R.plane("cell_map", H, W))).to(dev)
    out = torch.empty((H, W), dtype=torch.float32, device=dev)
    acc = torch.zeros(6, dtype=torch.int64, device=dev)
    err = ops.metric_err(dev)
    ops.split_cells(plane, rsq, rounds, out=out, acc=acc)               # the workspace and dev_err exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.split_cells(plane, rsq, rounds, out=out, acc=acc)
    seen_rounds = []
    for name in ("cell_map", "spiral", "noise05", "empty"):
        mask, counts = R.want(name, H, W, rsq, rounds)
        plane.copy_(torch.from_numpy(np.array(R.plane(name, H, W))))
        acc.zero_()
        err.zero_()
        out.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), torch.from_numpy(mask.astype(np.float32))), name
        assert acc.cpu().tolist() == counts, (name, acc.cpu().tolist(), counts)
        assert int(err.item()) == (BUDGET_BIT if counts[4] else 0), name
        seen_rounds.append(counts[3])
    err.zero_()
    assert seen_rounds[1] == 64 and seen_rounds[3] == 0 and 0 < seen_rounds[0] < 64, seen_rounds
    ops.check_metric_err(dev)


def test_a_hit_budget_is_counted_and_is_not_an_error():
    """check_metric_err clears the budget bit without raising: the map is complete for its budget, and counts[4] reports it."""
    from supervised_gan_amd import ops
    dev = _dev()
    H, W = 97, 130
    plane = torch.from_numpy(np.array(R.plane("spiral", H, W))).to(dev)
    acc = torch.zeros(6, dtype=torch.int64, device=dev)
    ops.split_cells(plane, 9, 8, acc=acc)
    assert acc.cpu().tolist()[4] == 1 and int(ops.metric_err(dev).item()) == BUDGET_BIT
    ops.check_metric_err(dev)
    assert int(ops.metric_err(dev).item()) == 0


def test_malformed_calls_are_refused_before_any_launch():
    from supervised_gan_amd import _lib, ops
    dev = _dev()
    l = _lib.lib()
    H, W = 37, 53
    need = l.sgan_split_workspace(H, W)
    assert need > 0
    ws = torch.full((need // 8 + 1,), 7, dtype=torch.int64, device=dev)
    plane = torch.ones((H, W), dtype=torch.float32, device=dev)
    out = torch.full((H, W), 7.0, dtype=torch.float32, device=dev)
    acc = torch.zeros(6, dtype=torch.int64, device=dev)
    err = ops.metric_err(dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    ok = (1, H, W, 9, 64)
    tail = (P(acc), P(ws), need, P(err), None)
    for args, message in (((None,) + ok + (P(out),) + tail, b"null pointer"),
                          ((P(plane),) + ok + (None,) + tail, b"null pointer"),
                          ((P(plane),) + ok + (P(out), P(acc), None, need, P(err), None), b"null pointer"),
                          ((P(plane),) + ok + (P(out), P(acc), P(ws), need, None, None), b"null pointer"),
                          ((P(plane), 1, 0, W, 9, 64, P(out)) + tail, b"bad shape"),
                          ((P(plane), 1, H, -1, 9, 64, P(out)) + tail, b"bad shape"),
                          ((P(plane), 1, 32768, 32768, 9, 64, P(out), P(acc), P(ws), 1 << 40, P(err), None), b"bad shape"),      # H W = 2^30
                          ((P(plane), 1, 32769, 1, 9, 64, P(out), P(acc), P(ws), 1 << 40, P(err), None), b"bad shape"),
                          ((P(plane), 0, H, W, 9, 64, P(out)) + tail, b"pixel stride"),
                          ((P(plane), 1, H, W, 0, 64, P(out)) + tail, b"bad parameter"),
                          ((P(plane), 1, H, W, 4097, 64, P(out)) + tail, b"bad parameter"),
                          ((P(plane), 1, H, W, 9, 0, P(out)) + tail, b"bad parameter"),
                          ((P(plane), 1, H, W, 9, 4097, P(out)) + tail, b"bad parameter"),
                          ((P(out),) + ok + (P(out),) + tail, b"aliases"),
                          ((P(plane),) + ok + (P(out), P(acc), P(ws), need - 16, P(err), None), b"nothing was launched"),
                          ((P(plane),) + ok + (P(out), P(acc), ctypes.c_void_p(ws.data_ptr() + 8), need, P(err), None), b"aligned")):
        assert l.sgan_split_cells(*args) == 1 and message in l.sgan_last_error(), (message, l.sgan_last_error())
    torch.cuda.synchronize()
    assert bool((ws == 7).all()) and bool((out == 7.0).all()) and acc.cpu().tolist() == [0] * 6      # untouched
    assert l.sgan_split_workspace(0, 5) < 0 and l.sgan_split_workspace(32768, 32768) < 0
    with pytest.raises(_lib.SganError, match="workspace"):
        ops.split_cells(plane, 9, 64, workspace=ws[:4])
    assert l.sgan_split_cells(P(plane), 1, H, W, 4096, 4096, P(out), None, P(ws), need, P(err), None) == 0      # the largest parameters, no acc
    torch.cuda.synchronize()
    assert bool((out == 1.0).all())
    ops.check_metric_err(dev)

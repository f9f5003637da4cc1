"""GPU tests of the region statistics (sgan_region_stats in sgan_regions.hip) against the host yardstick util.region_table: every
integer column of every row, exactly.

The shapes are the smallest at which each mechanism can go wrong.  The scan block is 1024 pixels and the counting workgroup 64 x 4:
1 x 1 and 1 x 70 (one row, a partial second wave), 37 x 53 (partial waves and rows), 64 x 16 / 65 x 17 / 130 x 67 (exactly one scan
block and one CCL tile, one pixel past both, several of each with ragged edges), 256 x 256 noise (one percolating region that crosses
every wave and workgroup, beside hundreds of small ones), 256 x 256 all free (one region: the largest sums, every lane the same
key), all wall (no rows), the 128 x 128 lattice of isolated pixels (4096 regions, the maximum for the size), and one 512 x 512
cell-like map."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def _noise(H, W, density, seed):
    """free mask: a pixel is wall with probability `density`"""
    return np.random.default_rng(seed).random((H, W)) >= density


def _lattice(H, W):
    m = np.zeros((H, W), bool)
    m[::2, ::2] = True
    return m


def _cells(n):
    y, x = np.mgrid[0:n, 0:n]
    return ~(((y % 32) < 2) | ((x % 32) < 2))


CASES = {
    "1x1_free": lambda: np.ones((1, 1), bool),
    "1x70": lambda: _noise(1, 70, 0.4, 1),
    "37x53": lambda: _noise(37, 53, 0.5, 2),
    "64x16": lambda: _noise(64, 16, 0.5, 3),
    "65x17": lambda: _noise(65, 17, 0.5, 4),
    "130x67": lambda: _noise(130, 67, 0.55, 5),
    "130x67_sparse_walls": lambda: _noise(130, 67, 0.3, 6),
    "256_noise": lambda: _noise(256, 256, 0.5, 7),
    "256_all_free": lambda: np.ones((256, 256), bool),
    "40x50_all_wall": lambda: np.zeros((40, 50), bool),
    "128_lattice": lambda: _lattice(128, 128),
    "512_cells": lambda: _cells(512),
}


def _labels(ops, free, dev):
    return ops.ccl_label(torch.from_numpy((~free).astype(np.float32)).to(dev))


def _fresh(dev, capacity):
    table = torch.full((capacity, 16), -7, dtype=torch.int64, device=dev)
    cursor = torch.zeros(2, dtype=torch.int32, device=dev)
    return table, cursor


@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_host_table_exactly(name):
    from supervised_gan_amd import ops
    from supervised_gan_amd.util import region_table
    dev = _dev()
    free = CASES[name]()
    want = region_table(free)
    H, W = free.shape
    assert want.shape[0] <= ((H + 1) // 2) * ((W + 1) // 2)
    capacity = want.shape[0] + 3
    table, cursor = _fresh(dev, capacity)
    labels = _labels(ops, free, dev)
    keep = labels.clone()
    ops.region_stats(labels, table, cursor)
    got, cur = table.cpu().numpy(), cursor.cpu().numpy()
    print("%s: %d regions, largest %d pixels" % (name, want.shape[0], int(want[:, 0].max()) if len(want) else 0))
    assert cur.tolist() == [want.shape[0], 1]
    assert np.array_equal(got[:len(want)], want), (name, np.argwhere(got[:len(want)] != want)[:8].tolist())
    assert (got[len(want):] == -7).all()                       # nothing behind the rows that were appended
    assert torch.equal(labels, keep)                           # the map is left alone
    if name == "256_all_free":
        assert want.shape[0] == 1 and want[0, 0] == 65536 and want[0, 13] == 4 * 256
    if name == "128_lattice":
        assert want.shape[0] == 4096
    if name == "256_noise":
        assert want[:, 0].max() > 256 * 256 // 4               # the percolating region
    ops.check_metric_err(dev)


def test_a_full_table_keeps_the_first_rows_and_raises_bit_32():
    from supervised_gan_amd import _lib, ops
    from supervised_gan_amd.util import region_table
    dev = _dev()
    free = _lattice(128, 128)
    want = region_table(free)
    labels = _labels(ops, free, dev)
    table, cursor = _fresh(dev, 1000)
    ops.region_stats(labels, table, cursor)
    assert cursor.cpu().tolist() == [1000, 1]
    assert np.array_equal(table.cpu().numpy(), want[:1000])
    assert int(ops.metric_err(dev).item()) == 32
    with pytest.raises(_lib.SganError, match="32 = region table full"):
        ops.check_metric_err(dev)
    ops.check_metric_err(dev)                                  # cleared by the check
    ops.region_stats(labels, table, cursor)                    # a full table takes nothing more; the ordinal still advances
    assert cursor.cpu().tolist() == [1000, 2] and np.array_equal(table.cpu().numpy(), want[:1000])
    assert int(ops.metric_err(dev).item()) == 32
    ops.metric_err(dev).zero_()


def test_labels_of_channel_0_of_a_padded_buffer():
    from supervised_gan_amd import ops
    from supervised_gan_amd.util import region_table
    dev = _dev()
    free = _noise(37, 53, 0.45, 11)
    buf = torch.from_numpy(np.random.default_rng(0).random((37, 53, 4)).astype(np.float32)).to(dev)
    buf[:, :, 0] = torch.from_numpy(np.where(free, 0.25, 0.75).astype(np.float32)).to(dev)
    plane = buf[:, :, 0]
    assert plane.stride() == (4 * 53, 4)
    want = region_table(free)
    table, cursor = _fresh(dev, len(want))                     # exactly full is not an overflow
    ops.region_stats(ops.ccl_label(plane), table, cursor)
    assert np.array_equal(table.cpu().numpy(), want) and cursor.cpu().tolist() == [len(want), 1]
    ops.check_metric_err(dev)


def test_two_images_append_to_one_table():
    from supervised_gan_amd import ops
    from supervised_gan_amd.util import region_table
    dev = _dev()
    a, b, z = _noise(65, 17, 0.5, 21), _noise(65, 17, 0.6, 22), np.zeros((65, 17), bool)
    want = np.concatenate([region_table(a, 0), region_table(z, 1), region_table(b, 2)])
    table, cursor = _fresh(dev, len(want) + 5)
    for m in (a, z, b):                                        # the all-wall image adds no row and still counts
        ops.region_stats(_labels(ops, m, dev), table, cursor)
    got = table.cpu().numpy()
    assert cursor.cpu().tolist() == [len(want), 3]
    assert np.array_equal(got[:len(want)], want)
    assert sorted(set(got[:len(want), 12].tolist())) == [0, 2] and (got[len(want):] == -7).all()
    ops.check_metric_err(dev)


def test_one_workspace_serves_two_shapes_in_turn():
    from supervised_gan_amd import _lib, ops
    from supervised_gan_amd.util import region_table
    dev = _dev()
    shapes = ((130, 67), (37, 53), (130, 67))
    need = max(_lib.lib().sgan_region_stats_workspace(H, W) for H, W in shapes)
    ws = torch.empty(need // 8 + 1, dtype=torch.int64, device=dev)
    for i, (H, W) in enumerate(shapes):
        ws.fill_(0x0101010101010101)                           # whatever the workspace held, the call initialises what it uses
        free = _noise(H, W, 0.5, 30 + i)
        want = region_table(free)
        table, cursor = _fresh(dev, len(want) + 1)
        ops.region_stats(_labels(ops, free, dev), table, cursor, workspace=ws)
        assert np.array_equal(table.cpu().numpy()[:len(want)], want) and cursor.cpu().tolist() == [len(want), 1], (H, W)
    ops.check_metric_err(dev)


def test_a_captured_call_replays_on_maps_with_other_region_counts():
    """Captured (labelling and statistics) on one map, replayed on two others: the launch sequence depends on the shape alone, and
    the table after the replays holds the three blocks one after the other."""
    from supervised_gan_amd import ops
    from supervised_gan_amd.util import region_table
    dev = _dev()
    H, W = 65, 67
    masks = [_noise(H, W, 0.5, 41), _lattice(H, W), np.ones((H, W), bool)]
    blocks = [region_table(m, i) for i, m in enumerate(masks)]
    assert len({len(b) for b in blocks}) == 3
    want = np.concatenate(blocks)
    plane = torch.from_numpy((~masks[0]).astype(np.float32)).to(dev)
    labels = torch.empty((H, W), dtype=torch.int32, device=dev)
    table, cursor = _fresh(dev, len(want) + 2)
    ops.region_stats(ops.ccl_label(plane, labels), table, cursor)      # the cached workspace and dev_err exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.region_stats(ops.ccl_label(plane, labels), table, cursor)
    table.fill_(-7)
    cursor.zero_()
    for m in masks:
        plane.copy_(torch.from_numpy((~m).astype(np.float32)).to(dev))
        g.replay()
    torch.cuda.synchronize()
    got = table.cpu().numpy()
    assert cursor.cpu().tolist() == [len(want), 3]
    assert np.array_equal(got[:len(want)], want) and (got[len(want):] == -7).all()
    ops.check_metric_err(dev)


def test_malformed_calls_are_refused_before_any_launch():
    from supervised_gan_amd import _lib, ops
    dev = _dev()
    l = _lib.lib()
    H, W = 37, 53
    need = l.sgan_region_stats_workspace(H, W)
    assert need > 0 and need % 16 == 0 and need >= 4 * H * W + 128 * ((H + 1) // 2) * ((W + 1) // 2)
    ws = torch.full((need // 8 + 1,), 7, dtype=torch.int64, device=dev)
    labels = torch.zeros((H, W), dtype=torch.int32, device=dev)
    table, cursor = _fresh(dev, 8)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    err = P(ops.metric_err(dev))
    assert l.sgan_region_stats(P(labels), H, W, P(table), 8, P(cursor), P(ws), need - 16, err, None) < 0
    assert b"workspace" in l.sgan_last_error() and b"nothing was launched" in l.sgan_last_error()
    assert l.sgan_region_stats(P(labels), 0, W, P(table), 8, P(cursor), P(ws), need, err, None) < 0 and b"bad shape" in l.sgan_last_error()
    assert l.sgan_region_stats(P(labels), H, 65537, P(table), 8, P(cursor), P(ws), need, err, None) < 0 and b"bad shape" in l.sgan_last_error()
    assert l.sgan_region_stats(P(labels), H, W, P(table), 0, P(cursor), P(ws), need, err, None) < 0 and b"capacity" in l.sgan_last_error()
    for hole in range(4):
        args = [P(labels), P(table), P(cursor), P(ws)]
        args[hole] = None
        assert l.sgan_region_stats(args[0], H, W, args[1], 8, args[2], args[3], need, err, None) < 0 and b"null pointer" in l.sgan_last_error()
    assert l.sgan_region_stats(P(labels), H, W, P(table), 8, P(cursor), P(ws), need, None, None) < 0 and b"null pointer" in l.sgan_last_error()
    torch.cuda.synchronize()
    assert bool((ws == 7).all()) and bool((table == -7).all()) and cursor.cpu().tolist() == [0, 0]      # untouched
    with pytest.raises(_lib.SganError, match="workspace"):
        ops.region_stats(labels, table, cursor, workspace=ws[:8])
    with pytest.raises(AssertionError):
        ops.region_stats(labels, table[:, :8], cursor)
    assert int(ops.metric_err(dev).item()) == 0

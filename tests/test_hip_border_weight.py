"""GPU tests of sgan_border_weight (sgan_border.hip) against the host yardstick util.border_weight_map, on labels from ops.ccl_label.

d1sq and d2sq are exact on every pixel.  bmap must satisfy |a - b| <= 1e-4 b + 1e-30: sqrtf is correctly rounded, the fp32 exponent
argument is at most (2 R)^2 / (2 sigma^2) <= 32 at R = 4 sigma and carries about 4 ulp (8e-6 absolute, which is the relative error it
leaves in the exponential), expf adds a few ulp; 1e-4 is a tenfold margin.

The kernel's tile is a 32 x 32 core with an R-pixel halo.  Shapes: 64 x 64 at R = 20 (2 x 2 cores: halos cross tile edges, tile
corners and the image border), 45 x 70 at R = 7 (ragged cores), 33 x 33 at R = 32 (a halo larger than the image), 45 x 70 at R = 1."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from supervised_gan_amd.util import border_weight_map  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = {"64x64_R20": (64, 64, 20, 5.0), "45x70_R7": (45, 70, 7, 2.0), "33x33_R32": (33, 33, 32, 8.0), "45x70_R1": (45, 70, 1, 0.5)}
MAPS = ["lattice", "lattice_dropped", "noise", "one_cell", "all_wall", "no_wall"]
W0 = 10.0


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def wall_map(name, H, W):
    """bool [H, W], True = wall.  The lattice has one-pixel walls every 9 pixels.  "Dropped": the cells along a band through the image
    centre, 19 pixels thick and parallel to the anti-diagonal, are turned into wall; a pixel in it has its two nearest cells across
    the band, up-left and down-right -- at 64 x 64, where the centre is the tile corner, in diagonal-neighbour tiles."""
    yy, xx = np.mgrid[:H, :W]
    if name in ("lattice", "lattice_dropped"):
        wall = (yy % 9 == 4) | (xx % 9 == 4)
        if name == "lattice_dropped":
            cy, cx = yy - H // 2, xx - W // 2
            wall = wall | ((abs(cy + cx) <= 9) & (abs(cy) <= 14) & (abs(cx) <= 14))
        return wall
    if name == "noise":
        return np.random.default_rng(H * 100 + W).random((H, W)) < 0.5
    if name == "one_cell":
        return ~((abs(yy - H // 3) <= 3) & (abs(xx - W // 2) <= 5))
    return np.full((H, W), name == "all_wall")


def device_labels(wall, dev):
    from supervised_gan_amd import ops
    return ops.ccl_label(torch.from_numpy(wall.astype(np.float32)).to(dev))


def run(labels, R, sigma, dev, planes=True):
    from supervised_gan_amd import ops
    H, W = labels.shape
    d1 = torch.full((H, W), -7, dtype=torch.int32, device=dev) if planes else None
    d2 = torch.full((H, W), -7, dtype=torch.int32, device=dev) if planes else None
    b = ops.border_weight(labels, R, W0, sigma, bmap=torch.full((H, W), 3.0, dtype=torch.float32, device=dev), d1sq=d1, d2sq=d2)
    return d1, d2, b


def compare(got, want, what):
    """got: (d1sq, d2sq, bmap) device tensors (the planes may be None); want: the yardstick's triple."""
    d1, d2, b = got
    e1, e2, eb = want
    if d1 is not None:
        assert np.array_equal(d1.cpu().numpy(), e1), (what, "d1sq")
        assert np.array_equal(d2.cpu().numpy(), e2), (what, "d2sq")
    a = b.cpu().numpy().astype(np.float64)
    err = np.abs(a - eb)
    worst = float((err / np.maximum(eb, 1e-300)).max()) if (eb > 0).any() else 0.0
    print(f"{what}: {int((e1 >= 0).sum())} pixels with one cell, {int((e2 >= 0).sum())} with two, bmap worst relative error {worst:.2e}")
    assert (err <= 1e-4 * eb + 1e-30).all(), (what, "bmap", worst)


@pytest.mark.parametrize("name", MAPS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_equals_the_host_yardstick(shape, name):
    from supervised_gan_amd import ops
    dev = _dev()
    H, W, R, sigma = SHAPES[shape]
    labels = device_labels(wall_map(name, H, W), dev)
    keep = labels.clone()
    want = border_weight_map(labels.cpu().numpy(), R, W0, sigma)
    got = run(labels, R, sigma, dev)
    compare(got, want, f"{shape} {name}")
    again = run(labels, R, sigma, dev)
    assert all(torch.equal(a, b) for a, b in zip(got, again))      # the same bits on a second run
    assert torch.equal(labels, keep) and int(ops.metric_err(dev).item()) == 0
    if name == "lattice" and R > 1:
        assert int((want[1] >= 0).sum()) > 0
    if name in ("one_cell", "all_wall", "no_wall"):
        assert float(got[2].abs().max()) == 0.0


@pytest.mark.parametrize("dx, included", [(4, True), (5, False)])
def test_radius_5_across_the_tile_boundary(dx, included):
    """The wall pixel (31, 31) is the last of its tile in both directions; cell one is its left neighbour, cell two a single pixel at
    offset (3, dx) in the diagonal-neighbour tile: (3, 4) lies on the disc of R = 5, (3, 5) outside it."""
    dev = _dev()
    wall = np.ones((64, 64), dtype=bool)
    wall[31, 30] = False
    wall[34, 31 + dx] = False
    labels = device_labels(wall, dev)
    d1, d2, b = run(labels, 5, 5.0, dev)
    compare((d1, d2, b), border_weight_map(labels.cpu().numpy(), 5, W0, 5.0), f"offset (3, {dx})")
    assert int(d1[31, 31]) == 1
    if included:
        assert int(d2[31, 31]) == 25 and abs(float(b[31, 31]) - W0 * np.exp(-36.0 / 50.0)) <= 1e-4 * W0
    else:
        assert int(d2[31, 31]) == -1 and float(b[31, 31]) == 0.0


def test_optional_planes_may_be_null_and_nothing_is_written_past_the_end():
    """45 x 70 at R = 7 (ragged cores): bmap alone gives the bits it has beside the planes, and every output ends in a sentinel."""
    from supervised_gan_amd import ops
    dev = _dev()
    H, W, R, sigma = SHAPES["45x70_R7"]
    labels = device_labels(wall_map("lattice", H, W), dev)
    _, _, b_with = run(labels, R, sigma, dev)
    _, _, b_alone = run(labels, R, sigma, dev, planes=False)
    assert torch.equal(b_with, b_alone)
    n, guard = H * W, 4096
    fb = torch.full((n + guard,), 3.0, dtype=torch.float32, device=dev)
    f1 = torch.full((n + guard,), -7, dtype=torch.int32, device=dev)
    f2 = torch.full((n + guard,), -7, dtype=torch.int32, device=dev)
    ops.border_weight(labels, R, W0, sigma, bmap=fb[:n].view(H, W), d1sq=f1[:n].view(H, W), d2sq=f2[:n].view(H, W))
    torch.cuda.synchronize()
    assert torch.equal(fb[:n].view(H, W), b_with)
    assert bool((fb[n:] == 3.0).all()) and bool((f1[n:] == -7).all()) and bool((f2[n:] == -7).all())


def test_refused_arguments_return_1_and_leave_the_outputs_untouched():
    from supervised_gan_amd import _lib, ops
    dev = _dev()
    l = _lib.lib()
    H, W = 33, 40
    labels = device_labels(wall_map("lattice", H, W), dev)
    b = torch.full((H, W), 3.0, dtype=torch.float32, device=dev)
    d1 = torch.full((H, W), -7, dtype=torch.int32, device=dev)
    d2 = torch.full((H, W), -7, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    call = lambda lab, h, w, r, sig, bm: l.sgan_border_weight(lab, h, w, r, 10.0, sig, bm, P(d1), P(d2), P(err), None)      # noqa: E731
    assert call(P(labels), H, W, 0, 5.0, P(b)) == 1
    assert call(P(labels), H, W, 33, 5.0, P(b)) == 1
    assert call(P(labels), H, W, 5, 0.0, P(b)) == 1
    assert call(P(labels), H, W, 5, -1.0, P(b)) == 1
    assert call(P(labels), H, W, 5, float("nan"), P(b)) == 1
    assert call(P(labels), 32768, 32768, 5, 5.0, P(b)) == 1      # H W = 2^30
    assert call(P(labels), 0, W, 5, 5.0, P(b)) == 1
    assert call(None, H, W, 5, 5.0, P(b)) == 1
    assert call(P(labels), H, W, 5, 5.0, None) == 1
    torch.cuda.synchronize()
    assert bool((b == 3.0).all()) and bool((d1 == -7).all()) and bool((d2 == -7).all()) and int(err.item()) == 0
    assert call(P(labels), H, W, 32, 5.0, P(b)) == 0             # the largest radius is taken
    torch.cuda.synchronize()
    assert not bool((b == 3.0).any())
    with pytest.raises(_lib.SganError, match="refused"):
        ops.border_weight(labels, 40, 10.0, 5.0)


def test_a_negative_label_is_wall_and_is_reported():
    from supervised_gan_amd import _lib
    dev = _dev()
    H, W, R, sigma = SHAPES["64x64_R20"]
    labels = device_labels(wall_map("lattice", H, W), dev)
    assert int(labels[30, 33]) > 0 and int(labels[4, 4]) == 0
    labels[30, 33] = -5      # a cell pixel beside the tile corner
    labels[4, 4] = -1        # a wall pixel
    want = border_weight_map(labels.cpu().numpy(), R, W0, sigma)
    assert want[0][30, 33] >= 0      # the yardstick reads it as wall: it has a nearest cell
    b = torch.full((H, W), 3.0, dtype=torch.float32, device=dev)
    d1 = torch.full((H, W), -7, dtype=torch.int32, device=dev)
    d2 = torch.full((H, W), -7, dtype=torch.int32, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    assert _lib.lib().sgan_border_weight(P(labels), H, W, R, W0, sigma, P(b), P(d1), P(d2), P(err), None) == 0
    torch.cuda.synchronize()
    assert int(err.item()) != 0
    compare((d1, d2, b), want, "negative label")


def test_a_captured_call_replays_on_other_maps():
    """ccl_label + border_weight + pixel_weight_sum captured on the lattice, replayed on the noise map, the lattice with a cell removed
    and the lattice again: planes as above.  The norm is sum_p (class_w[y_p] + bmap_p) over positive terms that each carry at most
    1e-4 relative error, one fp32 rounding in the per-pixel add and one in the result: |norm - want| <= (1e-4 + 2^-22) want."""
    from supervised_gan_amd import ops
    dev = _dev()
    H, W, R, sigma = SHAPES["64x64_R20"]
    cw = torch.tensor([2.0, 0.5], dtype=torch.float32, device=dev)

    def load(name):
        wall = wall_map(name, H, W)
        plane.copy_(torch.from_numpy(wall.astype(np.float32)))
        label.copy_(torch.from_numpy((~wall).astype(np.int64)).reshape(-1))      # class 0 = wall

    def enqueue():
        ops.ccl_label(plane, cells)
        ops.border_weight(cells, R, W0, sigma, bmap=b, d1sq=d1, d2sq=d2)
        ops.pixel_weight_sum(label, 2, cw, b.reshape(-1), norm)

    plane = torch.zeros((H, W), dtype=torch.float32, device=dev)
    label = torch.zeros(H * W, dtype=torch.int64, device=dev)
    cells = torch.zeros((H, W), dtype=torch.int32, device=dev)
    b = torch.zeros((H, W), dtype=torch.float32, device=dev)
    d1 = torch.zeros((H, W), dtype=torch.int32, device=dev)
    d2 = torch.zeros((H, W), dtype=torch.int32, device=dev)
    norm = torch.zeros((), dtype=torch.float32, device=dev)
    load("lattice")
    enqueue()                      # the cached workspaces and dev_err exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        enqueue()
    for name in ("noise", "lattice_dropped", "lattice"):
        load(name)
        b.fill_(3.0)
        d1.fill_(-7)
        d2.fill_(-7)
        norm.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        wall = wall_map(name, H, W)
        want = border_weight_map(cells.cpu().numpy(), R, W0, sigma)
        assert np.array_equal(cells.cpu().numpy() == 0, wall)
        compare((d1, d2, b), want, f"replay on {name}")
        want_norm = float(np.where(wall, 2.0, 0.5).sum() + want[2].sum())
        print(f"replay on {name}: norm {float(norm)!r}, yardstick {want_norm!r}")
        assert abs(float(norm) - want_norm) <= (1e-4 + 2.0 ** -22) * want_norm
    assert int(ops.metric_err(dev).item()) == 0

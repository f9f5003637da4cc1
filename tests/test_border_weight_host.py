"""CPU tests of util.border_weight_map -- the host yardstick of sgan_border_weight -- and of the --border_weight options.

The yardstick walks the disc's offsets in ascending distance over shifted copies of the map.  It is held against an independent
all-pairs brute force (for every wall pixel, every cell pixel within R, the minimum per label) and, where scipy imports, against
one Euclidean distance transform per cell; d1sq and d2sq must match exactly, bmap to 1e-12."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from supervised_gan_amd.util import border_weight_map  # noqa: E402


def brute_force(lab, R, w0, sigma):
    lab = np.asarray(lab)
    H, W = lab.shape
    d1 = np.full((H, W), -1, dtype=np.int64)
    d2 = np.full((H, W), -1, dtype=np.int64)
    b = np.zeros((H, W), dtype=np.float64)
    cells = [(y, x, int(lab[y, x])) for y in range(H) for x in range(W) if lab[y, x] > 0]
    for y in range(H):
        for x in range(W):
            if lab[y, x] > 0:
                continue
            best = {}
            for cy, cx, L in cells:
                d = (cy - y) ** 2 + (cx - x) ** 2
                if d <= R * R and d < best.get(L, 1 << 60):
                    best[L] = d
            m = sorted(best.values())
            if len(m) >= 1:
                d1[y, x] = m[0]
            if len(m) >= 2:
                d2[y, x] = m[1]
                b[y, x] = w0 * math.exp(-(math.sqrt(m[0]) + math.sqrt(m[1])) ** 2 / (2 * sigma * sigma))
    return d1, d2, b


def lattice(H, W, pitch, drop=()):
    """Square cells of (pitch - 1)^2 pixels separated by one-pixel walls; cell ids count from 1, `drop` lists ids turned into wall."""
    lab = np.zeros((H, W), dtype=np.int64)
    ny = (W + pitch - 1) // pitch
    for y in range(H):
        for x in range(W):
            if y % pitch and x % pitch:
                L = 1 + (y // pitch) * ny + x // pitch
                lab[y, x] = 0 if L in drop else L
    return lab


def noise(H, W, seed, density=0.5):
    """Per-pixel noise: a wall with probability `density`, else a cell id of its own (every free pixel its own cell is the hardest
    case for the pair rule: many labels at equal distances)."""
    rng = np.random.default_rng(seed)
    free = rng.random((H, W)) >= density
    return np.where(free, 1 + np.arange(H * W).reshape(H, W), 0).astype(np.int64)


def blobs(H, W, seed, n=6):
    """A few labelled discs of random radius, overlapping ones keep the later label."""
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W), dtype=np.int64)
    yy, xx = np.mgrid[:H, :W]
    for k in range(n):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(2, 6)
        lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k + 1
    return lab


MAPS = {"lattice": (lattice(24, 23, 6), 7, 2.0), "lattice_dropped": (lattice(24, 24, 5, drop=(7, 8)), 9, 3.0),
        "noise": (noise(19, 24, 1), 4, 1.5), "noise_sparse": (noise(24, 17, 2, 0.9), 12, 4.0), "blobs": (blobs(24, 24, 3), 24, 5.0),
        "blobs_r1": (blobs(20, 21, 4), 1, 0.5), "negative_label": (np.where(blobs(16, 16, 5) == 2, -3, blobs(16, 16, 5)), 6, 2.0)}


@pytest.mark.parametrize("name", list(MAPS))
def test_equals_the_all_pairs_brute_force(name):
    lab, R, sigma = MAPS[name]
    d1, d2, b = border_weight_map(lab, R, 10.0, sigma)
    e1, e2, eb = brute_force(lab, R, 10.0, sigma)
    assert d1.shape == lab.shape and b.dtype == np.float64
    assert np.array_equal(d1, e1) and np.array_equal(d2, e2)
    assert np.abs(b - eb).max() <= 1e-12
    assert ((d2 < 0) | (d1 <= d2)).all() and ((d1 >= 0) | (d2 < 0)).all()
    assert (b[lab > 0] == 0).all() and (d1[lab > 0] == -1).all() and (d2[lab > 0] == -1).all()


@pytest.mark.parametrize("name", [n for n in MAPS if n != "negative_label"])
def test_equals_one_distance_transform_per_cell(name):
    ndimage = pytest.importorskip("scipy.ndimage")
    lab, R, sigma = MAPS[name]
    ids = [int(v) for v in np.unique(lab) if v > 0]
    if len(ids) > 64:
        ids = ids[:: len(ids) // 64 + 1]      # the noise maps: a subset of the cells, the map reduced to them
        lab = np.where(np.isin(lab, ids), lab, 0)
    d1, d2, _ = border_weight_map(lab, R, 10.0, sigma)
    per_cell = np.stack([np.rint(ndimage.distance_transform_edt(lab != L) ** 2).astype(np.int64) for L in ids])
    per_cell = np.where(per_cell <= R * R, per_cell, 1 << 60)
    per_cell.sort(axis=0)
    wall = lab == 0
    e1 = np.where(wall & (per_cell[0] < 1 << 60), per_cell[0], -1)
    e2 = np.where(wall & (per_cell[1] < 1 << 60), per_cell[1], -1) if len(ids) > 1 else np.full(lab.shape, -1)
    assert np.array_equal(d1, e1) and np.array_equal(d2, e2)


def test_two_cells_separated_by_a_one_pixel_wall():
    lab = np.zeros((5, 7), dtype=np.int64)
    lab[:, :3], lab[:, 4:] = 1, 2
    d1, d2, b = border_weight_map(lab, 5, 10.0, 5.0)
    assert (d1[:, 3] == 1).all() and (d2[:, 3] == 1).all()
    assert np.allclose(b[:, 3], 10.0 * math.exp(-4.0 / 50.0), rtol=0, atol=1e-15)
    assert (b[:, :3] == 0).all() and (b[:, 4:] == 0).all()


def test_a_wall_pixel_equidistant_from_three_cells():
    lab = np.zeros((7, 7), dtype=np.int64)
    lab[3, 1], lab[1, 3], lab[3, 5] = 1, 2, 3      # each two pixels from the centre
    d1, d2, b = border_weight_map(lab, 5, 1.0, 2.0)
    assert d1[3, 3] == 4 and d2[3, 3] == 4
    assert abs(b[3, 3] - math.exp(-16.0 / 8.0)) <= 1e-15


def pair_at_offset(dy, dx, H=12, W=12, at=(2, 2)):
    """A wall pixel `at` beside cell 1, and a single pixel of cell 2 at (dy, dx) from it."""
    lab = np.zeros((H, W), dtype=np.int64)
    lab[at[0], at[1] - 1] = 1
    lab[at[0] + dy, at[1] + dx] = 2
    return lab


def test_radius_5_includes_offset_3_4_and_excludes_offset_3_5():
    d1, d2, b = border_weight_map(pair_at_offset(3, 4), 5, 10.0, 5.0)
    assert d1[2, 2] == 1 and d2[2, 2] == 25
    assert abs(b[2, 2] - 10.0 * math.exp(-36.0 / 50.0)) <= 1e-14
    d1, d2, b = border_weight_map(pair_at_offset(3, 5), 5, 10.0, 5.0)
    assert d1[2, 2] == 1 and d2[2, 2] == -1 and b[2, 2] == 0.0


def test_one_cell_all_wall_and_no_wall():
    one = np.zeros((9, 9), dtype=np.int64)
    one[3:6, 3:6] = 4
    d1, d2, b = border_weight_map(one, 3, 10.0, 1.0)
    assert (b == 0).all() and (d2 == -1).all() and d1[4, 2] == 1 and d1[0, 0] == -1 and d1[4, 4] == -1
    for lab in (np.zeros((6, 5), dtype=np.int64), np.full((6, 5), 3, dtype=np.int64)):
        d1, d2, b = border_weight_map(lab, 4, 10.0, 1.0)
        assert (b == 0).all() and (d1 == -1).all() and (d2 == -1).all()


# ---- options ----------------------------------------------------------------------------------------------------------------------
BASE = ["--name", "t", "--model", "segmentation", "--dataroot", "synthetic", "--gpu_ids", "-1"]


def parse(extra):
    from supervised_gan_amd.options import TrainOptions
    return TrainOptions().parse(BASE + extra, save=False, verbose=False)


def test_border_options_default_off_and_default_radius():
    opt = parse(["--which_model_netD", "None"])
    assert opt.border_weight is None and opt.border_radius is None and opt.border_class == 0
    for sigma, radius in ((5.0, 20), (0.2, 1), (2.6, 11), (8.0, 32), (9.0, 32)):
        opt = parse(["--which_model_netD", "None", "--border_weight", "10", str(sigma)])
        assert opt.border_weight == [10.0, sigma] and opt.border_radius == radius == min(32, math.ceil(4 * sigma))
    opt = parse(["--which_model_netD", "None", "--border_weight", "10", "5", "--border_radius", "7", "--border_class", "1"])
    assert opt.border_radius == 7 and opt.border_class == 1


def test_border_weight_is_refused_with_a_discriminator_with_sigmoid_and_with_a_bad_radius():
    with pytest.raises(AssertionError, match="--which_model_netD None"):
        parse(["--border_weight", "10", "5"])      # the default discriminator
    with pytest.raises(AssertionError, match="--which_model_netD None"):
        parse(["--which_model_netD", "n_layers", "--border_weight", "10", "5"])
    with pytest.raises(AssertionError, match="--use_sigmoid_ss"):
        parse(["--which_model_netD", "None", "--use_sigmoid_ss", "--border_weight", "10", "5"])
    with pytest.raises(AssertionError, match="--border_radius"):
        parse(["--which_model_netD", "None", "--border_weight", "10", "5", "--border_radius", "33"])
    with pytest.raises(AssertionError, match="SIGMA"):
        parse(["--which_model_netD", "None", "--border_weight", "10", "0"])

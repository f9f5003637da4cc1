"""CPU tests of the host yardsticks of the sliced Wasserstein score (util.lap_pyramid_ref, swd_descriptors_ref, swd_normalise_ref,
swd_ref, swd_draw): they pin the definition the device entries are held to -- against scipy where scipy has the same thing, and on
inputs whose answers are known -- plus the C surface of the new entries and the option checks of swd.py."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from supervised_gan_amd import util as U  # noqa: E402


def _collapse(levels):
    """The image a pyramid stands for: every level upsampled back to the finest size and added."""
    g = levels[-1]
    for lap in levels[-2::-1]:
        g = lap + U.lap_up_ref(g)
    return g


def test_pyramid_reconstructs_the_image():
    rng = np.random.RandomState(0)
    for shape in ((1, 64, 64), (3, 64, 96), (2, 48, 80), (1, 18, 34)):
        img = rng.uniform(-1, 1, shape)
        levels = U.lap_pyramid_ref(img)
        assert all(l.dtype == np.float64 for l in levels)
        # each level adds and subtracts the same up(G_{l+1}): what is left is the rounding of a handful of additions of values <= 2
        assert np.abs(_collapse(levels) - img).max() <= 8 * len(levels) * np.finfo(np.float64).eps


def test_pyramid_of_a_constant_image():
    levels = U.lap_pyramid_ref(np.full((2, 64, 96), 0.375))
    assert len(levels) == 3
    for lap in levels[:-1]:
        assert np.abs(lap).max() <= 4 * np.finfo(np.float64).eps      # the weights of every parity class of 4 g sum to 1
    assert np.abs(levels[-1] - 0.375).max() <= 4 * np.finfo(np.float64).eps


def test_pyramid_level_sizes():
    assert U.lap_level_sizes(64, 64) == [(64, 64), (32, 32), (16, 16)]
    assert U.lap_level_sizes(64, 96) == [(64, 96), (32, 48), (16, 24)]
    assert U.lap_level_sizes(48, 80) == [(48, 80), (24, 40)]          # 12 < 16: no third level
    assert U.lap_level_sizes(16, 16) == [(16, 16)] and U.lap_level_sizes(18, 34) == [(18, 34)] and U.lap_level_sizes(34, 66) == [(34, 66), (17, 33)]
    assert [l.shape for l in U.lap_pyramid_ref(np.zeros((3, 48, 80)))] == [(3, 48, 80), (3, 24, 40)]


def test_pyramid_border_rule_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    g = np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1]) / 256.0
    ramp = np.add.outer(np.arange(16.0) * 3, np.arange(16.0))[None]
    want = ndi.correlate(ramp[0], g, mode='mirror')
    assert np.abs(U.lap_down_ref(ramp)[0] - want[::2, ::2]).max() <= 1e-12
    # the interior of a ramp is reproduced; the mirrored border is not an extrapolation, so the corners differ from the ramp
    assert abs(want[8, 8] - ramp[0, 8, 8]) <= 1e-12 and abs(want[0, 0] - ramp[0, 0, 0]) > 0.1
    z = np.zeros((32, 32))
    z[::2, ::2] = ramp[0]
    assert np.abs(U.lap_up_ref(ramp)[0] - ndi.correlate(z, 4 * g, mode='mirror')).max() <= 1e-12


def test_descriptors_and_normalisation():
    rng = np.random.RandomState(1)
    levels = [rng.uniform(-1, 1, (2, 20, 24)).astype(np.float32) for _ in range(3)]
    pos = np.array([[0, 0, 0], [2, 13, 17], [1, 5, 6], [1, 5, 6]], np.int32)
    desc, mean, std = U.swd_descriptors_ref(levels, pos)
    assert desc.shape == (4, 98) and desc.dtype == np.float32
    assert desc[1, 49 + 2 * 7 + 3] == levels[2][1, 13 + 2, 17 + 3] and np.array_equal(desc[2], desc[3])
    assert np.allclose(mean, [desc[:, :49].mean(dtype=np.float64), desc[:, 49:].mean(dtype=np.float64)], rtol=0, atol=1e-15)
    assert np.allclose(std, [desc[:, :49].astype(np.float64).std(), desc[:, 49:].astype(np.float64).std()], rtol=0, atol=1e-15)
    n = U.swd_normalise_ref(desc, mean, std)
    assert n.dtype == np.float32
    assert np.abs(n.reshape(4, 2, 49).transpose(1, 0, 2).reshape(2, -1).mean(axis=1)).max() < 1e-6
    assert np.abs(n.reshape(4, 2, 49).transpose(1, 0, 2).reshape(2, -1).std(axis=1) - 1).max() < 1e-6
    # a constant channel: zero descriptors, not NaN
    flat = desc.copy()
    flat[:, 49:] = 0.25
    _, mean, std = U.swd_descriptors_ref([np.full((2, 7, 7), 0.25, np.float32)], np.zeros((1, 3), np.int32))
    assert std.tolist() == [0.0, 0.0]
    assert np.array_equal(U.swd_normalise_ref(flat, [0.0, 0.25], [1.0, 0.0])[:, 49:], np.zeros((4, 49), np.float32))
    # the sums the device accumulates give the same statistics
    s = np.concatenate([desc.reshape(4, 2, 49).astype(np.float64).sum(axis=(0, 2)), (desc.reshape(4, 2, 49).astype(np.float64) ** 2).sum(axis=(0, 2))])
    m2, s2 = U.swd_stats_from_sums(s, 4 * 49)
    d64 = desc.reshape(4, 2, 49).astype(np.float64).transpose(1, 0, 2).reshape(2, -1)
    assert np.allclose(m2, d64.mean(axis=1), rtol=0, atol=1e-15) and np.allclose(s2, d64.std(axis=1), rtol=1e-13, atol=0)


def test_swd_ref_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.RandomState(2)
    nA, nB = rng.randn(200, 49).astype(np.float32), (rng.randn(200, 49) * 1.5 + 0.3).astype(np.float32)
    _, dirs = U.swd_draw(5, 0, 1, 1, 16, 16, 49, 6)
    got = U.swd_ref(nA, nB, dirs)
    assert got.dtype == np.float64 and got.shape == (6,)
    for j in range(6):
        d = dirs[j].astype(np.float64)
        want = stats.wasserstein_distance(nA.astype(np.float64) @ d, nB.astype(np.float64) @ d)
        assert abs(got[j] - want) <= 1e-12 * max(1.0, want)


def test_swd_ref_exact_cases():
    rng = np.random.RandomState(3)
    nA = rng.randn(100, 98).astype(np.float32)
    _, dirs = U.swd_draw(1, 2, 1, 1, 16, 16, 98, 5)
    assert np.array_equal(U.swd_ref(nA, nA[rng.permutation(100)], dirs), np.zeros(5))
    a = np.arange(37, dtype=np.float32)[:, None]
    assert np.array_equal(U.swd_ref(a, a + 3, np.ones((1, 1), np.float32)), [3.0])
    assert np.array_equal(U.swd_ref(a, (a + 3)[::-1], -np.ones((1, 1), np.float32)), [3.0])


def test_swd_draw():
    pos, dirs = U.swd_draw(7, 1, 5, 16, 32, 48, 147, 64)
    pos2, dirs2 = U.swd_draw(7, 1, 5, 16, 32, 48, 147, 64)
    assert np.array_equal(pos, pos2) and np.array_equal(dirs, dirs2)
    assert pos.dtype == np.int32 and pos.shape == (80, 3) and dirs.dtype == np.float32 and dirs.shape == (64, 147)
    assert np.abs(np.sqrt((dirs.astype(np.float64) ** 2).sum(axis=1)) - 1).max() <= 1e-6
    assert np.array_equal(pos[:, 0], np.repeat(np.arange(5), 16))
    assert pos[:, 1].min() >= 0 and pos[:, 1].max() <= 32 - 7 and pos[:, 2].min() >= 0 and pos[:, 2].max() <= 48 - 7
    assert pos[:, 2].max() > 32 - 7                                      # x uses the width, not the height
    # the smallest level a patch fits: one position
    assert np.array_equal(U.swd_draw(0, 0, 2, 3, 7, 7, 49, 1)[0][:, 1:], np.zeros((6, 2), np.int32))
    other_pos, other_dirs = U.swd_draw(7, 1, 5, 16, 32, 48, 147, 64, set_index=1)
    assert np.array_equal(other_dirs, dirs) and not np.array_equal(other_pos, pos)      # one set of directions, positions per set
    assert not np.array_equal(U.swd_draw(7, 2, 5, 16, 32, 48, 147, 64)[1], dirs)
    assert not np.array_equal(U.swd_draw(8, 1, 5, 16, 32, 48, 147, 64)[1], dirs)


NEW = ("sgan_lap_pyramid", "sgan_swd_gather", "sgan_swd_workspace", "sgan_swd_distances")


def test_entry_points_are_declared_and_bound(built_lib):
    from supervised_gan_amd import _lib
    header = open(os.path.join(ROOT, "include", "sgan_hip.h")).read()
    raw = ctypes.CDLL(built_lib)
    for name in NEW:
        m = re.search(r"\b(int|int64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name + " is not declared in sgan_hip.h"
        assert hasattr(raw, name), name + " is not exported"
        assert len(m.group(2).split(",")) == len(_lib.SIGNATURES[name]), name
    assert _lib.RESTYPES["sgan_swd_workspace"] is ctypes.c_int64
    l = _lib.lib()
    # the projections of min(J, 512) directions of both sets
    assert l.sgan_swd_workspace(1000, 49, 3) >= 2 * 3 * 1000 * 4 and l.sgan_swd_workspace(1000, 49, 3) % 16 == 0
    assert l.sgan_swd_workspace(16384, 147, 4096) == 2 * 512 * 16384 * 4 and l.sgan_swd_workspace(1, 98, 1) > 0
    for bad in ((16385, 49, 8), (0, 49, 8), (64, 50, 8), (64, 196, 8), (64, 49, 0), (64, 49, 4097)):
        assert l.sgan_swd_workspace(*bad) < 0, bad
        assert b"1 <= N <= 16384" in l.sgan_last_error()
    # malformed arguments are refused before anything touches a device
    assert l.sgan_swd_distances(None, None, None, None, None, 64, 49, 8, None, None, 0, 0, None) < 0 and b"null pointer" in l.sgan_last_error()
    assert l.sgan_swd_gather(None, 64, 1, 64, 64, None, 4, None, 0, 4, None, None, None) < 0 and b"null pointer" in l.sgan_last_error()
    assert l.sgan_lap_pyramid(0, None, 64, None, 0, 1, 64, 64, None, 32, None) < 0 and b"null pointer" in l.sgan_last_error()
    p = ctypes.c_void_p(64)      # never dereferenced: the shape checks come before any launch
    assert l.sgan_lap_pyramid(0, p, 63, None, 0, 1, 63, 64, p, 32, None) < 0 and b"bad shape" in l.sgan_last_error()
    assert l.sgan_lap_pyramid(2, p, 64, None, 0, 1, 64, 64, p, 32, None) < 0 and b"mode" in l.sgan_last_error()
    assert l.sgan_lap_pyramid(1, p, 64, p, 31, 1, 64, 64, p, 64, None) < 0 and b"pitch" in l.sgan_last_error()
    assert l.sgan_swd_gather(p, 64, 4, 64, 64, p, 4, p, 0, 4, p, p, None) < 0 and b"bad shape" in l.sgan_last_error()
    assert l.sgan_swd_gather(p, 64, 1, 64, 64, p, 4, p, 2, 5, p, p, None) < 0 and b"rows" in l.sgan_last_error()
    assert l.sgan_swd_distances(p, p, p, p, p, 16385, 49, 8, p, p, 1 << 40, 0, None) < 0 and b"16384" in l.sgan_last_error()
    assert l.sgan_swd_distances(p, p, p, p, p, 64, 49, 8, p, p, 16, 0, None) < 0 and b"workspace" in l.sgan_last_error()
    assert l.sgan_swd_distances(p, p, p, p, p, 64, 49, 8, p, p, 1 << 20, 3, None) < 0 and b"variant" in l.sgan_last_error()


def test_driver_refusals(tmp_path, capsys):
    import swd
    base = ["--name", "x", "--dataroot", "synthetic", "--gpu_ids", "-1", "--checkpoints_dir", str(tmp_path), "--which_channel", "rg"]
    for extra, word in ((["--model", "fcgan", "--how_many", "129", "--swd_patches", "128"], "16384"),
                        (["--model", "segmentation"], "--model"),
                        (["--model", "fcgan", "--swd_channels", "2"], "--swd_channels"),
                        (["--model", "fcgan", "--swd_dirs", "4097"], "4096")):
        with pytest.raises(SystemExit) as e:
            swd.main(base + extra)
        assert e.value.code == 2
        assert word in capsys.readouterr().err
    assert "own" in swd.__doc__ and "brightness or contrast" in swd.__doc__

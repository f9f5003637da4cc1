"""Host tests of the region statistics: util.region_table (the yardstick of sgan_region_stats) against a plain per-region loop,
util.region_props on shapes with closed forms, the declarations of the device entry points, and tools/shape_compare.py."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _restated(free, ordinal=0):
    """The same 16 columns, one region at a time over its find_objects slice, in Python integers."""
    H, W = free.shape
    lab, k = ndimage.label(free, structure=np.ones((3, 3)))
    rows = []
    for i, (sy, sx) in enumerate(ndimage.find_objects(lab), start=1):
        area = sxx = syy = sxy = sx1 = sy1 = boundary = edges = 0
        xs, ys, root = [], [], None
        for y in range(sy.start, sy.stop):
            for x in range(sx.start, sx.stop):
                if lab[y, x] != i:
                    continue
                if root is None:
                    root = y * W + x
                out = sum(1 for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1))
                          if not (0 <= yy < H and 0 <= xx < W and lab[yy, xx] == i))
                area, sx1, sy1, sxx, syy, sxy = area + 1, sx1 + x, sy1 + y, sxx + x * x, syy + y * y, sxy + x * y
                boundary, edges = boundary + (out > 0), edges + out
                xs.append(x)
                ys.append(y)
        rows.append([area, min(xs), max(xs), min(ys), max(ys), sx1, sy1, sxx, syy, sxy, boundary, root, ordinal, edges, 0, 0])
    assert len(rows) == k
    return np.array(rows, dtype=np.int64).reshape(k, 16)


def _masks():
    rng = np.random.default_rng(5)
    for density, (H, W) in ((0.3, (96, 80)), (0.5, (96, 80)), (0.7, (96, 80)), (0.5, (1, 70)), (0.5, (37, 53)), (0.4, (7, 1))):
        yield "noise %.1f %dx%d" % (density, H, W), rng.random((H, W)) >= density
    yield "all wall", np.zeros((20, 31), bool)
    yield "all free", np.ones((33, 18), bool)
    lattice = np.zeros((31, 40), bool)
    lattice[::2, ::2] = True
    yield "lattice", lattice


def test_region_table_equals_a_per_region_loop():
    from supervised_gan_amd.util import REGION_COLS, region_table
    assert len(REGION_COLS) == 16
    for ordinal, (name, free) in enumerate(_masks()):
        got, want = region_table(free, ordinal), _restated(free, ordinal)
        assert got.dtype == np.int64 and got.shape == want.shape, name
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:5].tolist())
        assert np.all(np.diff(got[:, 11]) > 0)                                   # scipy's order is the order of the roots
        if name == "all wall":
            assert got.shape == (0, 16)
        if name == "all free":
            assert got.shape == (1, 16) and got[0, 0] == 33 * 18 and got[0, 13] == 2 * (33 + 18) and got[0, 10] == 2 * (33 + 18) - 4
        if name == "lattice":
            assert got.shape == (16 * 20, 16) and (got[:, 0] == 1).all() and (got[:, 13] == 4).all()
    other = region_table(np.ones((3, 3), np.float32))                            # any array form; the ordinal defaults to 0
    assert other.tolist() == [[9, 0, 2, 0, 2, 9, 9, 15, 15, 9, 8, 0, 0, 12, 0, 0]]


def _props_of(free):
    from supervised_gan_amd.util import region_props, region_table
    return region_props(region_table(free), free.shape)


def test_region_props_closed_forms():
    from supervised_gan_amd.util import REGION_PROPS
    close = lambda got, want: np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)      # noqa: E731
    # an a x b rectangle (a along x), once wide and once tall, away from the origin and from the border
    for a, b, x0, y0 in ((7, 3, 30, 40), (4, 9, 100, 5), (5, 5, 1, 1)):
        m = np.zeros((150, 160), bool)
        m[y0:y0 + b, x0:x0 + a] = True
        p = _props_of(m)
        assert tuple(p) == REGION_PROPS and all(v.shape == (1,) for v in p.values())
        close(p['area'], a * b)
        close(p['centroid_x'], x0 + (a - 1) / 2)
        close(p['centroid_y'], y0 + (b - 1) / 2)
        close(p['extent'], 1.0)
        close(p['equivalent_diameter'], math.sqrt(4 * a * b / math.pi))
        close(p['mu20'], a * a / 12)
        close(p['mu02'], b * b / 12)
        assert p['mu11'][0] == 0.0
        close(p['major_axis_length'], 4 * math.sqrt(max(a, b) ** 2 / 12))
        close(p['minor_axis_length'], 4 * math.sqrt(min(a, b) ** 2 / 12))
        if a == b:
            assert p['eccentricity'][0] == 0.0
        else:
            close(p['eccentricity'], math.sqrt(1 - (min(a, b) / max(a, b)) ** 2))
        want_angle = 0.0 if a >= b else math.pi / 2                              # the major axis along x, or along y
        assert p['orientation'][0] == want_angle
        close(p['compactness'], 4 * math.pi * a * b / (2 * (a + b)) ** 2)
        assert not p['touches_border'][0]
    # a single pixel, in a corner
    m = np.zeros((6, 9), bool)
    m[5, 8] = True
    p = _props_of(m)
    close(p['centroid_x'], 8.0)
    close(p['centroid_y'], 5.0)
    close(p['mu20'], 1 / 12)
    close(p['mu02'], 1 / 12)
    close(p['major_axis_length'], 4 * math.sqrt(1 / 12))
    close(p['minor_axis_length'], 4 * math.sqrt(1 / 12))
    close(p['equivalent_diameter'], math.sqrt(4 / math.pi))
    close(p['compactness'], math.pi / 4)
    assert p['eccentricity'][0] == 0.0 and p['orientation'][0] == 0.0 and p['extent'][0] == 1.0 and p['touches_border'][0]
    # a diagonal line of n pixels (8-connected): x = x0 + i, y = y0 + i, and its mirror image
    n = 11
    for sign in (1, -1):
        m = np.zeros((40, 40), bool)
        for i in range(n):
            m[20 + i, 15 + sign * i] = True
        p = _props_of(m)
        close(p['area'], n)
        close(p['mu20'], n * n / 12)
        close(p['mu02'], n * n / 12)
        close(p['mu11'], sign * (n * n - 1) / 12)
        close(p['major_axis_length'], 4 * math.sqrt((2 * n * n - 1) / 12))
        close(p['minor_axis_length'], 4 * math.sqrt(1 / 12))
        close(p['eccentricity'], math.sqrt(1 - 1 / (2 * n * n - 1)))
        close(p['orientation'], sign * math.pi / 4)
        close(p['extent'], 1 / n)
        close(p['compactness'], 4 * math.pi * n / (4 * n) ** 2)
        assert not p['touches_border'][0]
    # the four borders
    for y, x in ((0, 3), (3, 0), (5, 3), (3, 8)):
        m = np.zeros((6, 9), bool)
        m[y, x] = True
        assert _props_of(m)['touches_border'][0]
    assert all(v.shape == (0,) for v in _props_of(np.zeros((4, 4), bool)).values())


def test_entry_points_are_declared_and_bound(built_lib):
    from supervised_gan_amd import _lib
    header = open(os.path.join(ROOT, "include", "sgan_hip.h")).read()
    assert re.search(r"\bint64_t\s+sgan_region_stats_workspace\s*\(\s*int32_t H,\s*int32_t W\s*\)\s*;", header)
    assert re.search(r"\bint\s+sgan_region_stats\s*\(\s*const int32_t\* labels,\s*int32_t H,\s*int32_t W,\s*int64_t\* table,\s*int32_t capacity,\s*"
                     r"int32_t\* cursor,\s*void\* workspace,\s*int64_t workspace_bytes,\s*int32_t\* dev_err,\s*void\* stream\s*\)\s*;", header)
    assert len(_lib.SIGNATURES["sgan_region_stats"]) == 10 and len(_lib.SIGNATURES["sgan_region_stats_workspace"]) == 2
    assert _lib.RESTYPES["sgan_region_stats_workspace"] is ctypes.c_int64
    l = _lib.lib()
    # ranks for every pixel, and a staging row of 16 int64 for each of the ceil(H / 2) ceil(W / 2) regions an image can have
    assert l.sgan_region_stats_workspace(64, 64) >= 4 * 64 * 64 + 128 * 32 * 32 and l.sgan_region_stats_workspace(64, 64) % 16 == 0
    assert l.sgan_region_stats_workspace(1, 1) > 0 and l.sgan_region_stats_workspace(65, 17) >= 4 * 65 * 17 + 128 * 33 * 9
    assert l.sgan_region_stats_workspace(0, 5) < 0 and l.sgan_region_stats_workspace(5, -1) < 0
    assert l.sgan_region_stats_workspace(1 << 15, 1 << 15) < 0                   # sgan_ccl_label's limit, H W < 2^30
    assert b"bad shape" in l.sgan_last_error()
    assert l.sgan_region_stats_workspace(65536, 16383) > 0 and l.sgan_region_stats_workspace(65537, 1) < 0      # the documented limit on a side
    # malformed arguments are refused before anything touches a device
    assert l.sgan_region_stats(None, 8, 8, None, 4, None, None, 0, None, None) < 0 and b"null pointer" in l.sgan_last_error()


def _write_npz(path, areas, per_image, seed):
    from supervised_gan_amd.util import REGION_PROPS
    rng = np.random.default_rng(seed)
    props = rng.random((len(areas), len(REGION_PROPS)))
    props[:, REGION_PROPS.index('area')] = areas
    props[:, REGION_PROPS.index('touches_border')] = 0.0
    table = np.zeros((len(areas), 16), np.int64)
    table[:, 0] = areas
    table[:, 12] = np.repeat(np.arange(len(per_image)), per_image)
    np.savez(path, table=table, props=props, prop_names=np.array(REGION_PROPS), images=np.int64(len(per_image)), shape=np.array([64, 64]))


def test_shape_compare_tool(tmp_path):
    a, b = str(tmp_path / "a.npz"), str(tmp_path / "b.npz")
    _write_npz(a, [1, 2, 3, 4, 5, 6], [2, 4], 1)
    _write_npz(b, [11, 12, 13, 14, 15, 16], [3, 3], 2)
    tool = os.path.join(ROOT, "tools", "shape_compare.py")
    same = subprocess.run([sys.executable, tool, a, a], capture_output=True, text=True, timeout=120)
    assert same.returncode == 0, same.stderr[-2000:]
    rows = [l.split() for l in same.stdout.splitlines() if l and not l.startswith("#")]
    names = [r[0] for r in rows]
    assert "area" in names and "eccentricity" in names and "compactness" in names and "regions_per_image" in names
    assert "touches_border" not in names
    assert all(float(r[1]) == 0.0 and float(r[2]) == 0.0 for r in rows), same.stdout
    diff = subprocess.run([sys.executable, tool, a, b], capture_output=True, text=True, timeout=120)
    assert diff.returncode == 0, diff.stderr[-2000:]
    got = {r[0]: (float(r[1]), float(r[2])) for r in (l.split() for l in diff.stdout.splitlines() if l and not l.startswith("#"))}
    assert got["area"] == (1.0, 10.0)                                            # disjoint samples: KS 1, every quantile 10 apart
    assert got["regions_per_image"] == (0.5, 1.0)                                # {2, 4} against {3, 3}

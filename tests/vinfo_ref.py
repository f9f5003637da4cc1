"""Shared by the VInfo tests: an independent restatement of the information score from explicit probability tables, and the boundary
maps the tests score."""
import functools
import math

import numpy as np

STRUCT8 = np.ones((3, 3), dtype=np.int32)


def entropy(labels):
    """-sum p ln p of the empirical distribution of the rows of `labels` ([m] or [m, k] integers)."""
    _, counts = np.unique(labels, axis=0, return_counts=True)
    p = counts / counts.sum()
    return float(-(p * np.log(p)).sum())


def vinfo_restated(s, t):
    """VInfo of prediction s against truth t ([H, W], wall where > 0.5) written as the definition reads: label both maps, keep the
    pixels of truth regions, give every kept pixel on prediction wall a fresh prediction label of its own, then take the entropies of
    the explicit tables.  Returns (VInfo, H_S, H_T, I); NaN without a truth pixel, 1 when both partitions are one region."""
    from scipy import ndimage
    t_lab, _ = ndimage.label(~(np.asarray(t) > 0.5), structure=STRUCT8)
    s_lab, _ = ndimage.label(~(np.asarray(s) > 0.5), structure=STRUCT8)
    keep = t_lab > 0
    tl, sl = t_lab[keep].astype(np.int64), s_lab[keep].astype(np.int64)
    if tl.size == 0:
        return (float("nan"),) * 4
    on_wall = sl == 0
    sl[on_wall] = int(s_lab.max()) + 1 + np.arange(int(on_wall.sum()))
    h_s, h_t, h_st = entropy(sl), entropy(tl), entropy(np.stack([tl, sl], axis=1))
    info = h_s + h_t - h_st
    if h_s + h_t == 0.0:            # p = 1 in both tables: -1 ln 1 is an exact 0
        return 1.0, h_s, h_t, info
    return 2.0 * info / (h_s + h_t), h_s, h_t, info


def cell_map(H, W, period, wall, dy=0, dx=0):
    """Cells of `period` - `wall` free pixels between walls `wall` pixels thick, the grid shifted by (dy, dx)."""
    y, x = np.mgrid[0:H, 0:W]
    return ((((y + dy) % period) < wall) | (((x + dx) % period) < wall)).astype(np.float32)


def host_maps(count=50, seed=2012):
    """(name, prediction, truth) pairs up to 96 x 96: Bernoulli walls on both sides of the percolation threshold, and cell grids
    against a shifted copy of themselves with some walls broken and some pixels flipped."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        H, W = (int(v) for v in rng.integers(1, 97, size=2))
        if k % 2 == 0:
            ds, dt = rng.uniform(0.1, 0.65, size=2)
            s, t = (rng.random((H, W)) < ds).astype(np.float32), (rng.random((H, W)) < dt).astype(np.float32)
            out.append(("bernoulli%d_%dx%d_%.2f_%.2f" % (k, H, W, ds, dt), s, t))
        else:
            period, wall = int(rng.integers(4, 14)), int(rng.integers(1, 3))
            t = cell_map(H, W, period, wall)
            s = cell_map(H, W, period, wall, int(rng.integers(0, 3)), int(rng.integers(0, 3)))
            s[rng.random((H, W)) < 0.03] = 0.0          # broken walls merge cells
            s[rng.random((H, W)) < 0.02] = 1.0          # stray membrane: singletons
            out.append(("cells%d_%dx%d_p%d_w%d" % (k, H, W, period, wall), s, t))
    return out


DEVICE_SIZES = [(1, 1), (1, 64), (64, 1), (3, 65), (17, 130), (48, 80), (130, 70)]      # (H, W); CCL tiles are 16 rows x 64 columns


@functools.lru_cache(maxsize=None)
def device_pairs(H, W):
    """{name: (prediction, truth)} of one size for the device tests, computed once and shared (read-only)."""
    rng = np.random.default_rng(100 * H + W)
    y, x = np.mgrid[0:H, 0:W]
    free, wall = np.zeros((H, W), np.float32), np.ones((H, W), np.float32)
    checker = ((y + x) % 2 == 1).astype(np.float32)
    b30, b50 = ((rng.random((H, W)) < d).astype(np.float32) for d in (0.3, 0.5))
    b30b = (rng.random((H, W)) < 0.3).astype(np.float32)
    cells = cell_map(H, W, 9, 1)                        # 8-pixel cells, 1-pixel walls
    pairs = {"both_free": (free, free), "prediction_wall": (wall, free), "truth_wall": (free, wall), "checkerboard": (checker, checker),
             "checkerboard_vs_free": (checker, free), "bernoulli30": (b30, b30b), "bernoulli50": (b50, b30), "bernoulli30_vs_50": (b30, b50),
             "cells_shift2": (cell_map(H, W, 9, 1, 2, 2), cells), "cells_vs_bernoulli30": (b30, cells)}
    for s, t in pairs.values():
        s.setflags(write=False)
        t.setflags(write=False)
    return pairs


def hand_2x4():
    """A 2 x 4 pair with one singleton, and its score from -sum p ln p written out.
        truth       0 0 1 0      regions A = 4 pixels, B = 2 pixels; m = 6
                    0 0 1 0
        prediction  0 1 0 0      one region (8-connected round the wall pixel); the wall pixel lies in A: a singleton
                    0 0 0 0
    truth partition {4, 2}, prediction partition {5, 1}, joint {3 (A, region), 1 (A, singleton), 2 (B, region)}."""
    t = np.array([[0, 0, 1, 0], [0, 0, 1, 0]], np.float32)
    s = np.array([[0, 1, 0, 0], [0, 0, 0, 0]], np.float32)
    h = lambda *c: -sum(v / 6 * math.log(v / 6) for v in c)      # noqa: E731
    h_t, h_s, h_st = h(4, 2), h(5, 1), h(3, 1, 2)
    return s, t, 2 * (h_s + h_t - h_st) / (h_s + h_t)

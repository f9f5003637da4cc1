"""The cases the topology tests share (tests/test_topo_host.py, tests/test_hip_topo.py): float32 planes in the form the trainers hand
to ops.topo_accumulate (wall where > 0.5), built from a fixed seed, once per shape, and the host yardstick's counts of every pair,
computed once.

CASES are (H, W, window, stride): the smallest window, partial strips with overlapping windows, a window clamped to H, one full-size
window, overlapping full-size windows, and an odd window that straddles the 32-bit halves of a row mask."""
import functools

import numpy as np

CASES = ((16, 24, 8, 8), (33, 47, 16, 8), (5, 70, 64, 64), (64, 64, 64, 64), (128, 128, 64, 32), (96, 80, 33, 17))
NAMES = ("noise30", "noise50", "noise70", "cells", "cells_punched", "all_wall", "all_free", "serpentine", "checkerboard", "rings", "diagonals")
# (prediction, truth)
PAIRS = (("noise30", "noise50"), ("noise70", "noise50"), ("cells_punched", "cells"), ("all_wall", "cells"), ("all_free", "cells"),
         ("cells", "all_free"), ("serpentine", "checkerboard"), ("checkerboard", "serpentine"), ("rings", "diagonals"),
         ("diagonals", "rings"), ("noise50", "noise50"))


def serpentine(H, W):
    """One wall component one pixel wide that fills the plane: every other row, joined at alternating ends."""
    p = np.zeros((H, W), dtype=np.float32)
    p[0::2] = 1.0
    for y in range(1, H, 2):
        p[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1.0
    return p


def cells(H, W, period=11, shift=0):
    yy, xx = np.mgrid[0:H, 0:W]
    return ((((yy + shift) % period) < 2) | (((xx + shift) % period) < 2)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def planes(H, W):
    """name -> float32 [H, W]: the named planes of one shape (read-only, shared)."""
    rng = np.random.default_rng(7000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    out = {"noise%d" % d: (rng.random((H, W)) < d / 100.0).astype(np.float32) for d in (30, 50, 70)}
    out["cells"] = cells(H, W)
    punched = cells(H, W, shift=1)
    punched[rng.random((H, W)) < 0.08] = 0.0      # gaps in the walls: cells merge, walls fall apart
    out["cells_punched"] = punched
    out["all_wall"] = np.ones((H, W), dtype=np.float32)
    out["all_free"] = np.zeros((H, W), dtype=np.float32)
    out["serpentine"] = serpentine(H, W)
    out["checkerboard"] = ((yy + xx) % 2).astype(np.float32)
    ring = np.minimum(np.minimum(yy, H - 1 - yy), np.minimum(xx, W - 1 - xx))      # the distance to the plane's edge
    out["rings"] = (ring % 3 == 1).astype(np.float32)                               # nested one-pixel rings, two free pixels apart
    out["diagonals"] = ((yy + xx) % 5 == 0).astype(np.float32)
    for p in out.values():
        p.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want_betti(H, W, window, stride, s_name, t_name):
    """The first seven integers of util.topo_counts of one pair (the windowed part: no thinned planes), computed once."""
    from supervised_gan_amd.util import topo_counts
    p = planes(H, W)
    return topo_counts(p[s_name], p[t_name], window, stride)[:7].tolist()

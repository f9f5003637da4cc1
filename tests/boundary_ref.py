"""The cases the boundary tests share (tests/test_boundary_host.py, tests/test_hip_boundary.py): float32 planes in the form the
trainers hand to ops.edt_sq (wall where > 0.5), built from a fixed seed, once per shape.

Shapes: 1 x 1, a single row and a single column, odd sizes, and sizes one past every tile and segment edge of the kernels (32-row
segments, 64-lane waves, 256-pixel tiles); CHUNK_SHAPES are one past one and two of the 2048-column chunks the row pass stages, run
on a few planes only (the host yardstick is O(H W^2)); BIG is the one 512 x 512 case of the sparse and noise tests."""
import functools

import numpy as np

SHAPES = ((1, 1), (1, 67), (67, 1), (37, 53), (64, 64), (65, 130), (130, 65), (96, 257))
CHUNK_SHAPES = ((3, 2049), (2, 4500))
CHUNK_NAMES = ("corner_tl", "corner_br", "centre", "sparse", "dense", "last_column")
BIG = (512, 512)
BIG_NAMES = ("sparse", "dense")


def _plane(H, W, ys, xs):
    p = np.zeros((H, W), dtype=np.float32)
    p[ys, xs] = 1.0
    return p


@functools.lru_cache(maxsize=None)
def planes(H, W):
    """name -> float32 [H, W]: the named planes of one shape (read-only, shared)."""
    rng = np.random.default_rng(1000 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    out = {"no_wall": np.zeros((H, W), dtype=np.float32),
           "all_wall": np.ones((H, W), dtype=np.float32),
           "corner_tl": _plane(H, W, 0, 0), "corner_tr": _plane(H, W, 0, W - 1),
           "corner_bl": _plane(H, W, H - 1, 0), "corner_br": _plane(H, W, H - 1, W - 1),
           "centre": _plane(H, W, H // 2, W // 2),
           # two wall pixels at the same distance from the pixels between them (the two ends of the middle row or column)
           "equidistant": _plane(H, W, [H // 2, H // 2], [0, W - 1]) if W >= H else _plane(H, W, [0, H - 1], [W // 2, W // 2]),
           "checkerboard": ((yy + xx) % 2).astype(np.float32),
           "sparse": (rng.random((H, W)) < 1.0 / 200).astype(np.float32),
           "dense": (rng.random((H, W)) < 0.3).astype(np.float32),
           "last_row": _plane(H, W, H - 1, slice(None)),
           "last_column": _plane(H, W, slice(None), W - 1)}
    # values that must read as not wall (NaN, exactly 0.5, just below, negative, -inf) around a few that are wall (just above 0.5, inf)
    odd = rng.choice(np.array([np.nan, 0.5, 0.49999997, -1.0, -np.inf, 0.0], dtype=np.float32), size=(H, W))
    wall = rng.random((H, W)) < 0.05
    odd[wall] = rng.choice(np.array([0.50000006, 1.0, np.inf, 7.0], dtype=np.float32), size=int(wall.sum()))
    out["nan_and_half"] = odd.astype(np.float32)
    for p in out.values():
        p.setflags(write=False)
    return out


NAMES = ("no_wall", "all_wall", "corner_tl", "corner_tr", "corner_bl", "corner_br", "centre", "equidistant", "checkerboard", "sparse", "dense",
         "last_row", "last_column", "nan_and_half")
# (prediction, truth) pairs for the counts: both orders of empty against non-empty, both empty, near and far walls
PAIRS = (("dense", "sparse"), ("sparse", "dense"), ("no_wall", "sparse"), ("sparse", "no_wall"), ("no_wall", "no_wall"),
         ("corner_tl", "corner_br"), ("checkerboard", "all_wall"), ("centre", "equidistant"), ("nan_and_half", "last_row"),
         ("last_column", "dense"), ("all_wall", "all_wall"))


@functools.lru_cache(maxsize=None)
def want_edt(H, W, name):
    """util.edt_sq of one plane, computed once (read-only)."""
    from supervised_gan_amd.util import edt_sq
    e = edt_sq(planes(H, W)[name])
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def want_counts(H, W, s_name, t_name):
    """util.boundary_counts of one (prediction, truth) pair, computed once: (80 ints, 4 floats)."""
    from supervised_gan_amd.util import boundary_counts
    p = planes(H, W)
    counts, sums = boundary_counts(p[s_name], p[t_name])
    return counts.tolist(), sums.tolist()


def sums_close(got, want, counts):
    """The three fp64 sums against the yardstick's correctly rounded ones: max(2, n) 2^-52 relative, n the number of terms -- each term
    is one correctly rounded sqrt (half an ulp of the term), and n terms added in any order add at most (n - 1) 2^-53 relative."""
    terms = (int(counts[68]), int(counts[69]), int(counts[67]))
    return all(abs(g - w) <= max(2, n) * 2.0 ** -52 * abs(w) for g, w, n in zip(got[:3], want[:3], terms)) and got[3] == 0.0

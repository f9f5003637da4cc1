"""The case tables of the resampling parity tests (numpy only): Gaussian pre-filter, x2 bilinear upsampling, label pyramid.
tests/test_resample_ref_host.py checks the reference on them on the CPU, tests/test_hip_resample*.py run them on the GPU.

Each case is the smallest shape that reaches the edge named beside it; all data comes from a seeded RandomState.  The only large
cases are the GRID ones: one per kernel whose launch code caps its grid, just past cap * 256 work items so that the grid-stride loop
takes its second stride.  References are computed once per case and process (`ref`), and nothing changes them afterwards."""
import collections
import functools

import numpy as np

import resample_ref as R

PADV_IN, PADV_GRAD, PADV_BASE = 0.5, -0.75, 1.25      # what the padding channels of the inputs, gradients and bases hold (never 0)

# ---- Gaussian ------------------------------------------------------------------------------------------------------------------------
GEOMS = {                     # (k, pad, s)
    "k5s2": (5, 2, 2),        # production, scale 2
    "k9s4": (9, 4, 4),        # production, scale 4
    "k5s3": (5, 2, 3),        # s odd
    "k13s6": (13, 6, 6),      # the multi forward walks taps in chunks of 9: a second, partial chunk
    "k3s1": (3, 1, 1),        # every tap reaches every pixel in the adjoint
    "k4s2": (4, 1, 2),        # even k
    "k7s3p0": (7, 0, 3),      # no padding; trailing rows / columns no output reads (gradient exactly 0).  Single-job only.
}
SINGLE_ONLY = {"k7s3p0"}
IMAGES = {"1x1": (1, 1), "3x6": (3, 6), "37x41": (37, 41), "20x20": (20, 20)}      # 1x1, 3x6: smaller than the padding, Ho = 1
CHANS = {"c4r1": (4, 1), "c4r3": (4, 3), "c4r4": (4, 4), "c8r5": (8, 5), "c16r16": (16, 16)}      # (stored C, Creal)

# (geometry, image, channels, dense taps, sliced buffers, accumulate)
GAUSS_CROSS = [
    ("k5s2", "1x1", "c4r1", False, False, False), ("k5s2", "3x6", "c4r3", True, True, True), ("k5s2", "37x41", "c8r5", True, False, False),
    ("k5s2", "20x20", "c16r16", False, True, True), ("k5s2", "37x41", "c4r4", False, True, False),
    ("k9s4", "1x1", "c4r3", True, False, False), ("k9s4", "3x6", "c8r5", False, True, False), ("k9s4", "37x41", "c4r3", True, True, True),
    ("k9s4", "20x20", "c16r16", True, False, False),
    ("k5s3", "1x1", "c8r5", False, True, True), ("k5s3", "3x6", "c4r4", False, False, False), ("k5s3", "37x41", "c8r5", True, True, True),
    ("k5s3", "20x20", "c4r1", True, False, False),
    ("k13s6", "1x1", "c4r4", False, False, True), ("k13s6", "3x6", "c4r3", True, True, False), ("k13s6", "37x41", "c16r16", True, False, True),
    ("k13s6", "20x20", "c8r5", False, False, False),
    ("k3s1", "1x1", "c8r5", False, False, True), ("k3s1", "3x6", "c16r16", True, True, False), ("k3s1", "37x41", "c4r3", False, False, False),
    ("k3s1", "20x20", "c4r1", True, False, True),
    ("k4s2", "3x6", "c4r3", False, False, True), ("k4s2", "37x41", "c8r5", True, False, False), ("k4s2", "20x20", "c16r16", False, True, False),
    ("k7s3p0", "37x41", "c4r3", True, True, False), ("k7s3p0", "20x20", "c8r5", False, False, True),
]

GaussCase = collections.namedtuple("GaussCase", "name k pad s H W Ho Wo C Creal dense sliced acc x taps R base grid")


def dense_weight(taps):
    """(flat weight, g_chan_stride): the taps as the diagonal of a dense [nc, nc, k, k] weight whose other entries are NaN."""
    nc, k, _ = taps.shape
    w = np.full((nc, nc, k, k), np.nan, dtype=np.float32)
    w[np.arange(nc), np.arange(nc)] = taps
    return w.reshape(-1), (nc + 1) * k * k


def make_taps(rng, Creal, k):
    """Different on every channel, not symmetric under transpose or a flip of either axis, both signs."""
    return (rng.standard_normal((Creal, k, k)) * 0.3 + 0.1).astype(np.float32)


def _gauss_data(seed, k, pad, s, H, W, C, Creal):
    rng = np.random.RandomState(seed)
    Ho, Wo = R.gauss_out_size(H, k, pad, s), R.gauss_out_size(W, k, pad, s)
    assert Ho >= 1 and Wo >= 1
    x = np.full((H, W, C), PADV_IN, dtype=np.float32)
    x[..., :Creal] = (rng.standard_normal((H, W, Creal)) * 1.5 + 0.3).astype(np.float32)
    g = np.full((Ho, Wo, C), PADV_GRAD, dtype=np.float32)
    g[..., :Creal] = rng.standard_normal((Ho, Wo, Creal)).astype(np.float32)
    base = np.full((H, W, C), PADV_BASE, dtype=np.float32)
    base[..., :Creal] = (rng.standard_normal((H, W, Creal)) * 2.0 - 0.5).astype(np.float32)
    return Ho, Wo, x, make_taps(rng, Creal, k), g, base


def gauss_case(i, geom, image, chans, dense, sliced, acc, grid=None):
    k, pad, s = GEOMS[geom]
    (H, W), (C, Creal) = (IMAGES[image] if isinstance(image, str) else image), (CHANS[chans] if isinstance(chans, str) else chans)
    Ho, Wo, x, taps, g, base = _gauss_data(100 + i, k, pad, s, H, W, C, Creal)
    name = f"{geom}-{H}x{W}-c{C}r{Creal}" + ("-dense" if dense else "") + ("-sliced" if sliced else "") + ("-acc" if acc else "")
    return GaussCase(("grid-" if grid else "") + name, k, pad, s, H, W, Ho, Wo, C, Creal, dense, sliced, acc, x, taps, g, base, grid)


GAUSS = [gauss_case(i, *c) for i, c in enumerate(GAUSS_CROSS)]
GAUSS_MULTI_OK = [c for c in GAUSS if c.k <= 3 * c.s and (c.k, c.pad, c.s) != GEOMS["k7s3p0"]]

# Grid caps, read off csrc/sgan_ew.hip: sgan_gauss_down_fwd and sgan_gauss_down_bwd `if (blocks > 4096) blocks = 4096;` over
# cdiv(Ho Wo C/4, 256) resp. cdiv(H W C/4, 256); sgan_gauss_down_multi_bwd the same 4096 over the image; sgan_gauss_down_multi_fwd
# `if (blocks > 2048) blocks = 2048;` over the largest job's cdiv(Ho Wo C/4, 256).  C = 1024 (the k = 3 taps still fit the LDS limit
# k k C 4 <= 60000) makes 256 quads per pixel: 4096 * 256 / 256 = 4096 pixels is the cap, 64 x 65 = 4160 a shape just past it
# (not a multiple of the cap, so the second stride is a partial one); 2048 pixels for the multi forward, 32 x 65 = 2080.
GAUSS_GRID = gauss_case(900, "k3s1", (64, 65), (1024, 1021), False, False, True, grid="4096 x 256 < 64 * 65 * 256")
GAUSS_GRID_MULTI_FWD = gauss_case(901, "k3s1", (32, 65), (1024, 1021), False, False, False, grid="2048 x 256 < 32 * 65 * 256")

# multi-job sets: (image, channels, dense, sliced, [geometries]); five jobs: the wrapper launches 4 + 1, the second accumulating
MULTI_CROSS = [
    ("37x41", "c8r5", False, False, ["k9s4"]),
    ("37x41", "c4r3", True, False, ["k5s2", "k9s4"]),                    # what the multi-scale discriminators launch
    ("20x20", "c16r16", False, True, ["k5s3", "k3s1", "k13s6"]),
    ("37x41", "c8r5", True, True, ["k13s6", "k4s2", "k5s2", "k9s4"]),
    ("3x6", "c8r5", False, False, ["k5s2", "k9s4", "k5s3", "k13s6", "k3s1"]),
    ("20x20", "c4r3", False, True, ["k4s2", "k3s1", "k9s4", "k5s3", "k5s2"]),
]
MultiCase = collections.namedtuple("MultiCase", "name H W C Creal dense sliced jobs x base")      # jobs: GaussCase (x shared, base unused)


def multi_case(i, image, chans, dense, sliced, geoms):
    (H, W), (C, Creal) = IMAGES[image], CHANS[chans]
    jobs = [gauss_case(500 + 10 * i + j, g, image, chans, dense, sliced, False) for j, g in enumerate(geoms)]
    x, base = jobs[0].x, jobs[0].base
    jobs = [j._replace(name=f"set{i}.{n}-{j.name}", x=x, base=None) for n, j in enumerate(jobs)]
    return MultiCase(f"{len(geoms)}jobs-{H}x{W}-c{C}r{Creal}" + ("-dense" if dense else "") + ("-sliced" if sliced else ""), H, W, C, Creal,
                     dense, sliced, jobs, x, base)


MULTI = [multi_case(i, *c) for i, c in enumerate(MULTI_CROSS)]

# ---- bilinear ------------------------------------------------------------------------------------------------------------------------
# (H, W, C, sliced, statistics: none | plain | sliced)            reaches
BIL_CROSS = [
    (1, 1, 4, False, "plain"), (1, 1, 8, True, "none"), (1, 1, 64, False, "sliced"),          # every clamp at once
    (1, 5, 4, True, "sliced"), (1, 5, 8, False, "plain"), (1, 5, 64, True, "none"),           # H = 1
    (6, 1, 4, False, "none"), (6, 1, 8, True, "sliced"), (6, 1, 64, False, "plain"),          # W = 1
    (2, 3, 4, True, "plain"), (2, 3, 8, False, "sliced"), (2, 3, 64, True, "none"),           # no interior pixel
    (5, 7, 4, False, "sliced"), (5, 7, 8, True, "plain"), (5, 7, 64, False, "none"),          # interior and border, > 1 workgroup at C = 64
    (2, 2, 1024, False, "plain"), (2, 2, 1024, True, "sliced"),                               # one channel quad per thread of the workgroup
]
BIL_BWD_EXTRA = [(5, 7, 12, False, "none"), (1, 1, 12, True, "none")]                         # C = 12: the backward accepts it
BilCase = collections.namedtuple("BilCase", "name H W C sliced stats x R stats0 grid")


def bil_case(i, H, W, C, sliced, stats, grid=None):
    rng = np.random.RandomState(2000 + i)
    x = (rng.standard_normal((H, W, C)) * 1.5 + 0.3).astype(np.float32)
    g = rng.standard_normal((2 * H, 2 * W, C)).astype(np.float32)
    # non-zero sums already in the arena, small beside the sums added so that the bound N 2^-53 sum |v| also covers the last add
    stats0 = np.concatenate([-0.25 - 0.0005 * np.arange(C), 0.5 + 0.0005 * np.arange(C)]) if stats != "none" else None
    name = f"{H}x{W}-c{C}" + ("-sliced" if sliced else "") + ("" if stats == "none" else f"-stats_{stats}")
    return BilCase(("grid-" if grid else "") + name, H, W, C, sliced, stats, x, g, stats0, grid)


BIL = [bil_case(i, *c) for i, c in enumerate(BIL_CROSS)]
BIL_BWD = BIL + [bil_case(100 + i, *c) for i, c in enumerate(BIL_BWD_EXTRA)]
# sgan_bilinear_up2_fwd: `int blocks = sg_cdiv(total, 256 * 4); if (blocks > 2048) blocks = 2048;`, total = 4 H W C/4: the second
# stride needs total > 2048 * 1024, H W > 2048 at C = 1024.  sgan_bilinear_up2_bwd: `if (blocks > 4096) blocks = 4096;` over
# cdiv(H W C/4, 256): H W > 4096 at C = 1024.
BIL_GRID_FWD = bil_case(900, 32, 65, 1024, False, "plain", grid="2048 x 1024 < 4 * 32 * 65 * 256")
BIL_GRID_BWD = bil_case(901, 64, 65, 1024, False, "none", grid="4096 x 256 < 64 * 65 * 256")

# ---- pyramid -------------------------------------------------------------------------------------------------------------------------
LEVEL_LD = (4, 8, 12, 4, 16, 8)           # a different pixel stride per level buffer (the level is its first 4 channels ... see LEVEL_OFF)
LEVEL_OFF = (0, 4, 8, 0, 12, 0)
# (H, W, label sliced out of a 12-wide buffer, one-hot)
PYR_CROSS = [(64, 64, False, False), (64, 64, True, True), (64, 128, True, False), (64, 128, False, True), (128, 64, False, False),
             (128, 64, True, True)]
PYR_BWD = {                                # name: (levels present, accumulate)
    "all6-nan": ((0, 1, 2, 3, 4, 5), False),
    "only5-acc": ((5,), True),             # what generators.py launches: [None] * 5 + [d5], accumulate=True
    "middle-nan": ((1, 3, 4), False),
    "all6-acc": ((0, 1, 2, 3, 4, 5), True),
}
PyrCase = collections.namedtuple("PyrCase", "name H W sliced onehot x dl base grid")


def pyr_case(i, H, W, sliced, onehot, grid=None):
    rng = np.random.RandomState(3000 + i)
    if onehot:
        x = np.eye(4, dtype=np.float32)[rng.randint(0, 4, (H, W))]
    else:
        x = (rng.standard_normal((H, W, 4)) * 1.5 + 0.3).astype(np.float32)
    dl = [rng.standard_normal((H >> (s + 1), W >> (s + 1), 4)).astype(np.float32) * np.float32(2.0 ** s) for s in range(R.LEVELS)]
    base = (rng.standard_normal((H, W, 4)) * 0.5 + 0.2).astype(np.float32)
    name = f"{H}x{W}" + ("-sliced" if sliced else "") + ("-onehot" if onehot else "")
    return PyrCase(("grid-" if grid else "") + name, H, W, sliced, onehot, x, dl, base, grid)


PYR = [pyr_case(i, *c) for i, c in enumerate(PYR_CROSS)]
# sgan_avgpool_pyramid_bwd: `if (blocks > 4096) blocks = 4096;` over cdiv(H W, 256): H W > 4096 * 256 = 1024 * 1024, and
# 1024 x 1088 is the first shape past it with sides divisible by 64.  The forward launches one workgroup per tile, uncapped.
PYR_GRID_BWD = pyr_case(900, 1024, 1088, False, False, grid="4096 x 256 < 1024 * 1088")


def pyr_levels(case, present):
    return [case.dl[s] if s in present else None for s in range(R.LEVELS)]


# ---- references, once per case -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ref(kind, name, extra):
    fn, args = _JOBS[kind, name, extra]
    return fn(*args)


_JOBS = {}


def ref(kind, case, fn, args, extra=None):
    """fn(*args), computed once per (kind, case, extra) and shared by every test of the process; callers must not write to it."""
    _JOBS[kind, case.name, extra] = (fn, args)
    return _ref(kind, case.name, extra)

"""The case table of the reflection-pad parity tests: shapes, the parameter cross, and the data of every case (numpy only).
tests/test_pad_norm_ref_host.py checks the table on the CPU, tests/test_hip_pad_reflect.py runs it on the GPU.

Data with an activation is chosen so that no element of y = gamma * xhat + beta lies within KINK of zero: the forward kernel forms
y as x * sc + sh, the backward kernel as gamma * ((x - mean) * rstd) + beta, and for |x| <~ 8, |sc| <~ 2 the two differ by a few
fp32 ulps of |x * sc| (about 1e-6); a band ten times that keeps act'(y) the same on both sides and in float64.  The band only
SELECTS the data (the first seed of seed0 .. seed0 + 15 that satisfies it); no element is excluded from any comparison.  Padding
channels (logical C < stored C) hold x = 0, zero statistics and zero gamma / beta: y is exactly 0 there in every arithmetic, so they
are outside the band's concern and the margin is taken over the logical channels."""
import collections

import numpy as np

import pad_norm_ref as R

KINK = 1e-5
EPS = float(np.float32(1e-5))
SLOPE = float(np.float32(0.2))

# name: (H, W, stored C, logical C, pad)                      reaches
SHAPES = {
    "copy3": (8, 12, 4, 2, 3),       # network input path
    "min1": (3, 4, 8, 8, 1),         # smallest legal backward at pad 1 (2 pad < H)
    "min3": (7, 9, 12, 10, 3),       # smallest legal backward at pad 3: centre row and column collect both mirrors
    "fwdonly": (4, 5, 8, 8, 3),      # forward legal (pad < H), backward refused
    "pad0": (5, 7, 16, 16, 0),       # plain materialisation
    "wideC": (3, 4, 260, 260, 1),    # coefficient loop c += 256 runs twice
    "grid": (20, 28, 8, 8, 3),       # > 1 workgroup forward (26*34*2 > 1024) and backward (20*28*2 > 1024)
    "block": (6, 10, 32, 32, 1),     # the ResNet-block shape class
}

# (shape, norm, act, mask, sliced); norm: none | in | bn | relu_only (no statistics, y = x)
CROSS = [
    ("copy3", "none", "none", False, False), ("copy3", "none", "none", False, True), ("copy3", "none", "none", True, False),
    ("copy3", "relu_only", "relu", False, False),
    ("min1", "none", "none", False, False), ("min1", "in", "relu", False, False), ("min1", "bn", "lrelu", True, True),
    ("min1", "relu_only", "relu", False, False), ("min1", "in", "none", False, True),
    ("min3", "none", "none", False, False), ("min3", "none", "none", True, True), ("min3", "in", "relu", False, False),
    ("min3", "bn", "lrelu", True, False), ("min3", "bn", "none", False, True), ("min3", "relu_only", "relu", True, False),
    ("fwdonly", "none", "none", False, False), ("fwdonly", "in", "relu", True, False), ("fwdonly", "bn", "lrelu", False, True),
    ("pad0", "none", "none", False, False), ("pad0", "in", "relu", False, False), ("pad0", "bn", "none", True, True),
    ("wideC", "none", "none", False, False), ("wideC", "in", "relu", False, False), ("wideC", "bn", "lrelu", True, True),
    ("grid", "none", "none", False, False), ("grid", "in", "relu", False, False), ("grid", "bn", "lrelu", True, True),
    ("grid", "bn", "relu", False, False), ("grid", "relu_only", "relu", False, True), ("grid", "in", "none", True, False),
    ("block", "none", "none", True, False), ("block", "in", "relu", True, False), ("block", "bn", "relu", True, True),
    ("block", "bn", "lrelu", False, False), ("block", "in", "lrelu", True, True), ("block", "relu_only", "relu", True, False),
]

Case = collections.namedtuple("Case", "name shape H W C Cl pad norm act mask sliced seed x gamma beta m R stats count margin")


def _data(seed, H, W, C, Cl, pad, norm, mask):
    rng = np.random.default_rng(seed)
    x = np.zeros((H, W, C), dtype=np.float32)
    x[..., :Cl] = (rng.standard_normal((H, W, Cl)) * 1.5 + 0.3).astype(np.float32)
    gamma = beta = None
    if norm == "bn":
        gamma, beta = np.zeros(C, dtype=np.float32), np.zeros(C, dtype=np.float32)
        gamma[:Cl] = (rng.uniform(0.5, 1.5, Cl) * rng.choice([-1.0, 1.0], Cl)).astype(np.float32)
        beta[:Cl] = (rng.standard_normal(Cl) * 0.3).astype(np.float32)
    m = (rng.integers(0, 2, (H, W, C)) * 2).astype(np.float32) if mask else None
    Rr = rng.standard_normal((H + 2 * pad, W + 2 * pad, C)).astype(np.float32)       # the gradient of the padded tensor, every channel
    stats = R.stats_of(x) if norm in ("in", "bn") else None
    return x, gamma, beta, m, Rr, stats


def build(i, shape, norm, act, mask, sliced, seed0=None):
    """The case with its data: the first seed of seed0 .. seed0 + 15 whose data keeps KINK away from the activation's kink."""
    H, W, C, Cl, pad = SHAPES[shape]
    seed0 = 1000 * (i + 1) if seed0 is None else seed0
    name = f"{shape}-{norm}-{act}" + ("-mask" if mask else "") + ("-sliced" if sliced else "")
    for seed in range(seed0, seed0 + 16):
        x, gamma, beta, m, Rr, stats = _data(seed, H, W, C, Cl, pad, norm, mask)
        margin = None
        if act != "none":
            st = R.stats_of(x[..., :Cl]) if stats is not None else None
            margin = R.kink_margin(x[..., :Cl], st, None if gamma is None else gamma[:Cl], None if beta is None else beta[:Cl], H * W, EPS)
            if margin < KINK:
                continue
        return Case(name, shape, H, W, C, Cl, pad, norm, act, mask, sliced, seed, x, gamma, beta, m, Rr, stats, H * W, margin)
    raise AssertionError(f"{name}: no seed in [{seed0}, {seed0 + 16}) keeps |y| >= {KINK}")


CASES = [build(i, *c) for i, c in enumerate(CROSS)]


def norm_args(case, dtype):
    """The keyword arguments of the pad_norm_ref functions for a case."""
    return dict(stats=case.stats, gamma=case.gamma, beta=case.beta, count=case.count, eps=EPS, act=case.act, slope=SLOPE, mask=case.m,
                dtype=dtype)

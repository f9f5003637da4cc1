"""Shared by the object-score tests: an independent restatement of the match counts with explicit loops over object pairs, Python
integers and fractions.Fraction, and the boundary maps the tests score.  A map is float32 [H, W], 1.0 = wall, 0.0 = free; a pair is
(prediction s, truth t)."""
import functools
from fractions import Fraction

import numpy as np

STRUCT8 = np.ones((3, 3), dtype=np.int32)
TAUS = [Fraction(10 + k, 20) for k in range(10)]      # 0.5, 0.55 .. 0.95


def restated(s, t, min_area=1):
    """(counts: 16 Python ints, sums: (SIoU, SSEG) as Fractions) of prediction s against truth t, as the definition reads: label both
    maps, drop the regions below min_area, then for every pair of a truth and a predicted object take IoU = c / (a + b - c) as a
    Fraction and compare it with every threshold; SEG pairs are those that cover more than half of the truth object."""
    from scipy import ndimage
    t_lab, n_t = ndimage.label(~(np.asarray(t) > 0.5), structure=STRUCT8)
    s_lab, n_s = ndimage.label(~(np.asarray(s) > 0.5), structure=STRUCT8)
    truth = {i: int((t_lab == i).sum()) for i in range(1, n_t + 1)}
    pred = {j: int((s_lab == j).sum()) for j in range(1, n_s + 1)}
    truth = {i: a for i, a in truth.items() if a >= min_area}
    pred = {j: b for j, b in pred.items() if b >= min_area}
    tp, segn, siou, sseg = [0] * 10, 0, Fraction(0), Fraction(0)
    for i, a in truth.items():
        under = s_lab[t_lab == i]
        for j in sorted(set(int(v) for v in under)):
            if j not in pred:          # prediction wall (0), or an object that is too small
                continue
            c = int((under == j).sum())
            iou = Fraction(c, a + pred[j] - c)
            for k, tau in enumerate(TAUS):
                if iou > tau:
                    tp[k] += 1
            if iou > TAUS[0]:
                siou += iou
            if Fraction(c, a) > Fraction(1, 2):
                segn += 1
                sseg += iou
    return tp + [len(truth), len(pred), 1, segn, 0, 0], (siou, sseg)


def walls(H, W):
    return np.ones((H, W), dtype=np.float32)


def carve(m, y0, x0, h, w):
    """Frees the h x w rectangle at (y0, x0)."""
    m[y0:y0 + h, x0:x0 + w] = 0.0
    return m


def hand_cases():
    """{name: (s, t)} of small cores without a wall border (embed() supplies one); the answers are literals in the tests."""
    out = {}
    t = carve(carve(carve(walls(5, 11), 0, 0, 2, 3), 0, 4, 5, 2), 3, 7, 2, 4)
    out["identical3"] = (t.copy(), t)                                                      # areas 6, 10, 8
    out["iou_half"] = (carve(walls(1, 4), 0, 1, 1, 3), carve(walls(1, 4), 0, 0, 1, 3))      # c 2, u 4
    out["iou_three_quarters"] = (carve(walls(1, 4), 0, 0, 1, 3), carve(walls(1, 4), 0, 0, 1, 4))      # c 3, u 4
    out["swallowed"] = (carve(walls(6, 8), 0, 0, 6, 8), carve(walls(6, 8), 2, 3, 2, 2))      # a 4 inside b 48: IoU 1/12
    whole, halves = carve(walls(2, 7), 0, 0, 2, 7), carve(carve(walls(2, 7), 0, 0, 2, 3), 0, 4, 2, 3)
    out["split"] = (halves, whole)                                                          # one cell of 14 found as 6 + 6
    out["merged"] = (whole, halves)                                                         # cells of 6 + 6 found as one of 14
    t = carve(carve(carve(carve(walls(5, 14), 0, 0, 1, 1), 0, 2, 2, 2), 3, 0, 1, 5), 0, 7, 5, 6)
    out["areas_1_4_5_30"] = (t.copy(), t)
    return out


def embed(core, H, W, oy, ox):
    """`core` at (oy, ox) of an all-wall H x W map; the caller leaves a wall pixel around it wherever the image goes on."""
    m = walls(H, W)
    m[oy:oy + core.shape[0], ox:ox + core.shape[1]] = core
    return m


def random_cells(H, W, rng, lo=3, hi=12):
    """Rectangular cells of random sizes between one-pixel walls: cuts at random rows and columns."""
    m = np.zeros((H, W), dtype=np.float32)
    for axis, n in ((0, H), (1, W)):
        p = int(rng.integers(0, lo))
        while p < n:
            if axis == 0:
                m[p, :] = 1.0
            else:
                m[:, p] = 1.0
            p += int(rng.integers(lo, hi + 1)) + 1
    return m


def eroded(t, upto):
    """Every wall grows by one pixel to the right and downwards in the columns < upto: the cells there lose a row and a column,
    so their IoU with the original is (h - 1)(w - 1) / (h w), anything from 4/9 up; the cells beyond stay as they are."""
    s = t.copy()
    grown = t.copy()
    grown[1:, :] = np.maximum(grown[1:, :], t[:-1, :])
    grown[:, 1:] = np.maximum(grown[:, 1:], t[:, :-1])
    grown[1:, 1:] = np.maximum(grown[1:, 1:], t[:-1, :-1])
    s[:, :upto] = grown[:, :upto]
    return s


def shifted(t, rng):
    """The grid moved one pixel to the right, a few walls broken (merges) and a few stray wall pixels (splits, singletons)."""
    s = np.roll(t, 1, axis=1)
    s[rng.random(t.shape) < 0.02] = 0.0
    s[rng.random(t.shape) < 0.02] = 1.0
    return s


SHAPES = [(1, 70), (37, 53), (64, 64), (70, 130), (128, 128)]      # (H, W): rows shorter than a wave, not a multiple of one, 1 .. 3 segments


NOISE = {"noise": 0.55, "noise_dense": 0.68}      # per-pixel wall densities of the two noise-against-noise cases
# what the yardstick must count on them at the two largest shapes, min_area 1 (asserted by the tests that use the list)
NOISE_MIN_REGIONS = {"noise": 80, "noise_dense": 300}


def noise_is_rich(want):
    """want(H, W, name, min_area) -> 16 counts of the yardstick.  True when, at the two largest shapes, the noise cases have the many
    regions they are there for on both sides, and a min_area of 5 removes some of them but not all."""
    for H, W in SHAPES[-2:]:
        for name, least in NOISE_MIN_REGIONS.items():
            c1, c5 = want(H, W, name, 1), want(H, W, name, 5)
            if not (min(c1[10], c1[11]) >= least and 0 < c5[10] < c1[10] and 0 < c5[11] < c1[11]):
                return False
    return True


@functools.lru_cache(maxsize=None)
def cases(H, W):
    """{name: (s, t)} for one shape, computed once and shared (read-only): the hand-built cores that fit, embedded off the origin;
    random cells against an eroded and a shifted copy; per-pixel noise against noise; all-wall and no-wall on either side."""
    rng = np.random.default_rng(1000 * H + W)
    out = {}
    for name, (s, t) in hand_cases().items():
        h, w = s.shape
        oy, ox = (1 if H > h else 0), min(W - w, 17)      # a wall row above where there is room, and a start inside the first wave
        if h + oy <= H and w + 1 <= W and (H == h or h + oy + 1 <= H):
            out["hand_" + name] = (embed(s, H, W, oy, ox), embed(t, H, W, oy, ox))
    cells = random_cells(H, W, rng)
    out["cells_eroded"] = (eroded(cells, (2 * W) // 3), cells)
    out["cells_shifted"] = (shifted(cells, rng), cells)
    # free pixels percolate 8-connected up to a wall density of about 0.59.  At 0.55 one region still crosses every wave and lives among
    # a hundred small ones and singletons; at 0.68 there are hundreds of small regions, many of them around a min_area of 5.
    for name, density in NOISE.items():
        out[name] = ((rng.random((H, W)) < density).astype(np.float32), (rng.random((H, W)) < density).astype(np.float32))
    free, wall = np.zeros((H, W), np.float32), walls(H, W)
    out.update(all_wall=(wall, wall), no_wall=(free, free), prediction_wall=(wall, free), truth_wall=(free, wall))
    for s, t in out.values():
        s.setflags(write=False)
        t.setflags(write=False)
    return out

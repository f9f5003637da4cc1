"""CPU tests of the object-level scores (ObjF1, ObjAP, SEG, PQ): the host yardstick util.object_match_counts against an independent
restatement with explicit pair loops and Fractions (objects_ref.restated), hand-built maps whose answers are literals, the score
derivation, the options, and the C ABI's declarations."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import objects_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(name, s, t, min_area):
    """Yardstick against restatement: the integers equal, the sums within N_t 2^-52 relative of the exact rational sum."""
    from supervised_gan_amd.util import object_match_counts
    counts, sums = object_match_counts(s, t, min_area)
    want, (siou, sseg) = R.restated(s, t, min_area)
    assert counts.dtype == np.int64 and counts.shape == (16,) and sums.dtype == np.float64 and sums.shape == (2,), name
    assert counts.tolist() == want, (name, min_area, counts.tolist(), want)
    bound = max(1, want[10]) * 2.0 ** -52
    for got, exact in zip(sums.tolist(), (siou, sseg)):
        assert abs(Fraction(got) - exact) <= Fraction(bound) * exact, (name, min_area, got, float(exact))
    return counts.tolist(), sums.tolist()


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_yardstick_equals_the_restatement(H, W):
    for name, (s, t) in R.cases(H, W).items():
        for min_area in (1, 5):
            _check("%dx%d %s" % (H, W, name), s, t, min_area)


def test_case_list_spreads_over_the_thresholds():
    """What the device tests rely on: some case has 0 < TP_9 < TP_0 < min(N_t, N_s), some case SEGn > TP_0, and the noise pairs hold
    hundreds of regions."""
    from supervised_gan_amd.util import object_match_counts
    spread = seg = 0
    for H, W in R.SHAPES:
        for name, (s, t) in R.cases(H, W).items():
            c = object_match_counts(s, t)[0]
            spread += 0 < c[9] < c[0] < min(c[10], c[11])
            seg += c[13] > c[0]
    assert spread >= 3 and seg >= 3, (spread, seg)
    # the noise cases: many small regions beside the percolating one, and a min_area that cuts through them
    assert R.noise_is_rich(lambda H, W, name, min_area: object_match_counts(*R.cases(H, W)[name], min_area)[0])


def _padded(name):
    s, t = R.hand_cases()[name]
    h, w = s.shape
    return R.embed(s, h + 2, w + 2, 1, 1), R.embed(t, h + 2, w + 2, 1, 1)


def test_identical_maps():
    s, t = _padded("identical3")
    counts, sums = _check("identical3", s, t, 1)
    assert counts == [3] * 10 + [3, 3, 1, 3, 0, 0] and sums == [3.0, 3.0]


def test_iou_of_exactly_one_half_is_no_match():
    s, t = _padded("iou_half")
    counts, sums = _check("iou_half", s, t, 1)
    assert counts == [0] * 10 + [1, 1, 1, 1, 0, 0]      # 2 of the truth cell's 3 pixels: SEG counts it
    assert sums == [0.0, 0.5]


def test_iou_of_exactly_three_quarters():
    s, t = _padded("iou_three_quarters")
    counts, sums = _check("iou_three_quarters", s, t, 1)
    assert counts == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0] + [1, 1, 1, 1, 0, 0]      # matched for k <= 4 (0.70), not at k = 5 (0.75)
    assert sums == [0.75, 0.75]


def test_cell_swallowed_by_a_large_region_counts_for_seg_only():
    s, t = _padded("swallowed")
    counts, sums = _check("swallowed", s, t, 1)
    assert counts == [0] * 10 + [1, 1, 1, 1, 0, 0]
    assert sums[0] == 0.0 and abs(sums[1] - 1.0 / 12.0) <= 2.0 ** -52


def test_split_and_merged_cells():
    from supervised_gan_amd.util import object_scores
    s, t = _padded("split")               # one cell of 14 pixels found as two of 6: IoU 3/7 each, and neither covers more than half
    counts, sums = _check("split", s, t, 1)
    assert counts == [0] * 10 + [1, 2, 1, 0, 0, 0] and sums == [0.0, 0.0]
    assert list(object_scores(counts, sums).values()) == [0.0, 0.0, 0.0, 0.0]
    s, t = _padded("merged")              # two cells of 6 found as one of 14: IoU 3/7 each, and each lies wholly in the region
    counts, sums = _check("merged", s, t, 1)
    assert counts == [0] * 10 + [2, 1, 1, 2, 0, 0]
    assert sums[0] == 0.0 and abs(sums[1] - 6.0 / 7.0) <= 2 * 2.0 ** -52
    sc = object_scores(counts, sums)
    assert sc["ObjF1"] == 0.0 and sc["ObjAP"] == 0.0 and sc["PQ"] == 0.0 and abs(sc["SEG"] - 3.0 / 7.0) <= 2.0 ** -52


def test_min_area_leaves_small_regions_out():
    s, t = _padded("areas_1_4_5_30")
    assert _check("areas", s, t, 1)[0] == [4] * 10 + [4, 4, 1, 4, 0, 0]
    assert _check("areas", s, t, 5) == ([2] * 10 + [2, 2, 1, 2, 0, 0], [2.0, 2.0])      # 5 passes, 4 does not
    assert _check("areas", s, t, 6)[0] == [1] * 10 + [1, 1, 1, 1, 0, 0]
    assert _check("areas", s, t, 31)[0] == [0] * 10 + [0, 0, 1, 0, 0, 0]
    # the small regions are absent on both sides while the others keep their areas
    s2 = s.copy()
    s2[1:6, 10] = 1.0                     # a wall through the big cell: 5 x 2 + wall + 5 x 3 pixels
    counts, sums = _check("areas cut", s2, t, 5)
    assert counts[10:14] == [2, 3, 1, 1]  # truth 5, 30; prediction 5, 10, 15; SEG: only the 5-pixel cell (15 of 30 is not more than half)
    assert counts[:10] == [1] * 10 and sums == [1.0, 1.0]


def test_all_wall_and_no_wall():
    from supervised_gan_amd.util import object_scores
    free, wall = np.zeros((9, 12), np.float32), np.ones((9, 12), np.float32)
    zero = [0] * 10 + [0, 0, 1, 0, 0, 0]
    for s, t, n_t, n_s in ((wall, wall, 0, 0), (wall, free, 1, 0), (free, wall, 0, 1)):
        counts, sums = _check("walls", s, t, 1)
        assert counts == zero[:10] + [n_t, n_s] + zero[12:] and sums == [0.0, 0.0]
        assert list(object_scores(counts, sums).items()) == [("ObjF1", 0.0), ("ObjAP", 0.0), ("SEG", 0.0), ("PQ", 0.0)]
    counts, sums = _check("free", free, free, 1)
    assert counts == [1] * 10 + [1, 1, 1, 1, 0, 0] and sums == [1.0, 1.0]
    assert list(object_scores(counts, sums).values()) == [1.0, 1.0, 1.0, 1.0]


def test_object_scores_on_literal_counts():
    from supervised_gan_amd.util import OBJECT_METRICS, object_scores
    counts = [8, 8, 7, 6, 6, 5, 4, 2, 1, 0, 10, 12, 3, 9, 0, 0]
    sc = object_scores(counts, [6.5, 7.25])
    assert tuple(sc) == OBJECT_METRICS == ("ObjF1", "ObjAP", "SEG", "PQ")
    assert sc["ObjF1"] == 16.0 / 22.0 and sc["SEG"] == 0.725 and sc["PQ"] == 6.5 / 11.0
    ap = sum(Fraction(v, 22 - v) for v in counts[:10]) / 10
    assert abs(sc["ObjAP"] - float(ap)) <= 1e-15
    assert object_scores(np.array(counts, dtype=np.int64), np.array([6.5, 7.25])) == sc
    assert list(object_scores([0] * 16, [0.0, 0.0]).values()) == [0.0] * 4
    # every prediction matched at every threshold: N_t + N_s - TP_k stays positive
    assert list(object_scores([5] * 10 + [5, 5, 1, 5, 0, 0], [5.0, 5.0]).values()) == [1.0, 1.0, 1.0, 1.0]


def test_options_and_slot_names(tmp_path):
    from supervised_gan_amd import ops
    from supervised_gan_amd.options import TrainOptions
    base = ["--name", "t", "--gpu_ids", "-1", "--checkpoints_dir", str(tmp_path)]
    opt = TrainOptions().parse(base, save=False, verbose=False)
    assert opt.min_object_area == 1
    opt = TrainOptions().parse(base + "--which_metric RandScore ObjF1 SEG --best_metric ObjF1 --min_object_area 20".split(), save=False,
                               verbose=False)
    assert opt.min_object_area == 20 and opt.which_metric == ["RandScore", "ObjF1", "SEG"] and opt.best_metric == "ObjF1"
    assert ops.OBJECT_COUNTS[:10] == tuple("TP_%d" % k for k in range(10)) and len(ops.OBJECT_COUNTS) == 16
    assert ops.OBJECT_COUNTS[10:14] == ("N_t", "N_s", "images", "SEGn") and ops.OBJECT_SUMS == ("SIoU", "SSEG")


def test_entry_points_are_declared_and_bound(built_lib):
    from supervised_gan_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "sgan_hip.h")).read()
    assert re.search(r"\bint64_t\s+sgan_object_match_workspace\s*\(\s*int32_t H,\s*int32_t W\s*\)\s*;", header)
    assert re.search(r"\bint\s+sgan_object_match_accumulate\s*\(\s*const int32_t\* t_labels,\s*const int32_t\* s_labels,\s*int32_t H,\s*int32_t W,\s*"
                     r"int32_t min_area,\s*void\* workspace,\s*int64_t workspace_bytes,\s*int64_t\* acc_i,\s*double\* acc_f,\s*"
                     r"int64_t\* counts_out,\s*double\* sums_out,\s*int32_t\* dev_err,\s*void\* stream\s*\)\s*;", header)
    macros = dict(re.findall(r"#define (SGAN_OBJ_[A-Z0-9]+) (\d+)", header))
    assert macros == {"SGAN_OBJ_COUNTS": "16", "SGAN_OBJ_TP0": "0", "SGAN_OBJ_NT": "10", "SGAN_OBJ_NS": "11", "SGAN_OBJ_IMAGES": "12",
                      "SGAN_OBJ_SEGN": "13", "SGAN_OBJ_SUMS": "2", "SGAN_OBJ_SIOU": "0", "SGAN_OBJ_SSEG": "1"}
    for name, slot in (("N_t", "SGAN_OBJ_NT"), ("N_s", "SGAN_OBJ_NS"), ("images", "SGAN_OBJ_IMAGES"), ("SEGn", "SGAN_OBJ_SEGN")):
        assert ops.OBJECT_COUNTS.index(name) == int(macros[slot])
    assert len(_lib.SIGNATURES["sgan_object_match_accumulate"]) == 13 and len(_lib.SIGNATURES["sgan_object_match_workspace"]) == 2
    assert _lib.RESTYPES["sgan_object_match_workspace"] is ctypes.c_int64
    l = _lib.lib()
    # the pair table of >= 2 H W slots (a key and a count each) and a counter per label on either side
    assert l.sgan_object_match_workspace(64, 64) >= 12 * 2 * 64 * 64 + 8 * 64 * 64 and l.sgan_object_match_workspace(64, 64) % 16 == 0
    assert l.sgan_object_match_workspace(1, 1) > 0
    assert l.sgan_object_match_workspace(0, 5) < 0 and l.sgan_object_match_workspace(5, -1) < 0
    assert l.sgan_object_match_workspace(1 << 15, 1 << 15) < 0 and b"bad shape" in l.sgan_last_error()      # H W < 2^30, as the Rand count
    # malformed arguments are refused before anything touches a device
    assert l.sgan_object_match_accumulate(None, None, 8, 8, 1, None, 0, None, None, None, None, None, None) < 0
    assert b"null pointer" in l.sgan_last_error()

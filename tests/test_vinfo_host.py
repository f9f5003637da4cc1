"""CPU tests of util.compute_VInfo_scores, the host yardstick of the device information score: hand-checked maps, and agreement
with an independent restatement (tests/vinfo_ref.py: explicit probability tables, -sum p ln p) on random and cell-like maps."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import vinfo_ref as V  # noqa: E402


def _score(s, t):
    from supervised_gan_amd.util import compute_VInfo_scores
    out = compute_VInfo_scores(np.asarray(s, np.float32), np.asarray(t, np.float32))
    assert out.shape == (1,)
    return float(out[0])


def test_identical_maps_score_one():
    t = np.zeros((6, 9), np.float32)
    t[:, 4] = 1                      # two regions
    assert _score(t, t) == 1.0
    t[3, :] = 1                      # four regions
    assert _score(t, t) == 1.0


def test_one_prediction_region_over_two_equal_truth_regions_scores_zero():
    from supervised_gan_amd.util import compute_VInfo_parts
    t = np.zeros((6, 9), np.float32)
    t[:, 4] = 1
    s = np.zeros((6, 9), np.float32)
    p = compute_VInfo_parts(s, t)
    assert p["m"] == 48 and p["aux"] == 0 and p["H_S"] == 0.0 and abs(p["H_T"] - math.log(2)) < 1e-15
    assert p["VInfo"] == 0.0 and math.isnan(p["split"]) and p["merge"] == 0.0
    assert _score(s, t) == 0.0


def test_a_single_region_in_both_scores_one():
    z = np.zeros((5, 7), np.float32)
    assert _score(z, z) == 1.0
    assert _score(np.zeros((1, 1)), np.zeros((1, 1))) == 1.0
    assert _score(np.ones((1, 1)), np.zeros((1, 1))) == 1.0          # m == 1: one pixel is one segment in both, wall or not


def test_truth_all_wall_scores_nan():
    assert math.isnan(_score(np.zeros((5, 7)), np.ones((5, 7))))
    assert math.isnan(_score(np.ones((5, 7)), np.ones((5, 7))))


def test_prediction_all_wall_over_one_truth_region_scores_zero():
    from supervised_gan_amd.util import compute_VInfo_parts
    p = compute_VInfo_parts(np.ones((5, 7), np.float32), np.zeros((5, 7), np.float32))
    assert p["m"] == 35 and p["aux"] == 35 and p["H_T"] == 0.0 and abs(p["H_S"] - math.log(35)) < 1e-15
    assert p["VInfo"] == 0.0 and p["split"] == 0.0 and math.isnan(p["merge"])


def test_2x4_with_one_singleton():
    s, t, want = V.hand_2x4()
    got = _score(s, t)
    assert 0.0 < want < 1.0 and abs(got - want) < 1e-14, (got, want)
    assert abs(V.vinfo_restated(s, t)[0] - want) < 1e-14


def test_batched_shapes_as_compute_Rand_F_scores():
    from supervised_gan_amd.util import compute_VInfo_scores
    s, t, want = V.hand_2x4()
    z = np.zeros_like(t)
    out = compute_VInfo_scores(np.stack([s, z, t])[:, None], np.stack([t, z, t])[:, None])
    assert out.shape == (3,) and abs(out[0] - want) < 1e-14 and out[1] == 1.0 and out[2] == 1.0


def test_agrees_with_the_restatement_on_random_and_cell_like_maps():
    """50 maps up to 96 x 96; both forms are fp64 sums of fewer than 1e4 terms of size <= 1: 1e-12 absolute."""
    maps = V.host_maps()
    assert len(maps) == 50
    worst, seen = 0.0, set()
    for name, s, t in maps:
        got, (want, h_s, h_t, _) = _score(s, t), V.vinfo_restated(s, t)
        if math.isnan(want):
            assert math.isnan(got), name
            seen.add("nan")
            continue
        print("%s: VInfo %.15f restated %.15f diff %.2e (H_S %.4f H_T %.4f)" % (name, got, want, abs(got - want), h_s, h_t))
        assert abs(got - want) <= 1e-12, (name, got, want)
        assert 0.0 <= got <= 1.0, (name, got)
        worst = max(worst, abs(got - want))
        seen.add("mid" if 0.0 < got < 1.0 else "end")
    print("worst difference %.2e" % worst)
    assert "mid" in seen

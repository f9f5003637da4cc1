"""CPU tests of the topology scores (Betti0Err, Betti1Err, clDice): the host yardstick util.betti_window on hand-checked patterns and
against Gray's bit-quad Euler number, the window geometry, util.topo_counts / topo_scores, the options, train_ss.py's refusal of a
Betti error as --best_metric, and the C ABI's declarations."""
import os
import re
import sys

import numpy as np
import pytest

import topo_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _mask(rows):
    return np.array([[c == "#" for c in r] for r in rows], dtype=bool)


def test_betti_window_by_hand():
    from supervised_gan_amd.util import betti_window
    assert betti_window(np.zeros((8, 8), dtype=bool)) == (0, 0)
    assert betti_window(np.ones((8, 8), dtype=bool)) == (1, 0)
    one = np.zeros((8, 8), dtype=bool)
    one[3, 4] = True
    assert betti_window(one) == (1, 0)
    one[:] = False
    one[0, 0] = True                                   # ... in a corner
    assert betti_window(one) == (1, 0)
    ring = _mask(["........",
                  "..###...",
                  "..#.#...",
                  "..###...",
                  "........",
                  "........",
                  "........",
                  "........"])
    assert betti_window(ring) == (1, 1)
    # the same ring with its top side outside the window: what it encloses reaches the window's edge
    assert betti_window(ring[2:]) == (1, 0) and betti_window(ring[:, 3:]) == (1, 0)
    cut = _mask(["#.#.....",
                 "###.....",
                 "........",
                 "........"])
    assert betti_window(cut) == (1, 0)
    diag = _mask(["........",
                  "..#.....",
                  "...#....",
                  "........"])
    assert betti_window(diag) == (1, 0)                 # the wall is 8-connected
    block = _mask(["......",
                   ".####.",
                   ".#.##.",
                   ".##.#.",
                   ".####.",
                   "......"])
    assert betti_window(block) == (1, 2)                # the free space is 4-connected: two holes, not one
    # a ring closed only through a diagonal step still encloses its hole
    assert betti_window(_mask([".#..", "#.#.", ".#..", "...."])) == (1, 1)
    yy, xx = np.mgrid[0:8, 0:8]
    # wall on the odd squares: one diagonal-connected component; 32 free pixels, each alone, 14 of them on the edge
    assert betti_window((yy + xx) % 2 == 1) == (1, 18)
    # wall on the even squares: the same count mirrored
    assert betti_window((yy + xx) % 2 == 0) == (1, 18)
    assert betti_window(R.serpentine(8, 8)) == (1, 0) and betti_window(R.serpentine(64, 64)) == (1, 0)
    assert betti_window(R.serpentine(64, 64) < 0.5) == (32, 0)     # its free rows as wall: 32 bars, each touching nothing
    # a float map: exactly 0.5 and NaN are free
    m = np.where(ring, 1.0, 0.0).astype(np.float32)
    m[1, 3] = 0.5
    assert betti_window(m) == (1, 0)
    m[1, 3] = np.nan
    assert betti_window(m) == (1, 0)
    m[1, 3] = 0.50000006
    assert betti_window(m) == (1, 1)


def test_euler_identity_on_random_windows():
    from supervised_gan_amd.util import betti_window, euler_bitquads
    rng = np.random.default_rng(28)
    for k in range(200):
        h, w = (int(v) for v in rng.integers(8, 65, size=2))
        density = 0.1 + 0.8 * (k % 9) / 8.0
        wall = rng.random((h, w)) < density
        b0, b1 = betti_window(wall)
        assert b0 - b1 == euler_bitquads(wall), (k, h, w, density)
    assert euler_bitquads(np.zeros((8, 8), dtype=bool)) == 0 and euler_bitquads(np.ones((8, 8), dtype=bool)) == 1
    for name in R.NAMES:
        wall = R.planes(64, 64)[name] > 0.5
        b0, b1 = betti_window(wall)
        assert b0 - b1 == euler_bitquads(wall), name


@pytest.mark.parametrize("case,want", (((16, 24, 8, 8), (8, 8, [0, 8], [0, 8, 16])),
                                       ((33, 47, 16, 8), (16, 16, [0, 8, 16], [0, 8, 16, 24])),
                                       ((5, 70, 64, 64), (5, 64, [0], [0])),
                                       ((128, 128, 64, 32), (64, 64, [0, 32, 64], [0, 32, 64]))))
def test_topo_windows_geometry(case, want):
    from supervised_gan_amd.util import topo_windows
    assert topo_windows(*case) == want
    wh, ww, ys, xs = topo_windows(*case)
    assert ys[-1] + wh <= case[0] < ys[-1] + wh + case[3] and xs[-1] + ww <= case[1] < xs[-1] + ww + case[3]


def test_topo_windows_refuses_what_is_not_covered():
    from supervised_gan_amd.util import topo_windows
    for window, stride in ((7, 7), (65, 65), (16, 0), (16, 17)):
        with pytest.raises(AssertionError):
            topo_windows(64, 64, window, stride)


def test_counts_of_a_map_against_itself():
    from supervised_gan_amd.util import TOPO_COUNTS, TOPO_METRICS, thin, topo_counts, topo_scores
    assert TOPO_METRICS == ("Betti0Err", "Betti1Err", "clDice") and len(TOPO_COUNTS) == 12
    wall = R.planes(33, 47)["cells_punched"] > 0.5
    skel, _ = thin(wall)
    c = topo_counts(wall, wall, 16, 8, s_thin=skel, t_thin=skel)
    assert c.dtype == np.int64 and c.shape == (12,)
    named = dict(zip(TOPO_COUNTS, c.tolist()))
    assert named["windows"] == 12 and named["abs_d0"] == 0 and named["abs_d1"] == 0 and named["images"] == 1
    assert named["b0_s"] == named["b0_t"] > 0 and named["b1_s"] == named["b1_t"]
    assert named["skel_s"] == named["skel_s_in_t"] == named["skel_t"] == named["skel_t_in_s"] == int(skel.sum()) > 0
    scores = topo_scores(c)
    assert list(scores) == list(TOPO_METRICS) and dict(scores) == {"Betti0Err": 0.0, "Betti1Err": 0.0, "clDice": 1.0}
    # without the thinned planes the four skeleton counters stay 0; one side alone counts its two
    assert topo_counts(wall, wall, 16, 8)[7:11].tolist() == [0, 0, 0, 0]
    assert topo_counts(wall, wall, 16, 8, s_thin=skel)[7:11].tolist() == [int(skel.sum())] * 2 + [0, 0]
    # the default stride is the window
    assert topo_counts(wall, wall, 16)[0] == 2 * 2


def test_punching_one_gap_in_a_ring_opens_one_cell():
    from supervised_gan_amd.util import TOPO_COUNTS, topo_counts, topo_scores
    t = np.zeros((16, 16), dtype=np.float32)
    t[3:12, 3] = t[3:12, 11] = t[3, 3:12] = t[11, 3:12] = 1.0      # a ring inside the one 16 x 16 window
    s = t.copy()
    s[3, 7] = 0.0
    whole = dict(zip(TOPO_COUNTS, topo_counts(t, t, 16, 16).tolist()))
    gap = dict(zip(TOPO_COUNTS, topo_counts(s, t, 16, 16).tolist()))
    assert whole["b1_s"] == 1 and gap["b1_s"] == whole["b1_s"] - 1 and gap["b1_t"] == 1
    assert gap["abs_d1"] == 1 and gap["abs_d0"] == 0 and gap["b0_s"] == 1 and gap["windows"] == 1
    assert topo_scores(topo_counts(s, t, 16, 16))["Betti1Err"] == 1.0
    # a value of exactly 0.5 is free: the same gap
    h = t.copy()
    h[3, 7] = 0.5
    assert topo_counts(h, t, 16, 16).tolist() == topo_counts(s, t, 16, 16).tolist()
    # with four 8 x 8 windows the ring is cut by every window: nothing is enclosed in any of them
    assert dict(zip(TOPO_COUNTS, topo_counts(t, t, 8, 8).tolist()))["b1_t"] == 0


def test_topo_scores_on_zero_denominators():
    from supervised_gan_amd.util import topo_scores
    assert dict(topo_scores(np.zeros(12, dtype=np.int64))) == {"Betti0Err": 0.0, "Betti1Err": 0.0, "clDice": 0.0}
    # an empty prediction: no skeleton, precision reads 0, and so does clDice
    assert topo_scores([4, 6, 2, 0, 6, 0, 2, 0, 0, 50, 0, 1])["clDice"] == 0.0
    got = topo_scores([4, 6, 2, 9, 3, 1, 3, 40, 30, 50, 25, 1])
    assert got["Betti0Err"] == 1.5 and got["Betti1Err"] == 0.5 and got["clDice"] == 2 * 0.75 * 0.5 / 1.25
    # skeletons that miss each other entirely: 0 / 0 in the harmonic mean reads 0
    assert topo_scores([1, 0, 0, 1, 1, 0, 0, 10, 0, 10, 0, 1])["clDice"] == 0.0


def test_pooling_adds():
    from supervised_gan_amd.util import topo_counts
    p = R.planes(33, 47)
    a, b = topo_counts(p["noise30"], p["noise50"], 16, 8), topo_counts(p["rings"], p["diagonals"], 16, 8)
    assert a[:7].tolist() == R.want_betti(33, 47, 16, 8, "noise30", "noise50") and (a + b)[0] == 24 and (a + b)[11] == 2


def test_options(tmp_path):
    from supervised_gan_amd import ops, util
    from supervised_gan_amd.options import TrainOptions, topo_params
    base = ["--name", "t", "--gpu_ids", "-1", "--checkpoints_dir", str(tmp_path)]
    opt = TrainOptions().parse(base, save=False, verbose=False)
    assert opt.topo_window == 64 and opt.topo_stride == 64 and topo_params(opt) == (64, 64)
    opt = TrainOptions().parse(base + "--which_metric RandScore clDice Betti0Err Betti1Err --best_metric clDice --topo_window 32".split(),
                               save=False, verbose=False)
    assert opt.which_metric == ["RandScore", "clDice", "Betti0Err", "Betti1Err"] and topo_params(opt) == (32, 32)
    assert topo_params(TrainOptions().parse(base + "--topo_window 48 --topo_stride 16".split(), save=False, verbose=False)) == (48, 16)
    for bad in ("--topo_window 7", "--topo_window 65", "--topo_stride 0", "--topo_window 16 --topo_stride 17"):
        with pytest.raises(SystemExit):
            TrainOptions().parse(base + bad.split(), save=False, verbose=False)
    assert ops.TOPO_COUNTS == util.TOPO_COUNTS == ("windows", "abs_d0", "abs_d1", "b0_s", "b0_t", "b1_s", "b1_t", "skel_s", "skel_s_in_t",
                                                   "skel_t", "skel_t_in_s", "images")

    class Bare:
        pass
    assert topo_params(Bare()) == (64, 64)


def test_seg_metrics_names_and_values_without_a_device():
    """The three names come last in read()'s order, topo_i lies beside the accumulator table, and read() derives the scores and the
    image count from it; built for evaluation it prints the topology line."""
    import torch
    from supervised_gan_amd import seg_metrics, util
    assert seg_metrics.SCORES[-3:] == util.TOPO_METRICS and [n for n, _, _ in seg_metrics.TOPO_ACCUMULATORS] == ["topo_i"]
    assert "topo_i" not in [n for n, _, _ in seg_metrics.ACCUMULATORS]

    class Opt:
        which_metric = ["clDice", "Betti1Err", "RandScore", "Betti0Err"]
        add_background_onehot_acc = False
        boundary_tolerance = 2
        boundary_thin = False
        isTrain = True
        topo_window, topo_stride = 32, 16
    m = seg_metrics.SegMetrics(Opt(), torch.device("cpu"), 2)
    assert m.counts("topology") == dict.fromkeys(util.TOPO_COUNTS, 0) and "topo_i" not in m.acc
    ints = [4, 6, 2, 9, 3, 1, 3, 40, 30, 50, 25, 7]
    m._acc("topo_i").copy_(torch.tensor(ints))
    got = m.read()
    assert list(got) == ["RandScore", "Betti0Err", "Betti1Err", "clDice"]
    assert (got["Betti0Err"], got["Betti1Err"], got["clDice"]) == (1.5, 0.5, 2 * 0.75 * 0.5 / 1.25) and m.values["numAveragedImages"] == 7
    assert list(m.counts("topology").values()) == ints
    m.reset()
    assert not m.acc["topo_i"].any() and m.values["clDice"] == 0


def test_topology_line_is_printed_for_evaluation(capsys):
    import torch
    from supervised_gan_amd import seg_metrics

    class Opt:
        which_metric = ["Betti0Err", "clDice"]
        add_background_onehot_acc = False
        boundary_tolerance = 2
        boundary_thin = False
        isTrain = False
        topo_window, topo_stride = 32, 16
    m = seg_metrics.SegMetrics(Opt(), torch.device("cpu"), 2)
    m._acc("topo_i").copy_(torch.tensor([4, 6, 2, 9, 3, 1, 3, 40, 30, 50, 25, 1]))
    m.read()
    assert capsys.readouterr().out == ("topology: 4 windows of 32 at stride 16, mean b0 / b1 of the prediction 2.250 / 0.250, of the truth "
                                       "0.750 / 0.750, Tprec 0.7500, Tsens 0.5000\n")


def test_train_ss_refuses_a_betti_error_as_best_metric(tmp_path):
    import train_ss
    base = ["--name", "t", "--gpu_ids", "-1", "--checkpoints_dir", str(tmp_path), "--dataroot", "synthetic", "--model", "segmentation"]
    for name in ("Betti0Err", "Betti1Err"):
        assert name in train_ss.LOWER_IS_BETTER
        with pytest.raises(ValueError, match="best_metric.*lower is better"):
            train_ss.main(base + ["--which_metric", "clDice", name, "--best_metric", name])
    assert "clDice" not in train_ss.LOWER_IS_BETTER
    assert train_ss.should_save_best("clDice", {"clDice": 0.25}, -1.0) and not train_ss.should_save_best("clDice", {"clDice": 0.25}, 0.25)


def test_entry_points_are_declared_and_bound(built_lib):
    import ctypes
    from supervised_gan_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "sgan_hip.h")).read()
    assert "topology scores" in header
    assert re.search(r"\bint64_t\s+sgan_topo_workspace_bytes\s*\(\s*int32_t H,\s*int32_t W,\s*int32_t window,\s*int32_t stride\s*\)\s*;", header)
    assert re.search(r"\bint\s+sgan_topo_accumulate\s*\(\s*const float\* t,\s*int64_t t_ld,\s*const float\* s,\s*int64_t s_ld,\s*"
                     r"const float\* t_thin,\s*const float\* s_thin,\s*int32_t H,\s*int32_t W,\s*int32_t window,\s*int32_t stride,\s*"
                     r"void\* workspace,\s*int64_t workspace_bytes,\s*int64_t\* acc_i,\s*int64_t\* counts_out,\s*int32_t\* dev_err,\s*"
                     r"void\* stream\s*\)\s*;", header)
    macros = dict(re.findall(r"#define (SGAN_TOPO_[A-Z0-9_]+) (\d+)", header))
    assert macros == {"SGAN_TOPO_COUNTS": "12", "SGAN_TOPO_SKEL_S": "7", "SGAN_TOPO_IMAGES": "11", "SGAN_TOPO_ERR_BIT": "256"}
    assert len(ops.TOPO_COUNTS) == 12 and ops.TOPO_COUNTS.index("skel_s") == 7 and ops.TOPO_COUNTS.index("images") == 11
    assert "sgan_topo_workspace_bytes" in _lib.SIGNATURES and "sgan_topo_accumulate" in _lib.SIGNATURES
    assert _lib.RESTYPES["sgan_topo_workspace_bytes"] is ctypes.c_int64
    lib = _lib.lib()
    # the workspace entry needs no device: 16 bytes per window, the geometry of util.topo_windows
    for H, W, window, stride in R.CASES:
        from supervised_gan_amd.util import topo_windows
        _, _, ys, xs = topo_windows(H, W, window, stride)
        assert lib.sgan_topo_workspace_bytes(H, W, window, stride) == 16 * len(ys) * len(xs), (H, W, window, stride)
    for window, stride in ((7, 7), (65, 65), (16, 0), (16, 17)):
        assert lib.sgan_topo_workspace_bytes(64, 64, window, stride) < 0 and b"not covered" in lib.sgan_last_error()
        # refused before anything else is looked at: return 1, nothing launched
        assert lib.sgan_topo_accumulate(None, 1, None, 1, None, None, 64, 64, window, stride, None, 0, None, None, None, None) == 1
        assert b"not covered" in lib.sgan_last_error()
    for H, W in ((0, 4), (4, 0), (1, 32769), (32768, 32768)):
        assert lib.sgan_topo_workspace_bytes(H, W, 64, 64) < 0
    assert lib.sgan_topo_accumulate(None, 1, None, 1, None, None, 64, 64, 64, 64, None, 0, None, None, None, None) == 1
    assert b"null" in lib.sgan_last_error()

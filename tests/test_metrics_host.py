"""CPU-only tests of the segmentation-metric layer: the C ABI's argument checks, the three train_ss.py options, the integer form of
the Rand F-score the device computes, the link rule of its labelling, and the `best` checkpoint rule of train_ss.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

import metrics_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_null_calls_fail_before_any_launch(built_lib):
    from supervised_gan_amd import _lib
    l = _lib.lib()
    assert l.sgan_ccl_label(None, 1, 8, 8, None, None, None) < 0 and b"null" in l.sgan_last_error()
    assert l.sgan_rand_f_accumulate(None, None, 8, 8, None, 0, None, None, None, None, None) < 0 and b"null" in l.sgan_last_error()
    assert l.sgan_confusion_accumulate(None, 4, 2, None, None, 0, 0, 64, None, None, None) < 0 and b"null" in l.sgan_last_error()
    assert l.sgan_rand_f_workspace(0, 8) < 0 and b"bad shape" in l.sgan_last_error()
    # >= 2 table slots per pixel, the counters and the four sums
    for H, W in ((1, 1), (37, 53), (512, 512)):
        assert l.sgan_rand_f_workspace(H, W) >= 32 + 2 * H * W * 12 + 2 * 4 * (H * W + 1)
    # a shape is refused before the pointers are looked at any further
    buf = (ctypes.c_int32 * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert l.sgan_ccl_label(p, 1, 0, 8, p, p, None) < 0 and b"bad shape" in l.sgan_last_error()
    assert l.sgan_confusion_accumulate(p, 4, 17, None, p, 4, 0, 64, p, p, None) < 0 and b"C = 17" in l.sgan_last_error()
    assert l.sgan_confusion_accumulate(p, 4, 2, p, p, 4, 0, 64, p, p, None) < 0 and b"exactly one" in l.sgan_last_error()


def test_train_ss_options_parse_with_the_reference_defaults(tmp_path):
    from supervised_gan_amd.options import TestOptions, TrainOptions
    base = ["--name", "t", "--model", "segmentation", "--gpu_ids", "-1", "--checkpoints_dir", str(tmp_path)]
    for cls in (TrainOptions, TestOptions):
        opt = cls().parse(base, save=False, verbose=False)
        assert opt.valSize == 0 and opt.save_val_visuals is False and opt.best_metric == 'None'
    opt = TrainOptions().parse(base + "--valSize 384 --save_val_visuals --best_metric RandScore".split(), save=False, verbose=False)
    assert opt.valSize == 384 and opt.save_val_visuals is True and opt.best_metric == 'RandScore'
    import train_ss
    val = train_ss.validation_options(TrainOptions().parse(base + ["--loadSize", "300"], save=False, verbose=False))
    assert (val.phase, val.batchSize, val.serial_batches, val.no_flip, val.no_rotate) == ('val', 1, True, True, True)
    assert val.valSize == val.loadSize == val.fineSize == 300


def test_integer_sums_reproduce_compute_Rand_F_scores():
    """F from (A2, B2, AB2, aux) is util.compute_Rand_F_scores with the common 1 / n^2 cancelled: equal to fp64 rounding on random and
    structured maps, NaN for an all-wall truth, 1 for two all-free maps."""
    from supervised_gan_amd.util import _label_false_regions, compute_Rand_F_scores
    rng = np.random.default_rng(11)
    worst = 0.0
    for H, W in ((37, 53), (64, 64), (96, 80), (130, 70), (512, 512)):
        for dt, ds in ((0.25, 0.3), (0.4, 0.4), (0.55, 0.2)):
            t, s = (rng.random((H, W)) < dt).astype(np.float32), (rng.random((H, W)) < ds).astype(np.float32)
            got = M.f_from_sums(*M.rand_sums(_label_false_regions(t > 0.5), _label_false_regions(s > 0.5)))
            worst = max(worst, abs(got - compute_Rand_F_scores(s, t)[0]))
    assert worst < 1e-12, worst
    grid = np.zeros((24, 24), np.float32)
    grid[:, 8] = grid[:, 16] = grid[12, :] = 1
    free, wall = np.zeros((8, 8), np.float32), np.ones((8, 8), np.float32)
    lab = lambda m: _label_false_regions(m > 0.5)      # noqa: E731
    assert M.f_from_sums(*M.rand_sums(lab(grid), lab(grid))) == 1.0
    assert M.f_from_sums(*M.rand_sums(lab(free), lab(free))) == 1.0
    with np.errstate(all="ignore"):
        assert np.isnan(M.f_from_sums(*M.rand_sums(lab(wall), lab(free)))) and np.isnan(compute_Rand_F_scores(free, wall)[0])
        assert abs(M.f_from_sums(*M.rand_sums(lab(free), lab(wall))) - compute_Rand_F_scores(wall, free)[0]) < 1e-15


@pytest.mark.parametrize("H,W", [(1, 1), (1, 40), (37, 53), (40, 70)])
def test_link_rule_gives_scipys_components(H, W):
    """Four links per pixel, two of them only when the others do not imply them, are enough for 8-connectivity; and "the smaller
    index is the parent" makes the root the component's first raster pixel, which orders the labels as scipy does."""
    for kind, (m, ref) in M.maps_and_labels(H, W).items():
        lab = M.link_rule_labels(m > 0.5)
        assert np.array_equal(M.canonical(lab), ref), kind
        if min(H, W) >= 2:       # the patterns that are built to be ONE component are
            assert kind not in ("serpentine", "checkerboard", "diagonal", "free") or ref.max() == 1, kind


class _Stub:
    def __init__(self):
        self.saved = []

    def save(self, label):
        self.saved.append(label)


def _run_rule(train_ss, best_metric, scores):
    """The driver's use of the rule after each validation pass, on a stub model."""
    stub, best = _Stub(), -1.0
    for score in scores:
        accs = {"RandScore": score, "meanIU": 0.1}
        if train_ss.should_save_best(best_metric, accs, best):
            best = float(accs[best_metric])
            stub.save('best')
    return stub.saved, best


def test_best_checkpoint_rule(tmp_path):
    """Strict improvement saves, a tie does not, a NaN never does; --best_metric 'None' never saves, whichever string object holds
    the word (the rule compares by value, not identity)."""
    import train_ss
    scores = (0.5, 0.5, float("nan"), 0.4, 0.7, np.float64("nan"), np.float64(0.7))
    saved, best = _run_rule(train_ss, "RandScore", scores)
    assert saved == ['best', 'best'] and best == 0.7
    assert _run_rule(train_ss, "RandScore", (float("nan"),)) == ([], -1.0)
    assert _run_rule(train_ss, "RandScore", (0.0,)) == (['best'], 0.0)          # the first finite score beats the initial -1
    none = ''.join(['No', 'ne'])          # an equal string that is not the interned literal, as argparse hands it over
    assert none == 'None' and none is not 'None'      # noqa: F632
    assert _run_rule(train_ss, none, scores) == ([], -1.0)                      # accs has no 'None' key: looked up only when the rule is on
    from supervised_gan_amd.options import TrainOptions
    parsed = TrainOptions().parse(["--name", "t", "--gpu_ids", "-1", "--checkpoints_dir", str(tmp_path), "--best_metric", none],
                                  save=False, verbose=False).best_metric
    assert _run_rule(train_ss, parsed, scores) == ([], -1.0)
    with pytest.raises(ValueError, match="best_metric"):
        train_ss.main(["--name", "t", "--model", "segmentation", "--gpu_ids", "-1", "--checkpoints_dir", str(tmp_path), "--dataroot", "synthetic",
                       "--which_metric", "meanIU", "--best_metric", "RandScore", "--fineSize", "32"])

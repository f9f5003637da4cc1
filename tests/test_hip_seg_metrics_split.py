"""GPU tests of --clean_split inside seg_metrics.SegMetrics: every label-based score equals the options-off path run on planes the
host yardsticks cleaned -- util.split_cells alone, and with all four options the stages in the order close, specks, split, small
cells (util.clean_wall without min_cell, util.split_cells, util.clean_wall with min_cell alone).

Tolerances as tests/test_hip_seg_metrics_clean.py, whose planes these are: the integer accumulators are equal; the Rand sums are one
fp64 expression of exact integers per image on both sides, 1e-12 absolute; VInfo's fp64 sums repeat to rounding, 1e-10 relative; SEG
and PQ are fp64 sums of at most N_t <= H W = 4096 terms in (0, 1] in scheduling order, N_t 2^-52 relative; the boundary sums are
added in slot order and repeat to the bit."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import clean_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
REL = 1e-10      # tests/test_hip_segm_thin.py
NAMES = ["RandScore", "VInfo", "meanIU", "RandScoreThin", "VInfoThin", "ObjF1", "ObjAP", "SEG", "PQ", "BoundF", "HausD", "ASSD"]
SPLIT = dict(clean_split=3.0, clean_split_rounds=64)      # split_rsq 9
ALL = dict(clean_close=1.5, clean_min_wall=4, clean_min_cell=40, **SPLIT)


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def _opt(**clean):
    return types.SimpleNamespace(which_metric=list(NAMES), min_object_area=3, boundary_thin=False, boundary_tolerance=2,
                                 add_background_onehot_acc=False, isTrain=False, **clean)


def _pairs(dev):
    """test_hip_seg_metrics_clean.py's three 64 x 64 (fake_B, real_B, logit, label): the truth's cell map with gaps, specks and tiny
    rings, as soft values."""
    out = []
    for k in range(3):
        truth = R.cell_map(64, 64, seed=k, gaps=0, specks=0)
        pred = R.cell_map(64, 64, seed=k, gaps=8, specks=8).copy()
        for y, x in ((9, 12 + k), (30, 40), (50, 21)):
            pred[y:y + 5, x:x + 5] = True
            pred[y + 1:y + 4, x + 1:x + 4] = False
        soft = np.where(pred, 0.9, 0.1).astype(np.float32)
        fake = torch.from_numpy(np.stack([soft, 1 - soft])[None]).to(dev)
        real = torch.from_numpy(np.stack([truth, ~truth]).astype(np.float32)[None]).to(dev)
        label = torch.from_numpy((~truth).astype(np.int64)[None]).to(dev)
        out.append((fake, real, fake.clone(), label))
    return out


def _stages(plane, close_rsq, min_wall, min_cell, split_rsq, rounds):
    """The four stages in the pipeline's order on the host: (mask, clean counts, split counts)."""
    from supervised_gan_amd import util
    mask, clean = plane > 0.5, np.zeros(6, dtype=np.int64)
    if close_rsq or min_wall:
        mask, c = util.clean_wall(mask, close_rsq, min_wall, 0)
        clean += c
    mask, split = util.split_cells(mask, split_rsq, rounds)
    if min_cell:
        mask, c = util.clean_wall(mask, 0, 0, min_cell)
        clean[:5] += c[:5]
        clean[5] = 1
    return mask, clean, split


def _same_scores(m, ref, got, want):
    assert list(got) == NAMES == list(want)
    for name in ("obj_i", "bnd_i", "conf"):
        assert torch.equal(m.acc[name], ref.acc[name]), name
    for name in ("rand", "rand_thin"):
        a, b = m.acc[name].cpu().tolist(), ref.acc[name].cpu().tolist()
        print(name, a, b)
        assert a[1] == b[1] == 3.0 and abs(a[0] - b[0]) <= 1e-12, name
    for key in NAMES:
        print(key, got[key], want[key])
        if key in ("RandScore", "RandScoreThin"):
            assert abs(got[key] - want[key]) <= 1e-12, key
        elif key in ("meanIU", "ObjF1", "ObjAP", "BoundF", "HausD", "ASSD"):
            assert got[key] == want[key], key
        elif key in ("SEG", "PQ"):
            assert abs(got[key] - want[key]) <= 64 * 64 * 2.0 ** -52 * abs(want[key]), key
        else:
            assert abs(got[key] - want[key]) <= REL * abs(want[key]), key


@pytest.mark.parametrize("options", (SPLIT, ALL), ids=("split_only", "all_four"))
def test_scores_are_those_of_the_plain_path_on_yardstick_cleaned_planes(options, capsys):
    from supervised_gan_amd import ops, util
    from supervised_gan_amd.options import clean_params, split_params
    from supervised_gan_amd.seg_metrics import SegMetrics
    dev = _dev()
    m = SegMetrics(_opt(**options), dev, 2)
    ref = SegMetrics(_opt(), dev, 2)
    params = clean_params(m.opt) + split_params(m.opt)
    assert params == ((2, 4, 40) if options is ALL else (0, 0, 0)) + (9, 64)
    clean_total, split_total, order_matters = np.zeros(6, dtype=np.int64), np.zeros(6, dtype=np.int64), 0
    for fake, real, logit, label in _pairs(dev):
        m.accumulate(fake, real, logit, label)
        plane = fake[0, 0].cpu().numpy()
        mask, clean, split = _stages(plane, *params)
        clean_total += clean
        split_total += split
        assert torch.equal(m.cleaned.cpu(), torch.from_numpy(mask.astype(np.float32)))
        if options is ALL:      # the small cells filled BEFORE the split, and the split before everything else, give other maps
            early = util.split_cells(util.clean_wall(plane, 2, 4, 40)[0], 9, 64)[0]
            first = util.clean_wall(util.split_cells(plane, 9, 64)[0], 2, 4, 40)[0]
            order_matters += int((early != mask).any()) + int((first != mask).any())
        cleaned = fake.clone()
        cleaned[0, 0] = torch.from_numpy(mask.astype(np.float32)).to(dev)
        ref.accumulate(cleaned, real, logit, label)
    assert split_total[0] > 0 and split_total[1] > 0 and split_total[5] == 3, split_total      # the split cut the predictions
    assert list(m.counts("split").values()) == split_total.tolist() and list(m.counts("split")) == list(ops.SPLIT_COUNTS)
    assert set(ref.counts("split").values()) == {0} and "split_i" not in ref.acc and ref.cleaned is None
    if options is ALL:
        assert order_matters >= 2 and clean_total[0] > 0 and clean_total[2] > 0 and clean_total[4] > 0, (order_matters, clean_total)
        assert list(m.counts("clean").values()) == clean_total.tolist()
    else:
        assert "clean_i" not in m.acc and "clean_post_i" not in m.acc and set(m.counts("clean").values()) == {0}
    capsys.readouterr()
    got = m.read()
    lines = capsys.readouterr().out.splitlines()
    want = ref.read()
    assert not [l for l in capsys.readouterr().out.splitlines() if l.startswith(("clean:", "split:"))]
    line = "split: %d cores, cut %d pixels, labelled %d pixels in %d rounds, budget hit in %d of %d images (split_rsq 9, 64 rounds)"
    at = [i for i, l in enumerate(lines) if l.startswith("split:")]
    assert len(at) == 1 and lines[at[0]] == line % tuple(split_total), lines
    if options is ALL:
        clean_line = "clean: closed %d pixels, removed %d wall components (%d pixels), filled %d cells (%d pixels) in 3 images" % tuple(clean_total[:5])
        assert lines[at[0] - 1].startswith(clean_line), lines      # the split line comes right after the clean line
    else:
        assert not [l for l in lines if l.startswith("clean:")]
    _same_scores(m, ref, got, want)
    raw = SegMetrics(_opt(), dev, 2)      # the stage moved the scores: the raw predictions give other integers
    for fake, real, logit, label in _pairs(dev):
        raw.accumulate(fake, real, logit, label)
    assert not torch.equal(raw.acc["obj_i"], m.acc["obj_i"]) and not torch.equal(raw.acc["bnd_i"], m.acc["bnd_i"])
    assert torch.equal(raw.acc["conf"], m.acc["conf"])           # meanIU stays on the logits


def test_with_the_option_off_the_calls_are_the_parents():
    """--clean_split 0 with the other three set: one clean_wall call with all three parameters, no split workspace, no split
    counters, and the plane and counts of util.clean_wall."""
    from supervised_gan_amd import ops, util
    from supervised_gan_amd.seg_metrics import SegMetrics
    dev = _dev()
    for extra in ({}, dict(clean_split=0.0, clean_split_rounds=64), dict(clean_split=0.9)):      # floor(0.81) = 0
        m = SegMetrics(_opt(clean_close=1.5, clean_min_wall=4, clean_min_cell=10, **extra), dev, 2)
        for k in [k for k in ops._metric_ws if k[0] == "sgan_split_workspace"]:
            del ops._metric_ws[k]
        fake, real, logit, label = _pairs(dev)[0]
        m.accumulate(fake, real, logit, label)
        m.read()
        mask, counts = util.clean_wall(fake[0, 0].cpu().numpy(), 2, 4, 10)
        assert torch.equal(m.cleaned.cpu(), torch.from_numpy(mask.astype(np.float32)))
        assert list(m.counts("clean").values()) == counts.tolist()
        assert "split_i" not in m.acc and "clean_post_i" not in m.acc and "cleaned_mid" not in m.planes
        assert not [k for k in ops._metric_ws if k[0] == "sgan_split_workspace"]

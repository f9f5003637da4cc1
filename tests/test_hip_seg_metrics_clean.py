"""GPU tests of the cleaned prediction inside seg_metrics.SegMetrics: with --clean_close 1.5 --clean_min_wall 4 --clean_min_cell 10
every label-based score equals the options-off path run on planes the host yardstick util.clean_wall cleaned.

Tolerances: the integer accumulators are equal.  The Rand sums are one fp64 expression of exact integers per image on both sides,
compared to 1e-12 absolute as tests/test_hip_segm_thin.py compares them; VInfo's fp64 sums repeat to rounding, not to the bit: that
file's 1e-10 relative.  SEG and PQ are fp64 sums of at most N_t terms in (0, 1] in scheduling order, N_t 2^-52 relative
(include/sgan_hip.h) with N_t <= H W = 4096; the boundary sums are added in slot order and repeat to the bit."""
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


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def _opt(**clean):
    return types.SimpleNamespace(which_metric=list(NAMES), min_object_area=3, boundary_thin=False, boundary_tolerance=2,
                                 add_background_onehot_acc=False, isTrain=False, **clean)


def _pairs(dev):
    """Three 64 x 64 (fake_B, real_B, logit, label): the prediction is the truth's cell map with gaps, specks and tiny rings, as soft values."""
    out = []
    for k in range(3):
        truth = R.cell_map(64, 64, seed=k, gaps=0, specks=0)
        pred = R.cell_map(64, 64, seed=k, gaps=8, specks=8).copy()
        for y, x in ((9, 12 + k), (30, 40), (50, 21)):          # rings around 3 x 3 free pixels, which the 3 x 3 box does not close: regions too small to be a cell
            pred[y:y + 5, x:x + 5] = True
            pred[y + 1:y + 4, x + 1:x + 4] = False
        soft = np.where(pred, 0.9, 0.1).astype(np.float32)
        fake = torch.from_numpy(np.stack([soft, 1 - soft])[None]).to(dev)
        real = torch.from_numpy(np.stack([truth, ~truth]).astype(np.float32)[None]).to(dev)
        label = torch.from_numpy((~truth).astype(np.int64)[None]).to(dev)
        out.append((fake, real, fake.clone(), label))
    return out


def test_scores_are_those_of_the_parents_path_on_cleaned_planes(capsys):
    from supervised_gan_amd import ops, util
    from supervised_gan_amd.seg_metrics import SegMetrics
    dev = _dev()
    params = (2, 4, 10)
    m = SegMetrics(_opt(clean_close=1.5, clean_min_wall=4, clean_min_cell=10), dev, 2)
    ref = SegMetrics(_opt(), dev, 2)
    total = np.zeros(6, dtype=np.int64)
    for fake, real, logit, label in _pairs(dev):
        m.accumulate(fake, real, logit, label)
        mask, counts = util.clean_wall(fake[0, 0].cpu().numpy(), *params)
        total += counts
        assert torch.equal(m.cleaned.cpu(), torch.from_numpy(mask.astype(np.float32)))
        cleaned = fake.clone()
        cleaned[0, 0] = torch.from_numpy(mask.astype(np.float32)).to(dev)
        ref.accumulate(cleaned, real, logit, label)
    assert total[0] > 0 and total[2] > 0 and total[4] > 0, total      # every stage changed the predictions
    assert "cleaned" in m.planes and "cleaned" not in ref.planes and "clean_i" not in ref.acc and ref.cleaned is None
    assert list(m.counts("clean").values()) == total.tolist() and list(m.counts("clean")) == list(ops.CLEAN_COUNTS)
    assert set(ref.counts("clean").values()) == {0}
    capsys.readouterr()
    got = m.read()
    printed = capsys.readouterr().out
    want = ref.read()
    assert "clean: closed %d pixels, removed %d wall components (%d pixels), filled %d cells (%d pixels) in 3 images" % tuple(total[:5]) in printed
    assert "clean:" not in capsys.readouterr().out
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
        elif key in ("meanIU", "ObjF1", "ObjAP", "BoundF", "HausD", "ASSD"):      # functions of the equal integers, and of fp64 sums taken in slot order
            assert got[key] == want[key], key
        elif key in ("SEG", "PQ"):                                # fp64 sums of at most N_t <= H W terms in scheduling order
            assert abs(got[key] - want[key]) <= 64 * 64 * 2.0 ** -52 * abs(want[key]), key
        else:                                                     # VInfo, VInfoThin
            assert abs(got[key] - want[key]) <= REL * abs(want[key]), key
    # the cleaning moved the scores: the raw predictions give other integers
    raw = SegMetrics(_opt(), dev, 2)
    for fake, real, logit, label in _pairs(dev):
        raw.accumulate(fake, real, logit, label)
    assert not torch.equal(raw.acc["obj_i"], m.acc["obj_i"]) and not torch.equal(raw.acc["bnd_i"], m.acc["bnd_i"])
    assert torch.equal(raw.acc["conf"], m.acc["conf"])           # meanIU stays on the logits


def test_with_the_options_off_nothing_is_added():
    from supervised_gan_amd import ops
    from supervised_gan_amd.seg_metrics import SegMetrics
    dev = _dev()
    for opt in (_opt(), _opt(clean_close=0.0, clean_min_wall=0, clean_min_cell=0), _opt(clean_close=0.9)):      # floor(0.81) = 0
        m = SegMetrics(opt, dev, 2)
        for k in [k for k in ops._metric_ws if k[0] == "sgan_clean_workspace"]:
            del ops._metric_ws[k]
        fake, real, logit, label = _pairs(dev)[0]
        m.accumulate(fake, real, logit, label)
        m.read()
        assert "cleaned" not in m.planes and m.cleaned is None and "clean_i" not in m.acc
        assert not [k for k in ops._metric_ws if k[0] == "sgan_clean_workspace"]
        assert sorted(m.planes) == ["pred_dsq", "pred_labels", "thinned", "thinned_labels", "truth_dsq", "truth_labels"]

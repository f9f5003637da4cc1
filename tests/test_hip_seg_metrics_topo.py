"""GPU tests of the topology scores inside seg_metrics.SegMetrics, without a model: 64 x 64 pairs with
--which_metric RandScoreThin clDice Betti0Err Betti1Err.  read() equals util.topo_scores of util.topo_counts pooled over the pairs,
the prediction is thinned once for RandScoreThin and clDice, --clean_close 1.5 scores util.clean_wall's map, and with none of the
three names nothing of it exists.  The counters are exact integers and the scores one host function of them: no tolerance."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import clean_ref as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
ASKED = ["RandScoreThin", "clDice", "Betti0Err", "Betti1Err"]
WINDOW, STRIDE = 32, 16


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def _opt(which=ASKED, **more):
    return types.SimpleNamespace(which_metric=list(which), min_object_area=1, boundary_thin=False, boundary_tolerance=2,
                                 add_background_onehot_acc=False, isTrain=False, topo_window=WINDOW, topo_stride=STRIDE, **more)


def _pairs(dev):
    """Three 64 x 64 (fake_B, real_B, logit, label, the prediction's wall, the truth's wall): the truth's cell map with gaps and specks."""
    out = []
    for k in range(3):
        truth = C.cell_map(64, 64, seed=k, gaps=0, specks=0)
        pred = C.cell_map(64, 64, seed=k, gaps=8, specks=8)
        soft = np.where(pred, 0.9, 0.1).astype(np.float32)
        fake = torch.from_numpy(np.stack([soft, 1 - soft])[None]).to(dev)
        real = torch.from_numpy(np.stack([truth, ~truth]).astype(np.float32)[None]).to(dev)
        label = torch.from_numpy((~truth).astype(np.int64)[None]).to(dev)
        out.append((fake, real, fake.clone(), label, pred, truth))
    return out


def _host_total(pairs, clean=None):
    from supervised_gan_amd import util
    total = np.zeros(12, dtype=np.int64)
    for *_, pred, truth in pairs:
        if clean is not None:
            pred, _ = util.clean_wall(pred, *clean)
        total += util.topo_counts(pred, truth, WINDOW, STRIDE, s_thin=util.thin(pred)[0], t_thin=util.thin(truth)[0])
    return total


def test_read_equals_the_yardstick_and_the_prediction_is_thinned_once(capsys, monkeypatch):
    from supervised_gan_amd import ops, util
    from supervised_gan_amd.seg_metrics import SegMetrics
    dev = _dev()
    thinned = []
    real_thin = ops.thin
    monkeypatch.setattr(ops, "thin", lambda plane, **kw: (thinned.append(plane.data_ptr()), real_thin(plane, **kw))[1])
    m = SegMetrics(_opt(), dev, 2)
    pairs = _pairs(dev)
    for fake, real, logit, label, _, _ in pairs:
        m.accumulate(fake, real, logit, label)
    # per image: the prediction once (shared by RandScoreThin and clDice), the truth once
    assert len(thinned) == 6 and thinned[0::2] == [p[0].data_ptr() for p in pairs] and thinned[1::2] == [p[1].data_ptr() for p in pairs]
    assert sorted(m.planes) == ["thinned", "thinned_labels", "thinned_truth", "truth_labels"]
    want = _host_total(pairs)
    assert want[1] > 0 and want[2] > 0 and 0 < want[8] < want[7] and 0 < want[10] <= want[9]      # the gaps and specks moved every score
    assert list(m.counts("topology")) == list(ops.TOPO_COUNTS) and list(m.counts("topology").values()) == want.tolist()
    capsys.readouterr()
    got = m.read()
    printed = capsys.readouterr().out
    scores = util.topo_scores(want)
    assert list(got) == ["RandScoreThin", "Betti0Err", "Betti1Err", "clDice"]
    assert all(got[k] == scores[k] for k in util.TOPO_METRICS) and m.values["numAveragedImages"] == 3
    assert ("topology: %d windows of %d at stride %d, mean b0 / b1 of the prediction" % (want[0], WINDOW, STRIDE)) in printed
    assert want[0] == 3 * 9
    # the thinned truth is the device thinning of the last truth plane
    assert torch.equal(m.planes["thinned_truth"].cpu(), torch.from_numpy(util.thin(pairs[-1][5])[0].astype(np.float32)))
    # Betti errors alone: no thinning at all
    del thinned[:]
    b = SegMetrics(_opt(["Betti0Err", "Betti1Err"]), dev, 2)
    for fake, real, logit, label, _, _ in pairs:
        b.accumulate(fake, real, logit, label)
    assert not thinned and not b.planes and b.counts("topology")["skel_s"] == 0 and b.counts("topology")["skel_t"] == 0
    assert list(b.counts("topology").values())[:7] == want[:7].tolist()
    assert dict(b.read()) == {k: scores[k] for k in ("Betti0Err", "Betti1Err")}


def test_with_clean_close_the_scores_are_those_of_the_cleaned_map():
    from supervised_gan_amd import util
    from supervised_gan_amd.seg_metrics import SegMetrics
    dev = _dev()
    m = SegMetrics(_opt(clean_close=1.5, clean_min_wall=0, clean_min_cell=0), dev, 2)
    pairs = _pairs(dev)
    for fake, real, logit, label, _, _ in pairs:
        m.accumulate(fake, real, logit, label)
    want, raw = _host_total(pairs, clean=(2, 0, 0)), _host_total(pairs)
    assert want.tolist() != raw.tolist() and want[3] < raw[3]        # the closing joined wall fragments: fewer wall components in the prediction
    assert list(m.counts("topology").values()) == want.tolist()
    got, scores = m.read(), util.topo_scores(want)
    assert all(got[k] == scores[k] for k in util.TOPO_METRICS)


def test_with_none_of_the_three_names_nothing_is_added():
    from supervised_gan_amd import ops
    from supervised_gan_amd.seg_metrics import SegMetrics
    dev = _dev()
    ops._topo_ws.clear()
    m = SegMetrics(_opt(["RandScoreThin", "BoundF"]), dev, 2)
    fake, real, logit, label, _, _ = _pairs(dev)[0]
    m.accumulate(fake, real, logit, label)
    got = m.read()
    assert list(got) == ["RandScoreThin", "BoundF"] and "topo_i" not in m.acc and "thinned_truth" not in m.planes and not ops._topo_ws
    assert set(m.counts("topology").values()) == {0}
    assert m.values["clDice"] == 0 and m.values["Betti0Err"] == 0

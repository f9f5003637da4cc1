"""CPU tests of seg_metrics.SegMetrics, the owner of the segmentation accuracy state: the launch plan of accumulate() for every
combination of scores the trainers share work between (recorded from the accum_accs this class replaced, with the same stub), which
tensor goes where, a map size that changes between calls, and the read-back arithmetic on hand-filled accumulators."""
import types

import numpy as np
import pytest
import torch

THIN_BOTH = ["RandScoreThin", "VInfoThin"]
EVERY = ["RandScore", "VInfo", "meanIU", "RandScoreThin", "VInfoThin", "ObjF1", "BoundF"]
# --which_metric, --boundary_thin, the launches of one accumulate()
PLAN = [
    (["RandScore"], False, "ccl ccl rand_f"),
    (["VInfo"], False, "ccl ccl vinfo"),
    (["RandScore", "VInfo"], False, "ccl ccl vinfo"),
    (["ObjF1"], False, "ccl ccl object_match"),
    (["RandScore", "SEG"], False, "ccl ccl rand_f object_match"),
    (["VInfoThin"], False, "ccl thin ccl vinfo"),
    (["RandScoreThin"], False, "ccl thin ccl rand_f"),
    (THIN_BOTH, False, "ccl thin ccl vinfo"),
    (["RandScore", "RandScoreThin"], False, "ccl ccl rand_f thin ccl rand_f"),
    (["PQ", "VInfoThin"], False, "ccl ccl object_match thin ccl vinfo"),
    (["meanIU"], False, "as_nhwc confusion"),
    (["BoundF"], False, "edt edt boundary"),
    (["BoundF"], True, "thin edt edt boundary"),
    (["HausD", "RandScoreThin"], True, "ccl thin ccl rand_f edt edt boundary"),
    (EVERY, True, "ccl ccl vinfo object_match thin ccl vinfo as_nhwc confusion edt edt boundary"),
]


def _opt(which, boundary_thin=False, isTrain=True):
    return types.SimpleNamespace(which_metric=list(which), min_object_area=3, boundary_thin=boundary_thin, boundary_tolerance=2,
                                 add_background_onehot_acc=False, isTrain=isTrain)


@pytest.fixture
def calls(monkeypatch):
    """ops' metric entry points replaced by recorders of (short name, args, kwargs) that hand back their out / labels argument."""
    from supervised_gan_amd import ops
    rec = []

    def recorder(short, returns):
        def f(*a, **k):
            rec.append((short, a, k))
            return returns(a, k)
        return f
    monkeypatch.setattr(ops, "ccl_label", recorder("ccl", lambda a, k: a[1]))
    monkeypatch.setattr(ops, "thin", recorder("thin", lambda a, k: k["out"]))
    monkeypatch.setattr(ops, "edt_sq", recorder("edt", lambda a, k: k["out"]))
    monkeypatch.setattr(ops, "as_nhwc", recorder("as_nhwc", lambda a, k: a[0]))
    for name in ("rand_f", "vinfo", "object_match", "boundary", "confusion"):
        monkeypatch.setattr(ops, name + "_accumulate", recorder(name, lambda a, k: None))
    return rec


def _accumulate(m, n):
    z = torch.zeros(1, 2, n, n)
    m.accumulate(z, z.clone(), z.clone(), torch.zeros(1, n, n, dtype=torch.int64))


@pytest.mark.parametrize("which,boundary_thin,plan", PLAN, ids=["+".join(w) + ("+bt" if bt else "") for w, bt, _ in PLAN])
def test_launch_plan_and_which_tensor_goes_where(calls, which, boundary_thin, plan):
    from supervised_gan_amd.seg_metrics import SegMetrics
    m = SegMetrics(_opt(which, boundary_thin), torch.device("cpu"), 2)
    assert not m.acc and not m.planes and m.truth_labels is None          # nothing exists before a score asks for it
    for n in (8, 8, 16):                                                  # the same plan when the planes exist, and at a new size
        del calls[:]
        _accumulate(m, n)
        assert " ".join(c[0] for c in calls) == plan
        named = {}
        for short, a, k in calls:
            named.setdefault(short, []).append((a, k))
            for t in list(a[:2]) + [k.get("out")]:                        # every plane a recorder is handed has this call's size
                if torch.is_tensor(t) and short not in ("as_nhwc", "confusion"):
                    assert tuple(t.shape)[-2:] == (n, n), (short, t.shape)
        counting = [a for short in ("rand_f", "vinfo", "object_match") for a, _ in named.get(short, [])]
        if "ccl" in named:                                                # the truth is labelled first and once; every count reads it
            truth = named["ccl"][0][0][1]
            assert truth is m.truth_labels and all(a[0] is truth for a in counting)
            assert all(a[1] is not truth for a in counting)
            assert sum(1 for a, _ in named["ccl"] if a[1] is truth) == 1
        else:
            assert not counting and m.truth_labels is None
        if "thin" in named:
            (a, k), = named["thin"]
            thinned = k["out"]
            if "RandScoreThin" in which or "VInfoThin" in which:          # labelled as it lies, once
                assert sum(1 for a, _ in named["ccl"] if a[0] is thinned) == 1
            if "edt" in named:                                            # --boundary_thin: the second transform reads that plane
                assert named["edt"][1][0][0] is thinned
        if "boundary" in named:
            (a, k), = named["boundary"]
            assert a[0] is named["edt"][0][1]["out"] and a[1] is named["edt"][1][1]["out"] and a[0] is not a[1]
            assert a[2] is m.acc["bnd_i"] and a[3] is m.acc["bnd_f"]
        if "object_match" in named:
            (a, k), = named["object_match"]
            assert a[2] is m.acc["obj_i"] and a[3] is m.acc["obj_f"] and k == {"min_area": 3}
        if "confusion" in named:
            (a, k), = named["confusion"]
            assert a[1] == 2 and a[2] is m.acc["conf"] and tuple(k["label"].shape) == (1, n, n)
    # the accumulators the counting calls were handed, per row
    vinfo = [(a, k) for short, a, k in calls if short == "vinfo"]
    rand = [(a, k) for short, a, k in calls if short == "rand_f"]
    if which == ["RandScore", "VInfo"]:
        assert vinfo[0][0][2] is m.acc["vinfo"] and vinfo[0][1]["acc_rand"] is m.acc["rand"]
    if which == ["VInfo"]:
        assert vinfo[0][0][2] is m.acc["vinfo"] and vinfo[0][1]["acc_rand"] is None and "rand" not in m.acc
    if which == THIN_BOTH:
        assert vinfo[0][0][2] is m.acc["vinfo_thin"] and vinfo[0][1]["acc_rand"] is m.acc["rand_thin"] and sorted(m.acc) == ["rand_thin", "vinfo_thin"]
    if which == ["RandScore", "RandScoreThin"]:
        assert rand[0][0][2] is m.acc["rand"] and rand[1][0][2] is m.acc["rand_thin"]
    if which == EVERY:
        assert vinfo[0][1]["acc_rand"] is m.acc["rand"] and vinfo[1][0][2] is m.acc["vinfo_thin"] and vinfo[1][1]["acc_rand"] is m.acc["rand_thin"]
        assert sorted(m.acc) == ["bnd_f", "bnd_i", "conf", "obj_f", "obj_i", "rand", "rand_thin", "vinfo", "vinfo_thin"]
    if which == ["meanIU"]:
        assert sorted(m.acc) == ["conf"] and not m.planes                 # a score that was never asked for made nothing


def test_options_are_read_at_each_call(calls):
    """which_metric, --boundary_thin, --min_object_area and the background class of the confusion matrix follow the options object."""
    from supervised_gan_amd.seg_metrics import SegMetrics
    opt = _opt(["RandScore"])
    m = SegMetrics(opt, torch.device("cpu"), 2)
    _accumulate(m, 8)
    opt.which_metric, opt.boundary_thin, opt.min_object_area = ["BoundF", "SEG"], True, 7
    del calls[:]
    _accumulate(m, 8)
    assert " ".join(c[0] for c in calls) == "ccl ccl object_match thin edt edt boundary" and calls[2][2] == {"min_area": 7}
    opt.which_metric, opt.add_background_onehot_acc = ["meanIU"], True
    del calls[:]
    _accumulate(m, 8)
    assert [c[0] for c in calls] == ["as_nhwc", "as_nhwc", "confusion"] and calls[2][2]["add_background"] is True
    assert tuple(m.acc["conf"].shape) == (3, 3)
    with pytest.raises(AssertionError):                                   # binary segmentation only, for everything but meanIU
        opt.which_metric = ["RandScore"]
        SegMetrics(opt, torch.device("cpu"), 3).accumulate(*[torch.zeros(1, 3, 8, 8)] * 3, torch.zeros(1, 8, 8, dtype=torch.int64))
    with pytest.raises(AssertionError):                                   # batch 1
        SegMetrics(opt, torch.device("cpu"), 2).accumulate(*[torch.zeros(2, 2, 8, 8)] * 3, torch.zeros(2, 8, 8, dtype=torch.int64))


ALL = ["RandScore", "VInfo", "meanIU", "RandScoreThin", "VInfoThin", "ObjF1", "ObjAP", "SEG", "PQ", "BoundF", "HausD", "ASSD"]
OBJ_I = [9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 12, 11, 3, 7, 0, 0]
OBJ_F = [6.5, 5.25]
BND_I = [10, 6, 4, 2, 1, 1] + [0] * 25 + [1] + [12, 5, 3, 2, 2] + [0] * 27 + [25, 24, 2, 2, 24, 24, 25, 36] + [0] * 8
BND_F = [20.5, 18.25, 11.0, 0.0]
CONF = [[50, 10], [6, 62]]
# what the get_current_accs this class replaced printed for these counters, built for evaluation
PRINTED = ("objects: TP at IoU > 0.50 .. 0.95: 9 8 7 6 5 4 3 2 1 0, N_t 12, N_s 11 (min area 3)\n"
           "boundary: P/R/F at tolerance 0 .. 5: 0.4000/0.5000/0.4444 0.6400/0.7083/0.6724 0.8000/0.8333/0.8163 0.8800/0.9167/0.8980 "
           "0.9200/1.0000/0.9583 0.9600/1.0000/0.9796, worst distance 6.000 (N_s 25, N_t 24%s)\n")


def _filled(which, isTrain=True, boundary_thin=False):
    from supervised_gan_amd.seg_metrics import ACCUMULATORS, SegMetrics
    m = SegMetrics(_opt(which, boundary_thin, isTrain), torch.device("cpu"), 2)
    fill = {"rand": [1.5, 2.0], "vinfo": [1.25, 2.0], "conf": CONF, "rand_thin": [2.25, 3.0], "vinfo_thin": [0.75, 3.0],
            "obj_i": OBJ_I, "obj_f": OBJ_F, "bnd_i": BND_I, "bnd_f": BND_F}
    assert [n for n, _, _ in ACCUMULATORS] == list(fill)
    for name, dtype, _ in ACCUMULATORS:
        m._acc(name).copy_(torch.tensor(fill[name], dtype=dtype))
    return m


def test_read_back_values_key_order_and_reset(capsys):
    from supervised_gan_amd import ops, util
    m = _filled(ALL)
    accs = m.read()
    assert capsys.readouterr().out == ""                                  # a trainer built for training prints nothing
    conf = np.array(CONF, dtype=np.float64)
    rel, sel, tp = conf.sum(axis=1), conf.sum(axis=0), np.diag(conf)
    want = {"RandScore": 0.75, "VInfo": 0.625, "meanIU": float(np.mean(tp / np.maximum(1, rel + sel - tp))), "RandScoreThin": 0.75, "VInfoThin": 0.25}
    want.update(util.object_scores(np.array(OBJ_I), np.array(OBJ_F)))
    want.update(util.boundary_scores(np.array(BND_I), np.array(BND_F), 2))
    assert list(accs) == ALL and dict(accs) == want
    v = m.values
    assert v["numAveragedImages"] == 3 and v["numAveragedPixels"] == 128 and np.array_equal(v["confusion"], conf)
    assert v["pixelAcc"] == tp.sum() / max(1, 128) == 0.875 and v["meanAcc"] == float(np.mean(tp / np.maximum(1, rel)))
    assert all(v[k] == accs[k] for k in ALL)
    # the keys follow the request, in the documented order, whatever the order they were asked in
    for which in (["meanIU", "RandScore"], ["PQ", "VInfoThin", "HausD", "ObjF1"], ["ASSD", "BoundF", "VInfo", "RandScoreThin"]):
        m.opt.which_metric = which
        got = m.read()
        assert list(got) == [k for k in ALL if k in which] and all(got[k] == want[k] for k in which)
    # the image count is the largest of the families'
    m.acc["bnd_i"][ops.BOUNDARY_COUNTS.index("images")] = 5
    m.read()
    assert m.values["numAveragedImages"] == 5
    m.acc["rand"][1] = 8
    m.read()
    assert m.values["numAveragedImages"] == 8 and m.values["RandScore"] == 1.5 / 8
    counts = m.counts("objects")
    assert list(counts) == list(ops.OBJECT_COUNTS + ops.OBJECT_SUMS) and list(counts.values()) == OBJ_I + OBJ_F
    counts = m.counts("boundary")
    assert list(counts) == list(ops.BOUNDARY_COUNTS + ops.BOUNDARY_SUMS) and [counts[k] for k in ops.BOUNDARY_COUNTS[:72]] == BND_I[:66] + [5] + BND_I[67:72]
    # reset: every accumulator and every value back to 0
    m.opt.which_metric = ALL
    m.reset()
    assert all(not t.any() for t in m.acc.values()) and set(m.values.values()) == {0}
    accs = m.read()
    assert list(accs) == ALL and all(x == 0 for x in accs.values()) and m.values["numAveragedImages"] == 0 == m.values["numAveragedPixels"]
    assert m.counts("objects")["images"] == 0 and m.counts("boundary")["images"] == 0


def test_a_family_that_never_ran_reads_zero(capsys):
    """Only the confusion matrix was ever taken: the other scores read 0, the counts are zeros, and evaluation prints no table."""
    from supervised_gan_amd.seg_metrics import SegMetrics
    m = SegMetrics(_opt(ALL, isTrain=False), torch.device("cpu"), 2)
    assert all(x == 0 for x in m.read().values()) and not m.acc
    m._acc("conf").copy_(torch.tensor(CONF))
    accs = m.read()
    assert accs["meanIU"] == 0.7762237762237763 and all(accs[k] == 0 for k in ALL if k != "meanIU")
    assert m.values["numAveragedImages"] == 0 and set(m.counts("objects").values()) == {0} == set(m.counts("boundary").values())
    assert capsys.readouterr().out == "" and sorted(m.acc) == ["conf"]


@pytest.mark.parametrize("boundary_thin", [False, True])
def test_evaluation_prints_the_two_tables(capsys, boundary_thin):
    m = _filled(ALL, isTrain=False, boundary_thin=boundary_thin)
    m.read()
    assert capsys.readouterr().out == PRINTED % (", prediction thinned" if boundary_thin else "")
    m.opt.which_metric = ["RandScore", "SEG"]                             # each table only with a score of its family
    m.read()
    assert capsys.readouterr().out == PRINTED.split("\n")[0] + "\n"
    m.opt.which_metric = ["RandScore", "meanIU"]
    m.read()
    assert capsys.readouterr().out == ""


def test_trainer_methods_mirror_the_values(calls):
    """SegMetricsMixin: the public names the drivers call, and what read() derived as attributes of the trainer."""
    from supervised_gan_amd.seg_metrics import SegMetricsMixin

    class Trainer(SegMetricsMixin):
        pass
    t = Trainer()
    t.seg_metrics = _filled(["RandScore", "meanIU", "PQ"])
    assert list(t.get_current_accs()) == ["RandScore", "meanIU", "PQ"]
    assert (t.RandScore, t.numAveragedImages, t.numAveragedPixels, t.pixelAcc, t.HausD) == (0.75, 3, 128, 0.875, 5.5)
    assert np.array_equal(t.confusion, np.array(CONF, dtype=np.float64))
    assert t.get_object_counts()["N_t"] == 12 and t.get_boundary_counts()["max_dsq_t"] == 36
    t.reset_accs()
    assert (t.RandScore, t.meanIU, t.numAveragedImages, t.confusion) == (0, 0, 0, 0) and t.get_object_counts()["N_t"] == 0
    t.fake_B, t.real_B, t.logit, t.label = torch.zeros(1, 2, 8, 8), torch.zeros(1, 2, 8, 8), torch.zeros(1, 2, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int64)
    t.accum_accs()
    t.compute_current_Rand_score()          # the reference's two method names: that score alone, whatever --which_metric says
    t.compute_current_accuracy()
    assert " ".join(c[0] for c in calls) == "ccl ccl rand_f object_match as_nhwc confusion ccl ccl rand_f as_nhwc confusion"

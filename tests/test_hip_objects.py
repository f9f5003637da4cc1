"""GPU tests of the object-level scores on the device (sgan_object_match_accumulate in sgan_metrics.hip): the 16 integers and the two
fp64 sums against the host yardstick util.object_match_counts, repeatability, the workspace paths, the refusals, graph capture, the
neighbouring Rand / VInfo entries, the trainers' ObjF1 / ObjAP / SEG / PQ and the train_ss.py / test_ss.py drivers.

Tolerance: the integers are equal.  SIoU and SSEG are sums of at most N_t correctly rounded quotients in (0, 1] added in an order that
depends on scheduling, against the yardstick's correctly rounded sum of the same quotients: N_t 2^-52 relative (one term: equal)."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import objects_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
MIN_AREAS = (1, 5)


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _want(H, W, name, min_area):
    """The yardstick on one case, computed once: (16 ints, 2 floats)."""
    from supervised_gan_amd.util import object_match_counts
    s, t = R.cases(H, W)[name]
    counts, sums = object_match_counts(s, t, min_area)
    return counts.tolist(), sums.tolist()


def _sums_close(got, want, n_t):
    return all(abs(g - w) <= max(1, n_t) * 2.0 ** -52 * abs(w) for g, w in zip(got, want))


def _labels(dev, s, t):
    from supervised_gan_amd import ops
    return ops.ccl_label(torch.from_numpy(np.array(t)).to(dev)), ops.ccl_label(torch.from_numpy(np.array(s)).to(dev))


def _fresh(dev):
    return torch.zeros(16, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.float64, device=dev)


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_counts_equal_the_host_yardstick(H, W):
    from supervised_gan_amd import ops
    dev = _dev()
    ws = ops.object_match_workspace(H, W, dev).clone()
    ws.fill_(-1)                                           # garbage on entry: the call initialises what it uses
    for name, (s, t) in R.cases(H, W).items():
        t_lab, s_lab = _labels(dev, s, t)
        for min_area in MIN_AREAS:
            acc_i, acc_f = _fresh(dev)
            counts, sums = torch.full((16,), -3, dtype=torch.int64, device=dev), torch.full((2,), -3.0, dtype=torch.float64, device=dev)
            ops.object_match_accumulate(t_lab, s_lab, acc_i, acc_f, min_area=min_area, counts_out=counts, sums_out=sums, workspace=ws)
            assert int(ops.metric_err(dev).item()) == 0, name
            want_c, want_s = _want(H, W, name, min_area)
            got_c, got_s = counts.cpu().tolist(), sums.cpu().tolist()
            print("%dx%d %s min_area %d: device %s %r, host %s %r" % (H, W, name, min_area, got_c[:14], got_s, want_c[:14], want_s))
            assert got_c == want_c, (name, min_area, got_c, want_c)
            assert _sums_close(got_s, want_s, want_c[10]), (name, min_area, got_s, want_s)
            assert acc_i.cpu().tolist() == got_c and acc_f.cpu().tolist() == got_s      # zeroed accumulators hold this pair alone


def test_case_list_spreads_over_the_thresholds():
    """On the yardstick's output: the list holds a case whose matches thin out over the thresholds without vanishing, and a case
    where SEG counts cells that no threshold matches.  A list where every threshold agrees would prove little."""
    all_cases = [_want(H, W, name, 1)[0] for H, W in R.SHAPES for name in R.cases(H, W)]
    assert any(0 < c[9] < c[0] < min(c[10], c[11]) for c in all_cases)
    assert any(c[13] > c[0] for c in all_cases)
    # the noise pairs: a percolating region among many small ones (many keys per wave, many pairs in the table), and a min_area of 5
    # that cuts through them
    assert R.noise_is_rich(lambda H, W, name, min_area: _want(H, W, name, min_area)[0])


def test_repeatability_accumulation_and_workspaces():
    from supervised_gan_amd import ops
    dev = _dev()
    (Ha, Wa, na), (Hb, Wb, nb) = (70, 130, "cells_eroded"), (37, 53, "noise")
    ta, sa = _labels(dev, *R.cases(Ha, Wa)[na])
    ta2, sa2 = _labels(dev, *R.cases(Ha, Wa)["cells_shifted"])
    tb, sb = _labels(dev, *R.cases(Hb, Wb)[nb])
    want_a, want_a2, want_b = _want(Ha, Wa, na, 1), _want(Ha, Wa, "cells_shifted", 1), _want(Hb, Wb, nb, 1)
    # two calls on one pair through the cached workspace, then another pair into the same accumulators
    acc_i, acc_f = _fresh(dev)
    counts, sums = torch.zeros((3, 16), dtype=torch.int64, device=dev), torch.zeros((3, 2), dtype=torch.float64, device=dev)
    ops.object_match_accumulate(ta, sa, acc_i, acc_f, counts_out=counts[0], sums_out=sums[0])
    ops.object_match_accumulate(ta, sa, acc_i, acc_f, counts_out=counts[1], sums_out=sums[1])
    ops.object_match_accumulate(ta2, sa2, acc_i, acc_f, counts_out=counts[2], sums_out=sums[2])
    ops.check_metric_err(dev)
    c, f = counts.cpu().numpy(), sums.cpu().numpy()
    assert c[0].tolist() == want_a[0] and c[1].tolist() == want_a[0] and c[2].tolist() == want_a2[0]
    assert _sums_close(f[0], want_a[1], want_a[0][10]) and _sums_close(f[1], f[0], 2 * want_a[0][10]) and _sums_close(f[2], want_a2[1], want_a2[0][10])
    assert acc_i.cpu().numpy().tolist() == (c[0] + c[1] + c[2]).tolist() and acc_i[12].item() == 3
    assert acc_f.cpu().numpy().tolist() == ((f[0] + f[1]) + f[2]).tolist()      # added in call order by one thread: the same three additions
    # one passed-in workspace, sized for the larger shape and full of garbage, serves both shapes' calls on one stream
    ws = torch.full((ops.object_match_workspace(Ha, Wa, dev).numel(),), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=dev)
    assert ws.numel() >= ops.object_match_workspace(Hb, Wb, dev).numel()
    out = torch.zeros((4, 16), dtype=torch.int64, device=dev)
    acc_i, acc_f = _fresh(dev)
    for k, (tl, sl) in enumerate(((ta, sa), (tb, sb), (ta, sa), (tb, sb))):
        ops.object_match_accumulate(tl, sl, acc_i, acc_f, counts_out=out[k], workspace=ws)
    ops.check_metric_err(dev)
    assert out.cpu().tolist() == [want_a[0], want_b[0], want_a[0], want_b[0]]
    # the optional outputs may be left out
    acc_i, acc_f = _fresh(dev)
    ops.object_match_accumulate(tb, sb, acc_i, acc_f, min_area=5)
    ops.check_metric_err(dev)
    want = _want(Hb, Wb, nb, 5)
    assert acc_i.cpu().tolist() == want[0] and _sums_close(acc_f.cpu().tolist(), want[1], want[0][10])


def test_malformed_calls_are_refused_before_any_launch():
    from supervised_gan_amd import _lib, ops
    dev = _dev()
    l = _lib.lib()
    H, W = 37, 53
    need = l.sgan_object_match_workspace(H, W)
    assert need > 0 and need % 16 == 0
    ws = torch.full((need // 8 + 1,), 7, dtype=torch.int64, device=dev)
    lab = torch.zeros((H, W), dtype=torch.int32, device=dev)
    acc_i, acc_f = _fresh(dev)
    err = ops.metric_err(dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    call = l.sgan_object_match_accumulate
    for args, message in (((None, P(lab), H, W, 1, P(ws), need, P(acc_i), P(acc_f), None, None, P(err), None), b"null pointer"),
                          ((P(lab), None, H, W, 1, P(ws), need, P(acc_i), P(acc_f), None, None, P(err), None), b"null pointer"),
                          ((P(lab), P(lab), H, W, 1, None, need, P(acc_i), P(acc_f), None, None, P(err), None), b"null pointer"),
                          ((P(lab), P(lab), H, W, 1, P(ws), need, None, P(acc_f), None, None, P(err), None), b"null pointer"),
                          ((P(lab), P(lab), H, W, 1, P(ws), need, P(acc_i), None, None, None, P(err), None), b"null pointer"),
                          ((P(lab), P(lab), H, W, 1, P(ws), need, P(acc_i), P(acc_f), None, None, None, None), b"null pointer"),
                          ((P(lab), P(lab), H, W, 0, P(ws), need, P(acc_i), P(acc_f), None, None, P(err), None), b"min_area"),
                          ((P(lab), P(lab), H, W, -3, P(ws), need, P(acc_i), P(acc_f), None, None, P(err), None), b"min_area"),
                          ((P(lab), P(lab), 0, W, 1, P(ws), need, P(acc_i), P(acc_f), None, None, P(err), None), b"bad shape"),
                          ((P(lab), P(lab), H, W, 1, P(ws), need - 16, P(acc_i), P(acc_f), None, None, P(err), None), b"nothing was launched")):
        assert call(*args) < 0 and message in l.sgan_last_error(), (message, l.sgan_last_error())
    torch.cuda.synchronize()
    assert bool((ws == 7).all()) and acc_i.cpu().tolist() == [0] * 16 and acc_f.cpu().tolist() == [0.0, 0.0]      # untouched
    assert l.sgan_object_match_workspace(0, 5) < 0
    with pytest.raises(_lib.SganError, match="workspace"):
        ops.object_match_accumulate(lab, lab, acc_i, acc_f, workspace=ws[:8])
    with pytest.raises(_lib.SganError, match="min_area"):
        ops.object_match_accumulate(lab, lab, acc_i, acc_f, min_area=0)


def test_label_out_of_range_is_flagged_and_left_out():
    from supervised_gan_amd import _lib, ops
    dev = _dev()
    H, W = 37, 53
    s, t = R.cases(H, W)["cells_shifted"]
    t_lab, s_lab = _labels(dev, s, t)
    bad = t_lab.clone()
    bad[0, 0] = H * W + 1                                  # one more than any label can be
    bad[5, 7] = -2
    acc_i, acc_f = _fresh(dev)
    ops.object_match_accumulate(bad, s_lab, acc_i, acc_f)
    with pytest.raises(_lib.SganError, match="0x4"):
        ops.check_metric_err(dev)
    assert acc_i[12].item() == 1 and 0 <= acc_i[0].item() <= acc_i[10].item() <= H * W
    # the flag is cleared by the check, and the next call is as good as any
    acc_i, acc_f = _fresh(dev)
    ops.object_match_accumulate(t_lab, s_lab, acc_i, acc_f)
    ops.check_metric_err(dev)
    assert acc_i.cpu().tolist() == _want(H, W, "cells_shifted", 1)[0]


def test_capture_replays_on_another_pair():
    """Captured on one pair, replayed on a pair with another number of regions: a single chain of launches that depends on the
    shape alone."""
    from supervised_gan_amd import ops
    dev = _dev()
    H, W = 70, 130
    first, second = _want(H, W, "cells_eroded", 5), _want(H, W, "noise", 5)
    assert first[0][10] != second[0][10] and first[0][11] != second[0][11]
    t_lab, s_lab = _labels(dev, *R.cases(H, W)["cells_eroded"])
    t2, s2 = _labels(dev, *R.cases(H, W)["noise"])
    acc_i, acc_f = _fresh(dev)
    counts, sums = torch.zeros(16, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.float64, device=dev)
    ops.object_match_accumulate(t_lab, s_lab, acc_i, acc_f, min_area=5, counts_out=counts, sums_out=sums)      # workspace and dev_err exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.object_match_accumulate(t_lab, s_lab, acc_i, acc_f, min_area=5, counts_out=counts, sums_out=sums)
    acc_i.zero_()
    acc_f.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == first[0] and _sums_close(sums.cpu().tolist(), first[1], first[0][10])
    t_lab.copy_(t2)
    s_lab.copy_(s2)
    g.replay()
    torch.cuda.synchronize()
    eager_c, eager_s = torch.zeros(16, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.float64, device=dev)
    ops.object_match_accumulate(t2, s2, *_fresh(dev), min_area=5, counts_out=eager_c, sums_out=eager_s)
    ops.check_metric_err(dev)
    assert counts.cpu().tolist() == eager_c.cpu().tolist() == second[0]
    assert _sums_close(sums.cpu().tolist(), eager_s.cpu().tolist(), 2 * second[0][10])
    assert acc_i.cpu().tolist() == [a + b for a, b in zip(first[0], second[0])]


def test_rand_and_vinfo_are_untouched():
    """rand_f_accumulate and vinfo_accumulate before and after an object_match_accumulate on the same stream: the same integers."""
    from supervised_gan_amd import ops
    dev = _dev()
    H, W = 70, 130
    for name in ("cells_shifted", "noise"):
        t_lab, s_lab = _labels(dev, *R.cases(H, W)[name])
        rand = torch.zeros((2, 4), dtype=torch.int64, device=dev)
        parts = torch.zeros((2, len(ops.VINFO_PARTS)), dtype=torch.float64, device=dev)
        acc = torch.zeros((4, 2), dtype=torch.float64, device=dev)
        ops.rand_f_accumulate(t_lab, s_lab, acc[0], sums_out=rand[0])
        ops.vinfo_accumulate(t_lab, s_lab, acc[1], parts_out=parts[0])
        ops.object_match_accumulate(t_lab, s_lab, *_fresh(dev))
        ops.rand_f_accumulate(t_lab, s_lab, acc[2], sums_out=rand[1])
        ops.vinfo_accumulate(t_lab, s_lab, acc[3], parts_out=parts[1])
        ops.check_metric_err(dev)
        rand, parts, acc = rand.cpu().numpy(), parts.cpu().numpy(), acc.cpu().numpy()
        assert rand[0].tolist() == rand[1].tolist() and rand[0][0] > 0, name
        assert acc[0].tolist() == acc[2].tolist(), name           # the F-score is a function of the integers
        m, aux = ops.VINFO_PARTS.index("m"), ops.VINFO_PARTS.index("aux")
        assert parts[0][m] == parts[1][m] and parts[0][aux] == parts[1][aux], name
        for n in ("SA", "SB", "SAB"):                             # fp64 sums in scheduling order: tests/test_hip_vinfo.py's bound
            k = ops.VINFO_PARTS.index(n)
            assert abs(parts[0][k] - parts[1][k]) <= 2 * H * W * 2.0 ** -53 * abs(parts[0][k]), (name, n)


def _net_argv(ckpt, metrics, name="objects"):
    return ["--name", name, "--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "64",
            "--which_model_netG", "resnet_6blocks", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout",
            "--checkpoints_dir", str(ckpt), "--dataroot", "synthetic", "--manualSeed", "4", "--which_metric", *metrics]


_TRAIN = ["--which_model_netD", "n_layers", "--n_layers_D", "2", "--ndf", "8", "--scale_factor", "1", "--lambda_D", "1.0", "--weights", "1", "2",
          "--no_lsgan", "--print_freq", "1", "--valSize", "64"]
ASKED = ["RandScore", "ObjF1", "ObjAP", "SEG", "PQ", "meanIU"]


def _pooled(pairs, min_area):
    """util.object_scores of the yardstick's pooled counts on (fake_B, real_B) tensors, and the pooled numbers themselves."""
    from supervised_gan_amd.util import object_match_counts, object_scores
    counts, sums = np.zeros(16, dtype=np.int64), np.zeros(2, dtype=np.float64)
    for fb, rb in pairs:
        c, f = object_match_counts(fb[0, 0].cpu().numpy(), rb[0, 0].cpu().numpy(), min_area)
        counts, sums = counts + c, sums + f
    return object_scores(counts, sums), counts, sums


def _scores_match(accs, want, counts):
    """ObjF1 and ObjAP come from equal integers through one function; SEG and PQ carry the sums' bound, pooled N_t terms."""
    bound = max(1, int(counts[10])) * 2.0 ** -52
    return (accs["ObjF1"] == want["ObjF1"] and accs["ObjAP"] == want["ObjAP"]
            and all(abs(accs[k] - want[k]) <= bound * abs(want[k]) for k in ("SEG", "PQ")))


def test_trainer_scores_and_key_order(tmp_path, monkeypatch):
    from supervised_gan_amd import ops
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    _dev()
    opt = TrainOptions().parse(_net_argv(tmp_path, ASKED) + _TRAIN, save=False, verbose=False)
    model = create_model(opt)
    labellings = []
    real_ccl = ops.ccl_label
    monkeypatch.setattr(ops, "ccl_label", lambda *a, **k: (labellings.append(1), real_ccl(*a, **k))[1])
    seen = []
    for data in SyntheticDataset(opt, 3):
        model.set_input(data)
        model.optimize_parameters()
        model.accum_accs()
        seen.append((model.fake_B.detach().clone(), model.real_B.detach().clone(), model.logit.detach().clone(), model.label.clone()))
    assert len(labellings) == 6                                   # each map labelled once per accum_accs, for RandScore and the objects together
    accs = model.get_current_accs()
    assert list(accs) == ["RandScore", "meanIU", "ObjF1", "ObjAP", "SEG", "PQ"] and model.numAveragedImages == 3
    conf = model.confusion.copy()
    want, counts, sums = _pooled([(fb, rb) for fb, rb, _, _ in seen], 1)
    pooled = model.get_object_counts()
    print("trainer: device %r, host %r; pooled %r" % (dict(accs), dict(want), dict(pooled)))
    assert list(pooled) == list(ops.OBJECT_COUNTS) + list(ops.OBJECT_SUMS)
    assert [pooled[k] for k in ops.OBJECT_COUNTS] == counts.tolist() and counts[12] == 3
    assert _scores_match(accs, want, counts)
    assert all(0.0 <= accs[k] <= 1.0 for k in ("ObjF1", "ObjAP", "SEG", "PQ"))
    # the same maps without the new names: RandScore and the confusion matrix are the same bits
    model.opt.which_metric = ["RandScore", "meanIU"]
    model.reset_accs()
    for fb, rb, logit, label in seen:
        model.fake_B, model.real_B, model.logit = fb, rb, logit
        model.label.copy_(label)
        model.accum_accs()
    plain = model.get_current_accs()
    assert list(plain) == ["RandScore", "meanIU"]
    assert plain["RandScore"] == accs["RandScore"] and plain["meanIU"] == accs["meanIU"] and np.array_equal(model.confusion, conf)
    # the object scores alone, with small regions left out: the maps are labelled for them, and reset_accs() started from zero
    model.opt.which_metric = ["SEG", "ObjF1"]
    model.opt.min_object_area = 4
    model.reset_accs()
    assert model.get_current_accs() == {"ObjF1": 0, "SEG": 0} and model.get_object_counts()["images"] == 0
    labellings.clear()
    model.accum_accs()
    only = model.get_current_accs()
    want1, counts1, _ = _pooled([seen[-1][:2]], 4)
    assert len(labellings) == 2 and list(only) == ["ObjF1", "SEG"] and model.numAveragedImages == 1
    assert only["ObjF1"] == want1["ObjF1"] and abs(only["SEG"] - want1["SEG"]) <= max(1, int(counts1[10])) * 2.0 ** -52 * abs(want1["SEG"])


def test_segmentation_cycle_borrows_the_object_scores(tmp_path):
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    _dev()
    argv = ["--name", "objc", "--model", "segmentation_cycle", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "64",
            "--which_model_netG1", "resnet_6blocks", "--ngf1", "8", "--which_model_netG2", "resnet_6blocks", "--ngf2", "8", "--norm", "instance",
            "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout1", "--no_dropout2", "--checkpoints_dir", str(tmp_path),
            "--dataroot", "synthetic", "--manualSeed", "4", "--which_metric", *ASKED, "--min_object_area", "3",
            "--which_model_netD2", "n_layers", "--n_layers_D2", "2", "--ndf2", "8", "--scale_factor2", "1", "--lambda_D2", "1.0", "--no_lsgan2",
            "--print_freq", "1", "--valSize", "64"]
    opt = TrainOptions().parse(argv, save=False, verbose=False)
    model = create_model(opt)
    for data in SyntheticDataset(opt, 1):
        model.set_input(data)
        model.optimize_parameters()
        model.accum_accs()
    accs = model.get_current_accs()
    assert list(accs) == ["RandScore", "meanIU", "ObjF1", "ObjAP", "SEG", "PQ"] and model.numAveragedImages == 1
    want, counts, _ = _pooled([(model.fake_B.detach(), model.real_B.detach())], 3)
    print("cycle: device %r, host %r" % (dict(accs), dict(want)))
    assert [model.get_object_counts()[k] for k in ("TP_0", "N_t", "N_s", "SEGn")] == [int(counts[k]) for k in (0, 10, 11, 13)]
    assert _scores_match(accs, want, counts)


def test_drivers_carry_the_object_scores(tmp_path):
    """train_ss.py in a fresh process keeps its `best` checkpoint by ObjF1 and logs it; test_ss.py on that checkpoint prints the
    per-threshold line."""
    _dev()
    metrics = ["RandScore", "ObjF1", "SEG"]
    argv = _net_argv(tmp_path / "ckpt", metrics) + _TRAIN + ["--best_metric", "ObjF1", "--min_object_area", "4", "--max_steps", "2",
                                                            "--val_epoch_size", "1"]
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "train_ss.py")] + argv, cwd=ROOT,
                         capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    log = (tmp_path / "ckpt" / "objects" / "acc_log.txt").read_text().splitlines()
    assert sum(l.startswith("(train,") for l in log) == 2 and sum(l.startswith("(val,") for l in log) == 1, log
    assert all("RandScore:" in l and "ObjF1:" in l and "SEG:" in l and "PQ" not in l for l in log), log
    values = [float(l.split(key + ":")[1].split()[0]) for l in log for key in ("ObjF1", "SEG")]
    assert all(0.0 <= v <= 1.0 for v in values), values
    assert "saving the best model (epoch 1, ObjF1" in run.stdout
    assert (tmp_path / "ckpt" / "objects" / "best_net_G.pth").exists()
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "test_ss.py")]
                         + _net_argv(tmp_path / "ckpt", metrics) + ["--min_object_area", "4", "--results_dir", str(tmp_path / "res"),
                                                                   "--how_many", "2"], cwd=ROOT, capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    line = [l for l in run.stdout.splitlines() if l.startswith("objects: TP at IoU > 0.50 .. 0.95:")]
    assert len(line) == 1 and line[0].endswith("(min area 4)"), run.stdout[-2000:]
    tp = [int(v) for v in line[0].split(":")[2].split(",")[0].split()]
    assert len(tp) == 10 and all(a >= b >= 0 for a, b in zip(tp, tp[1:])), line
    assert "ObjF1: " in run.stdout and "SEG: " in run.stdout

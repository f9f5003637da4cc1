"""GPU tests of the thinned scores in the segmentation trainers (`--which_metric RandScoreThin VInfoThin`): the running means
against the host yardsticks on the trainer's own tensors, the un-thinned values untouched by the new names, and one test_ss.py run.

Tolerances: Rand 1e-12 absolute (one fp64 expression of exact integers on both sides); VInfo 1e-10 relative, the tolerance of
tests/test_hip_vinfo.py (fp64 sums of at most H W = 4096 terms in scheduling order)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
REL = 1e-10
ALL = ["RandScore", "VInfo", "RandScoreThin", "VInfoThin", "meanIU"]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")


def _net_argv(ckpt, metrics, name="thin"):
    return ["--name", name, "--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "64",
            "--which_model_netG", "resnet_6blocks", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout",
            "--checkpoints_dir", str(ckpt), "--dataroot", "synthetic", "--manualSeed", "4", "--which_metric", *metrics]


_TRAIN = ["--which_model_netD", "n_layers", "--n_layers_D", "2", "--ndf", "8", "--scale_factor", "1", "--lambda_D", "1.0", "--weights", "1", "2",
          "--no_lsgan", "--print_freq", "1", "--valSize", "64"]


def _close(got, want, rel=REL):
    return abs(got - want) <= rel * abs(want)


def test_running_means_equal_the_host_yardsticks_and_leave_the_others_alone(tmp_path, capsys):
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    from supervised_gan_amd.util import compute_Rand_F_scores, compute_VInfo_scores, compute_thinned_scores, thin
    _need_gpu()
    opt = TrainOptions().parse(_net_argv(tmp_path, ALL) + _TRAIN, save=False, verbose=False)
    model = create_model(opt)
    seen = []
    for data in SyntheticDataset(opt, 3):
        model.set_input(data)
        model.optimize_parameters()
        model.accum_accs()
        seen.append((model.fake_B.detach().clone(), model.real_B.detach().clone(), model.logit.detach().clone(), model.label.clone()))
    accs = model.get_current_accs()
    assert list(accs) == ["RandScore", "VInfo", "meanIU", "RandScoreThin", "VInfoThin"] and model.numAveragedImages == 3
    conf = model.confusion.copy()
    host = {k: [] for k in ("RandScore", "VInfo", "RandScoreThin", "VInfoThin")}
    thinned_something = False
    for fb, rb, _, _ in seen:
        s, t = fb[0, 0].cpu().numpy(), rb[0, 0].cpu().numpy()
        host["RandScore"].append(float(compute_Rand_F_scores(s, t)[0]))
        host["VInfo"].append(float(compute_VInfo_scores(s, t)[0]))
        r, v = compute_thinned_scores(s, t)
        host["RandScoreThin"].append(float(r[0]))
        host["VInfoThin"].append(float(v[0]))
        thinned_something |= thin(s > 0.5)[1] > 0
    for k, vals in host.items():
        print("%s device %r host %r (%r)" % (k, float(accs[k]), float(np.mean(vals)), vals))
    assert thinned_something                                   # the predictions had walls thicker than a line
    assert all(math.isfinite(v) for vals in host.values() for v in vals)
    for k in ("RandScore", "RandScoreThin"):
        assert abs(float(accs[k]) - float(np.mean(host[k]))) <= 1e-12, k
    for k in ("VInfo", "VInfoThin"):
        assert _close(float(accs[k]), float(np.mean(host[k]))), k
    # the same maps without the two new names: the un-thinned values and the confusion matrix are the same bits
    model.opt.which_metric = ["RandScore", "VInfo", "meanIU"]
    model.reset_accs()
    for fb, rb, logit, label in seen:
        model.fake_B, model.real_B, model.logit = fb, rb, logit
        model.label.copy_(label)
        model.accum_accs()
    plain = model.get_current_accs()
    assert list(plain) == ["RandScore", "VInfo", "meanIU"]
    assert plain["RandScore"] == accs["RandScore"] and plain["meanIU"] == accs["meanIU"] and np.array_equal(model.confusion, conf)
    # VInfo's fp64 sums arrive in an order that depends on scheduling (include/sgan_hip.h: "repeat to rounding, not to the bit"), so
    # two runs of the parent's own path are compared as tests/test_hip_vinfo.py compares them
    print("VInfo with the new names %r, without %r" % (float(accs["VInfo"]), float(plain["VInfo"])))
    assert _close(float(plain["VInfo"]), float(accs["VInfo"]))
    # the thinned scores alone: the truth is labelled for them, and the keys follow the request
    model.opt.which_metric = ["VInfoThin"]
    model.reset_accs()
    model.fake_B, model.real_B = seen[-1][0], seen[-1][1]
    model.accum_accs()
    only = model.get_current_accs()
    assert list(only) == ["VInfoThin"] and _close(float(only["VInfoThin"]), host["VInfoThin"][-1]) and model.numAveragedImages == 1
    model.opt.which_metric = ["RandScoreThin"]
    model.reset_accs()
    model.accum_accs()
    only = model.get_current_accs()
    assert list(only) == ["RandScoreThin"] and abs(float(only["RandScoreThin"]) - host["RandScoreThin"][-1]) <= 1e-12
    # test_ss.py on the checkpoint of this trainer prints both new keys
    model.opt.which_metric = ALL
    model.save("latest")
    capsys.readouterr()
    import test_ss
    accs_t, ce = test_ss.main(_net_argv(tmp_path, ALL) + ["--results_dir", str(tmp_path / "res"), "--how_many", "2"])
    printed = capsys.readouterr().out
    assert list(accs_t) == ["RandScore", "VInfo", "meanIU", "RandScoreThin", "VInfoThin"]
    assert "RandScoreThin: " in printed and "VInfoThin: " in printed
    assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in accs_t.values()), accs_t
    assert ce.shape == (2,) and np.isfinite(ce).all()


def test_without_the_new_names_nothing_is_added(tmp_path):
    """Neither name requested: no thinning buffer exists after accum_accs and the keys are the old ones."""
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    from supervised_gan_amd import ops
    _need_gpu()
    opt = TrainOptions().parse(_net_argv(tmp_path, ["RandScore", "VInfo", "meanIU"]) + _TRAIN, save=False, verbose=False)
    model = create_model(opt)
    for data in SyntheticDataset(opt, 1):
        model.set_input(data)
        model.optimize_parameters()
    thin_ws = lambda: [k for k in ops._metric_ws if k[0] == "sgan_thin_workspace"]      # noqa: E731
    for k in thin_ws():
        del ops._metric_ws[k]
    model.accum_accs()
    assert list(model.get_current_accs()) == ["RandScore", "VInfo", "meanIU"]
    m = model.seg_metrics
    assert sorted(m.acc) == ["conf", "rand", "vinfo"] and sorted(m.planes) == ["pred_labels", "truth_labels"] and not thin_ws()


def test_segmentation_cycle_borrows_the_thinned_scores(tmp_path):
    """`--model segmentation_cycle` takes its accuracy methods from SegmentationModel: one step with all five names, the two new
    scores against the host yardstick on the trainer's tensors."""
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    from supervised_gan_amd.util import compute_thinned_scores
    _need_gpu()
    argv = ["--name", "thinc", "--model", "segmentation_cycle", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "64",
            "--which_model_netG1", "resnet_6blocks", "--ngf1", "8", "--which_model_netG2", "resnet_6blocks", "--ngf2", "8", "--norm", "instance",
            "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout1", "--no_dropout2", "--checkpoints_dir", str(tmp_path),
            "--dataroot", "synthetic", "--manualSeed", "4", "--which_metric", *ALL,
            "--which_model_netD2", "n_layers", "--n_layers_D2", "2", "--ndf2", "8", "--scale_factor2", "1", "--lambda_D2", "1.0", "--no_lsgan2",
            "--print_freq", "1", "--valSize", "64"]
    opt = TrainOptions().parse(argv, save=False, verbose=False)
    model = create_model(opt)
    for data in SyntheticDataset(opt, 1):
        model.set_input(data)
        model.optimize_parameters()
        model.accum_accs()
    accs = model.get_current_accs()
    assert list(accs) == ["RandScore", "VInfo", "meanIU", "RandScoreThin", "VInfoThin"] and model.numAveragedImages == 1
    r, v = compute_thinned_scores(model.fake_B.detach()[0, 0].cpu().numpy(), model.real_B.detach()[0, 0].cpu().numpy())
    print("cycle: RandScoreThin %r host %r, VInfoThin %r host %r" % (float(accs["RandScoreThin"]), float(r[0]), float(accs["VInfoThin"]), float(v[0])))
    assert math.isfinite(float(r[0])) and abs(float(accs["RandScoreThin"]) - float(r[0])) <= 1e-12
    assert _close(float(accs["VInfoThin"]), float(v[0]))


def test_a_map_size_that_changes_between_calls(tmp_path):
    """train_ss.py validates at --valSize: one trainer with all twelve names and --boundary_thin takes a 64 x 64 pair, a 32 x 32 pair
    and the 64 x 64 pair again.  The pooled integers equal the sums of the host yardsticks over the three pairs, the Rand scores
    agree to 1e-12 and the information scores to REL."""
    from supervised_gan_amd import ops, util
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    _need_gpu()
    names = ALL + list(util.OBJECT_METRICS) + list(util.BOUNDARY_METRICS)
    assert len(names) == 12
    opt = TrainOptions().parse(_net_argv(tmp_path, names, "resize") + _TRAIN + ["--boundary_thin"], save=False, verbose=False)
    model = create_model(opt)
    for data in SyntheticDataset(opt, 1):
        model.set_input(data)
        model.optimize_parameters()
    big = [model.fake_B.detach().clone(), model.real_B.detach().clone(), model.logit.detach().clone(), model.label.clone()]
    small = [t[..., 16:48, 16:48].contiguous() for t in big]
    pairs = [big, small, big]
    for model.fake_B, model.real_B, model.logit, model.label in pairs:
        model.accum_accs()
    accs = model.get_current_accs()
    assert list(accs) == ["RandScore", "VInfo", "meanIU", "RandScoreThin", "VInfoThin"] + list(util.OBJECT_METRICS) + list(util.BOUNDARY_METRICS)
    assert model.numAveragedImages == 3 and model.numAveragedPixels == 2 * 64 * 64 + 32 * 32
    obj, bnd, conf = np.zeros(16, dtype=np.int64), np.zeros(80, dtype=np.int64), np.zeros((2, 2), dtype=np.int64)
    host = {k: [] for k in ("RandScore", "VInfo", "RandScoreThin", "VInfoThin")}
    for fb, rb, logit, label in pairs:
        s, t = fb[0, 0].cpu().numpy(), rb[0, 0].cpu().numpy()
        obj += util.object_match_counts(s, t, opt.min_object_area)[0]
        c = util.boundary_counts(util.thin(s > 0.5)[0], t)[0]
        bnd[:70] += c[:70]
        bnd[70:72] = np.maximum(bnd[70:72], c[70:72])            # the two largest distances are kept, not summed
        pred = logit[0].cpu().numpy().argmax(axis=0)
        conf += np.bincount(label[0].cpu().numpy().ravel() * 2 + pred.ravel(), minlength=4).reshape(2, 2)
        host["RandScore"].append(float(util.compute_Rand_F_scores(s, t)[0]))
        host["VInfo"].append(float(util.compute_VInfo_scores(s, t)[0]))
        r, v = util.compute_thinned_scores(s, t)
        host["RandScoreThin"].append(float(r[0]))
        host["VInfoThin"].append(float(v[0]))
    for k, vals in host.items():
        print("%s device %r host %r (%r)" % (k, float(accs[k]), float(np.mean(vals)), vals))
    assert all(math.isfinite(v) for vals in host.values() for v in vals)
    pooled_obj, pooled_bnd = model.get_object_counts(), model.get_boundary_counts()
    assert [pooled_obj[k] for k in ops.OBJECT_COUNTS] == obj.tolist() and obj[12] == 3 and obj[10] > 0
    assert [pooled_bnd[k] for k in ops.BOUNDARY_COUNTS] == bnd.tolist() and bnd[66] == 3 and bnd[65] > 0
    assert np.array_equal(model.confusion, conf)
    for k in ("RandScore", "RandScoreThin"):
        assert abs(float(accs[k]) - float(np.mean(host[k]))) <= 1e-12, k
    for k in ("VInfo", "VInfoThin"):
        assert _close(float(accs[k]), float(np.mean(host[k]))), k

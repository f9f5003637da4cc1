"""GPU tests of the information score on the device (sgan_vinfo_accumulate in sgan_metrics.hip): its parts against the host yardstick
util.compute_VInfo_parts, the Rand F-score it adds from the same counting pass against sgan_rand_f_accumulate bit for bit, the
trainers' running mean, and one train_ss.py run that selects its `best` checkpoint by VInfo.

Tolerance of the fp64 sums SA, SB, SAB and of the score: 1e-10 relative.  They are sums of at most H W <= 9100 positive terms added
in an order that depends on scheduling, H W 2^-53 ~ 1e-12 relative, with two decades of margin for the two `log` implementations."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import vinfo_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
REL = 1e-10


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def _close(got, want, rel=REL):
    """NaN matches NaN only; otherwise |got - want| <= rel * |want| (an exact 0 has to be met exactly)."""
    if math.isnan(want) or math.isnan(got):
        return math.isnan(want) and math.isnan(got)
    return abs(got - want) <= rel * abs(want)


@pytest.mark.parametrize("H,W", V.DEVICE_SIZES)
def test_parts_equal_the_host_yardstick(H, W):
    from supervised_gan_amd import ops
    from supervised_gan_amd.util import compute_VInfo_parts
    dev = _dev()
    names = ops.VINFO_PARTS
    ws = ops.vinfo_workspace(H, W, dev)
    ws.fill_(-1)                                           # the call zeroes what it uses
    kinds = set()
    for kind, (s, t) in V.device_pairs(H, W).items():
        t_lab = ops.ccl_label(torch.from_numpy(t.copy()).to(dev))
        s_lab = ops.ccl_label(torch.from_numpy(s.copy()).to(dev))
        acc, acc_r, ref_r = (torch.zeros(2, dtype=torch.float64, device=dev) for _ in range(3))
        parts = torch.zeros((2, len(names)), dtype=torch.float64, device=dev)
        for k in range(2):                                 # two calls on one workspace
            ops.vinfo_accumulate(t_lab, s_lab, acc, acc_rand=acc_r, parts_out=parts[k], workspace=ws)
            ops.rand_f_accumulate(t_lab, s_lab, ref_r)
        assert int(ops.metric_err(dev).item()) == 0, kind
        first, again = (dict(zip(names, row)) for row in parts.cpu().tolist())
        want = compute_VInfo_parts(s, t)
        print("%dx%d %s: " % (H, W, kind) + ", ".join("%s %r (host %r)" % (n, first[n], want[n]) for n in ("SA", "SB", "SAB", "m", "aux", "VInfo")))
        assert first["m"] == want["m"] and first["aux"] == want["aux"], kind
        for n in ("SA", "SB", "SAB", "VInfo"):
            assert _close(first[n], want[n]), (kind, n, first[n], want[n])
        for n in ("H_S", "H_T", "I", "split", "merge"):    # which of them are NaN, and which entropy is exactly 0, comes from the integers
            assert math.isnan(first[n]) == math.isnan(want[n]), (kind, n, first[n], want[n])
        assert (first["H_S"] == 0.0) == (want["H_S"] == 0.0) and (first["H_T"] == 0.0) == (want["H_T"] == 0.0), (kind, first, want)
        # the second call: integers again exactly; the fp64 sums to twice the rounding of one sum of H W terms, whatever the order
        assert again["m"] == first["m"] and again["aux"] == first["aux"], kind
        for n in ("SA", "SB", "SAB"):
            assert _close(again[n], first[n], 2 * H * W * 2.0 ** -53), (kind, n, again[n], first[n])
        assert _close(again["VInfo"], first["VInfo"]), kind
        # running sums: VInfo twice; the Rand F-score exactly what sgan_rand_f_accumulate adds
        got, got_r, want_r = acc.cpu().numpy(), acc_r.cpu().numpy(), ref_r.cpu().numpy()
        assert got[1] == 2 and _close(float(got[0]), first["VInfo"] + again["VInfo"], 1e-15), (kind, got)
        assert got_r[1] == 2 and want_r[1] == 2 and (got_r[0] == want_r[0] or (np.isnan(got_r[0]) and np.isnan(want_r[0]))), (kind, got_r, want_r)
        kinds.add("nan" if math.isnan(want["VInfo"]) else "one" if want["VInfo"] == 1.0 else "zero" if want["VInfo"] == 0.0 else "mid")
    # one pixel is one segment in both maps whatever they hold: no 0 and nothing in between at 1 x 1
    assert kinds == ({"nan", "one"} if H * W == 1 else {"nan", "one", "zero", "mid"}), kinds


def test_rand_accumulator_is_optional_and_untouched():
    from supervised_gan_amd import ops
    dev = _dev()
    s, t = V.device_pairs(48, 80)["cells_shift2"]
    t_lab, s_lab = ops.ccl_label(torch.from_numpy(t.copy()).to(dev)), ops.ccl_label(torch.from_numpy(s.copy()).to(dev))
    acc = torch.zeros(2, dtype=torch.float64, device=dev)
    ops.vinfo_accumulate(t_lab, s_lab, acc)                # no acc_rand, no parts_out, the cached workspace
    ops.check_metric_err(dev)
    from supervised_gan_amd.util import compute_VInfo_scores
    got = acc.cpu().numpy()
    assert got[1] == 1 and _close(float(got[0]), float(compute_VInfo_scores(s, t)[0]))


def test_short_workspace_is_refused_before_any_launch():
    from supervised_gan_amd import _lib, ops
    dev = _dev()
    l = _lib.lib()
    H, W = 37, 53
    need, need_rand = l.sgan_vinfo_workspace(H, W), l.sgan_rand_f_workspace(H, W)
    assert need > need_rand > 0 and need % 16 == 0
    ws = torch.full((need // 8 + 1,), 7, dtype=torch.int64, device=dev)
    lab = torch.zeros((H, W), dtype=torch.int32, device=dev)
    acc, acc_r = torch.zeros(2, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.float64, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    for short in (need - 16, need_rand):             # the Rand workspace is too small as well
        rc = l.sgan_vinfo_accumulate(P(lab), P(lab), H, W, P(ws), short, P(acc), P(acc_r), None, P(ops.metric_err(dev)), None)
        assert rc < 0 and b"workspace" in l.sgan_last_error() and b"nothing was launched" in l.sgan_last_error()
    torch.cuda.synchronize()
    assert bool((ws == 7).all()) and acc.cpu().tolist() == [0.0, 0.0] and acc_r.cpu().tolist() == [0.0, 0.0]         # untouched
    with pytest.raises(_lib.SganError, match="workspace"):
        ops.vinfo_accumulate(lab, lab, acc, workspace=ws[:8])
    assert l.sgan_vinfo_workspace(0, 5) < 0


def _segm_argv(ckpt, metrics):
    return ["--name", "vinfo", "--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "64",
            "--which_model_netG", "resnet_6blocks", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout",
            "--checkpoints_dir", str(ckpt), "--dataroot", "synthetic", "--manualSeed", "4", "--which_metric", *metrics,
            "--which_model_netD", "n_layers", "--n_layers_D", "2", "--ndf", "8", "--scale_factor", "1", "--lambda_D", "1.0", "--weights", "1", "2",
            "--no_lsgan", "--print_freq", "1", "--valSize", "64"]


def test_trainer_running_means(tmp_path):
    """Three steps of a 64 x 64 `segmentation` trainer with both scores asked for: VInfo is the mean of the yardstick on the trainer's
    tensors; RandScore is, to the bit, what the same trainer accumulates on the same tensors when RandScore alone is asked for."""
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    from supervised_gan_amd.util import compute_VInfo_scores
    _dev()
    opt = TrainOptions().parse(_segm_argv(tmp_path, ["RandScore", "VInfo"]), save=False, verbose=False)
    model = create_model(opt)
    seen, host = [], []
    for data in SyntheticDataset(opt, 3):
        model.set_input(data)
        model.optimize_parameters()
        model.accum_accs()
        seen.append((model.fake_B.detach().clone(), model.real_B.detach().clone()))
    accs = model.get_current_accs()
    assert list(accs) == ["RandScore", "VInfo"] and model.numAveragedImages == 3
    for fb, rb in seen:
        host.append(float(compute_VInfo_scores(fb[0, 0].cpu().numpy(), rb[0, 0].cpu().numpy())[0]))
    print("VInfo device %r host %r (%r)" % (accs["VInfo"], float(np.mean(host)), host))
    assert all(0.0 <= v <= 1.0 for v in host) and _close(float(accs["VInfo"]), float(np.mean(host)))
    model.opt.which_metric = ["RandScore"]
    model.reset_accs()
    assert model.get_current_accs() == {"RandScore": 0}
    for fb, rb in seen:
        model.fake_B, model.real_B = fb, rb
        model.accum_accs()
    alone = model.get_current_accs()
    assert list(alone) == ["RandScore"] and alone["RandScore"] == accs["RandScore"] and 0.0 < alone["RandScore"] <= 1.0
    model.opt.which_metric = ["VInfo"]
    model.reset_accs()
    model.accum_accs()
    only = model.get_current_accs()
    assert list(only) == ["VInfo"] and _close(float(only["VInfo"]), host[-1]) and model.numAveragedImages == 1


def test_train_ss_keeps_its_best_checkpoint_by_vinfo(tmp_path):
    """train_ss.py in a fresh process: VInfo in the running accuracies, the validation line and the `best` rule."""
    _dev()
    argv = _segm_argv(tmp_path / "ckpt", ["VInfo"]) + ["--best_metric", "VInfo", "--max_steps", "3", "--val_epoch_size", "1"]
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "train_ss.py")] + argv, cwd=ROOT,
                         capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    log = (tmp_path / "ckpt" / "vinfo" / "acc_log.txt").read_text().splitlines()
    assert sum(l.startswith("(train,") for l in log) == 3 and sum(l.startswith("(val,") for l in log) == 1, log
    assert all("VInfo:" in l and "RandScore" not in l for l in log)
    values = [float(l.split("VInfo:")[1].split()[0]) for l in log]
    assert all(0.0 <= v <= 1.0 for v in values), values
    assert "saving the best model (epoch 1, VInfo" in run.stdout
    assert (tmp_path / "ckpt" / "vinfo" / "best_net_G.pth").exists()

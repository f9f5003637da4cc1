"""GPU tests of the drivers with the topology scores: train_ss.py with --graph captures ops.topo_accumulate into its validation pass,
logs the three scores and keeps its `best` checkpoint by clDice; test_ss.py on that checkpoint prints them and the `topology:` line."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
ASKED = ["RandScore", "clDice", "Betti0Err", "Betti1Err"]
REPORTED = ["RandScore", "Betti0Err", "Betti1Err", "clDice"]      # read()'s order


def _net_argv(ckpt):
    return ["--name", "topo", "--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "64",
            "--which_model_netG", "resnet_6blocks", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout",
            "--checkpoints_dir", str(ckpt), "--dataroot", "synthetic", "--manualSeed", "4", "--which_metric", *ASKED, "--topo_window", "32",
            "--topo_stride", "16"]


_TRAIN = ["--which_model_netD", "n_layers", "--n_layers_D", "2", "--ndf", "8", "--scale_factor", "1", "--lambda_D", "1.0", "--weights", "1", "2",
          "--no_lsgan", "--print_freq", "1", "--valSize", "64"]


def test_drivers_carry_the_topology_scores(tmp_path):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    argv = _net_argv(tmp_path / "ckpt") + _TRAIN + ["--best_metric", "clDice", "--max_steps", "3", "--val_epoch_size", "1", "--graph"]
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "train_ss.py")] + argv, cwd=ROOT,
                         capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    log = (tmp_path / "ckpt" / "topo" / "acc_log.txt").read_text().splitlines()
    assert sum(l.startswith("(train,") for l in log) >= 2 and sum(l.startswith("(val,") for l in log) == 1, log
    assert all(all(key + ":" in l for key in REPORTED) for l in log), log
    values = {key: [float(l.split(key + ":")[1].split()[0]) for l in log] for key in REPORTED[1:]}
    # a 32 x 32 window holds at most 512 components of either kind
    assert all(0.0 <= v <= 1.0 for v in values["clDice"]) and all(0.0 <= v <= 512.0 for v in values["Betti0Err"] + values["Betti1Err"]), values
    assert "saving the best model (epoch 1, clDice" in run.stdout
    assert (tmp_path / "ckpt" / "topo" / "best_net_G.pth").exists()
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "test_ss.py")]
                         + _net_argv(tmp_path / "ckpt") + ["--results_dir", str(tmp_path / "res"), "--how_many", "2"],
                         cwd=ROOT, capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    line = [l for l in run.stdout.splitlines() if l.startswith("topology: ")]
    assert len(line) == 1 and line[0].startswith("topology: 18 windows of 32 at stride 16, mean b0 / b1 of the prediction"), run.stdout[-2000:]
    assert "Tprec" in line[0] and "Tsens" in line[0]
    assert all(key in run.stdout for key in REPORTED), run.stdout[-2000:]

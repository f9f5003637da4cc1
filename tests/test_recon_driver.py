"""recon.py (the reference's reconstruction driver loop) after train.py: PNGs, index.html, the summary line; other models refused."""
import os
import re
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NET = ["--model", "fcgan", "--which_direction", "A", "--dataset_mode", "single", "--fineSize", "64", "--input_nc", "2",
       "--which_model_netG", "deconv", "--n_layers_G", "3", "--ngf", "8", "--noise_nc", "8", "--noiseSize", "4", "--norm", "instance",
       "--no_dropout", "--which_channel", "rg", "--gpu_ids", "0", "--dataroot", "synthetic", "--manualSeed", "3"]


def test_train_then_recon(tmp_path, capsys):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    import recon as recon_driver
    import train as train_driver
    net = ["--name", "drv_recon", "--checkpoints_dir", str(tmp_path / "ckpt")] + NET
    train_driver.main(net + ["--which_model_netD", "n_layers", "--n_layers_D", "3", "--ndf", "8", "--scale_factor", "1",
                             "--lambda_D", "1", "--n_update_G", "1", "--no_lsgan", "--max_steps", "2", "--print_freq", "1"])
    capsys.readouterr()
    written, _ = recon_driver.main(net + ["--results_dir", str(tmp_path / "res"), "--how_many", "2", "--recon_steps", "2"])
    out = capsys.readouterr().out
    assert len(written) == 4 and all(os.path.exists(p) for p in written)          # real + fake per image
    assert os.path.exists(tmp_path / "res" / "drv_recon" / "test_latest" / "index.html")
    line = [l for l in out.splitlines() if l.startswith("BCE: ")][-1]
    nums = re.fullmatch(r"BCE: mean (\S+) std (\S+); noise: mean (\S+) std (\S+); noise init: mean (\S+) std (\S+)", line)
    assert nums is not None, line
    assert all(float(v) == float(v) for v in nums.groups()) and float(nums.group(1)) > 0


def test_recon_refuses_other_models(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "recon.py"), "--name", "x", "--model", "cgan", "--dataroot", "synthetic",
                        "--gpu_ids", "-1", "--checkpoints_dir", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "only --model fcgan" in r.stderr, (r.returncode, r.stderr[-2000:])

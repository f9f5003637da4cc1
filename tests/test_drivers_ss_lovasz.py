"""train_ss.py with the Lovasz-softmax term, `--which_model_netD None --lovasz_weight 0.5 --lovasz_classes 0 1 --graph`, at 64 x 64
for a few iterations: the graphed run logs a finite G_Lovasz in (0, 1] beside G_CE and saves its checkpoints; another --model
refuses the option by name."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NET = ["--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "64", "--which_model_netG",
       "resnet_6blocks", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout", "--dataroot",
       "synthetic", "--manualSeed", "4", "--which_model_netD", "None", "--weights", "1", "2", "--lovasz_weight", "0.5", "--lovasz_classes",
       "0", "1", "--print_freq", "1", "--valSize", "64", "--save_epoch_freq", "1"]
DRIVER = ["--epoch_size", "1", "--val_epoch_size", "1"]      # train_ss.py's own arguments


@pytest.mark.gpu
def test_graphed_run_logs_the_term_and_saves(tmp_path):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    import train_ss
    from supervised_gan_amd import ops
    ckpt = tmp_path / "ckpt"
    m, _ = train_ss.main(NET + DRIVER + ["--checkpoints_dir", str(ckpt), "--name", "graphed", "--niter", "2", "--niter_decay", "1", "--graph"])
    torch.cuda.synchronize()
    assert m.lovasz == (0.5, (0, 1))
    lines = [l for l in (ckpt / "graphed" / "loss_log.txt").read_text().splitlines() if l.startswith("(epoch:")]
    assert len(lines) == 3 and all("G_CE:" in l and "G_Lovasz:" in l and "G_GAN" not in l for l in lines), lines
    terms = [float(l.split("G_Lovasz:")[1].split()[0]) for l in lines[1:]]      # the first line names the captured tensor before a replay
    last = m.get_current_errors()["G_Lovasz"]
    print(f"logged G_Lovasz {terms}, last {last!r}")
    assert np.isfinite(terms + [last]).all() and all(0.0 < t <= 1.0 for t in terms + [last])
    pth = sorted(f for f in os.listdir(ckpt / "graphed") if f.endswith(".pth"))
    assert {"1_net_G.pth", "3_net_G.pth", "latest_net_G.pth"} <= set(pth), pth
    ops.check_metric_err(m.device)


@pytest.mark.parametrize("model", ["cgan", "fcgan"])
def test_another_model_refuses_the_option_by_name(model):
    from supervised_gan_amd.options import TrainOptions
    argv = ["--name", "t", "--model", model, "--dataroot", "synthetic", "--gpu_ids", "-1", "--lovasz_weight", "0.5", "--lovasz_classes", "0", "1"]
    with pytest.raises(AssertionError, match="--lovasz_weight.*--model segmentation"):
        TrainOptions().parse(argv, save=False, verbose=False)

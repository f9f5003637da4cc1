"""train_ss.py with the Dice / Tversky and focal terms, `--which_model_netD None --dice_weight 0.5 --focal_weight 0.5 --graph`, at
64 x 64 for a few iterations: the graphed run logs finite G_Dice and G_Focal beside G_CE and saves its checkpoints; another --model
refuses either option by name."""
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
       "synthetic", "--manualSeed", "4", "--which_model_netD", "None", "--weights", "1", "2", "--dice_weight", "0.5", "--dice_classes",
       "0", "1", "--focal_weight", "0.5", "--print_freq", "1", "--valSize", "64", "--save_epoch_freq", "1"]
DRIVER = ["--epoch_size", "1", "--val_epoch_size", "1"]      # train_ss.py's own arguments


@pytest.mark.gpu
def test_graphed_run_logs_both_terms_and_saves(tmp_path):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    import train_ss
    from supervised_gan_amd import ops
    ckpt = tmp_path / "ckpt"
    m, _ = train_ss.main(NET + DRIVER + ["--checkpoints_dir", str(ckpt), "--name", "graphed", "--niter", "2", "--niter_decay", "1", "--graph"])
    torch.cuda.synchronize()
    assert m.segterms == (0.5, (0, 1), 0.5, 0.5, 1.0, 1.0, 0.5, 2.0)
    lines = [l for l in (ckpt / "graphed" / "loss_log.txt").read_text().splitlines() if l.startswith("(epoch:")]
    assert len(lines) == 3 and all("G_CE:" in l and "G_Dice:" in l and "G_Focal:" in l and "G_GAN" not in l for l in lines), lines
    dice = [float(l.split("G_Dice:")[1].split()[0]) for l in lines[1:]]      # the first line names the captured tensors before a replay
    focal = [float(l.split("G_Focal:")[1].split()[0]) for l in lines[1:]]
    last = m.get_current_errors()
    print(f"logged G_Dice {dice}, G_Focal {focal}, last {last['G_Dice']!r} {last['G_Focal']!r}")
    assert np.isfinite(dice + focal).all() and all(0.0 < t < 1.0 for t in dice + [last["G_Dice"]]) and all(t > 0.0 for t in focal + [last["G_Focal"]])
    pth = sorted(f for f in os.listdir(ckpt / "graphed") if f.endswith(".pth"))
    assert {"1_net_G.pth", "3_net_G.pth", "latest_net_G.pth"} <= set(pth), pth
    ops.check_metric_err(m.device)


@pytest.mark.parametrize("flag", ["--dice_weight", "--focal_weight"])
@pytest.mark.parametrize("model", ["cgan", "fcgan"])
def test_another_model_refuses_the_option_by_name(model, flag):
    from supervised_gan_amd.options import TrainOptions
    argv = ["--name", "t", "--model", model, "--dataroot", "synthetic", "--gpu_ids", "-1", flag, "0.5"]
    with pytest.raises(AssertionError, match=flag + ".*--model segmentation"):
        TrainOptions().parse(argv, save=False, verbose=False)

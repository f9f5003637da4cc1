"""GPU test of test_ss.py with the --clean_* options: the scores are taken on the cleaned wall map, the pooled counts of the cleaning
stage are printed and the cleaned map joins the result page as fake_B_clean; without the options none of that happens."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
ASKED = ["RandScore", "ObjF1", "BoundF"]
CLEAN = ["--clean_close", "1.5", "--clean_min_wall", "4", "--clean_min_cell", "10"]


def _net_argv(ckpt, name="clean"):
    return ["--name", name, "--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "64",
            "--which_model_netG", "resnet_6blocks", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout",
            "--checkpoints_dir", str(ckpt), "--dataroot", "synthetic", "--manualSeed", "4", "--which_metric", *ASKED]


_TRAIN = ["--which_model_netD", "n_layers", "--n_layers_D", "2", "--ndf", "8", "--scale_factor", "1", "--lambda_D", "1.0", "--weights", "1", "2",
          "--no_lsgan", "--print_freq", "1", "--valSize", "64"]


def _clean_images(res):
    return sorted(f for _, _, files in os.walk(res) for f in files if f.endswith("_fake_B_clean.png"))


def test_test_ss_scores_prints_and_shows_the_cleaned_map(tmp_path, capsys):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    import test_ss
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    opt = TrainOptions().parse(_net_argv(tmp_path) + _TRAIN, save=False, verbose=False)
    model = create_model(opt)                    # a checkpoint for test_ss.py to load: one step of the trainer
    for data in SyntheticDataset(opt, 1):
        model.set_input(data)
        model.optimize_parameters()
    model.save("latest")
    capsys.readouterr()
    accs, ce = test_ss.main(_net_argv(tmp_path) + CLEAN + ["--results_dir", str(tmp_path / "res"), "--how_many", "2"])
    printed = capsys.readouterr().out
    assert list(accs) == ASKED and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in accs.values()), accs
    assert ce.shape == (2,) and np.isfinite(ce).all()
    line = [l for l in printed.splitlines() if l.startswith("clean: ")]
    assert len(line) == 1 and "in 2 images (close_rsq 2, min wall 4, min cell 10)" in line[0], printed[-2000:]
    assert _clean_images(tmp_path / "res") == ["synthetic_0000_fake_B_clean.png", "synthetic_0001_fake_B_clean.png"]
    plain, _ = test_ss.main(_net_argv(tmp_path) + ["--results_dir", str(tmp_path / "res_plain"), "--how_many", "2"])
    printed = capsys.readouterr().out
    assert list(plain) == ASKED and "clean: " not in printed and _clean_images(tmp_path / "res_plain") == []
    assert os.listdir(tmp_path / "res_plain")    # the page itself was written

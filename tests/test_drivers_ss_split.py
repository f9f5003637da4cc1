"""GPU test of the drivers with --clean_split: test_ss.py takes the scores on the split wall map, prints the pooled counts of the
stage after the `clean:` line and adds the final map to the result page as fake_B_clean; train_ss.py validates with it, eager and
under --graph, to the same scores; without the option none of that happens and the scores are those of --clean_split 0.
The tiny nets and sizes of test_drivers_ss_clean.py."""
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
SPLIT = ["--clean_split", "2", "--clean_split_rounds", "16"]


def _net_argv(ckpt, name="split"):
    return ["--name", name, "--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "64",
            "--which_model_netG", "resnet_6blocks", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout",
            "--checkpoints_dir", str(ckpt), "--dataroot", "synthetic", "--manualSeed", "4", "--which_metric", *ASKED]


_TRAIN = ["--which_model_netD", "n_layers", "--n_layers_D", "2", "--ndf", "8", "--scale_factor", "1", "--lambda_D", "1.0", "--weights", "1", "2",
          "--no_lsgan", "--print_freq", "1", "--valSize", "64"]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")


def _clean_images(res):
    return sorted(f for _, _, files in os.walk(res) for f in files if f.endswith("_fake_B_clean.png"))


def _lines(printed, prefix):
    return [l for l in printed.splitlines() if l.startswith(prefix)]


def test_test_ss_scores_prints_and_shows_the_split_map(tmp_path, capsys):
    _need_gpu()
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
    # all four options: the split line follows the clean line
    accs, ce = test_ss.main(_net_argv(tmp_path) + CLEAN + SPLIT + ["--results_dir", str(tmp_path / "res"), "--how_many", "2"])
    printed = capsys.readouterr().out
    assert list(accs) == ASKED and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in accs.values()), accs
    assert ce.shape == (2,) and np.isfinite(ce).all()
    score_lines = [l for l in printed.splitlines() if l.startswith(("clean: ", "split: "))]
    assert len(score_lines) == 2 and score_lines[0].startswith("clean: ") and score_lines[1].startswith("split: "), printed[-2000:]
    assert "in 2 images (close_rsq 2, min wall 4, min cell 10)" in score_lines[0]
    assert score_lines[1].endswith("of 2 images (split_rsq 4, 16 rounds)"), score_lines[1]
    at = printed.splitlines().index(score_lines[0])
    assert printed.splitlines()[at + 1] == score_lines[1]
    assert _clean_images(tmp_path / "res") == ["synthetic_0000_fake_B_clean.png", "synthetic_0001_fake_B_clean.png"]
    # the split alone: its line, no clean line, and the map on the page
    alone, _ = test_ss.main(_net_argv(tmp_path) + SPLIT + ["--results_dir", str(tmp_path / "res_split"), "--how_many", "2"])
    printed = capsys.readouterr().out
    assert list(alone) == ASKED and len(_lines(printed, "split: ")) == 1 and not _lines(printed, "clean: ")
    assert _clean_images(tmp_path / "res_split") == ["synthetic_0000_fake_B_clean.png", "synthetic_0001_fake_B_clean.png"]
    # the option absent, and set to 0: no line, no image, the same scores
    plain, ce_plain = test_ss.main(_net_argv(tmp_path) + ["--results_dir", str(tmp_path / "res_plain"), "--how_many", "2"])
    printed = capsys.readouterr().out
    assert list(plain) == ASKED and not _lines(printed, "split: ") and not _lines(printed, "clean: ")
    assert _clean_images(tmp_path / "res_plain") == []
    zero, ce_zero = test_ss.main(_net_argv(tmp_path) + ["--clean_split", "0", "--results_dir", str(tmp_path / "res_zero"), "--how_many", "2"])
    printed_zero = capsys.readouterr().out
    assert dict(zero) == dict(plain) and np.array_equal(ce_zero, ce_plain) and not _lines(printed_zero, "split: ")
    assert _clean_images(tmp_path / "res_zero") == []
    assert sorted(os.listdir(tmp_path / "res_zero")) == sorted(os.listdir(tmp_path / "res_plain"))
    results = lambda text: text[text.index("Segmentation results:"):]      # noqa: E731
    assert results(printed_zero) == results(printed)      # the scores and the cross entropy, line for line


def test_train_ss_validates_with_the_split_eager_and_graphed(tmp_path, capsys):
    _need_gpu()
    import train_ss
    runs = {}
    for graph in (False, True):
        argv = _net_argv(tmp_path, "g%d" % graph) + _TRAIN + CLEAN + SPLIT + ["--val_epoch_size", "2", "--max_steps", "2"]
        model, _ = train_ss.main(argv + (["--graph"] if graph else []))
        torch.cuda.synchronize()
        accs = model.get_current_accs()
        assert list(accs) == ASKED and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in accs.values()), accs
        split = model.get_split_counts()
        assert split["images"] == 2 and split["labelled_pixels"] > 0, split      # the validation pass was the last to accumulate
        assert model.get_clean_counts()["images"] == 2
        runs[graph] = (dict(accs), dict(split))
    capsys.readouterr()
    assert runs[False][1]["images"] == runs[True][1]["images"]

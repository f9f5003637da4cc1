"""GPU test of test_ss.py with --whole_image / --tta d4 on an image folder: every pixel of every image is predicted and scored, the result
page shows full-size predictions, and a second run gives the same accuracies (there is no random crop).  Without the flags the same
folder goes through the crop path as before."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
H, W = 168, 200
ASKED = ["RandScore", "meanIU"]


def _net_argv(tmp_path):
    return ["--name", "tile_drv", "--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "single", "--fineSize", "128",
            "--which_model_netG", "unet_128", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout",
            "--checkpoints_dir", str(tmp_path / "ckpt"), "--manualSeed", "4", "--resize_or_crop", "crop", "--which_metric", *ASKED]


def _write_folder(root):
    from PIL import Image
    os.makedirs(root / "test")
    yy, xx = np.mgrid[:H, :W]
    for i in range(2):
        wall = ((yy % (14 + 4 * i) < 2) | (xx % 20 < 2)).astype(np.uint8) * 255
        img = np.stack([wall, 255 - wall, np.random.RandomState(i).randint(0, 256, size=(H, W), dtype=np.uint8)], axis=2)
        Image.fromarray(img).save(str(root / "test" / ("section_%d.png" % i)))


def _run(monkeypatch, argv):
    """test_ss.main(argv) -> (accs, ce, the model it built)."""
    import test_ss
    made = []
    real = test_ss.create_model

    def create(opt):
        made.append(real(opt))
        return made[-1]

    monkeypatch.setattr(test_ss, "create_model", create)
    accs, ce = test_ss.main(argv)
    return accs, ce, made[-1]


def _predictions(res):
    return sorted(os.path.join(d, f) for d, _, files in os.walk(res) for f in files if f.endswith("_prediction.png"))


def test_test_ss_predicts_and_scores_whole_images(tmp_path, monkeypatch):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from PIL import Image
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    _write_folder(tmp_path / "data")
    opt = TrainOptions().parse(_net_argv(tmp_path) + ["--dataroot", "synthetic", "--which_model_netD", "None"], save=False, verbose=False)
    create_model(opt).save("latest")                     # a freshly initialised unet_128 for test_ss.py to load
    folder = ["--dataroot", str(tmp_path / "data")]
    tile = ["--whole_image", "--tile", "128", "--tile_margin", "16", "--tta", "d4"]
    runs = []
    for k in range(2):
        accs, ce, model = _run(monkeypatch, _net_argv(tmp_path) + folder + tile + ["--results_dir", str(tmp_path / ("res%d" % k))])
        assert list(accs) == ASKED and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in accs.values()), accs
        assert ce.shape == (2,) and np.isfinite(ce).all() and (ce > 0).all()
        assert model.numAveragedPixels == 2 * H * W and model.numAveragedImages == 2
        shown = _predictions(tmp_path / ("res%d" % k))
        assert [os.path.basename(f) for f in shown] == ["section_0_prediction.png", "section_1_prediction.png"]
        assert all(Image.open(f).size == (W, H) for f in shown)
        runs.append((dict(accs), ce))
    assert runs[0][0] == runs[1][0]                      # no random crop: the same accuracies on every run
    # without the flags: one --fineSize crop per file, as before
    accs, ce, model = _run(monkeypatch, _net_argv(tmp_path) + folder + ["--results_dir", str(tmp_path / "res_crop")])
    assert list(accs) == ASKED and ce.shape == (2,) and model.numAveragedPixels == 2 * 128 * 128
    assert all(Image.open(f).size == (128, 128) for f in _predictions(tmp_path / "res_crop"))

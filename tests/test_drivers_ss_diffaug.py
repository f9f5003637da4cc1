"""GPU test of the drivers under `--diffaug translation,cutout,color`: train.py (cgan) and train_ss.py (segmentation with a
discriminator) on the synthetic feeder, eager and graphed, save the usual checkpoints; test.py and test_ss.py load them and, having no
such option, build no augmentation state."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

AUG = ["--diffaug", "translation,cutout,color"]
D_NET = ["--which_model_netD", "n_layers", "--n_layers_D", "3", "--ndf", "8", "--scale_factor", "1", "--lambda_D", "1.0", "--weights", "1", "2",
         "--no_lsgan", "--print_freq", "1"]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_train_then_test_cgan_with_diffaug(tmp_path, graph):
    _need_gpu()
    import test as test_driver
    import train as train_driver
    net = ["--name", "drv_da", "--model", "cgan", "--which_direction", "AtoB", "--dataset_mode", "single", "--fineSize", "256",
           "--which_model_netG", "unet_128", "--ngf", "8", "--norm", "instance", "--which_channel", "rg_b", "--gpu_ids", "0", "--no_dropout",
           "--checkpoints_dir", str(tmp_path / "ckpt"), "--dataroot", "synthetic", "--manualSeed", "4"]
    m = train_driver.main(net + D_NET + AUG + ["--max_steps", "2"] + (["--graph"] if graph else []))
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in m.get_current_errors().values())
    assert m.diffaug is not None and int(m.diffaug.offset.item()) >= 12      # 6 blocks a step (graphed: the warm-up steps draw too)
    pth = sorted(f for f in os.listdir(tmp_path / "ckpt" / "drv_da") if f.endswith(".pth"))
    assert {"latest_net_D_0.pth", "latest_net_G.pth"} <= set(pth), pth
    out = test_driver.main(net + ["--results_dir", str(tmp_path / "res"), "--how_many", "2"])
    assert len(out) == 4 and all(os.path.exists(p) for p in out)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_train_ss_then_test_ss_with_diffaug(tmp_path, graph):
    _need_gpu()
    import test_ss
    import train_ss
    net = ["--name", "drv_ss_da", "--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "256",
           "--which_model_netG", "unet_128", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout",
           "--checkpoints_dir", str(tmp_path / "ckpt"), "--dataroot", "synthetic", "--manualSeed", "4", "--which_metric", "RandScore", "meanIU"]
    model, best = train_ss.main(net + D_NET + AUG + ["--valSize", "256", "--best_metric", "RandScore", "--val_epoch_size", "1", "--max_steps", "2"]
                                + (["--graph"] if graph else []))
    torch.cuda.synchronize()
    assert model.diffaug is not None and model.diffaug.colour_mask == 1 and int(model.diffaug.offset.item()) >= 12
    errors = model.get_current_errors()
    assert set(errors) == {"G_CE", "G_GAN", "D_real", "D_fake"} and all(np.isfinite(v) for v in errors.values()), errors
    assert best <= 1.0
    ckpt = tmp_path / "ckpt" / "drv_ss_da"
    assert (ckpt / "latest_net_G.pth").exists() and (ckpt / "latest_net_D_0.pth").exists()
    accs, ce = test_ss.main(net + ["--results_dir", str(tmp_path / "res"), "--how_many", "2", "--which_epoch", "latest"])
    assert list(accs) == ["RandScore", "meanIU"] and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in accs.values())
    assert ce.shape == (2,) and np.isfinite(ce).all()
    # the test side has no such option and no state
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TestOptions
    t = create_model(TestOptions().parse(net, save=False, verbose=False))
    assert t.diffaug is None and not hasattr(t.opt, "diffaug")

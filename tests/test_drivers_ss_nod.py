"""GPU test of train_ss.py / test_ss.py on the supervised baseline, `--model segmentation --which_model_netD None`: the run trains on the
cross-entropy alone, validates, keeps a `best` checkpoint, logs G_CE only, and test_ss.py loads its discriminator-less directory."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("graph", [False, True])
def test_train_ss_then_test_ss_without_discriminators(tmp_path, graph):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    import test_ss
    import train_ss
    net = ["--name", "drv_nod", "--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "256",
           "--which_model_netG", "unet_128", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout",
           "--checkpoints_dir", str(tmp_path / "ckpt"), "--dataroot", "synthetic", "--manualSeed", "4", "--which_model_netD", "None",
           "--which_metric", "RandScore", "meanIU"]
    train = ["--weights", "1", "2", "--print_freq", "1", "--valSize", "256", "--best_metric", "meanIU", "--epoch_size", "2", "--niter", "1",
             "--niter_decay", "1", "--save_epoch_freq", "1", "--val_epoch_size", "2"]
    model, best = train_ss.main(net + train + (["--graph"] if graph else []))
    torch.cuda.synchronize()
    assert not hasattr(model, "netD") and not hasattr(model, "optimizer_D")
    accs = model.get_current_accs()
    assert list(accs) == ["RandScore", "meanIU"] and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in accs.values()), accs
    assert 0.0 <= best <= 1.0 and best >= accs["meanIU"] and model.numAveragedImages == 2
    ckpt = tmp_path / "ckpt" / "drv_nod"
    pth = sorted(f for f in os.listdir(ckpt) if f.endswith(".pth"))
    assert pth == ["1_net_G.pth", "2_net_G.pth", "best_net_G.pth", "latest_net_G.pth"], pth
    acc_log = (ckpt / "acc_log.txt").read_text().splitlines()
    assert sum(l.startswith("(train,") for l in acc_log) == 4 and sum(l.startswith("(val,") for l in acc_log) == 2, acc_log
    assert all("RandScore:" in l and "meanIU:" in l for l in acc_log)
    loss_log = [l for l in (ckpt / "loss_log.txt").read_text().splitlines() if l.startswith("(epoch:")]
    assert len(loss_log) == 4 and all("G_CE:" in l and "G_GAN" not in l and "D_real" not in l for l in loss_log), loss_log
    for which in ("latest", "best"):
        accs_t, ce = test_ss.main(net + ["--results_dir", str(tmp_path / "res"), "--how_many", "3", "--which_epoch", which])
        assert list(accs_t) == ["RandScore", "meanIU"] and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in accs_t.values())
        assert ce.shape == (3,) and np.isfinite(ce).all() and (ce > 0).all()

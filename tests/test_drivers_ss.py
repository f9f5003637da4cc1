"""GPU tests of train_ss.py / test_ss.py: the segmentation trainers with the accuracies accumulated on the device after every step,
the validation pass, the `best` checkpoint and the accuracy log; and the device metrics against the host arithmetic they replace."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")


def _argv(tmp_path, name):
    net = ["--name", name, "--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "256",
           "--which_model_netG", "unet_128", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout",
           "--checkpoints_dir", str(tmp_path / "ckpt"), "--dataroot", "synthetic", "--manualSeed", "4",
           "--which_metric", "RandScore", "meanIU"]
    d = ["--which_model_netD", "n_layers", "--n_layers_D", "3", "--ndf", "8", "--scale_factor", "1", "--lambda_D", "1.0", "--weights", "1", "2",
         "--no_lsgan", "--print_freq", "1", "--valSize", "256", "--best_metric", "RandScore"]
    return net, d


def _host_rand(model):
    from supervised_gan_amd.util import compute_Rand_F_scores
    return float(compute_Rand_F_scores(model.fake_B.detach()[0, 0].cpu().numpy(), model.real_B.detach()[0, 0].cpu().numpy())[0])


def _parent_accuracy(model):
    """pixelAcc, meanAcc, meanIU as the host implementation this path replaces computed them, in torch on the same tensors."""
    k = model.num_classes
    labels, pred = model.label, model.logit.detach().argmax(dim=1)
    conf = torch.bincount((labels.reshape(-1) * k + pred.reshape(-1)), minlength=k * k).reshape(k, k).double().cpu().numpy()
    rel, sel, tp = conf.sum(axis=1), conf.sum(axis=0), np.diag(conf)
    return tp.sum() / max(1, labels.numel()), float(np.mean(tp / np.maximum(1, rel))), float(np.mean(tp / np.maximum(1, rel + sel - tp)))


@pytest.mark.parametrize("graph", [False, True])
def test_train_ss_then_test_ss(tmp_path, graph):
    _need_gpu()
    import test_ss
    import train_ss
    net, d = _argv(tmp_path, "drv_ss")
    # two epochs of two steps: a (replayed) step follows a validation pass
    model, best = train_ss.main(net + d + ["--epoch_size", "2", "--niter", "1", "--niter_decay", "1", "--save_epoch_freq", "1",
                                           "--val_epoch_size", "2", "--save_val_visuals"] + (["--graph"] if graph else []))
    torch.cuda.synchronize()
    accs = model.get_current_accs()
    assert list(accs) == ["RandScore", "meanIU"] and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in accs.values()), accs
    assert best >= accs["RandScore"] and model.numAveragedImages == 2            # the validation pass was the last to accumulate
    ckpt = tmp_path / "ckpt" / "drv_ss"
    assert (ckpt / "best_net_G.pth").exists() and (ckpt / "latest_net_G.pth").exists()
    log = (ckpt / "acc_log.txt").read_text().splitlines()
    assert sum(l.startswith("(train,") for l in log) == 4 and sum(l.startswith("(val,") for l in log) == 2, log
    assert all("RandScore:" in l and "meanIU:" in l for l in log)
    assert sorted(os.listdir(ckpt / "val" / "epoch002")) == ["synthetic_0000_label.png", "synthetic_0000_prediction.png",
                                                             "synthetic_0001_label.png", "synthetic_0001_prediction.png"]
    for which in ("latest", "best"):
        accs_t, ce = test_ss.main(net + ["--results_dir", str(tmp_path / "res"), "--how_many", "3", "--which_epoch", which])
        assert list(accs_t) == ["RandScore", "meanIU"] and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in accs_t.values())
        assert ce.shape == (3,) and np.isfinite(ce).all() and (ce > 0).all()


@pytest.mark.parametrize("graph", [False, True])
def test_one_step_run_scores_what_the_host_function_scores(tmp_path, graph):
    """One optimizer step (graphed: the capture and one replay), one validation image: the RandScore the run returns is
    util.compute_Rand_F_scores on channel 0 of the trainer's last fake_B / real_B, and the accuracies are the host implementation's
    arithmetic on its last logit / label."""
    _need_gpu()
    import train_ss
    net, d = _argv(tmp_path, "drv_ss1")
    model, best = train_ss.main(net + d + ["--val_epoch_size", "1"] + (["--max_steps", "2", "--graph"] if graph else ["--max_steps", "1"]))
    accs = model.get_current_accs()
    assert best == accs["RandScore"]
    host = _host_rand(model)
    print("RandScore device %r host %r" % (accs["RandScore"], host))
    assert abs(accs["RandScore"] - host) < 1e-9 and model.numAveragedImages == 1
    pa, ma, miu = _parent_accuracy(model)
    assert (model.pixelAcc, model.meanAcc, model.meanIU) == (pa, ma, miu) and accs["meanIU"] == miu
    assert model.numAveragedPixels == 256 * 256


def test_accum_after_a_step_changes_no_value():
    """A step plus accum_accs, twice: pixelAcc / meanAcc / meanIU equal the parent implementation's running arithmetic, and the
    background-class form (--add_background_onehot_acc) equals its torch expression as well."""
    _need_gpu()
    import tempfile
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    from supervised_gan_amd.util import compute_Rand_F_scores
    from pathlib import Path
    with tempfile.TemporaryDirectory() as tmp:
        net, d = _argv(Path(tmp), "acc")
        for extra in ([], ["--add_background_onehot_acc"]):
            opt = TrainOptions().parse(net + d + extra, save=False, verbose=False)
            model = create_model(opt)
            k = model.num_classes + (1 if extra else 0)
            conf, rand = np.zeros((k, k)), []
            for data in SyntheticDataset(opt, 2):
                model.set_input(data)
                model.optimize_parameters()
                model.accum_accs()
                if extra:
                    bg = lambda t: torch.cat([t, 1.0 - torch.clamp(t.sum(dim=1, keepdim=True), max=1)], 1).argmax(dim=1)      # noqa: E731
                    labels, pred = bg(model.real_B), bg(model.fake_B.detach())
                else:
                    labels, pred = model.label, model.logit.detach().argmax(dim=1)
                conf += torch.bincount((labels.reshape(-1) * k + pred.reshape(-1)), minlength=k * k).reshape(k, k).double().cpu().numpy()
                rand.append(_host_rand(model))
            accs = model.get_current_accs()
            rel, sel, tp = conf.sum(axis=1), conf.sum(axis=0), np.diag(conf)
            assert np.array_equal(model.confusion, conf) and model.numAveragedPixels == 2 * 256 * 256
            assert model.pixelAcc == tp.sum() / (2 * 256 * 256)
            assert model.meanAcc == float(np.mean(tp / np.maximum(1, rel))) and model.meanIU == float(np.mean(tp / np.maximum(1, rel + sel - tp)))
            assert abs(accs["RandScore"] - np.mean(rand)) < 1e-9 and model.numAveragedImages == 2
            model.reset_accs()
            assert model.get_current_accs()["meanIU"] == 0 and model.numAveragedImages == 0


def test_a_replay_after_an_eager_forward_scores_the_steps_own_tensors(tmp_path):
    """GraphedStep.reinstall(): a validation forward between two replays leaves fake_B / logit naming its own tensors; after
    reinstall() the attributes are the captured step's again, and the accuracies of the next replayed step equal the host's
    arithmetic on them."""
    _need_gpu()
    from supervised_gan_amd.graph_step import GraphedStep
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    net, d = _argv(tmp_path, "reinstall")
    opt = TrainOptions().parse(net + d, save=False, verbose=False)
    model = create_model(opt)
    data = list(SyntheticDataset(opt, 3))
    g = GraphedStep(model)
    assert not g.captured
    g.capture(data[0])
    g.step(data[1])
    assert g.captured
    step_fake, step_logit = model.fake_B, model.logit
    model.set_input(data[2])
    with torch.no_grad():
        model.forward(val_mode=True)
    assert model.fake_B is not step_fake and model.fake_B.data_ptr() != step_fake.data_ptr()
    g.reinstall()
    assert model.fake_B is step_fake and model.logit is step_logit
    g.step(data[0])
    model.reset_accs()
    model.accum_accs()
    accs = model.get_current_accs()
    assert abs(accs["RandScore"] - _host_rand(model)) < 1e-9
    assert (model.pixelAcc, model.meanAcc, model.meanIU) == _parent_accuracy(model)


def test_validation_draws_its_latent_at_noiseSizeVal(tmp_path):
    """A generator that takes a latent (crn: H / 64 x W / 64): trained at 256 with --noiseSize 4, validated at --valSize 128, which
    only a latent of --noiseSizeVal 2 fits."""
    _need_gpu()
    import train_ss
    argv = ["--name", "drv_ss_crn", "--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "256",
            "--which_model_netG", "crn", "--upsample_mode", "bilinear", "--n_layers_CRN_block", "2", "--ngf", "8", "--noise_nc", "8",
            "--noiseSize", "4", "--noiseSizeVal", "2", "--valSize", "128", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0",
            "--no_dropout", "--checkpoints_dir", str(tmp_path / "ckpt"), "--dataroot", "synthetic", "--manualSeed", "4",
            "--which_metric", "RandScore", "meanIU", "--best_metric", "meanIU", "--which_model_netD", "n_layers", "--n_layers_D", "3",
            "--ndf", "8", "--scale_factor", "1", "--lambda_D", "1.0", "--no_lsgan", "--print_freq", "1", "--max_steps", "2",
            "--val_epoch_size", "1"]
    model, best = train_ss.main(argv)
    accs = model.get_current_accs()
    assert tuple(model.noise.shape) == (1, 8, 2, 2) and tuple(model.fake_B.shape) == (1, 2, 128, 128)
    assert model.numAveragedPixels == 128 * 128 and best == accs["meanIU"] and 0.0 <= best <= 1.0
    assert abs(accs["RandScore"] - _host_rand(model)) < 1e-9
    assert (tmp_path / "ckpt" / "drv_ss_crn" / "best_net_G.pth").exists()


def test_train_ss_then_test_ss_segmentation_cycle(tmp_path):
    """`--model segmentation_cycle` through both drivers: the accuracy methods it borrows from SegmentationModel, forward(val_mode)."""
    _need_gpu()
    import test_ss
    import train_ss
    net = ["--name", "drv_ssc", "--model", "segmentation_cycle", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "256",
           "--which_model_netG1", "unet_128", "--ngf1", "8", "--which_model_netG2", "unet_128", "--ngf2", "8", "--norm", "instance",
           "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout1", "--no_dropout2", "--checkpoints_dir", str(tmp_path / "ckpt"),
           "--dataroot", "synthetic", "--manualSeed", "4", "--which_metric", "RandScore", "meanIU"]
    d = ["--which_model_netD2", "n_layers", "--n_layers_D2", "3", "--ndf2", "8", "--scale_factor2", "1", "--lambda_D2", "1.0", "--no_lsgan2",
         "--max_steps", "2", "--print_freq", "1", "--valSize", "256", "--best_metric", "RandScore", "--val_epoch_size", "1"]
    model, best = train_ss.main(net + d)
    accs = model.get_current_accs()
    assert model.name() == "SegmentationCycleModel" and best == accs["RandScore"]
    assert abs(accs["RandScore"] - _host_rand(model)) < 1e-9 and (model.pixelAcc, model.meanAcc, model.meanIU) == _parent_accuracy(model)
    files = sorted(f for f in os.listdir(tmp_path / "ckpt" / "drv_ssc") if f.startswith("best"))
    assert files == ["best_net_D2_0.pth", "best_net_G1.pth", "best_net_G2.pth"]
    accs_t, ce = test_ss.main(net + ["--results_dir", str(tmp_path / "res"), "--how_many", "2", "--which_epoch", "best"])
    assert list(accs_t) == ["RandScore", "meanIU"] and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in accs_t.values())
    assert ce.shape == (2,) and np.isfinite(ce).all()

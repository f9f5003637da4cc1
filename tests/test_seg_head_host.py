"""Host-side checks of the discriminator-less segmentation trainer (`--which_model_netD None`) and its fused loss head: the C ABI
declares and binds the two entry points, the trainer builds without discriminators on the CPU, and the composition that serves
seg_head calls outside the kernel's envelope reproduces the torch expressions of the reference."""
import os
import re

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["sgan_label_weight_sum", "sgan_seg_head"]


def _header():
    with open(os.path.join(ROOT, "include", "sgan_hip.h")) as f:
        return f.read()


def test_header_declares_and_lib_binds_the_new_entry_points():
    from supervised_gan_amd import _lib
    h = _header()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, h), "include/sgan_hip.h does not declare " + name
        assert name in _lib.SIGNATURES, "_lib.py does not bind " + name
    # one ctypes argument per declared parameter
    for name in NEW_ENTRIES:
        params = re.search(r"\bint\s+%s\s*\((.*?)\);" % name, h, re.S).group(1)
        assert len(params.split(",")) == len(_lib.SIGNATURES[name]), name
    with open(os.path.join(ROOT, "supervised-gan_amd", "csrc", "Makefile")) as f:
        assert "sgan_seghead.hip" in f.read()


def test_workspace_and_mode_constants_match_the_header():
    from supervised_gan_amd import _lib, ops
    h = _header()
    assert int(re.search(r"#define\s+SGAN_SEGHEAD_WS_BYTES\s+(\d+)", h).group(1)) == ops.SEGHEAD_WS_BYTES
    for mode in ("SOFTMAX", "SIGMOID"):
        v = int(re.search(r"#define\s+SGAN_SEGHEAD_%s\s+(\d+)" % mode, h).group(1))
        assert v == getattr(_lib, "SEGHEAD_" + mode) == getattr(ops, "SEGHEAD_" + mode)


def test_not_covered_calls_answer_one_without_a_launch(built_lib):
    """C > 16 or a NULL required pointer: status 1, decided before anything touches a device."""
    from supervised_gan_amd import _lib
    l = _lib.lib()
    assert l.sgan_seg_head(None, 4, 16, 2, 0, None, 0, None, 0, None, None, 4, None, 0, None, None, None) == 1
    assert l.sgan_label_weight_sum(None, 16, 2, None, None, None, None) == 1


def _argv(tmp, extra=()):
    return ["--name", "t", "--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "128",
            "--which_model_netG", "unet_128", "--ngf", "8", "--which_model_netD", "None", "--norm", "instance", "--which_channel", "b_rg",
            "--gpu_ids", "-1", "--no_dropout", "--weights", "1", "3", "--n_update_G", "2", "--checkpoints_dir", str(tmp), *extra]


def test_trainer_without_discriminators_builds_on_cpu(tmp_path):
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    from supervised_gan_amd.segm_model import SegmentationModel
    opt = TrainOptions().parse(_argv(tmp_path), save=False, verbose=False)
    assert opt.which_model_netD == "None" and opt.isTrain
    m = create_model(opt)
    assert isinstance(m, SegmentationModel) and m.num_classes == 2
    for name in ("netD", "optimizer_D", "fake_pool", "criterionGAN"):
        assert not hasattr(m, name), name
    assert hasattr(m, "optimizer_G")
    m.save("t")
    assert sorted(os.listdir(tmp_path / "t")) == ["t_net_G.pth"]
    m.optimizer_G.sync_lr = lambda: None
    m.update_learning_rate()
    assert abs(m.optimizer_G.param_groups[0]["lr"] - (2e-4 - 2e-4 / 100)) < 1e-12
    assert m.step_pools() == [] and len(m.step_zeroing()) == 0
    program = m.step_program()
    lists = [item for item in program if isinstance(item, list)]
    syncs = [item for item in program if isinstance(item, tuple)]
    assert len(lists) == 4 and len(syncs) == 2 and all(s == ("sync", m.optimizer_G) for s in syncs)
    assert lists[0] == [m.optimizer_G.zero_grad, m.backward_G] and lists[1] == [m.optimizer_G.step, m.sample_noise]
    # --continue_train reads the generator's file only
    m2 = create_model(TrainOptions().parse(_argv(tmp_path, ["--continue_train", "--which_epoch", "t"]), save=False, verbose=False))
    for (k, a), (_, b) in zip(m.netG.state_dict().items(), m2.netG.state_dict().items()):
        assert torch.equal(a, b), k


def test_with_discriminators_the_step_is_the_conditional_gans(tmp_path):
    """With discriminators the segmentation step stays CGANModel's: D then G, optimizer_D's zeroing folded into the step's first
    launch, one ImagePool fed by _pool_source()."""
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    argv = _argv(tmp_path)
    i = argv.index("--which_model_netD")
    argv[i + 1] = "n_layers"
    m = create_model(TrainOptions().parse(argv + ["--ndf", "8", "--n_layers_D", "3", "--scale_factor", "1", "--lambda_D", "1.0"],
                                          save=False, verbose=False))
    assert len(m.netD) == 1 and hasattr(m, "optimizer_D") and not m.no_netD
    assert m.step_stages() == [(m.optimizer_D, m.backward_D, 1), (m.optimizer_G, m.backward_G, 2)]
    m.optimizer_D.take_zeroing = lambda: "the zeroing of D"
    assert m.step_zeroing() == "the zeroing of D"
    assert m.step_pools() == [(m.fake_pool, m._pool_source)]


def test_seg_head_composition_on_cpu_tensors():
    from supervised_gan_amd import losses, ops
    g = torch.Generator().manual_seed(11)
    for C_ in (2, 3, 5):
        z = (torch.randn(1, C_, 9, 7, generator=g) * 1.5).requires_grad_(True)
        lab = torch.randint(0, C_, (1, 9, 7), generator=g)
        lab[0, :, 0] = -100
        cw = torch.tensor([2.0, 5.0, 0.5, 3.0, 1.5][:C_])
        for w in (None, cw):
            p, loss = losses.seg_head(z, lab, w, None, ops.SEGHEAD_SOFTMAX)
            assert (p.detach() - F.softmax(z.detach(), 1)).abs().max() < 1e-6
            assert abs(float(loss.detach()) - float(F.cross_entropy(z.detach(), lab, weight=w))) < 1e-6
        t = F.one_hot(lab.clamp(min=0), C_).permute(0, 3, 1, 2).float()
        for nw in (0, 2, C_):
            w = cw[:nw] if nw else None
            p, loss = losses.seg_head(z, t, w, None, ops.SEGHEAD_SIGMOID)
            wm = None
            if nw:
                wm = torch.ones_like(t[:, :1])
                for i in range(nw):
                    wm = wm + t.narrow(1, i, 1) * (cw[i] - 1.0)
            assert (p.detach() - torch.sigmoid(z.detach())).abs().max() < 1e-6
            assert abs(float(loss.detach()) - float(F.binary_cross_entropy(torch.sigmoid(z.detach()), t, weight=wm))) < 1e-6
        loss.backward()
        assert z.grad is not None and torch.isfinite(z.grad).all()

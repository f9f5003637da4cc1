"""hipGraph replay of the training step (graph_step.GraphedStep) against eager launches of the same trainer: same seeds, same
inputs, same ImagePool draws => the same losses and generator outputs (up to the order of floating-point atomics)."""
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FCGAN = ["--model", "fcgan", "--which_direction", "A", "--dataset_mode", "single", "--fineSize", "128", "--input_nc", "2",
         "--which_model_netG", "deconv", "--n_layers_G", "5", "--ngf", "8", "--noise_nc", "8", "--noiseSize", "2", "--no_dropout",
         "--which_channel", "rg", "--which_model_netD", "n_layers", "--n_layers_D", "3", "3", "3", "--ndf", "8",
         "--scale_factor", "1", "2", "4", "--lambda_D", "0.5", "0.4", "0.1", "--n_update_G", "2", "--no_lsgan"]
CGAN = ["--model", "cgan", "--which_direction", "AtoB", "--dataset_mode", "single", "--fineSize", "256", "--which_model_netG", "unet_128",
        "--ngf", "8", "--which_channel", "rg_b", "--which_model_netD", "n_layers", "--n_layers_D", "3", "4", "--ndf", "8",
        "--scale_factor", "1", "1", "--lambda_D", "0.5", "0.5", "--weights", "2", "4", "--no_lsgan", "--n_update_G", "2",
        "--add_gaussian_noise"]
TWOSTAGE = ["--model", "twostage_cycle", "--which_direction", "AtoB", "--dataset_mode", "single", "--fineSize", "256",
            "--transform_1to2", "bilinear_2", "--which_channel", "rg_b", "--which_model_netG1", "fcgan", "--n_layers_G1", "5", "--ngf1", "8",
            "--n_layers_D1", "3", "3", "--ndf1", "8", "--scale_factor1", "1", "2", "--lambda_D1", "0.5", "0.4", "--which_model_netG2", "crn",
            "--ngf2", "8", "--upsample_mode2", "bilinear", "--n_layers_CRN_block2", "2", "--which_model_netF2", "unet_128", "--nff2", "8",
            "--n_layers_D2", "3", "4", "--ndf2", "8", "--scale_factor2", "1", "2", "--lambda_D2", "0.6", "0.4", "--noise_nc1", "8",
            "--noiseSize1", "2", "--noise_nc2", "8", "--noiseSize2", "4", "--no_dropout1", "--no_dropout2", "--no_lsgan1",
            "--GAN_losses_D2", "real_fake", "fake_fake", "--GAN_losses_G2", "real_fake", "fake_fake"]


# twostage_factd (models/twostage_factD_model.py): no cycle, D1_i / D2_i pairs whose maps nest (4-layer D1 on the half-size label)
FACTD = ["--model", "twostage_factd", "--which_direction", "AtoB", "--dataset_mode", "single", "--fineSize", "256",
         "--transform_1to2", "bilinear_2", "--which_channel", "rg_b", "--which_model_netG1", "fcgan", "--n_layers_G1", "5", "--ngf1", "8",
         "--n_layers_D1", "4", "4", "--ndf1", "8", "--scale_factor1", "1", "2", "--lambda_D1", "0.5", "0.4", "--which_model_netG2", "crn",
         "--ngf2", "8", "--upsample_mode2", "bilinear", "--n_layers_CRN_block2", "2", "--n_layers_D2", "3", "3", "--ndf2", "8",
         "--scale_factor2", "1", "2", "--lambda_D2", "0.6", "0.4", "--noise_nc1", "8", "--noiseSize1", "2", "--noise_nc2", "8",
         "--noiseSize2", "4", "--no_dropout1", "--no_dropout2", "--no_lsgan1", "--no_lsgan2",
         "--GAN_losses_D2", "real_fake", "fake_fake", "--GAN_losses_G2", "real_fake", "fake_fake"]


CGAN_CYCLE = ["--model", "cgan_cycle", "--which_direction", "AtoB", "--dataset_mode", "single", "--fineSize", "256", "--which_channel", "rg_b",
              "--which_model_netG1", "unet_128", "--ngf1", "8", "--which_model_netG2", "unet_128", "--ngf2", "8", "--n_layers_D1", "3", "3",
              "--ndf1", "8", "--scale_factor1", "1", "2", "--lambda_D1", "0.6", "0.4", "--no_dropout1", "--no_dropout2", "--no_lsgan1",
              "--weights", "2", "4"]


# the segmentation trainers: class logits out of G (G1), one discriminator on cat(image, one-hot) / cat(one-hot, image)
SEGM = ["--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "128", "--which_model_netG", "unet_128",
        "--ngf", "8", "--which_channel", "b_rg", "--no_dropout", "--which_model_netD", "n_layers", "--n_layers_D", "3", "--ndf", "8",
        "--scale_factor", "1", "--lambda_D", "1.0", "--weights", "1", "2", "--no_lsgan"]
SEGM_CYCLE = ["--model", "segmentation_cycle", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "128",
              "--which_channel", "b_rg", "--which_model_netG1", "unet_128", "--ngf1", "8", "--which_model_netG2", "unet_128", "--ngf2", "8",
              "--no_dropout1", "--no_dropout2", "--which_model_netD2", "n_layers", "--n_layers_D2", "3", "--ndf2", "8", "--scale_factor2", "1",
              "--lambda_D2", "1.0", "--no_lsgan2"]


def _build(argv):
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    opt = TrainOptions().parse(["--name", "g", "--norm", "instance", "--gpu_ids", "0", "--manualSeed", "5", "--checkpoints_dir", "/tmp/sgan_ckpt",
                                *argv], save=False, verbose=False)
    torch.manual_seed(0)
    return create_model(opt)


def _ring(hw, n=4):
    g = torch.Generator().manual_seed(77)
    return [{"A": (torch.rand(1, 3, hw, hw, generator=g) * 2 - 1).cuda(), "B": (torch.rand(1, 3, hw, hw, generator=g) * 2 - 1).cuda(),
             "A_paths": ["s"], "B_paths": ["s"]} for _ in range(n)]


@pytest.mark.parametrize("argv,hw,out", [(FCGAN, 128, "fake"), (CGAN, 256, "fake_B"), (TWOSTAGE, 256, "fake_B_from_fake_A"),
                                         (CGAN_CYCLE, 256, "recon_A"), (FACTD, 256, "fake_B_from_fake_A"), (SEGM, 128, "fake_B"),
                                         (SEGM_CYCLE, 128, "recon_A")],
                         ids=["fcgan", "cgan", "twostage_cycle", "cgan_cycle", "twostage_factd", "segmentation", "segmentation_cycle"])
def test_graphed_step_equals_eager(argv, hw, out):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd.graph_step import GraphedStep
    ring = _ring(hw)
    seq = [0, 0, 1, 2, 3]          # capture() warms up with two eager steps on its example input
    def eager():
        random.seed(11)
        m = _build(argv)
        errs = []
        for i in seq:
            m.set_input(ring[i])
            m.optimize_parameters()
            errs.append(list(m.get_current_errors().values()))
        return m, errs
    a, ea = eager()
    c, _ = eager()           # a second eager run: how far two runs of the SAME launches drift apart (atomics order + Adam)
    random.seed(11)
    b = _build(argv)
    gs = GraphedStep(b)
    gs.capture(ring[0])
    eb = []
    for i in seq[2:]:
        gs.step(ring[i])
        eb.append(list(b.get_current_errors().values()))
    torch.cuda.synchronize()
    ea, eb = np.asarray(ea[2:]), np.asarray(eb)
    assert np.isfinite(eb).all()
    assert np.abs(ea - eb).max() < 2e-2 * max(1.0, np.abs(ea).max()), (ea, eb)      # trajectory tolerance of the step tests
    # five Adam steps amplify the atomics' rounding order pixel-wise (sign-like first updates): compare in relative L2
    ya, yb, yc = (getattr(m, out).detach().double() for m in (a, b, c))
    drift_eager = float((ya - yc).norm() / ya.norm())
    drift_graph = float((ya - yb).norm() / ya.norm())
    print(f"relative L2 drift after {len(seq)} steps: eager vs eager {drift_eager:.2e}, eager vs graph {drift_graph:.2e}")
    # two eager runs drift 3-8 % apart here and the figure itself varies run to run; a replay that dropped or reordered work
    # gives uncorrelated outputs (relative L2 ~ 1.4) or NaNs
    assert drift_graph < max(0.15, 4 * drift_eager)


def test_captured_step_keeps_its_arenas_through_a_foreign_eager_step():
    """A captured program owns the pool its statistics arenas came from (ops.arena_scope in GraphedStep.capture): an eager step of
    another model in the same process -- another arena sequence, which makes ArenaPool.take() replace slots in place -- leaves
    every slot the graphs point into alive at its address, shares no memory with them, and the replays after it still follow the
    eager trajectory."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import ops
    from supervised_gan_amd.graph_step import GraphedStep
    ring, seq = _ring(128), [0, 0, 1, 2, 3]
    random.seed(11)
    a = _build(FCGAN)
    ea = []
    for i in seq:
        a.set_input(ring[i])
        a.optimize_parameters()
        ea.append(list(a.get_current_errors().values()))
    random.seed(11)
    b = _build(FCGAN)
    gs = GraphedStep(b)
    gs.capture(ring[0])
    gs.step(ring[1])
    eb = [list(b.get_current_errors().values())]
    torch.cuda.synchronize()
    own = gs._arenas
    slots = list(own.slots)
    spans = [(s.data_ptr(), s.data_ptr() + s.numel() * s.element_size()) for s in slots]
    assert len(slots) >= 4 and own is not ops.arenas()      # the step's arenas: G forward(s), the D pass, the G passes
    # the foreign step: its python-random pool draws must not shift the ones the fcgan trajectory is compared on
    rnd = random.getstate()
    other = _build(CGAN)
    other.set_input(_ring(256, 1)[0])
    other.optimize_parameters()
    other.optimize_parameters()      # the second step walks the process-wide pool again: clean slots of the first are reused or replaced
    torch.cuda.synchronize()
    random.setstate(rnd)
    foreign = ops.arenas().slots
    assert len(foreign) >= 2 and [s.numel() for s in foreign] != [s.numel() for s in slots]      # it did use a pool, with another sequence
    assert len(own.slots) == len(slots) and all(s is t for s, t in zip(own.slots, slots))
    assert [(s.data_ptr(), s.data_ptr() + s.numel() * s.element_size()) for s in own.slots] == spans
    for f in foreign:
        f0, f1 = f.data_ptr(), f.data_ptr() + f.numel() * f.element_size()
        assert all(f1 <= s0 or s1 <= f0 for s0, s1 in spans), "a slot of the process-wide pool overlaps one the graphs point into"
    for i in seq[3:]:
        gs.step(ring[i])
        eb.append(list(b.get_current_errors().values()))
    torch.cuda.synchronize()
    ea, eb = np.asarray(ea[2:]), np.asarray(eb)
    assert np.isfinite(eb).all()
    assert np.abs(ea - eb).max() < 2e-2 * max(1.0, np.abs(ea).max()), (ea, eb)      # the tolerance of test_graphed_step_equals_eager

"""--diffaug through the trainers on the device: the discriminator and generator gradients of a step against a step
whose augmentation the test applies on the host (util.diffaug_ref / diffaug_bwd_ref in a plain torch autograd function, under the
records the device drew); the latent stream with and without the option; the records under --graph against util.diffaug_params, and
against an eager run; what the image pool keeps; the option beside --ema_decay and --elastic.

Tolerances are those of the step-parity tests of the same trainers (test_hip_step.py): 1e-3 of the largest reference entry for
fcgan and cgan, 2e-3 max(1e-3, that) for segmentation."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from supervised_gan_amd import util  # noqa: E402

pytestmark = pytest.mark.gpu

HW = 128
D_NET = ["--which_model_netD", "n_layers", "--n_layers_D", "3", "--ndf", "8", "--scale_factor", "1", "--lambda_D", "1.0", "--no_lsgan"]
# the smallest option sets of test_graph_step.py / test_hip_ema_train.py; segmentation with a discriminator as test_hip_step.build_segm
ARCH = {
    "segmentation": ["--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", str(HW),
                     "--which_model_netG", "unet_128", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--no_dropout",
                     "--weights", "1", "2"] + D_NET,
    "fcgan": ["--model", "fcgan", "--which_direction", "A", "--dataset_mode", "single", "--fineSize", str(HW), "--input_nc", "2",
              "--which_model_netG", "deconv", "--n_layers_G", "5", "--ngf", "8", "--noise_nc", "8", "--noiseSize", "2", "--no_dropout",
              "--which_channel", "rg", "--norm", "instance", "--which_model_netD", "n_layers", "--n_layers_D", "3", "3", "3", "--ndf", "8",
              "--scale_factor", "1", "2", "4", "--lambda_D", "0.5", "0.4", "0.1", "--no_lsgan"],
    "cgan": ["--model", "cgan", "--which_direction", "AtoB", "--dataset_mode", "single", "--fineSize", str(HW), "--which_model_netG",
             "unet_128", "--ngf", "8", "--which_channel", "rg_b", "--norm", "batch", "--no_dropout", "--weights", "2", "4"] + D_NET,
}
POLICY = ("translation", "cutout", "brightness", "contrast")
AUG = {"segmentation": ["--diffaug", "translation,cutout,color"], "cgan": ["--diffaug", "translation,cutout,color"],
       "fcgan": ["--diffaug", "translation,cutout,color", "--diffaug_color_channels", "g"]}      # fcgan here trains on (r, g)
MASK = {"segmentation": 0b001, "cgan": 0b100, "fcgan": 0b10}      # cat(b | scores), cat(r, g | b), (r, g)
SEED = 5
KINDS = ["cgan", "fcgan", "segmentation"]


def build(kind, ckpt, extra=(), drop=()):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    argv = ["--name", "t", "--gpu_ids", "0", "--manualSeed", str(SEED), "--checkpoints_dir", str(ckpt)]
    argv += [a for a in ARCH[kind] if a not in drop] + list(extra)
    torch.manual_seed(0)
    return create_model(TrainOptions().parse(argv, save=False, verbose=False))


def data(i):
    g = torch.Generator().manual_seed(100 + i)
    return {"A": (torch.rand(1, 3, HW, HW, generator=g) * 2 - 1).cuda(), "B": (torch.rand(1, 3, HW, HW, generator=g) * 2 - 1).cuda(),
            "A_paths": ["s"], "B_paths": ["s"]}


def records(m):
    arr = m.diffaug.records.cpu().numpy()
    return [tuple(float(v) for v in row[:2].view(np.float32)) + tuple(int(v) for v in row[2:]) for row in arr]


class HostAug(torch.autograd.Function):
    """The transform on the host: util.diffaug_ref forward, util.diffaug_bwd_ref backward, float64, on a logical [1, C, H, W] tensor."""

    @staticmethod
    def forward(ctx, x, rec, mask):
        ctx.rec, ctx.mask = rec, mask
        y = util.diffaug_ref(x.detach()[0].permute(1, 2, 0).cpu().numpy(), rec, mask)
        return torch.from_numpy(y).permute(2, 0, 1)[None].to(device=x.device, dtype=torch.float32).contiguous()

    @staticmethod
    def backward(ctx, g):
        dx = util.diffaug_bwd_ref(g[0].permute(1, 2, 0).cpu().numpy(), ctx.rec, ctx.mask)
        return torch.from_numpy(dx).permute(2, 0, 1)[None].to(device=g.device, dtype=torch.float32).contiguous(), None, None


def grads(nets):
    """The weight gradients (a bias in front of a normalisation has none but rounding noise, as in the step-parity tests; the fixed
    Gaussian pre-filter of a coarser-scale discriminator has none at all)."""
    return [p.grad.detach().double().cpu().clone() for net in nets for p in net.parameters() if p.dim() > 1 and p.grad is not None]


def stages(m, inp, z):
    """One step, stage by stage (the order of optimize_parameters): (discriminator gradients, generator gradients)."""
    if z is not None:
        m.noise_source = lambda: z
    m.set_input(inp)
    m.forward()
    m.optimizer_D.zero_grad()
    m.backward_D()
    gd = grads(m.netD)
    recs_d = records(m)[:2] if m.diffaug is not None else None
    m.optimizer_D.step()
    m.optimizer_G.zero_grad()
    m.backward_G()
    torch.cuda.synchronize()
    return gd, grads([m.netG]), recs_d


@pytest.mark.parametrize("kind", KINDS)
def test_step_gradients_equal_a_host_augmented_step(tmp_path, kind):
    z = torch.randn(1, 8, 2, 2, generator=torch.Generator().manual_seed(3)).cuda() if kind == "fcgan" else None
    a = build(kind, tmp_path, AUG[kind])
    assert a.diffaug is not None and a.diffaug.colour_mask == MASK[kind] and a.diffaug.policy == POLICY
    gd_a, gg_a, recs_d = stages(a, data(0), z)
    rec_g = records(a)[2]
    assert a.diffaug.records.shape == (4, 8) and int(a.diffaug.offset.item()) == 6      # two draws of the D stage, one of the G stage
    assert recs_d + [rec_g] == util.diffaug_params(SEED + 7919, 0, [(HW, HW)] * 3, POLICY)
    b = build(kind, tmp_path)
    assert b.diffaug is None
    by_slot = {0: recs_d, 2: [rec_g]}
    b._augment = lambda tensors, slot: [HostAug.apply(t, r, MASK[kind]) for t, r in zip(tensors, by_slot[slot])]
    gd_b, gg_b, _ = stages(b, data(0), z)
    plain = build(kind, tmp_path)
    gd_p, gg_p, _ = stages(plain, data(0), z)
    for what, got, ref, base in (("D", gd_a, gd_b, gd_p), ("G", gg_a, gg_b, gg_p)):
        worst, moved = 0.0, 0.0
        for x, y, p in zip(got, ref, base):
            scale = float(y.abs().max())
            tol = 2e-3 * max(1e-3, scale) if kind == "segmentation" else 1e-3 * scale
            dev = float((x - y).abs().max())
            worst = max(worst, dev / max(scale, 1e-30))
            moved = max(moved, float((p - y).abs().max()) / max(scale, 1e-30))
            assert dev <= tol, (what, dev, tol)
        print(f"{kind}: {what} gradients against the host-augmented step: worst {worst:.2e} of the largest entry; "
              f"the step without augmentation differs by {moved:.2e}")
        assert moved > 1e-2      # the augmentation is in the gradients: the unaugmented step is somewhere else


@pytest.mark.parametrize("kind", ["fcgan", "cgan"])
def test_other_streams_draw_what_they_drew(tmp_path, kind):
    """Two steps with and without the option.  fcgan: the latent of every step, tensor against tensor.  cgan, here with dropout on:
    the first step's fake_B (drawn masks, equal weights) and the position of the generator's dropout stream after both steps -- a
    mask is a function of the key and that position alone."""
    seen = {}
    for aug in (False, True):
        m = build(kind, tmp_path, AUG[kind] if aug else [], drop=("--no_dropout",) if kind == "cgan" else ())
        got = []
        for i in range(2):
            m.set_input(data(i))
            m.optimize_parameters()
            got.append(m.noise.detach().cpu().clone() if kind == "fcgan" else m.netG._rng_offset.cpu().clone())
            if i == 0 and kind == "cgan":
                got.append(m.fake_B.detach().cpu().clone())
        got.append(m._rng_offset.cpu().clone())
        seen[aug] = got
    assert len(seen[True]) == len(seen[False]) and all(torch.equal(x, y) for x, y in zip(seen[True], seen[False]))
    if kind == "fcgan":
        assert not torch.equal(seen[True][0], seen[True][1])
    else:
        assert int(seen[True][0]) > 0      # the dropout stream did draw


@pytest.mark.parametrize("kind", ["cgan", "fcgan"])
def test_graphed_records_follow_the_stream(tmp_path, kind):
    """Three replays: the records left behind are util.diffaug_params at consecutive offsets (6 blocks a step: two D-stage tensors,
    one G-stage tensor), all different; an eager run from the same seed draws the same sequence."""
    from supervised_gan_amd.graph_step import GraphedStep
    m = build(kind, tmp_path, AUG[kind])
    gs = GraphedStep(m)
    gs.capture(data(0))
    torch.cuda.synchronize()
    off = int(m.diffaug.offset.item())
    assert off > 0 and off % 6 == 0      # the warm-up steps drew too
    got = []
    for i in range(1, 4):
        gs.step(data(i))
        torch.cuda.synchronize()
        got.append(records(m)[:3])
        assert got[-1] == util.diffaug_params(SEED + 7919, off + 6 * (i - 1), [(HW, HW)] * 3, POLICY)
    assert int(m.diffaug.offset.item()) == off + 18
    assert len({r for step in got for r in step}) == 9
    e = build(kind, tmp_path, AUG[kind])
    seq = []
    for i in range(off // 6 + 3):
        e.set_input(data(i))
        e.optimize_parameters()
        seq.append(records(e)[:3])
    assert seq[-3:] == got


def test_pool_keeps_plain_images(tmp_path):
    m = build("cgan", tmp_path, AUG["cgan"])
    m.set_input(data(0))
    m.optimize_parameters()
    torch.cuda.synchronize()
    assert m.fake_pool.num_imgs == 1
    kept = m.fake_pool._slots[0]
    want = torch.cat((m.real_A, m.fake_B), 1).detach()
    assert torch.equal(kept.reshape(want.shape), want)      # cat(real_A, fake_B) as the generator made it: no shift, no cutout, no colour


def test_runs_beside_ema(tmp_path):
    m = build("cgan", tmp_path, AUG["cgan"] + ["--ema_decay", "0.9"])
    for i in range(2):
        m.set_input(data(i))
        m.optimize_parameters()
    torch.cuda.synchronize()
    e = m.get_current_errors()
    assert all(np.isfinite(v) for v in e.values()), e
    assert int(m.diffaug.offset.item()) == 12 and m.ema.count == 2


def test_runs_beside_elastic(tmp_path):
    """--elastic deforms the crops an image-folder feeder hands out; --diffaug then augments what the discriminators see of them."""
    from PIL import Image
    from supervised_gan_amd.data import create_dataset
    os.makedirs(tmp_path / "imgs" / "train")
    rng = np.random.default_rng(0)
    for i in range(2):
        Image.fromarray(rng.integers(0, 256, (140, 140, 3), dtype=np.uint8)).save(str(tmp_path / "imgs" / "train" / ("t%d.png" % i)))
    m = build("cgan", tmp_path, AUG["cgan"] + ["--elastic", "3", "10", "--dataroot", str(tmp_path / "imgs"), "--loadSize", "140",
                                               "--resize_or_crop", "crop", "--nThreads", "0"])
    feeder = create_dataset(m.opt)
    for i in range(2):
        m.set_input(feeder[i])
        m.optimize_parameters()
    torch.cuda.synchronize()
    e = m.get_current_errors()
    assert m.opt.elastic == (3, 10.0) and all(np.isfinite(v) for v in e.values()), e
    assert int(m.diffaug.offset.item()) == 12

"""GPU tests of the Tversky / focal loss terms inside the segmentation trainer, at 64 x 64 on synthetic data with the drivers' small
generator: the step against a twin whose term is composed from torch ops on the same logits, weights of 0 against the plain trainer
bit for bit, and one replay of the graphed step against the eager step of a twin with the captured trainer's weights."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_seg_terms_host import plain_losses      # noqa: E402

pytestmark = pytest.mark.gpu

NET = ["--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "64", "--which_model_netG",
       "resnet_6blocks", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout", "--dataroot",
       "synthetic", "--manualSeed", "4", "--weights", "1", "2"]
NO_D = ("--which_model_netD", "None")
WITH_D = ("--which_model_netD", "n_layers", "--n_layers_D", "1", "--ndf", "8", "--scale_factor", "1", "--lambda_D", "0.5", "--no_lsgan")
TERMS = ("--dice_weight", "0.5", "--dice_classes", "0", "1", "--tversky", "0.3", "0.7", "--tversky_power", "0.75", "--focal_weight", "0.25",
         "--focal_gamma", "2")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")


def build(tmp_path, extra=()):
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    opt = TrainOptions().parse(NET + ["--name", "t", "--checkpoints_dir", str(tmp_path)] + list(extra), save=False, verbose=False)
    torch.manual_seed(4)
    return opt, create_model(opt)


def one_pass(m, data):
    """set_input, forward and backward_G from clean gradients, no optimizer step: the weights stay as they are."""
    m.set_input(data)
    m.forward()
    m.logit.retain_grad()
    m.optimizer_G.zero_grad()
    m.backward_G()


def first_layer_grad(m):
    name, p = next((k, p) for k, p in m.netG.named_parameters() if k.endswith(".weight"))
    return name, p.grad.detach().clone()


def rel(a, b):
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-12)


def compose_from_torch_ops(m):
    """Replace the trainer's node by the plain formulas in torch fp32 ops on the same logits (autograd takes them back)."""
    lam_d, classes, a, b, s, E, lam_f, gamma = m.segterms

    def with_terms(loss):
        C = m.logit.shape[1]
        z = m.logit[0].permute(1, 2, 0).reshape(-1, C)
        if m.use_sigmoid_ss:
            mode, lt = 1, m.real_B[0].permute(1, 2, 0).reshape(-1, C)
        else:
            mode, lt = 0, m.label.reshape(-1)
        m.loss_G_Dice, m.loss_G_Focal = plain_losses(z, lt, mode, list(classes), a, b, s, E, gamma, m.class_weights)
        return loss + lam_d * m.loss_G_Dice + lam_f * m.loss_G_Focal
    m._with_seg_terms = with_terms


@pytest.mark.parametrize("case", ["softmax_no_D", "sigmoid_with_D"])
def test_step_equals_the_torch_composition(tmp_path, case):
    """The same seed builds two trainers with the same weights; one runs the HIP node, the other the torch composition.  Losses and
    the generator's first-layer weight gradient agree by the project's rule max|a - b| / (max|b| + 1e-12) <= 1e-3 (the floor of
    max(1e-3, 4 e_ref): the comparison is with an fp32 composition itself)."""
    _need_gpu()
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    extra = TERMS + (NO_D if case == "softmax_no_D" else WITH_D + ("--use_sigmoid_ss",))
    opt, m = build(tmp_path, extra)
    assert m.no_netD == (case == "softmax_no_D") and m.use_sigmoid_ss == (case != "softmax_no_D")
    assert m.segterms == (0.5, (0, 1), 0.3, 0.7, 1.0, 0.75, 0.25, 2.0)
    data = SyntheticDataset(opt, 1).ring[0]
    one_pass(m, data)
    _, twin = build(tmp_path, extra)
    compose_from_torch_ops(twin)
    one_pass(twin, data)
    torch.cuda.synchronize()
    assert torch.equal(m.logit.detach(), twin.logit.detach())      # the same weights and input: the same logits
    rest = m.loss_G_CE.detach() if m.no_netD else m.loss_G_GAN.detach() + m.loss_G_CE.detach()
    assert torch.equal(m.loss_G.detach(), rest + 0.5 * m.loss_G_Dice.detach() + 0.25 * m.loss_G_Focal.detach())
    for name in ("loss_G_Dice", "loss_G_Focal", "loss_G"):
        a, b = getattr(m, name).detach(), getattr(twin, name).detach()
        print(f"{case} {name}: HIP {float(a)!r}, torch composition {float(b)!r}, rel {rel(a, b):.3e}")
        assert rel(a, b) <= 1e-3 and float(a) > 0.0, name
    e = rel(m.logit.grad, twin.logit.grad)
    k, g = first_layer_grad(m)
    k2, g2 = first_layer_grad(twin)
    e1 = rel(g, g2)
    print(f"{case}: d loss / d logits rel {e:.3e}; {k} gradient rel {e1:.3e} (max {float(g2.abs().max()):.3e})")
    assert k == k2 and float(g2.abs().max()) > 0.0 and e <= 1e-3 and e1 <= 1e-3
    if m.no_netD:
        assert list(m.get_current_errors()) == ["G_CE", "G_Dice", "G_Focal"]


def test_weights_zero_give_the_parents_losses_bit_for_bit(tmp_path):
    _need_gpu()
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    out = {}
    for name, extra in (("plain", ()), ("zero", ("--dice_weight", "0", "--focal_weight", "0", "--dice_classes", "5")),
                        ("dice", ("--dice_weight", "0.5")), ("focal", ("--focal_weight", "0.5"))):
        opt, m = build(tmp_path, NO_D + extra)
        one_pass(m, SyntheticDataset(opt, 1).ring[0])
        torch.cuda.synchronize()
        out[name] = m
    plain, zero = out["plain"], out["zero"]
    assert plain.segterms is None and zero.segterms is None and not hasattr(zero, "_st_bufs")
    assert torch.equal(plain.loss_G.detach(), zero.loss_G.detach()) and torch.equal(plain.logit.grad, zero.logit.grad)
    assert list(zero.get_current_errors()) == ["G_CE"] and zero.get_current_errors() == plain.get_current_errors()
    # one term on: the other is switched off in the call, is not logged and takes no gradient
    assert list(out["dice"].get_current_errors()) == ["G_CE", "G_Dice"] and list(out["focal"].get_current_errors()) == ["G_CE", "G_Focal"]
    assert float(out["dice"].loss_G_Focal) == 0.0 and float(out["focal"].loss_G_Dice) == 0.0
    for name in ("dice", "focal"):
        m = out[name]
        assert torch.equal(m.loss_G_CE.detach(), plain.loss_G_CE.detach())      # the head beside the node is untouched
        assert not torch.equal(m.logit.grad, plain.logit.grad) and bool(torch.isfinite(m.logit.grad).all())


def test_graphed_replay_equals_the_eager_step(tmp_path):
    """The captured step (warm-up, capture, one replay) against the eager pass of a twin that loaded the captured trainer's weights
    from a checkpoint written right after the capture, on the same image: loss_G, G_CE, G_Dice and G_Focal and the node's gradient
    buffer bit for bit -- the node's launches are streaming passes and ordered sums."""
    _need_gpu()
    from supervised_gan_amd.graph_step import GraphedStep
    from supervised_gan_amd.optim import FusedAdam
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    extra = NO_D + TERMS
    opt, m = build(tmp_path, extra)
    m.optimizer_G = FusedAdam(m.netG.parameters(), lr=opt.lr, betas=(opt.beta1, 0.999), zero_grads_in_step=False)
    data = SyntheticDataset(opt, 1).ring[0]
    g = GraphedStep(m)
    g.capture(data)      # raises if the node cannot be captured
    m.save("latest")
    _, twin = build(tmp_path, extra + ("--continue_train",))
    one_pass(twin, data)
    torch.cuda.synchronize()
    want = [t.detach().clone() for t in (twin.loss_G, twin.loss_G_CE, twin.loss_G_Dice, twin.loss_G_Focal, twin._st_bufs.dz)]
    g.step(data)
    torch.cuda.synchronize()
    got = [m.loss_G.detach(), m.loss_G_CE.detach(), m.loss_G_Dice.detach(), m.loss_G_Focal.detach(), m._st_bufs.dz]
    print(f"eager {[float(v) for v in want[:4]]}, graphed {[float(v) for v in got[:4]]}, max |dz| {float(got[4].abs().max()):.3e}")
    assert list(m.get_current_errors()) == ["G_CE", "G_Dice", "G_Focal"]
    assert 0.0 < float(got[2]) < 1.0 and float(got[3]) > 0.0 and float(got[4].abs().max()) > 0.0
    for a, b, what in zip(want, got, ("loss_G", "G_CE", "G_Dice", "G_Focal", "dz")):
        assert torch.equal(a, b), what

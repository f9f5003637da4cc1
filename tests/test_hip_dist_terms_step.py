"""GPU tests of the boundary / Hausdorff loss terms inside the segmentation trainer, at 64 x 64 on synthetic data with the drivers'
small generator: the step's loss against the plain trainer's plus the weighted terms and the terms against the fp64 yardstick fed
the step's own logits and label; weights of 0 against the plain trainer bit for bit; one replay of the graphed step against the
eager step of a twin with the captured trainer's weights, and a second replay on another image.

Pass rule, the project's: max|a - b| / (max|b| + 1e-12) <= max(1e-3, 4 e_ref), e_ref the same statistic of the fp32 torch composition
on the CPU."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_dist_terms_ref_host import rel, torch_dist_terms      # noqa: E402

pytestmark = pytest.mark.gpu

NET = ["--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "64", "--which_model_netG",
       "resnet_6blocks", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout", "--dataroot",
       "synthetic", "--manualSeed", "4", "--weights", "1", "2"]
NO_D = ("--which_model_netD", "None")
WITH_D = ("--which_model_netD", "n_layers", "--n_layers_D", "1", "--ndf", "8", "--scale_factor", "1", "--lambda_D", "0.5", "--no_lsgan")
LAM_B, LAM_H, ALPHA, CLS = 0.05, 0.01, 1.0, 1
TERMS = ("--boundary_loss_weight", str(LAM_B), "--hausdorff_weight", str(LAM_H), "--hausdorff_alpha", str(ALPHA), "--dist_class", str(CLS))


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
    """set_input, forward, backward_D where there are discriminators (get_current_errors logs its losses) and backward_G from clean
    gradients, no optimizer step: the weights stay as they are."""
    m.set_input(data)
    m.forward()
    if m.has_netD:
        m.optimizer_D.zero_grad()
        m.backward_D()
    m.logit.retain_grad()
    m.optimizer_G.zero_grad()
    m.backward_G()


def first_layer_grad(m):
    name, p = next((k, p) for k, p in m.netG.named_parameters() if k.endswith(".weight"))
    return name, p.grad.detach().clone()


def trel(a, b):
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-12)


def yardstick(m):
    """The terms of the trainer's current logits and label from the host yardsticks: the maps from util.signed_edt_sq of the label's
    class plane and of the trainer's own prediction plane thresholded at > 0.5 (the same fp32 values the device thresholds).  Returns
    (L_B, L_H, lambda_B dz_B + lambda_H dz_H [H, W, C], t_sdsq, p_sdsq, and the same three numbers from the fp32 torch composition)."""
    from supervised_gan_amd.util import dist_terms_ref, signed_edt_sq
    C, H, W = m.logit.shape[1:]
    z = m.logit.detach()[0].permute(1, 2, 0).reshape(-1, C).cpu().numpy()
    label = m.label[0].cpu().numpy()
    t_s = signed_edt_sq(label == CLS)
    p_s = signed_edt_sq(m.fake_B.detach()[0, CLS].cpu().numpy())
    if m.use_sigmoid_ss:
        mode, lt = 1, m.real_B.detach()[0].permute(1, 2, 0).reshape(-1, C).cpu().numpy()
    else:
        mode, lt = 0, label.reshape(-1)
    LB, LH, _, dB, dH = dist_terms_ref(z, lt, mode, CLS, t_s, p_s, True, ALPHA)
    t32 = torch_dist_terms(z, lt, mode, CLS, t_s, p_s, ALPHA, dtype=torch.float32)
    return (LB, LH, (LAM_B * dB + LAM_H * dH).reshape(H, W, C), t_s, p_s, (t32[0], t32[1], (LAM_B * t32[2] + LAM_H * t32[3]).reshape(H, W, C)))


def judge(name, got, ref64, ref32):
    e, e_ref = rel(got, ref64), rel(ref32, ref64)
    print(f"{name}: step vs fp64 yardstick {e:.3e}, fp32 composition vs fp64 {e_ref:.3e}")
    assert e <= max(1e-3, 4 * e_ref), (name, e, e_ref)


def check_against_yardstick(m, tag):
    LB, LH, dz, t_s, p_s, f32 = yardstick(m)
    errs = m.get_current_errors()
    C = m.logit.shape[1]
    assert np.array_equal(m._dl_tsdsq.cpu().numpy(), t_s), tag + ": t_sdsq"
    assert np.array_equal(m._dl_psdsq.cpu().numpy(), p_s), tag + ": p_sdsq"
    assert t_s.any() and p_s.any(), tag
    judge(tag + " G_Boundary", [errs["G_Boundary"]], [LB], [f32[0]])
    judge(tag + " G_Hausdorff", [errs["G_Hausdorff"]], [LH], [f32[1]])
    got = m._dl_bufs.dz.cpu().numpy().astype(np.float64)
    assert not got[:, :, C:].any(), tag
    judge(tag + " node dz", got[:, :, :C], dz, f32[2])
    assert float(np.abs(dz).max()) > 0.0 and errs["G_Hausdorff"] > 0.0, tag


@pytest.mark.parametrize("case", ["softmax_no_D", "sigmoid_no_D", "softmax_with_D", "sigmoid_with_D"])
def test_step_adds_the_weighted_terms(tmp_path, case):
    """The same seed builds two trainers with the same weights, one with the options and one without: the same logits, and loss_G
    with the options is loss_G without them plus lambda_B L_B + lambda_H L_H, the terms read from get_current_errors."""
    _need_gpu()
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    extra = (NO_D if case.endswith("no_D") else WITH_D) + (("--use_sigmoid_ss",) if case.startswith("sigmoid") else ())
    opt, m = build(tmp_path, extra + TERMS)
    assert m.no_netD == case.endswith("no_D") and m.use_sigmoid_ss == case.startswith("sigmoid")
    assert m.distterms == (LAM_B, LAM_H, ALPHA, CLS)
    data = SyntheticDataset(opt, 1).ring[0]
    one_pass(m, data)
    _, plain = build(tmp_path, extra)
    one_pass(plain, data)
    torch.cuda.synchronize()
    assert plain.distterms is None and torch.equal(m.logit.detach(), plain.logit.detach())      # the same weights and input: the same logits
    errs = m.get_current_errors()
    assert list(errs)[-2:] == ["G_Boundary", "G_Hausdorff"] and list(errs)[:-2] == list(plain.get_current_errors())
    want = float(plain.loss_G.detach()) + LAM_B * errs["G_Boundary"] + LAM_H * errs["G_Hausdorff"]
    got = float(m.loss_G.detach())
    print(f"{case}: loss_G {got!r}, without the options {float(plain.loss_G.detach())!r} + terms = {want!r}; G_Boundary {errs['G_Boundary']!r}, "
          f"G_Hausdorff {errs['G_Hausdorff']!r}")
    assert abs(got - want) / (abs(want) + 1e-12) <= 1e-3
    check_against_yardstick(m, case)
    # the gradient of the logits is the plain trainer's plus the node's
    e = trel(m.logit.grad, plain.logit.grad + m._dl_bufs.dz.permute(2, 0, 1)[:m.logit.shape[1]].unsqueeze(0))
    k, g = first_layer_grad(m)
    k2, g2 = first_layer_grad(plain)
    print(f"{case}: d loss / d logits vs plain + node rel {e:.3e}; {k} gradient moved by rel {trel(g, g2):.3e}")
    assert e <= 1e-3 and k == k2 and bool(torch.isfinite(g).all()) and not torch.equal(g, g2)


def test_weights_zero_give_the_parents_step_bit_for_bit(tmp_path):
    _need_gpu()
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    out = {}
    for name, extra in (("plain", ()), ("zero", ("--boundary_loss_weight", "0", "--hausdorff_weight", "0", "--dist_class", "5", "--hausdorff_alpha", "9")),
                        ("boundary", ("--boundary_loss_weight", "0.05")), ("hausdorff", ("--hausdorff_weight", "0.01"))):
        opt, m = build(tmp_path, NO_D + extra)
        one_pass(m, SyntheticDataset(opt, 1).ring[0])
        torch.cuda.synchronize()
        out[name] = m
    plain, zero = out["plain"], out["zero"]
    assert plain.distterms is None and zero.distterms is None and not [k for k in vars(zero) if k.startswith("_dl_")]
    assert torch.equal(plain.loss_G.detach(), zero.loss_G.detach()) and torch.equal(plain.logit.grad, zero.logit.grad)
    # behind d loss / d logits both trainers run the same launches; the weight-gradient kernels add with floating-point atomics, so
    # two runs of one trainer differ in the last bits there: the project's rule for them, bits for everything the term could touch
    ga, gb = first_layer_grad(plain), first_layer_grad(zero)
    assert ga[0] == gb[0] and trel(gb[1], ga[1]) <= 1e-3
    assert list(zero.get_current_errors()) == ["G_CE"] and zero.get_current_errors() == plain.get_current_errors()
    # one term on: the other is switched off in the call, is not logged and takes no gradient
    assert list(out["boundary"].get_current_errors()) == ["G_CE", "G_Boundary"]
    assert list(out["hausdorff"].get_current_errors()) == ["G_CE", "G_Hausdorff"]
    assert float(out["boundary"].loss_G_Hausdorff) == 0.0 and float(out["hausdorff"].loss_G_Boundary) == 0.0
    assert out["boundary"]._dl_psdsq is None      # the prediction's map belongs to the Hausdorff term
    for name in ("boundary", "hausdorff"):
        m = out[name]
        assert torch.equal(m.loss_G_CE.detach(), plain.loss_G_CE.detach())      # the head beside the node is untouched
        assert not torch.equal(m.logit.grad, plain.logit.grad) and bool(torch.isfinite(m.logit.grad).all())


def test_graphed_replay_equals_the_eager_step(tmp_path):
    """The captured step (warm-up, capture, one replay) against the eager pass of a twin that loaded the captured trainer's weights
    from a checkpoint written right after the capture, on the same image: loss_G, G_CE, G_Boundary, G_Hausdorff, both maps and the
    node's gradient buffer bit for bit -- integers, streaming passes and ordered sums -- and the generator's first-layer weight
    gradient by the project's rule.  A second replay on another image recomputes both maps: against the yardstick on the new label."""
    _need_gpu()
    from supervised_gan_amd.graph_step import GraphedStep
    from supervised_gan_amd.optim import FusedAdam
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    extra = NO_D + TERMS
    opt, m = build(tmp_path, extra)
    m.optimizer_G = FusedAdam(m.netG.parameters(), lr=opt.lr, betas=(opt.beta1, 0.999), zero_grads_in_step=False)
    ring = SyntheticDataset(opt, 2).ring
    data, other = ring[0], ring[1]
    g = GraphedStep(m)
    g.capture(data)      # raises if the node cannot be captured
    m.save("latest")
    _, twin = build(tmp_path, extra + ("--continue_train",))
    one_pass(twin, data)
    torch.cuda.synchronize()
    want = [t.detach().clone() for t in (twin.loss_G, twin.loss_G_CE, twin.loss_G_Boundary, twin.loss_G_Hausdorff, twin._dl_tsdsq, twin._dl_psdsq,
                                         twin._dl_bufs.dz)]
    k2, g2 = first_layer_grad(twin)
    g.step(data)
    torch.cuda.synchronize()
    got = [m.loss_G.detach(), m.loss_G_CE.detach(), m.loss_G_Boundary.detach(), m.loss_G_Hausdorff.detach(), m._dl_tsdsq, m._dl_psdsq, m._dl_bufs.dz]
    print(f"eager {[float(v) for v in want[:4]]}, graphed {[float(v) for v in got[:4]]}, max |dz| {float(got[6].abs().max()):.3e}")
    assert list(m.get_current_errors()) == ["G_CE", "G_Boundary", "G_Hausdorff"]
    assert float(got[3]) > 0.0 and float(got[6].abs().max()) > 0.0
    for a, b, what in zip(want, got, ("loss_G", "G_CE", "G_Boundary", "G_Hausdorff", "t_sdsq", "p_sdsq", "dz")):
        assert torch.equal(a, b), what
    k, g1 = first_layer_grad(m)
    e = trel(g1, g2)
    print(f"{k}: graphed vs eager gradient rel {e:.3e} (max {float(g2.abs().max()):.3e})")
    assert k == k2 and float(g2.abs().max()) > 0.0 and e <= 1e-3
    check_against_yardstick(m, "graphed replay")
    # another image: set_input refreshes the truth's map, the replay the prediction's
    before = [m._dl_tsdsq.clone(), m._dl_psdsq.clone()]
    g.step(other)
    torch.cuda.synchronize()
    assert not torch.equal(before[0], m._dl_tsdsq) and not torch.equal(before[1], m._dl_psdsq)
    check_against_yardstick(m, "second replay, another image")

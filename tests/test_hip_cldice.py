"""GPU tests of the soft-clDice term (sgan_cldice.hip) against the fp64 yardstick util.soft_cldice_ref fed the same fp32 inputs, and
of the term inside the segmentation trainer.

The error bounds are counted, not observed (u = 2^-24, widened by 2^-10 for the second-order terms):
  S_K     delta_0 is one rounding; an iteration adds four (delta_j, 1 - S, their product, the sum): k_S = 1 + 4 K.  Every rounded
          value is at most S_K (delta_j <= S_j <= S_K, both factors of the product are in [0, 1]) and d S_j / d S_{j-1} = 1 - delta_j,
          d S_j / d delta_j = 1 - S_{j-1} are at most 1, so |S - S_ref| <= k_S u S_ref at every pixel.
  sums    sums of non-negative terms carrying that relative error, added in fp64 (n 2^-52): |X - X_ref| <= (k_S u + n 2^-52) X_ref.
  L       Tprec and Tsens are ratios of two such sums, +1 each: 2 k_S u relative; their harmonic mean H = 1 - L <= 1 carries the
          larger of the two, and L is rounded to fp32 once: |L - L_ref| <= (2 k_S + 1) u.
  dL/dP   bounded per pixel by k u M(x), M the yardstick's backward with every contribution in absolute value.  On the longest path:
          the seed gA T + gB: (s / (p + s))^2 carries 8 k_S u, / (B + 1) one k_S more, gB's (A + 1) / (B + 1)^2 three: 11 k_S, the
          conversion to fp32 and the sum: k_seed = 11 k_S + 2;
          the pointwise chain: g (1 - delta_j) per level, the factor carrying (1 + amp) u for its two roundings and the product one:
          K (2 + amp); then g (1 - S_{j-1}), the factor carrying (k_S amp + 1) u, and the product: k_S amp + 2.  amp is the largest
          v / (1 - v) over the yardstick's delta_j and S_j below 1: an absolute error of 1 - v relative to 1 - v (a factor that is
          exactly 0 is exactly 0 on the device too: some delta_i is then 1.0 - 0.0);
          the gathers: a level adds at most 15 terms, 14 roundings, over K + 2 levels;
          the direct term gC S(T) (fewer roundings than the seed), its product and its sum, and the upstream factor: 3.
          k = k_seed + K (2 + amp) + k_S amp + 2 + 14 (K + 2) + 3.
Every I_j must hold the yardstick's bits: min rounds nothing."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

SHAPES = ((5, 7), (1, 40), (33, 47), (64, 64), (96, 80))
ITERS = (1, 5, 16)
KINDS = ("random", "plateaus", "binary")
U = 2.0 ** -24 * (1.0 + 2.0 ** -10)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")


def planes(H, W, kind, seed):
    rng = np.random.default_rng(seed)
    P = (0.25 + 0.5 * rng.random((H, W))).astype(np.float32)
    if kind == "plateaus":      # a saturated softmax: stretches of exact 0.0 and 1.0 between the soft values
        sat = rng.random((H, W))
        P[sat < 0.3] = 0.0
        P[sat > 0.7] = 1.0
    elif kind == "binary":
        P = (rng.random((H, W)) < 0.5).astype(np.float32)
    T = (rng.random((H, W)) < 0.4).astype(np.float32)
    return P, T


def bounds(P, T, K):
    """The yardstick's results and the counted bounds of the module docstring."""
    from supervised_gan_amd import util
    L, dP, SP, ST, I, M = util.soft_cldice_ref(P, T, K)
    _, _, delta, S, _, _ = util.soft_skeleton_ref(P, K)
    sums = util.soft_cldice_sums(SP, T.astype(np.float64), ST, P.astype(np.float64))
    v = np.concatenate([np.ravel(a) for a in delta + S])
    v = v[v < 1.0]
    amp = float((v / (1.0 - v)).max()) if v.size else 0.0
    k_S = 1 + 4 * K
    k = (11 * k_S + 2) + K * (2 + amp) + k_S * amp + 2 + 14 * (K + 2) + 3
    return dict(L=L, dP=dP, SP=SP, ST=ST, I=I, M=M, sums=sums[:4], k_S=k_S, k=k, amp=amp)


def run_device(P, T, K, layout="dense"):
    """The term on the device: (I planes, S(P), S(T), state, loss, dP).  layout "window": P lies as a window inside a wider buffer (a
    row stride, pixel stride 1); "nhwc": P and T are each channel 1 of a 3-channel pixel-interleaved buffer, windows of a wider one
    (pixel stride 3, the kind of plane the trainer passes), so the strided T arguments of the finish and the backward are used too."""
    from supervised_gan_amd import ops
    dev = torch.device("cuda", 0)
    H, W = P.shape

    def place(X):
        if layout == "dense":
            return torch.from_numpy(X).to(dev)
        if layout == "window":
            big = torch.full((H + 3, W + 5), float("nan"), dtype=torch.float32, device=dev)
            x = big[2:2 + H, 3:3 + W]
        else:
            big = torch.full((H + 3, W + 5, 3), float("nan"), dtype=torch.float32, device=dev)
            x = big[2:2 + H, 3:3 + W, 1]
            assert x.stride() == (3 * (W + 5), 3)
        x.copy_(torch.from_numpy(X))
        return x
    p = place(P)
    t = place(T) if layout == "nhwc" else torch.from_numpy(T).to(dev)
    work = ops.new_cldice_workspace(H, W, K, dev, backward=True)
    work.fill_(float("nan"))      # the workspace may hold anything
    sp = ops.soft_skeleton(p, K, work=work)
    st = ops.soft_skeleton(t, K)
    state = ops.new_cldice_state(dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    ops.cldice_finish(sp, t, st, p, state, loss)
    dp = ops.cldice_backward(t, st, state, K, work)
    torch.cuda.synchronize()
    I = work[:(K + 2) * H * W].reshape(K + 2, H, W).cpu().numpy()
    return I, sp.cpu().numpy(), st.cpu().numpy(), state[:8].cpu().numpy(), float(loss), dp.cpu().numpy()


@pytest.mark.parametrize("H,W", SHAPES)
def test_term_against_the_yardstick(H, W):
    _need_gpu()
    for K in ITERS:
        for kind in KINDS:
            P, T = planes(H, W, kind, 1000 * H + 10 * K + KINDS.index(kind))
            want = bounds(P, T, K)
            I, sp, st, state, loss, dp = run_device(P, T, K)
            what = f"{H} x {W}, K = {K}, {kind}"
            for j in range(K + 2):
                assert np.array_equal(I[j].view(np.uint32), want["I"][j].view(np.uint32)), (what, j)
            k_S, k, n = want["k_S"], want["k"], H * W
            e_s = np.abs(sp.astype(np.float64) - want["SP"])
            assert np.array_equal(st.astype(np.float64), want["ST"]), what      # a binary plane: every value is exact
            e_sum = [abs(float(state[i]) - want["sums"][i]) for i in range(4)]
            b_sum = [(k_S * U + n * 2.0 ** -52) * want["sums"][i] for i in range(4)]
            e_l, b_l = max(abs(float(state[4]) - want["L"]), abs(loss - want["L"])), (2 * k_S + 1) * U
            e_g, b_g = np.abs(dp.astype(np.float64) - want["dP"]), k * U * want["M"]
            ratio = float((e_g / np.where(b_g > 0, b_g, 1.0)).max())
            print(f"{what}: S err {e_s.max():.2e} (bound {float((k_S * U * want['SP']).max()):.2e}), sums {max(e_sum):.2e} ({max(b_sum):.2e}), "
                  f"L {e_l:.2e} ({b_l:.2e}), dP {e_g.max():.2e} (k = {k:.0f}, amp = {want['amp']:.2f}, bound {b_g.max():.2e}, worst ratio {ratio:.3f})")
            assert (e_s <= k_S * U * want["SP"]).all(), what
            assert all(e <= b for e, b in zip(e_sum, b_sum)), (what, e_sum, b_sum)
            assert e_l <= b_l, (what, e_l, b_l)
            assert (e_g <= b_g).all(), (what, ratio)
            assert np.isfinite(dp).all() and np.abs(dp).max() > 0.0


def test_two_runs_give_the_same_bits_and_the_strides_are_honoured():
    """Dense twice, P as a window of a wider map, P and T as channels of a pixel-interleaved buffer: the same bits in every I_j,
    both skeletons, the state, the loss and the gradient, on a shape of several workgroups; the strided gradient is also held to
    the yardstick's bound."""
    _need_gpu()
    for (H, W), K, kind in (((33, 47), 5, "plateaus"), ((5, 7), 16, "random")):
        P, T = planes(H, W, kind, 5)
        a = run_device(P, T, K)
        assert np.abs(a[5]).max() > 0.0
        for layout in ("dense", "window", "nhwc"):
            b = run_device(P, T, K, layout)
            for x, y in zip(a, b):
                assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), (H, W, layout)
        want = bounds(P, T, K)
        assert (np.abs(b[5].astype(np.float64) - want["dP"]) <= want["k"] * U * want["M"]).all()


def test_refusals_launch_nothing():
    _need_gpu()
    from supervised_gan_amd import ops
    from supervised_gan_amd._lib import SganError
    from supervised_gan_amd.losses import soft_cldice
    dev = torch.device("cuda", 0)
    p = torch.rand(8, 8, device=dev)
    for K in (0, 17):
        with pytest.raises(SganError, match="not covered"):
            ops.soft_skeleton(p, K)
        with pytest.raises(SganError, match="not covered"):
            soft_cldice(p, p, K)
    small = torch.empty(8, dtype=torch.float32, device=dev)
    with pytest.raises(SganError, match="workspace"):
        ops.soft_skeleton(p, 3, work=small)
    with pytest.raises(SganError):
        ops.soft_skeleton(p.cpu(), 3)


def test_autograd_node_scales_by_the_upstream_gradient():
    _need_gpu()
    from supervised_gan_amd.losses import soft_cldice
    P, T = planes(33, 47, "random", 9)
    want = bounds(P, T, 5)
    dev = torch.device("cuda", 0)
    p = torch.from_numpy(P).to(dev).requires_grad_(True)
    t = torch.from_numpy(T).to(dev)
    loss = soft_cldice(p, t, 5)
    (0.5 * loss).backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - want["L"]) <= (2 * want["k_S"] + 1) * U
    e = np.abs(p.grad.cpu().numpy().astype(np.float64) - 0.5 * want["dP"])
    assert (e <= want["k"] * U * 0.5 * want["M"]).all()


# ---- through the model: 32 x 32, the drivers' small generator (resnet_6blocks, ngf 8; the U-Nets need 128 pixels) ------------------
NET = ["--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "32", "--which_model_netG",
       "resnet_6blocks", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout", "--dataroot",
       "synthetic", "--manualSeed", "4", "--which_model_netD", "None", "--weights", "1", "2"]


def build(tmp_path, extra=()):
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    opt = TrainOptions().parse(NET + ["--name", "t", "--checkpoints_dir", str(tmp_path)] + list(extra), save=False, verbose=False)
    torch.manual_seed(4)
    return opt, create_model(opt)


def grads(m):
    return {k: p.grad.detach().clone() for k, p in m.netG.named_parameters()}




def one_pass(m, data):
    """set_input, forward and backward_G from clean gradients, no optimizer step: the weights stay as they are."""
    m.set_input(data)
    m.forward()
    m.logit.retain_grad()
    m.optimizer_G.zero_grad()
    m.backward_G()


def device_launches(fn):
    """Counter of the names of everything the device ran for fn() -- kernels, copies and fills -- as torch.profiler's device
    activity records it (the instrument of tests/test_hip_factd_step.py)."""
    from collections import Counter
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = Counter()
    for e in prof.events():
        if str(getattr(e, "device_type", "")).endswith("CUDA"):
            own = re.search(r"\bsg_\w+", e.name)      # the library's kernels by their plain name, anything else as recorded
            names[own.group(0) if own else e.name] += 1
    return names


def same_within_the_rule(ga, gb):
    """The project's rule for two runs of the order-dependent weight-gradient kernels (tests/test_hip_segm_nod.py): 1e-4 of the
    tensor's maximum; a bias in front of an InstanceNorm has an analytically zero gradient, its residue is taken over the layer's
    weight gradient."""
    for k, g in ga.items():
        scale = ga.get(k.replace(".bias", ".weight"), g)
        assert float((g - gb[k]).abs().max()) <= 1e-4 * float(scale.abs().max()) + 1e-12, k


def term_gradient_at_the_logits(m, K, lam):
    """lam * d soft-clDice / d logits on a path of its own from a copy of the trainer's logits: (loss, gradient)."""
    from supervised_gan_amd.losses import class_probability_plane, soft_cldice
    z = m.logit.detach().clone().requires_grad_(True)
    p = class_probability_plane(z, 0, m.use_sigmoid_ss)
    loss = soft_cldice(p, (m.label[0] == 0).float(), K)
    (lam * loss).backward()
    return loss.detach(), z.grad


def test_loss_is_head_plus_weighted_term_and_weight_zero_changes_nothing(tmp_path):
    """forward + backward_G of three trainers from the same seed: without the option, with --cldice_weight 0, with 0.5 (K = 3).

    Launches.  Every trainer runs the pass once (lazy buffers) and once more under the profiler, which counts what the device ran,
    by name.  Weight 0 must run exactly what no option runs.  Weight 0.5 adds, by the launch plan of DESIGN.md R29:
      the term         2 K + 6 = 12 sg_cld_* kernels: K + 1 erosions and the skeleton, the finish, the delta planes and K + 2 gathers
                       (the truth's skeleton belongs to set_input, outside the counted pass);
      its own p        sg_softmax_fwd_kernel; on the way back the layout copy of the planar gradient autograd builds for the plane
                       (sgan_to_nhwc, its planar kernel) and sg_softmax_bwd_kernel; and one more layout copy (sgan_to_nhwc), because
                       the sum of two gradients at the logits is a tensor of autograd's, no buffer of the library's: 4;
      autograd         lam * L and the sum with the head's loss: 2; back: the gradient times lam, a zero fill and a copy for each
                       of the two selects of p[0, c], and the sum of the two gradients that arrive at the logits: 6.
    24 in all at K = 3.  ATen names its kernels by their template arguments, which follow the strides of what they are given, so
    only the library's kernels are compared name by name between the trainer with the term and the one without; the total counts
    everything.
    Bits.  Weight 0 against no option: the loss and d loss / d logits agree bit for bit.  The weight gradients behind them are NOT
    compared bit for bit: two runs of the trainer WITHOUT the option already differ there (measured on the card: 33 of 36 gradient
    tensors, the backward-weight kernels add in the order their workgroups arrive), so they are held to the project's rule for them.
    d loss_G / d logits with the term is the head's gradient plus 0.5 times the term's through the softmax backward, one fp32 sum."""
    _need_gpu()
    from supervised_gan_amd.losses import class_probability_plane
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    from collections import Counter
    K = 3
    out, launches = {}, {}
    for name, extra in (("plain", ()), ("zero", ("--cldice_weight", "0")), ("on", ("--cldice_weight", "0.5", "--cldice_iters", str(K)))):
        opt, m = build(tmp_path, extra)
        data = SyntheticDataset(opt, 1).ring[0]
        one_pass(m, data)
        m.set_input(data)

        def counted(m=m):
            m.forward()
            m.logit.retain_grad()
            m.optimizer_G.zero_grad()
            m.backward_G()
        launches[name] = device_launches(counted)
        torch.cuda.synchronize()
        out[name] = (m, m.loss_G.detach().clone(), grads(m), list(m.get_current_errors()), m.logit.grad.clone())
    total = {k: sum(v.values()) for k, v in launches.items()}
    added = launches["on"] - launches["plain"]
    print(f"launches {total}; added by the term: {dict(added)}")
    own = {k: Counter({n: c for n, c in v.items() if n.startswith("sg_")}) for k, v in launches.items()}
    assert total["plain"] > 20 and sum(own["plain"].values()) > 20, launches["plain"]
    assert launches["zero"] == launches["plain"]
    assert not (own["plain"] - own["on"]), "the term takes no launch of the library's away"
    assert dict(own["on"] - own["plain"]) == {
        "sg_cld_erode_kernel": K + 1, "sg_cld_skel_kernel": 1, "sg_cld_finish_kernel": 1, "sg_cld_bwd_delta_kernel": 1,
        "sg_cld_bwd_gather_kernel": K + 2, "sg_softmax_fwd_kernel": 1, "sg_softmax_bwd_kernel": 1, "sg_planes_to_nhwc4_kernel": 1,
        "sg_to_nhwc_kernel": 1}, dict(added)
    assert total["on"] == total["plain"] + (2 * K + 6) + 4 + 8, (total, dict(added))

    assert out["plain"][3] == out["zero"][3] == ["G_CE"] and out["on"][3] == ["G_CE", "G_clDice"]
    assert out["zero"][0].cldice is None and out["plain"][0].cldice is None
    assert torch.equal(out["plain"][1], out["zero"][1]) and torch.equal(out["plain"][4], out["zero"][4])
    same_within_the_rule(out["plain"][2], out["zero"][2])
    m = out["on"][0]
    head, term = m.loss_G_CE.detach(), m.loss_G_clDice.detach()
    assert torch.equal(m.loss_G.detach(), head + 0.5 * term) and 0.0 < float(term) < 1.0
    assert torch.equal(head, out["plain"][1])      # the head's loss is untouched by the term beside it
    # the term against the yardstick on the planes the trainer read
    P = class_probability_plane(m.logit.detach(), 0).cpu().numpy()      # the term's own softmax of the same logits
    T = (m.label[0] == 0).float().cpu().numpy()
    want = bounds(P, T, K)
    print(f"G_clDice {float(term)!r}, yardstick {want['L']!r}; head {float(head)!r}")
    assert abs(float(term) - want["L"]) <= (2 * want["k_S"] + 1) * U
    alone, dz = term_gradient_at_the_logits(m, K, 0.5)
    assert torch.equal(alone, term) and float(dz.abs().max()) > 0.0
    assert torch.equal(out["on"][4], out["plain"][4] + dz)


WITH_D = ("--which_model_netD", "n_layers", "--n_layers_D", "1", "--ndf", "8", "--scale_factor", "1", "--lambda_D", "0.5", "--no_lsgan")


@pytest.mark.parametrize("case", ["sigmoid", "with_D", "with_D_sigmoid"])
def test_the_other_heads(tmp_path, case):
    """The sigmoid head without discriminators (the term's own sigmoid of the logits) and the trainer with a discriminator (the term
    reads the plane of fake_B), softmax and sigmoid: loss_G is the rest of the loss plus 0.5 times the term, one fp32 product and
    sum; the term is the yardstick's on the plane the trainer holds; its gradient reaches the logits and the weights."""
    _need_gpu()
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    K = 2
    extra = ("--cldice_weight", "0.5", "--cldice_iters", str(K)) + (WITH_D if case.startswith("with_D") else ()) \
        + (("--use_sigmoid_ss",) if case.endswith("sigmoid") else ())
    opt, m = build(tmp_path, extra)
    assert m.use_sigmoid_ss == case.endswith("sigmoid") and m.no_netD == (case == "sigmoid")
    data = SyntheticDataset(opt, 1).ring[0]
    if not m.no_netD:      # one whole step first: the discriminator's stage, and its logged losses, exist only after it
        m.set_input(data)
        m.optimize_parameters()
    one_pass(m, data)
    torch.cuda.synchronize()
    rest = m.loss_G_CE.detach() if m.no_netD else m.loss_G_GAN.detach() + m.loss_G_CE.detach()
    term = m.loss_G_clDice.detach()
    assert torch.equal(m.loss_G.detach(), rest + 0.5 * term)
    assert list(m.get_current_errors())[-1] == "G_clDice"
    P = m.fake_B.detach()[0, 0].cpu().numpy()
    T = (m.label[0] == 0).float().cpu().numpy()
    want = bounds(P, T, K)
    print(f"{case}: G_clDice {float(term)!r}, yardstick {want['L']!r}")
    assert abs(float(term) - want["L"]) <= (2 * want["k_S"] + 1) * U
    alone, dz = term_gradient_at_the_logits(m, K, 0.5)
    assert torch.equal(alone, term) and float(dz.abs().max()) > 0.0
    if m.no_netD:      # the head's gradient is what the trainer holds without the option, from the same seed
        _, plain = build(tmp_path, ("--use_sigmoid_ss",))
        one_pass(plain, data)
        assert torch.equal(m.logit.grad, plain.logit.grad + dz)
    assert all(float(g.abs().max()) > 0.0 for k, g in grads(m).items() if k.endswith(".weight"))


def test_graphed_step_gives_the_bits_of_the_eager_step(tmp_path):
    """The captured step (two warm-up steps, then one replay) against the eager pass of a twin that loaded the captured trainer's
    weights from a checkpoint written right after the capture, on the same image, with --cldice_weight 0.5.  Both start from the same
    bits, so no optimizer update lies between what is compared.  The optimizer of the captured trainer is the same FusedAdam without
    zero_grads_in_step, so that the gradients of the replay are still there after its update.

    Bit for bit: loss_G, G_CE, G_clDice, and the term's gradient plane dp (the node's persistent buffer: what the captured backward
    handed to the softmax backward).  The term alone is also re-run eagerly on the very plane the replay read (I_0 of its workspace)
    and must give the replay's loss and dp: its launches are gathers and ordered sums, so this holds by construction.
    The generator's weight gradients are non-zero on both sides and agree within the project's rule for them; they cannot agree bit
    for bit, the backward-weight kernels add in the order their workgroups arrive (see the test above)."""
    _need_gpu()
    from supervised_gan_amd.graph_step import GraphedStep
    from supervised_gan_amd.losses import soft_cldice
    from supervised_gan_amd.optim import FusedAdam
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    K = 5
    extra = ("--cldice_weight", "0.5")
    opt, m = build(tmp_path, extra)
    m.optimizer_G = FusedAdam(m.netG.parameters(), lr=opt.lr, betas=(opt.beta1, 0.999), zero_grads_in_step=False)
    data = SyntheticDataset(opt, 1).ring[0]
    g = GraphedStep(m)
    g.capture(data)
    m.save("latest")
    _, twin = build(tmp_path, extra + ("--continue_train",))
    one_pass(twin, data)
    torch.cuda.synchronize()
    want = (twin.loss_G.detach().clone(), twin.loss_G_CE.detach().clone(), twin.loss_G_clDice.detach().clone(), twin._cld_bufs.dp.clone())
    want_grads = grads(twin)
    g.step(data)
    torch.cuda.synchronize()
    got = (m.loss_G.detach(), m.loss_G_CE.detach(), m.loss_G_clDice.detach(), m._cld_bufs.dp)
    print(f"eager {[float(v) for v in want[:3]]}, graphed {[float(v) for v in got[:3]]}, max |dp| {float(got[3].abs().max()):.3e}")
    assert list(m.get_current_errors()) == ["G_CE", "G_clDice"]
    assert float(got[3].abs().max()) > 0.0 and 0.0 < float(got[2]) < 1.0
    for a, b, what in zip(want, got, ("loss_G", "G_CE", "G_clDice", "dp")):
        assert torch.equal(a, b), what
    # the term alone, eagerly, on the plane the replay read
    H, W = m._cld_truth.shape
    p = m._cld_bufs.work[:H * W].reshape(H, W).clone().requires_grad_(True)
    alone = soft_cldice(p, m._cld_truth, K, t_skel=m._cld_tskel)
    (0.5 * alone).backward()
    assert torch.equal(alone.detach(), got[2]) and torch.equal(p.grad, got[3])
    got_grads = grads(m)
    assert all(float(got_grads[k].abs().max()) > 0.0 and float(v.abs().max()) > 0.0 for k, v in want_grads.items() if k.endswith(".weight"))
    same_within_the_rule(want_grads, got_grads)

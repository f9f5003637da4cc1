"""GPU tests of the Lovasz-softmax term (sgan_lovasz.hip) against the fp64 yardstick util.lovasz_ref fed the same fp32 inputs, and of
the term inside the segmentation trainer.

pi must be the yardstick's, bit for bit: the keys are unique integers.  The other bounds are counted, not observed (u = 2^-24, the
relative error of one rounding to fp32; eps = 2^-53, of one rounding to fp64):
  g       the device keeps g in fp64, so no rounding from fp64 to fp32 enters: device and yardstick each make ONE fp64 division of
          the same exact integers (I, U (U - 1) < 2^41): |g - g_ref| <= 2 eps g_ref.
  L_c     N products e g (eps each, on top of g's) added in fp64 in some fixed order (at most N - 1 roundings on any partial sum of
          non-negative terms), on either side: |L_c - L_c_ref| <= 2 (N + 2) eps L_c_ref.
  L       the sum of at most 8 L_c and the division by m: 9 eps more on either side, then ONE rounding to fp32:
          |L - L_ref| <= (u + (2 N + 22) eps) L_ref, and L_ref <= 1.
  dL/dp   per element gout * s * g_k * (1 / m): g (2 eps between the sides), the scale 1 / m (eps) and three products (eps each) in
          fp64 on either side, then ONE rounding to fp32: |dp - dp_ref| <= (u + 10 eps) M with M = |dp_ref| per pixel.  No fp32
          value is subnormal here (g >= 2^-41 or 0).  Where the yardstick's gradient is 0 (s = 0, g = 0, an absent or unlisted
          class) the bound is 0: the device's must be exactly 0."""
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

# one chunk of the LDS sort is 4096 keys: (64, 64) is exactly one, (64, 65) one past it (two chunks, the first global merge),
# (96, 100) pads 9600 to 16384 (two stages of global merges), (130, 257) pads 33410 to 65536: four stages, ten global merge launches
SHAPES = ((1, 1), (1, 2), (5, 7), (33, 47), (64, 64), (64, 65), (96, 100), (130, 257))
KINDS = ("random", "plateaus", "binary", "quantised", "all_wrong", "absent", "full")
LISTS = ((0,), (2, 0), (1, 0, 2))
C = 3
U = 2.0 ** -24
EPS = 2.0 ** -53


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")


def inputs(H, W, kind, seed):
    """(P [3, H, W] fp32 in [0, 1], label [H, W] int64)."""
    rng = np.random.default_rng(seed)
    P = rng.random((C, H, W)).astype(np.float32)
    label = rng.integers(0, C, (H, W))
    if kind == "plateaus":      # a saturated softmax: stretches of exact 0.0 and 1.0 between the soft values
        sat = rng.random((C, H, W))
        P[sat < 0.3] = 0.0
        P[sat > 0.7] = 1.0
    elif kind == "binary":
        P = (P < 0.5).astype(np.float32)
    elif kind == "quantised":      # multiples of 1 / 8: massive ties between foreground and background pixels
        P = (np.round(P * 8) / 8).astype(np.float32)
    elif kind == "all_wrong":
        P = np.stack([1.0 - (label == c) for c in range(C)]).astype(np.float32)
    elif kind == "absent":      # class 0, listed in every list, does not occur
        label = rng.integers(1, C, (H, W))
    elif kind == "full":      # class 0 covers every pixel; the others are absent
        label = np.zeros((H, W), np.int64)
    return P, label.astype(np.int64)


def run_device(P, label, classes, layout="dense", gout=None):
    """The term on the device from a NaN-filled workspace into a NaN-filled gradient: (pi, g, the 18 doubles of the state, G of the
    listed classes, loss, dp) as numpy."""
    from supervised_gan_amd import ops
    dev = torch.device("cuda", 0)
    _, H, W = P.shape
    if layout == "dense":
        p = torch.from_numpy(P).to(dev)
    elif layout == "window":
        big = torch.full((C, H + 3, W + 5), float("nan"), dtype=torch.float32, device=dev)
        p = big[:, 2:2 + H, 3:3 + W]
        p.copy_(torch.from_numpy(P))
    else:      # the channels of a pixel-interleaved buffer, a window of a wider one: the kind of prediction the trainer passes
        big = torch.full((H + 3, W + 5, C + 1), float("nan"), dtype=torch.float32, device=dev)
        p = big[2:2 + H, 3:3 + W, :C].permute(2, 0, 1)
        assert p.stride() == (1, (C + 1) * (W + 5), C + 1)
        p.copy_(torch.from_numpy(P))
    lab = torch.from_numpy(label).to(dev)
    n = len(classes)
    work = ops.new_lovasz_workspace(H, W, n, dev)
    work.fill_(float("nan"))      # the workspace may hold anything
    dp = torch.full((1, C, H, W), float("nan"), dtype=torch.float32, device=dev)
    loss = ops.lovasz_forward(p, lab, classes, work)
    g = None if gout is None else torch.tensor(gout, dtype=torch.float32, device=dev)
    ops.lovasz_backward(p, classes, work, dp=dp, gout=g)
    torch.cuda.synchronize()
    perm, gw, state, G = ops.lovasz_views(work, H, W, n)
    return perm.cpu().numpy(), gw.cpu().numpy(), state[:18].cpu().numpy(), G[:n].cpu().numpy(), float(loss), dp[0].cpu().numpy()


def check(P, label, classes, got, what, gamma=1.0):
    """One device result against the yardstick, by the bounds of the module docstring; returns the yardstick's result."""
    from supervised_gan_amd.util import lovasz_ref
    want = lovasz_ref(P, label, classes)
    L, dP, perm, g, Lc, M = want
    pi, gw, state, G, loss, dp = got
    N, n = label.size, len(classes)
    assert pi.dtype == np.int32 and np.array_equal(pi, perm), what
    assert np.array_equal(G[:n], [(label == c).sum() for c in classes]), what
    e_g = np.abs(gw - g)
    assert (e_g <= 2 * EPS * g).all(), (what, float(e_g.max()))
    present = [(label == c).any() for c in classes]
    m = sum(present)
    assert state[1] == m and np.array_equal(state[10:10 + n], [1.0 / m if ok else 0.0 for ok in present]), what
    e_lc = np.abs(state[2:2 + n] - Lc)
    assert (e_lc <= 2 * (N + 2) * EPS * Lc).all(), (what, e_lc, Lc)
    e_l, b_l = abs(loss - L), (U + (2 * N + 22) * EPS) * L
    e_d, b_d = np.abs(dp.astype(np.float64) - gamma * dP), (U + 10 * EPS) * abs(gamma) * M
    print(f"{what}: m = {m}, L {loss!r} (error {e_l:.2e}, bound {b_l:.2e}), g error {float(e_g.max()):.2e}, "
          f"dp error {float(e_d.max()):.2e} (bound {float(b_d.max()):.2e})")
    assert e_l <= b_l and abs(float(state[0]) - L) <= b_l, (what, e_l, b_l)
    assert not np.isnan(dp).any(), what + ": the whole gradient is written"
    assert (e_d <= b_d).all(), what
    assert not dp[dP == 0.0].any(), what
    if m == 0:
        assert loss == 0.0 and not dp.any()
    return want


@pytest.mark.parametrize("H,W", SHAPES)
def test_term_against_the_yardstick(H, W):
    _need_gpu()
    for kind in KINDS:
        for classes in LISTS:
            P, label = inputs(H, W, kind, 1000 * H + 10 * W + KINDS.index(kind))
            want = check(P, label, classes, run_device(P, label, classes), f"{H} x {W}, {kind}, classes {classes}")
            if kind in ("random", "quantised") and H * W >= 35:      # every class occurs
                assert want[0] > 0.0 and np.abs(want[1]).max() > 0.0


@pytest.mark.parametrize("H,W", ((512, 512), (1024, 1024)))
def test_large_quantised(H, W):
    """512 x 512, the trainer's size, and 1024 x 1024, exactly the cap: the pixel index needs all 20 bits."""
    _need_gpu()
    P, label = inputs(H, W, "quantised", H)
    check(P, label, (0, 1), run_device(P, label, (0, 1)), f"{H} x {W}, quantised")


def test_two_runs_give_the_same_bits_and_the_strides_are_honoured():
    _need_gpu()
    for (H, W), kind, classes in (((130, 257), "quantised", (2, 0)), ((33, 47), "plateaus", (1, 0, 2)), ((64, 65), "random", (0,))):
        P, label = inputs(H, W, kind, 5)
        a = run_device(P, label, classes)
        assert np.abs(a[5]).max() > 0.0
        for layout in ("dense", "window", "nhwc"):
            b = run_device(P, label, classes, layout)
            for x, y in zip(a, b):
                assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), (H, W, layout)
        check(P, label, classes, b, f"{H} x {W}, nhwc")


def test_refusals_launch_nothing():
    _need_gpu()
    from supervised_gan_amd import ops
    from supervised_gan_amd._lib import SganError
    from supervised_gan_amd.losses import lovasz_softmax
    dev = torch.device("cuda", 0)
    p = torch.rand(1, C, 8, 8, device=dev)
    lab = torch.zeros(8, 8, dtype=torch.int64, device=dev)
    work = ops.new_lovasz_workspace(8, 8, 1, dev)
    for classes in ((), tuple(range(9))):
        with pytest.raises(SganError, match="not covered"):
            ops.lovasz_forward(p, lab, classes, work)
        with pytest.raises(SganError, match="not covered"):
            lovasz_softmax(p, lab, classes)
    with pytest.raises(SganError, match="not covered"):      # by shape arithmetic only: nothing of that size is allocated
        ops.new_lovasz_workspace(1024, 1025, 1, dev)
    with pytest.raises(SganError, match="not covered"):
        ops.lovasz_forward(torch.empty((1, 1, 1024, 1025), device=dev), lab, (0,), work)
    with pytest.raises(SganError, match="classes"):
        ops.lovasz_forward(p, lab, (0, 0), work)
    with pytest.raises(SganError, match="classes"):
        ops.lovasz_forward(p, lab, (C,), work)
    small = torch.empty(8, dtype=torch.float64, device=dev)
    with pytest.raises(SganError, match="workspace too small"):
        ops.lovasz_forward(p, lab, (0,), small)
    with pytest.raises(SganError, match="workspace too small"):
        ops.lovasz_backward(p, (0,), small)
    with pytest.raises(SganError):
        ops.lovasz_forward(p.cpu(), lab.cpu(), (0,), work)
    with pytest.raises(SganError):
        lovasz_softmax(p.cpu(), lab.cpu(), (0,))


def test_autograd_node_scales_by_the_upstream_gradient():
    _need_gpu()
    from supervised_gan_amd.losses import lovasz_softmax
    from supervised_gan_amd.util import lovasz_ref
    P, label = inputs(33, 47, "random", 9)
    L, dP, _, _, _, M = lovasz_ref(P, label, (0, 2))
    dev = torch.device("cuda", 0)
    p = torch.from_numpy(P).to(dev)[None].requires_grad_(True)
    loss = lovasz_softmax(p, torch.from_numpy(label).to(dev), (0, 2))
    (0.375 * loss).backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - L) <= (U + (2 * label.size + 22) * EPS) * L
    e = np.abs(p.grad[0].cpu().numpy().astype(np.float64) - 0.375 * dP)
    assert (e <= (U + 10 * EPS) * 0.375 * M).all() and not p.grad[0, 1].any() and float(p.grad.abs().max()) > 0.0
    # the unit upstream gradient takes the path without the scalar
    p2 = torch.from_numpy(P).to(dev)[None].requires_grad_(True)
    lovasz_softmax(p2, torch.from_numpy(label).to(dev), (0, 2)).backward()
    assert (np.abs(p2.grad[0].cpu().numpy().astype(np.float64) - dP) <= (U + 10 * EPS) * M).all()


def test_term_captures_into_a_graph():
    """Forward and backward on persistent buffers under torch.cuda.graph (one chain, no parallel branches); two replays on two
    different inputs copied into the captured buffers give the eager bits for each."""
    _need_gpu()
    from supervised_gan_amd import ops
    from supervised_gan_amd.losses import LovaszBuffers
    dev = torch.device("cuda", 0)
    H, W, classes = 64, 65, (2, 0)
    cases = [inputs(H, W, kind, 11) for kind in ("quantised", "absent")] + [inputs(H, W, "random", 12)]
    p = torch.from_numpy(cases[2][0]).to(dev)[None].clone()
    lab = torch.from_numpy(cases[2][1]).to(dev).clone()
    bufs = LovaszBuffers(C, H, W, len(classes), dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):      # a warm-up run outside the capture
        ops.lovasz_forward(p, lab, classes, bufs.work, loss_out=bufs.loss)
        ops.lovasz_backward(p, classes, bufs.work, dp=bufs.dp)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.lovasz_forward(p, lab, classes, bufs.work, loss_out=bufs.loss)
        ops.lovasz_backward(p, classes, bufs.work, dp=bufs.dp)
    for P, label in cases[:2]:
        want = run_device(P, label, classes)
        p.copy_(torch.from_numpy(P).to(dev)[None])
        lab.copy_(torch.from_numpy(label).to(dev))
        bufs.dp.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        perm, gw, state, G = ops.lovasz_views(bufs.work, H, W, len(classes))
        got = (perm.cpu().numpy(), gw.cpu().numpy(), state[:18].cpu().numpy(), G[:len(classes)].cpu().numpy(), float(bufs.loss),
               bufs.dp[0].cpu().numpy())
        for x, y in zip(want, got):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
        check(P, label, classes, got, "replay")


# ---- through the model: 32 x 32, the drivers' small generator (resnet_6blocks, ngf 8; the U-Nets need 128 pixels) ------------------
NET = ["--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "32", "--which_model_netG",
       "resnet_6blocks", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout", "--dataroot",
       "synthetic", "--manualSeed", "4", "--which_model_netD", "None", "--weights", "1", "2"]
WITH_D = ("--which_model_netD", "n_layers", "--n_layers_D", "1", "--ndf", "8", "--scale_factor", "1", "--lambda_D", "0.5", "--no_lsgan")


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
    """Counter of the names of everything the device ran for fn(), as torch.profiler's device activity records it (the instrument
    of tests/test_hip_cldice.py)."""
    from collections import Counter
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = Counter()
    for e in prof.events():
        if str(getattr(e, "device_type", "")).endswith("CUDA"):
            own = re.search(r"\bsg_\w+", e.name)
            names[own.group(0) if own else e.name] += 1
    return names


def same_within_the_rule(ga, gb):
    """The project's rule for two runs of the order-dependent weight-gradient kernels (tests/test_hip_segm_nod.py): 1e-4 of the
    tensor's maximum; a bias in front of an InstanceNorm has an analytically zero gradient, its residue is taken over the layer's
    weight gradient."""
    for k, g in ga.items():
        scale = ga.get(k.replace(".bias", ".weight"), g)
        assert float((g - gb[k]).abs().max()) <= 1e-4 * float(scale.abs().max()) + 1e-12, k


def term_against_the_yardstick(m, classes):
    """G_Lovasz against the yardstick on the planes the trainer read: fake_B with discriminators, else the term's own softmax /
    sigmoid of the trainer's logits."""
    from supervised_gan_amd.losses import sigmoid_channels, softmax_channels
    from supervised_gan_amd.util import lovasz_ref
    if m.no_netD:
        p = sigmoid_channels(m.logit.detach()) if m.use_sigmoid_ss else softmax_channels(m.logit.detach())
    else:
        p = m.fake_B.detach()
    label = m.label[0].cpu().numpy()
    L = lovasz_ref(p.cpu().numpy(), label, classes)[0]
    term = float(m.loss_G_Lovasz.detach())
    print(f"G_Lovasz {term!r}, yardstick {L!r}")
    assert abs(term - L) <= (U + (2 * label.size + 22) * EPS) * L and 0.0 < term <= 1.0
    return L


def test_loss_is_head_plus_weighted_term_and_weight_zero_changes_nothing(tmp_path):
    """forward + backward_G of three trainers from the same seed: without the option, with --lovasz_weight 0, with 0.5 over the
    classes 0 and 1.  Every trainer runs the pass once (lazy buffers) and once more under the profiler.  Weight 0 must run exactly
    the device launches of no option and give the same loss and d loss / d logits bit for bit; the weight gradients behind them are
    held to the project's rule (the backward-weight kernels add in the order their workgroups arrive).  Weight 0.5 adds the term's
    launches by the plan of DESIGN.md R30 (at 32 x 32 one chunk: the chunk sort, count, offsets, weights, finish, backward), takes
    none of the library's away, and loss_G = head + 0.5 term in fp32 with the head's loss that of the plain trainer."""
    _need_gpu()
    from collections import Counter
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    out, launches = {}, {}
    for name, extra in (("plain", ()), ("zero", ("--lovasz_weight", "0")), ("on", ("--lovasz_weight", "0.5", "--lovasz_classes", "0", "1"))):
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
    own = {k: Counter({n: c for n, c in v.items() if n.startswith("sg_")}) for k, v in launches.items()}
    print(f"launches {({k: sum(v.values()) for k, v in launches.items()})}; added by the term: {dict(launches['on'] - launches['plain'])}")
    assert sum(own["plain"].values()) > 20, launches["plain"]
    assert launches["zero"] == launches["plain"]
    assert not (own["plain"] - own["on"]), "the term takes no launch of the library's away"
    added = {k: v for k, v in (own["on"] - own["plain"]).items() if k.startswith("sg_lov_")}
    assert added == {"sg_lov_sort_chunk_kernel": 1, "sg_lov_count_kernel": 1, "sg_lov_offsets_kernel": 1, "sg_lov_weights_kernel": 1,
                     "sg_lov_finish_kernel": 1, "sg_lov_bwd_kernel": 1}, added
    assert out["plain"][3] == out["zero"][3] == ["G_CE"] and out["on"][3] == ["G_CE", "G_Lovasz"]
    assert out["zero"][0].lovasz is None and out["plain"][0].lovasz is None and out["on"][0].lovasz == (0.5, (0, 1))
    assert torch.equal(out["plain"][1], out["zero"][1]) and torch.equal(out["plain"][4], out["zero"][4])
    same_within_the_rule(out["plain"][2], out["zero"][2])
    m = out["on"][0]
    head, term = m.loss_G_CE.detach(), m.loss_G_Lovasz.detach()
    assert torch.equal(m.loss_G.detach(), head + 0.5 * term)
    assert torch.equal(head, out["plain"][1])      # the head's loss is untouched by the term beside it
    term_against_the_yardstick(m, (0, 1))
    assert not torch.equal(out["on"][4], out["plain"][4]) and bool(torch.isfinite(out["on"][4]).all())      # the term reaches the logits
    assert all(float(g.abs().max()) > 0.0 for k, g in out["on"][2].items() if k.endswith(".weight"))


@pytest.mark.parametrize("case", ["sigmoid", "with_D", "with_cldice"])
def test_the_other_heads(tmp_path, case):
    """The sigmoid head without discriminators (the term's own sigmoid of the logits), the trainer with a discriminator (the term
    reads fake_B), and the term beside --cldice_weight: loss_G is the rest of the loss plus 0.5 times the term, one fp32 product and
    sum; the term is the yardstick's on the planes the trainer holds; its gradient reaches the weights."""
    _need_gpu()
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    extra = ("--lovasz_weight", "0.5") + (WITH_D if case == "with_D" else ()) + (("--use_sigmoid_ss",) if case == "sigmoid" else ()) \
        + (("--cldice_weight", "0.25", "--cldice_iters", "2") if case == "with_cldice" else ())
    opt, m = build(tmp_path, extra)
    assert m.use_sigmoid_ss == (case == "sigmoid") and m.no_netD == (case != "with_D")
    data = SyntheticDataset(opt, 1).ring[0]
    if not m.no_netD:      # one whole step first: the discriminator's stage, and its logged losses, exist only after it
        m.set_input(data)
        m.optimize_parameters()
    one_pass(m, data)
    torch.cuda.synchronize()
    rest = m.loss_G_CE.detach() if m.no_netD else m.loss_G_GAN.detach() + m.loss_G_CE.detach()
    if case == "with_cldice":
        rest = rest + 0.25 * m.loss_G_clDice.detach()
        assert list(m.get_current_errors())[-2:] == ["G_clDice", "G_Lovasz"]
    term = m.loss_G_Lovasz.detach()
    assert torch.equal(m.loss_G.detach(), rest + 0.5 * term)
    assert list(m.get_current_errors())[-1] == "G_Lovasz"
    term_against_the_yardstick(m, (0,))
    assert all(float(g.abs().max()) > 0.0 for k, g in grads(m).items() if k.endswith(".weight"))

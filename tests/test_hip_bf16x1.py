"""The one-plane 16-bit arithmetic mode ("bf16x1", SGAN_MATH_BF16X1) of the conv kernels.

A product is hi(a) * hi(b) alone, on the planes bf16x3 uses: forward fp16 of the prologue-transformed activation x fp16 of w * 2^10,
backward-data / backward-weight bf16 (fp16 of dY * 2^s where max|dY| was published), fp32 accumulation.  The exactness tests hold
every pass to an fp64 convolution of the operands ROUNDED THE WAY THE KERNEL ROUNDS THEM, with a gate ten times below the distance of
the bf16x3 result from that same reference: a kernel that still formed the lo products fails."""
import os

import numpy as np
import pytest
import torch

from plane_model import _bf16, _conv, _dgrad_ref, _f16, _prologue, _shift, _wgrad_ref
from test_hip_bf16x3 import SHAPES, TILES, _select_tile

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import _lib, ops
    _lib.lib()
    prev = ops.get_math()
    yield ops
    ops.set_math(prev)
    os.environ.pop("SGAN_TILE3", None)
    os.environ.pop("SGAN_IGEMM3P", None)


def _l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def _x1_name(name3):
    """The one-plane twin of a bf16x3 kernel name."""
    return name3[:-1] + ",x1>"


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{c[0]}_k{c[1]}s{c[2]}_{c[4]}to{c[5]}_{c[6]}x{c[7]}" for c in SHAPES])
def test_bf16x1_single_plane_exact(ops, shape, tile):
    """Forward (with the InstanceNorm / BatchNorm + activation prologue), backward-data and backward-weight, bf16 and fp16 planes,
    against fp64 of the kernel-rounded operands; every launch the bf16x3 mode serves with a split kernel must run its x1 twin, and
    every launch it serves with the exact-fp32 kernels (maps under 256 pixels) must do so in bf16x1 too, bit-identical to f32."""
    from hip_utils import from_buf, from_master, master_weight, pad_vec, stats_of, to_buf
    from supervised_gan_amd import _lib
    kind, k, s, p, cin, cout, H, W, norm, act = shape
    tr = kind == "convT"
    _select_tile(tile)
    g = torch.Generator().manual_seed(41)
    x = torch.randn(1, cin, H, W, generator=g) * 1.5 + 0.3
    wshape = (cin, cout, k, k) if tr else (cout, cin, k, k)
    w = torch.randn(*wshape, generator=g) * 0.05
    b = torch.randn(cout, generator=g) * 0.1
    gamma = (1 + 0.2 * torch.randn(cin, generator=g)) if norm == "bn" else None
    beta = (0.1 * torch.randn(cin, generator=g)) if norm == "bn" else None
    Ho, Wo = _conv(tr, torch.zeros(1, cin, H, W), torch.zeros(wshape), None, s, p).shape[2:]
    R = torch.randn(1, cout, Ho, Wo, generator=g)
    desc = ops.conv_desc(1 if tr else 0, k, s, p, H, W, cin, Ho, Wo, cout, cin, cout)
    xb, wm, bb, Rb = to_buf(x), master_weight(w, tr), pad_vec(b), to_buf(R)
    st_in = stats_of(x) if norm else None
    in_norm = ops.norm_desc(st_in, pad_vec(gamma) if gamma is not None else None, pad_vec(beta) if beta is not None else None,
                            H * W, 1e-5, act, 0.2)
    a = _prologue(x, st_in, gamma, beta, norm, act, H * W)
    amax = float(R.abs().max())
    sh = _shift(amax)

    def run(mode, published):
        ops.set_math(mode)
        Rs = Rb.clone()
        if published:
            Rs._sgan_amax = Rs.abs().max().reshape(1).float()
        ob = torch.full((Ho, Wo, cout), float("nan"), device="cuda")
        ops.conv_fwd(desc, xb, in_norm, wm, bb, ob, 0, None)
        kf = _lib.lib().sgan_last_kernel().decode()
        din = torch.full((H, W, cin), float("nan"), device="cuda")
        ops.conv_dgrad(desc, Rs, wm._sgan_wt, din, None, None, None, w_transposed=True)      # the raw product: no epilogue
        kd = _lib.lib().sgan_last_kernel().decode()
        dw, db = torch.zeros_like(wm), torch.zeros_like(bb)
        ops.conv_wgrad(desc, xb, in_norm, Rs, dw, db)
        kw = _lib.lib().sgan_last_kernel().decode()
        torch.cuda.synchronize()
        return dict(fwd=from_buf(ob, cout), dgrad=from_buf(din, cin), wgrad=from_master(dw, k, cin, cout, tr), db=db[:cout].cpu(),
                    names=(kf, kd, kw))

    try:
        for published in (False, True):
            r32, r3, r1 = run("f32", published), run("bf16x3", published), run("bf16x1", published)
            # operands as the kernel rounds them (forward: fp16 both, weights scaled by 2^10)
            if published:
                dy_r, wd_r, a_w = _f16(R, sh), _f16(w, 10), _f16(a)
            else:
                dy_r, wd_r, a_w = _bf16(R), _bf16(w), _bf16(a)
            refs = dict(fwd=_conv(tr, _f16(a), _f16(w, 10), b.double(), s, p),
                        dgrad=_dgrad_ref(tr, dy_r, wd_r, s, p, (1, cin, H, W)),
                        wgrad=_wgrad_ref(tr, a_w, dy_r, wshape, s, p))
            for i, what in enumerate(("fwd", "dgrad", "wgrad")):
                n3, n1 = r3["names"][i], r1["names"][i]
                if "igemm3" in n3 or "wgrad3" in n3:
                    assert n1 == _x1_name(n3), (what, n3, n1)
                    e1, e3 = _l2(r1[what], refs[what]), _l2(r3[what], refs[what])
                    print(f"{what} (published max {published}): bf16x1 {e1:.2e}, bf16x3 {e3:.2e} from the rounded-operand fp64 ({n1})")
                    assert e3 > 1e-5, (what, e3)          # the rounding is visible: the gate below means something
                    assert e1 < e3 / 10, (what, e1, e3)
                    assert torch.isfinite(r1[what]).all()
                else:
                    # not covered by the 16-bit kernels: the exact-fp32 kernel in every mode, the same bits
                    assert n1 == n3 == r32["names"][i] and "x1" not in n1, (what, n1, n3, r32["names"][i])
                    assert torch.equal(r1[what], r32[what]), what
            assert _l2(r1["db"], R.double().sum((0, 2, 3))) < 1e-5      # the bias gradient sums fp32 dY before any rounding
    finally:
        ops.set_math("bf16x3")


def test_bf16x1_fallbacks_run_fp32(ops):
    """Maps under 256 pixels and Cin % 8 != 0: the exact-fp32 kernels, results bit-identical to the f32 mode (backward-weight: up to
    the order of its fp32 atomics, which differs from run to run in any mode)."""
    from hip_utils import master_weight, stats_of, to_buf
    from supervised_gan_amd import _lib
    _select_tile("auto")
    g = torch.Generator().manual_seed(5)
    for cin, cout, H in ((32, 64, 12), (12, 32, 40), (64, 32, 15)):
        x = torch.randn(1, cin, H, H, generator=g)
        wm = master_weight(torch.randn(cout, cin, 4, 4, generator=g) * 0.05, False)
        Ho = H // 2 + 1
        desc = ops.conv_desc(0, 4, 2, 2, H, H, cin, Ho, Ho, cout, cin, cout)
        nd = ops.norm_desc(stats_of(x), None, None, H * H, 1e-5, 2, 0.2)
        R = to_buf(torch.randn(1, cout, Ho, Ho, generator=g))
        res = {}
        for mode in ("f32", "bf16x1"):
            ops.set_math(mode)
            ob = torch.full((Ho, Ho, cout), float("nan"), device="cuda")
            ops.conv_fwd(desc, to_buf(x), nd, wm, None, ob)
            kf = _lib.lib().sgan_last_kernel().decode()
            din = torch.full((H, H, cin), float("nan"), device="cuda")
            ops.conv_dgrad(desc, R, wm._sgan_wt, din, None, None, None, w_transposed=True)
            kd = _lib.lib().sgan_last_kernel().decode()
            dw = torch.zeros_like(wm)
            ops.conv_wgrad(desc, to_buf(x), nd, R, dw, None)
            kw = _lib.lib().sgan_last_kernel().decode()
            torch.cuda.synchronize()
            res[mode] = (ob, din, dw, (kf, kd, kw))
        ops.set_math("bf16x3")
        assert res["f32"][3] == res["bf16x1"][3], (cin, H, res["f32"][3], res["bf16x1"][3])
        assert not any("igemm3" in n or "wgrad3" in n for n in res["bf16x1"][3]), res["bf16x1"][3]
        assert torch.equal(res["f32"][0], res["bf16x1"][0]) and torch.equal(res["f32"][1], res["bf16x1"][1]), (cin, H)
        assert _l2(res["bf16x1"][2], res["f32"][2]) < 1e-6, (cin, H)      # the fp32 backward-weight kernel: up to the order of its atomics


_FUSED_SEEN = {}


@pytest.mark.parametrize("mix", ["x1", "wgrad_x1"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{c[0]}_k{c[1]}s{c[2]}_{c[4]}to{c[5]}_{c[6]}x{c[7]}" for c in SHAPES])
def test_bf16x1_fused_backward_equals_the_two_launches(ops, shape, mix):
    """sgan_conv_bwd_fused in bf16x1 against the two grouped launches on the same two-problem job lists (input gradients bit for bit
    or within the two-wave-group rounding, the rest up to the order of atomic adds).  mix "wgrad_x1": the backward-data half in
    bf16x3 beside a one-plane backward-weight half -- the route of backward-data into a layer without a normalisation; with <= 32
    result channels the gradient carries its published maximum (fp16 planes: the fused launch carries them for that tile only)."""
    from hip_utils import master_weight, pad_vec, rel, stats_of, to_buf
    from supervised_gan_amd import _lib
    kind, k, s, p, cin, cout, H, W, norm, act = shape
    tr = kind == "convT"
    _select_tile("auto")
    g = torch.Generator().manual_seed(17)
    wshape = (cin, cout, k, k) if tr else (cout, cin, k, k)
    wm = master_weight(torch.randn(*wshape, generator=g) * 0.05, tr)
    probs = []
    for h, w_ in ((H, W), (H + 3, W + 2)):
        x = torch.randn(1, cin, h, w_, generator=g) * 1.5 + 0.3
        ho, wo = ((h - 1) * s - 2 * p + k, (w_ - 1) * s - 2 * p + k) if tr else ((h + 2 * p - k) // s + 1, (w_ + 2 * p - k) // s + 1)
        nd = ops.norm_desc(stats_of(x), None, None, h * w_, 1e-5, act, 0.2) if norm else None
        probs.append((to_buf(x), nd, to_buf(torch.randn(1, cout, ho, wo, generator=g)), h, w_, ho, wo))
    dmath = "bf16x3" if mix == "wgrad_x1" else None
    res = {}
    ops.set_math("bf16x1")
    try:
        for mode in ("apart", "fused"):
            dw, db = torch.zeros_like(wm), torch.zeros(pad_vec(torch.zeros(cout)).numel(), device="cuda")
            djobs, wjobs, keep = [], [], []
            for xb, nd, dy, h, w_, ho, wo in probs:
                desc = ops.conv_desc(1 if tr else 0, k, s, p, h, w_, cin, ho, wo, cout, cin, cout)
                din = torch.full((h, w_, cin), float("nan"), device="cuda")
                sums = torch.zeros(2 * cin, dtype=torch.float64, device="cuda") if norm else None
                if mix == "wgrad_x1" and cin <= 32:
                    dy._sgan_amax = dy.abs().max().reshape(1).float()
                djobs.append((desc, dy, wm._sgan_wt, din, xb, nd, sums, 0, False, True, 0))
                wjobs.append((desc, xb, nd, dy.view_as(dy), dw, db))      # an untagged alias: bf16 planes in both runs
                keep.append((din, sums))
            if mode == "apart":
                ops.conv_wgrad_grouped(wjobs)
                kw = _lib.lib().sgan_last_kernel().decode()
                with ops.math_scope(dmath):
                    ops.conv_dgrad_grouped(djobs)
                kd = _lib.lib().sgan_last_kernel().decode()
            else:
                fused = ops.conv_bwd_grouped(djobs, wjobs, dmath)
                kfu = _lib.lib().sgan_last_kernel().decode()
                if fused:
                    assert kfu == ("sg_bwd_fused_kernel<x1>" if mix == "x1" else "sg_bwd_fused_kernel<wgrad x1>"), kfu
            torch.cuda.synchronize()
            res[mode] = (keep, dw, db)
    finally:
        ops.set_math("bf16x3")
    print(f"fused launch: {fused}; apart: {kd} + {kw}")
    if "wgrad3" in kw:
        assert kw.endswith(",x1>"), kw
    if "igemm3" in kd:
        assert kd.endswith(",x1>") == (mix == "x1"), kd
    _FUSED_SEEN[(shape, mix)] = fused
    for (da, sa), (df, sf) in zip(res["apart"][0], res["fused"][0]):
        assert torch.isfinite(df).all()
        assert torch.equal(da, df) or rel(df, da) < 4e-6
        if sa is not None:
            assert rel(sf, sa) < (1e-12 if torch.equal(da, df) else 4e-6)
    assert rel(res["fused"][1], res["apart"][1]) < 2e-6 and rel(res["fused"][2], res["apart"][2]) < 2e-6


def test_bf16x1_fused_backward_is_taken(ops):
    """The comparison above is vacuous where the fused entry point declines: the stride-1 convs with >= 64 channels on both sides
    must have gone through the fused launch in bf16x1, and the mixed launch must have been taken at least once."""
    want = [c for c in SHAPES if c[0] == "conv" and c[2] == 1 and c[4] >= 64 and c[5] >= 64 and c[6] * c[7] >= 256]
    assert want and all(_FUSED_SEEN.get((c, "x1")) for c in want), {c: _FUSED_SEEN.get((c, "x1")) for c in want}
    assert sum(bool(v) for (c, m), v in _FUSED_SEEN.items() if m == "x1") > len(want)
    assert any(v for (c, m), v in _FUSED_SEEN.items() if m == "wgrad_x1"), _FUSED_SEEN


# ---- whole training step (BASELINE configs[1]: fcgan 512^2, deconv G + 3 PatchGAN D) ----

def _fcgan_run(mode, nsteps):
    import sgan_oracle as O
    from test_hip_step import build_model, real3, step1_with_captures
    from supervised_gan_amd import ops
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fcgan_step_full.npz"))
    cfg = O.FCGANConfig(n_update_G=2)
    ops.set_math(mode)
    try:
        m = build_model(cfg, int(g["n_init_noise_draws"]))
        cap = step1_with_captures(m, real3(cfg, 0))
        losses = [list(m.get_current_errors().values())]
        for step in range(1, nsteps):
            m.set_input({"A": real3(cfg, step), "A_paths": ["synthetic"]})
            m.optimize_parameters()
            losses.append(list(m.get_current_errors().values()))
        torch.cuda.synchronize()
    finally:
        ops.set_math("bf16x3")
    del m
    torch.cuda.empty_cache()
    return cap, np.asarray(losses, dtype=np.float64)


def _dev(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def test_bf16x1_fcgan_step_and_20_step_loss_curves():
    """SURVEY 8(d)'s gate for a 16-bit mode: the step-1 statistic max|a - b| / max|b| against the f32 mode for `fake`, the losses and
    every gradient (printed; loose caps), and the 20-step loss curves of f32, bf16x3 and bf16x1 on identical latents and batches: at
    every step the worst loss deviation from the f32 curve within max(2e-2 * max(1, max|L_f32|), 4 * the bf16x3 curve's worst).
    Measured on an MI355X: fake 9.5e-4 (bf16x3 1.0e-6), losses 6.5e-5 (8.8e-6), gradients median 5.8e-2 (2.6e-2) -- the worst
    gradient tensor is ~2 in BOTH 16-bit modes: bias gradients of layers in front of a normalisation, zero up to rounding in every mode;
    20-step curves: worst deviation 0.079 (bf16x3 0.074), growing from 3e-5 at step 1 as Adam's sign-like updates amplify any
    difference."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    runs = {mode: _fcgan_run(mode, 20) for mode in ("f32", "bf16x3", "bf16x1")}
    (c32, l32), (c3, l3), (c1, l1) = runs["f32"], runs["bf16x3"], runs["bf16x1"]
    stats = {"fake": (_dev(c1["fake"], c32["fake"]), _dev(c3["fake"], c32["fake"]))}
    stats["losses"] = (max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(c1["loss_D"] + [c1["loss_G"]], c32["loss_D"] + [c32["loss_G"]])),
                       max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(c3["loss_D"] + [c3["loss_G"]], c32["loss_D"] + [c32["loss_G"]])))
    gx1 = [_dev(c1["gradG"][k], v) for k, v in c32["gradG"].items()]
    gx3 = [_dev(c3["gradG"][k], v) for k, v in c32["gradG"].items()]
    for i, d in enumerate(c32["gradD"]):
        gx1 += [_dev(c1["gradD"][i][k], v) for k, v in d.items()]
        gx3 += [_dev(c3["gradD"][i][k], v) for k, v in d.items()]
    stats["gradients (worst)"] = (max(gx1), max(gx3))
    stats["gradients (median)"] = (float(np.median(gx1)), float(np.median(gx3)))
    for k, (v1, v3) in stats.items():
        print(f"max|a-b|/max|b| vs f32, {k}: bf16x1 {v1:.2e}  bf16x3 {v3:.2e}")
    dev1, dev3 = np.abs(l1 - l32), np.abs(l3 - l32)
    print("20-step loss curves, worst |L - L_f32| per step: bf16x1", np.round(dev1.max(1), 5).tolist(), "bf16x3", np.round(dev3.max(1), 5).tolist())
    assert np.isfinite(l1).all() and np.isfinite(l3).all()
    assert stats["fake"][0] < 1e-2 and stats["losses"][0] < 1e-2 and stats["gradients (median)"][0] < 0.2
    assert np.isfinite(c1["fake"].numpy()).all()
    bound = np.maximum(2e-2 * np.maximum(1.0, np.abs(l32).max(1)), 4 * dev3.max(1))
    assert (dev1.max(1) <= bound).all(), (dev1.max(1), bound)


def test_bf16x1_graphed_step_equals_eager():
    """hipGraph replay in bf16x1 (the mode current at capture is the mode replayed) against eager launches, fcgan at 128^2 with 32
    generator / discriminator channels (layers wide enough for the 16-bit kernels); the drift rule of test_graphed_step_equals_eager."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    import random

    from test_graph_step import FCGAN, _build, _ring
    from supervised_gan_amd import ops
    from supervised_gan_amd.graph_step import GraphedStep
    argv = FCGAN + ["--ngf", "32", "--ndf", "32", "--math", "bf16x1"]
    prev = ops.get_math()
    try:
        ring = _ring(128)
        seq = [0, 0, 1, 2, 3]

        def eager():
            random.seed(11)
            m = _build(argv)
            assert ops.get_math() == "bf16x1"
            errs = []
            for i in seq:
                m.set_input(ring[i])
                m.optimize_parameters()
                errs.append(list(m.get_current_errors().values()))
            return m, errs
        a, ea = eager()
        c, _ = eager()
        random.seed(11)
        b = _build(argv)
        gs = GraphedStep(b)
        gs.capture(ring[0])
        eb = []
        for i in seq[2:]:
            gs.step(ring[i])
            eb.append(list(b.get_current_errors().values()))
        torch.cuda.synchronize()
    finally:
        ops.set_math(prev)
    ea, eb = np.asarray(ea[2:]), np.asarray(eb)
    assert np.isfinite(eb).all()
    assert np.abs(ea - eb).max() < 2e-2 * max(1.0, np.abs(ea).max()), (ea, eb)
    ya, yb, yc = (m.fake.detach().double() for m in (a, b, c))
    drift_eager = float((ya - yc).norm() / ya.norm())
    drift_graph = float((ya - yb).norm() / ya.norm())
    print(f"bf16x1, relative L2 drift after {len(seq)} steps: eager vs eager {drift_eager:.2e}, eager vs graph {drift_graph:.2e}")
    assert drift_graph < max(0.15, 4 * drift_eager)

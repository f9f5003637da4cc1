"""The 16-bit plane conv kernels (bf16x3, bf16x1) across operand scales, against the CPU model of their arithmetic (plane_model.py).

Every other parity test draws x ~ 1.5 N(0,1) + 0.3, w ~ 0.05 N(0,1), dY ~ N(0,1); here each operand in turn is swept over the powers
of two where fp16 planes go subnormal or approach 65504, where sg_f16_shift sits at a power of two, at zero and at its clamp, and
where bf16 planes sit near the ends of the fp32 exponent range.  Gates:
  G1  per element |y_gpu - y_model| <= K 2^-24 M: the kernel forms exactly the documented plane products (they are exact in fp32), so
      what is left is fp32 accumulation of K terms in some order, bounded by K u sum|a||b| with u = 2^-24 whatever the order.
      (Forward: K + 1 and |b| 2^-24 more for the bias add; K 2^-149 for results in fp32's subnormal range.)  Shape A, whose
      LeakyReLU-only prologue the host reproduces bit for bit, and every raw backward-data product.
  G2  where the host's prologue may differ from the kernel's by an fp32 ulp of mean / rstd (shapes B, C) and for backward-weight:
      L2 distance from fp64 truth <= 2 x the model's own distance + K 2^-24.
  G3  inside the documented domains (plane_model.*_CONTRACT / *_FP32): max-norm relative error under 1e-3, and bf16x3 on fp16 planes
      under the 3e-6 of test_igemm3_vs_fp32_kernel_and_fp64; every result finite.
Each test asserts through sgan_last_kernel() that a split kernel ran (else the sweep would test the exact-fp32 fallback)."""
import os

import pytest
import torch
import torch.nn.functional as F

import plane_model as pm
from test_hip_bf16x3 import _select_tile

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPE_B = ("convT", 4, 2, 1, 64, 32, 16, 16, "bn", 1)
SHAPE_C = ("conv", 3, 1, 1, 64, 64, 16, 16, "in", 1)


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


@pytest.fixture(scope="module")
def base_a():
    return pm.shape_a_operands()


def _last():
    from supervised_gan_amd import _lib
    return _lib.lib().sgan_last_kernel().decode()


def _split_ran(name, mode):
    assert "igemm3" in name or "wgrad3" in name or name.startswith("sg_bwd_fused_kernel"), name
    assert ("x1" in name) == (mode == "bf16x1"), (name, mode)


def _g1(what, got, model, M, K, extra=0.0):
    """Worst per-element |got - model| in units of its bound."""
    got = got.double().cpu()
    assert torch.isfinite(got).all(), what
    bound = K * U * M + extra + K * 2.0 ** -149
    worst = float(((got - model).abs() / bound).max())
    print(f"  G1 {what}: worst |gpu - model| / (K u M) = {worst:.3g}")
    assert worst <= 1.0, (what, worst)


def _g2(what, got, model, truth, K):
    got = got.double().cpu()
    assert torch.isfinite(got).all(), what
    dg, dm = pm.rel_l2(got, truth), pm.rel_l2(model, truth)
    print(f"  G2 {what}: L2 from fp64 gpu {dg:.3g}, model {dm:.3g}")
    assert dg <= 2 * dm + K * U, (what, dg, dm)


def _g3(what, got, truth, mode, planes, contract, fp32):
    """contract / fp32: whether the swept operand is inside the documented domains."""
    e = pm.rel_max(got, truth)      # hip_utils.rel without its 1e-12 floor on the denominator, which would hide everything at 2^-100
    print(f"  G3 {what}: max-norm relative {e:.3g} (contract {contract}, fp32-equivalent {fp32})")
    if contract and pm.contract_applies(mode, planes):
        assert e < 1e-3, (what, e)
    if fp32 and mode == "bf16x3" and planes == "f16":
        assert e < 3e-6, (what, e)


def _publish(buf):
    buf._sgan_amax = buf.abs().max().reshape(1).float()
    return buf


def _dims(shape):
    kind, k, s, p, cin, cout, H, W, norm, act = shape
    tr = kind == "convT"
    Ho, Wo = ((H - 1) * s - 2 * p + k, (W - 1) * s - 2 * p + k) if tr else ((H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1)
    return tr, (cin, cout, k, k) if tr else (cout, cin, k, k), Ho, Wo


def _run_wgrad(ops, desc, xb, nd, dyb, wm, shape, mode):
    from hip_utils import from_master, pad_vec
    kind, k, s, p, cin, cout = shape[:6]
    dw, db = torch.zeros_like(wm), pad_vec(torch.zeros(cout))
    ops.conv_wgrad(desc, xb, nd, dyb, dw, db)
    _split_ran(_last(), mode)
    return from_master(dw, k, cin, cout, kind == "convT")


def _check_wgrad(what, got, a, dy, amax, shape, mode, contract, fp32):
    """G2 + G3 of a backward-weight result; a: the host's fp32 prologue output, amax: the published maximum or None."""
    kind, k, s, p = shape[:4]
    tr, wshape, Ho, Wo = _dims(shape)
    truth = pm.truth_wgrad(tr, a, dy, wshape, s, p)
    _g2(what, got, pm.model_wgrad(mode, tr, a, dy, wshape, s, p, amax), truth, Ho * Wo)
    planes = "bf16" if amax is None else "f16"
    _g3(what, got, truth, mode, planes, contract, fp32)


@pytest.mark.parametrize("mode", pm.MODES)
def test_shape_a_activation_scale(ops, base_a, mode):
    """x * 2^e through LeakyReLU-on-load: forward (fp16 planes of the unscaled activation: subnormal lo planes from e = -8 down,
    subnormal hi planes at e = -16 / -24, hi planes up to 49.6e3 at e = 13) and backward-weight on the same activations.  The bias
    is scaled with x so that its rounding does not hide the conv's."""
    from hip_utils import from_buf, master_weight, pad_vec, to_buf
    kind, k, s, p, cin, cout, H, W, norm, act = pm.A_SHAPE
    tr, wshape, Ho, Wo = _dims(pm.A_SHAPE)
    x, w, b, dy = base_a
    _select_tile("auto")
    ops.set_math(mode)
    desc = ops.conv_desc(0, k, s, p, H, W, cin, Ho, Wo, cout, cin, cout)
    nd = ops.norm_desc(None, None, None, H * W, 1e-5, act, 0.2)
    wm, dyb = master_weight(w, tr), to_buf(dy)
    K = k * k * cin
    for e in (-24, -16, -12, -8, 0, 8, 13):
        xs, bs = pm.pow2(x, e), pm.pow2(b, e)
        a = pm._prologue(xs, None, None, None, None, act, H * W)
        amax_a = float(a.abs().max())
        contract, fp32 = pm.inside(pm.ACT_CONTRACT, amax_a), pm.inside(pm.ACT_FP32, amax_a)
        print(f"{mode} x * 2^{e}: max|a| = {amax_a:.3g}")
        xb = to_buf(xs)
        ob = torch.full((Ho, Wo, cout), float("nan"), device="cuda")
        ops.conv_fwd(desc, xb, nd, wm, pad_vec(bs), ob, 0, None)
        _split_ran(_last(), mode)
        got = from_buf(ob, cout)
        M = pm.magnitude_fwd(mode, tr, a, w, s, p)
        _g1("fwd", got, pm.model_fwd(mode, tr, a, w, bs, s, p), M, K + 1, U * bs.double().abs().view(1, -1, 1, 1))
        _g3("fwd", got, pm.truth_fwd(tr, a, w, bs, s, p), mode, "f16", contract, fp32)
        for published in (False, True):
            d = _publish(dyb.clone()) if published else dyb
            gw = _run_wgrad(ops, desc, xb, nd, d, wm, pm.A_SHAPE, mode)
            # bf16 planes carry the fp32 exponent: inside the contract at every activation scale
            _check_wgrad(f"wgrad (published {published})", gw, a, dy, float(dy.abs().max()) if published else None, pm.A_SHAPE, mode,
                         contract if published else True, fp32 and published)


@pytest.mark.parametrize("mode", pm.MODES)
def test_shape_a_weight_scale(ops, base_a, mode):
    """max|w| from 2^-24 (w * 2^10 at fp16's subnormal boundary) to 2^5 (w * 2^10 = 2^15): forward and the raw backward-data product
    through the transposed copy, bf16 planes and (published maximum) fp16 planes; the packed copies remade by master_weight."""
    from hip_utils import from_buf, master_weight, pad_vec, to_buf
    kind, k, s, p, cin, cout, H, W, norm, act = pm.A_SHAPE
    tr, wshape, Ho, Wo = _dims(pm.A_SHAPE)
    x, w, b, dy = base_a
    _select_tile("auto")
    ops.set_math(mode)
    desc = ops.conv_desc(0, k, s, p, H, W, cin, Ho, Wo, cout, cin, cout)
    nd = ops.norm_desc(None, None, None, H * W, 1e-5, act, 0.2)
    a = pm._prologue(x, None, None, None, None, act, H * W)
    xb, dyb, amax = to_buf(x), to_buf(dy), float(dy.abs().max())
    w0 = float(w.abs().max())
    for wmax in (2.0 ** -24, 2.0 ** -10, 0.05 * 4, 2.0 ** 5):
        ws, bs = (w.double() * (wmax / w0)).float(), (b.double() * (wmax / w0)).float()
        wmax_r = float(ws.abs().max())
        contract, fp32 = pm.inside(pm.W_CONTRACT, wmax_r), pm.inside(pm.W_FP32, wmax_r)
        print(f"{mode} max|w| = {wmax_r:.3g}")
        wm = master_weight(ws, tr)
        ob = torch.full((Ho, Wo, cout), float("nan"), device="cuda")
        ops.conv_fwd(desc, xb, nd, wm, pad_vec(bs), ob, 0, None)
        _split_ran(_last(), mode)
        got = from_buf(ob, cout)
        _g1("fwd", got, pm.model_fwd(mode, tr, a, ws, bs, s, p), pm.magnitude_fwd(mode, tr, a, ws, s, p), k * k * cin + 1,
            U * bs.double().abs().view(1, -1, 1, 1))
        _g3("fwd", got, pm.truth_fwd(tr, a, ws, bs, s, p), mode, "f16", contract, fp32)
        truth = pm.truth_dgrad(tr, dy, ws, s, p, x.shape)
        for published in (False, True):
            d = _publish(dyb.clone()) if published else dyb
            din = torch.full((H, W, cin), float("nan"), device="cuda")
            ops.conv_dgrad(desc, d, wm._sgan_wt, din, None, None, None, w_transposed=True)      # the raw product: no epilogue
            _split_ran(_last(), mode)
            gd, am = from_buf(din, cin), amax if published else None
            _g1(f"dgrad (published {published})", gd, pm.model_dgrad(mode, tr, dy, ws, s, p, x.shape, am),
                pm.magnitude_dgrad(mode, tr, dy, ws, s, p, x.shape, am), k * k * cout)
            _g3(f"dgrad (published {published})", gd, truth, mode, "f16" if published else "bf16", contract if published else True,
                fp32 and published)


def _gradient_cases(dy):
    """(label, dY, published): the scale sweep on bf16 and on fp16 planes, and the shift's edge cases."""
    cases = []
    for e in (-100, -30, 0, 30, 100):
        cases += [(f"dY * 2^{e}", pm.pow2(dy, e), False), (f"dY * 2^{e}", pm.pow2(dy, e), True)]
    unit = dy.double() / dy.abs().max().double()            # the largest element is exactly +-1
    cases.append(("max|dY| = 2^3 exactly", (unit * 8.0).float(), True))
    cases.append(("max|dY| one ulp under 2^3", (unit * (8.0 * (1.0 - 2.0 ** -24))).float(), True))
    out = pm.pow2(dy, -10)
    out[0, 5, 7, 9] = 2.0 ** 10                              # one element 2^20 times the bulk: the bulk's lo planes are fp16 subnormals
    cases.append(("one outlier 2^20 times the bulk", out, True))
    return cases


@pytest.mark.parametrize("mode", pm.MODES)
def test_shape_a_gradient_scale(ops, base_a, mode):
    """dY * 2^e, unpublished (bf16 planes near the ends of the fp32 exponent range) and published (fp16 planes of dY * 2^s: the shift
    at its clamp for e = -100, at and one ulp under a power of two, with an outlier; scale-back 2^(-10 - s)): the raw backward-data
    product and backward-weight.  An all-zero dY with a published maximum of 0 gives exact zeros."""
    from hip_utils import from_buf, master_weight, to_buf
    kind, k, s, p, cin, cout, H, W, norm, act = pm.A_SHAPE
    tr, wshape, Ho, Wo = _dims(pm.A_SHAPE)
    x, w, b, dy = base_a
    _select_tile("auto")
    ops.set_math(mode)
    desc = ops.conv_desc(0, k, s, p, H, W, cin, Ho, Wo, cout, cin, cout)
    nd = ops.norm_desc(None, None, None, H * W, 1e-5, act, 0.2)
    a = pm._prologue(x, None, None, None, None, act, H * W)
    xb, wm = to_buf(x), master_weight(w, tr)
    assert float((dy.double() / dy.abs().max().double() * 8.0).float().abs().max()) == 8.0
    for label, d, published in _gradient_cases(dy):
        amax_r = float(d.abs().max())
        am = amax_r if published else None
        contract, fp32 = pm.inside(pm.G_CONTRACT, amax_r), pm.inside(pm.G_FP32, amax_r) and published
        print(f"{mode} {label}, published {published}: max|dY| = {amax_r:.3g}, shift {pm._shift(amax_r) if published else None}")
        db_ = _publish(to_buf(d)) if published else to_buf(d)
        din = torch.full((H, W, cin), float("nan"), device="cuda")
        ops.conv_dgrad(desc, db_, wm._sgan_wt, din, None, None, None, w_transposed=True)
        _split_ran(_last(), mode)
        gd = from_buf(din, cin)
        _g1("dgrad", gd, pm.model_dgrad(mode, tr, d, w, s, p, x.shape, am), pm.magnitude_dgrad(mode, tr, d, w, s, p, x.shape, am), k * k * cout)
        _g3("dgrad", gd, pm.truth_dgrad(tr, d, w, s, p, x.shape), mode, "f16" if published else "bf16", contract, fp32)
        gw = _run_wgrad(ops, desc, xb, nd, db_, wm, pm.A_SHAPE, mode)
        _check_wgrad("wgrad", gw, a, d, am, pm.A_SHAPE, mode, contract, fp32)
    zb = to_buf(torch.zeros_like(dy))
    zb._sgan_amax = torch.zeros(1, device="cuda")
    din = torch.full((H, W, cin), float("nan"), device="cuda")
    ops.conv_dgrad(desc, zb, wm._sgan_wt, din, None, None, None, w_transposed=True)
    _split_ran(_last(), mode)
    gw = _run_wgrad(ops, desc, xb, nd, zb, wm, pm.A_SHAPE, mode)
    assert torch.equal(din, torch.zeros_like(din)) and torch.equal(gw, torch.zeros_like(gw))


@pytest.mark.parametrize("mode", pm.MODES)
def test_shape_a_fused_backward_gradient_scale(ops, base_a, mode):
    """One sgan_conv_bwd_fused launch (two problems; <= 32 result channels: the 128 x 32 backward-data tile, the only one the fused
    launch carries on fp16 planes) against the two grouped launches across the gradient scales, and its backward-data half against
    the plane model: a fused launch that kept a stale choice of planes, shift or scale-back fails G1."""
    from hip_utils import from_buf, master_weight, pad_vec, rel, to_buf
    kind, k, s, p, cin, cout, H, W, norm, act = pm.A_SHAPE
    tr, wshape, _, _ = _dims(pm.A_SHAPE)
    x, w, b, dy = base_a
    _select_tile("auto")
    ops.set_math(mode)
    wm = master_weight(w, tr)
    g = torch.Generator().manual_seed(7)
    probs = []
    for h, w_ in ((H, W), (H + 3, W + 2)):
        ho, wo = h + 2 * p - k + 1, w_ + 2 * p - k + 1
        xs = torch.randn(1, cin, h, w_, generator=g) * 1.5 + 0.3
        probs.append((h, w_, ho, wo, to_buf(xs), torch.randn(1, cout, ho, wo, generator=g)))
    nd_of = lambda h, w_: ops.norm_desc(None, None, None, h * w_, 1e-5, act, 0.2)
    for e in (-100, -30, 0, 30, 100):
        for published in (False, True):
            res = {}
            for how in ("apart", "fused"):
                dw, db = torch.zeros_like(wm), pad_vec(torch.zeros(cout))
                djobs, wjobs, keep = [], [], []
                for h, w_, ho, wo, xb, d0 in probs:
                    d = pm.pow2(d0, e)
                    desc = ops.conv_desc(0, k, s, p, h, w_, cin, ho, wo, cout, cin, cout)
                    dyb = _publish(to_buf(d)) if published else to_buf(d)
                    din = torch.full((h, w_, cin), float("nan"), device="cuda")
                    djobs.append((desc, dyb, wm._sgan_wt, din, None, None, None, 0, False, True, 0))
                    wjobs.append((desc, xb, nd_of(h, w_), dyb.view_as(dyb), dw, db))      # an untagged alias: bf16 planes in both runs
                    keep.append((din, d, (1, cin, h, w_)))
                if how == "apart":
                    ops.conv_wgrad_grouped(wjobs)
                    _split_ran(_last(), mode)
                    ops.conv_dgrad_grouped(djobs)
                    _split_ran(_last(), mode)
                else:
                    assert ops.conv_bwd_grouped(djobs, wjobs, None) is True
                    assert _last().startswith("sg_bwd_fused_kernel"), _last()
                    _split_ran(_last(), mode)
                torch.cuda.synchronize()
                res[how] = (keep, dw, db)
            print(f"{mode} fused, dY * 2^{e}, published {published}")
            for (da, _, _), (df, d, xshape) in zip(res["apart"][0], res["fused"][0]):
                assert torch.isfinite(df).all()
                assert torch.equal(da, df) or rel(df, da) < 4e-6          # the gate of test_fused_backward_equals_the_two_launches
                am = float(d.abs().max()) if published else None
                _g1("fused dgrad", from_buf(df, cin), pm.model_dgrad(mode, tr, d, w, s, p, xshape, am),
                    pm.magnitude_dgrad(mode, tr, d, w, s, p, xshape, am), k * k * cout)
            assert torch.isfinite(res["fused"][1]).all()
            assert rel(res["fused"][1], res["apart"][1]) < 2e-6 and rel(res["fused"][2], res["apart"][2]) < 2e-6


def norm_case(shape, e, seed=43):
    """Operands of shapes B / C at x * 2^e (CPU only): the post-normalisation activation is scale-free while var >> eps."""
    kind, k, s, p, cin, cout, H, W, norm, act = shape
    tr, wshape, Ho, Wo = _dims(shape)
    g = torch.Generator().manual_seed(seed)
    x = pm.pow2(torch.randn(1, cin, H, W, generator=g) * 1.5 + 0.3, e)
    w = torch.randn(*wshape, generator=g) * 0.05
    b = torch.randn(cout, generator=g) * 0.1
    gamma = (1 + 0.2 * torch.randn(cin, generator=g)) if norm == "bn" else None
    beta = (0.1 * torch.randn(cin, generator=g)) if norm == "bn" else None
    dy = torch.randn(1, cout, Ho, Wo, generator=g)
    xd = x.double()
    a64 = F.instance_norm(xd, eps=1e-5) if norm == "in" else F.batch_norm(xd, None, None, gamma.double(), beta.double(), training=True, eps=1e-5)
    return x, w, b, gamma, beta, dy, F.relu(a64)


@pytest.mark.parametrize("mode", pm.MODES)
@pytest.mark.parametrize("shape,tile", [(SHAPE_B, "auto"), (SHAPE_C, "auto"), (SHAPE_C, "patch")], ids=["B_convT_bn", "C_conv_in", "C_conv_in_patch"])
def test_norm_shapes_raw_activation_scale(ops, shape, tile, mode):
    """BatchNorm(gamma, beta) + ReLU and InstanceNorm + ReLU on load at raw scales 2^-6, 1, 2^20: the fp64 statistics and the fp32
    prologue at extreme raw scales, forward and backward-weight (G2: the host prologue is not bit-exact here)."""
    from hip_utils import from_buf, master_weight, pad_vec, stats_of, to_buf
    kind, k, s, p, cin, cout, H, W, norm, act = shape
    tr, wshape, Ho, Wo = _dims(shape)
    _select_tile(tile)
    ops.set_math(mode)
    try:
        desc = ops.conv_desc(1 if tr else 0, k, s, p, H, W, cin, Ho, Wo, cout, cin, cout)
        for e in (-6, 0, 20):
            x, w, b, gamma, beta, dy, a64 = norm_case(shape, e)
            st = stats_of(x)
            nd = ops.norm_desc(st, pad_vec(gamma) if gamma is not None else None, pad_vec(beta) if beta is not None else None, H * W, 1e-5, act, 0.2)
            a = pm._prologue(x, st, gamma, beta, norm, act, H * W)
            amax_a = float(a.abs().max())
            contract, fp32 = pm.inside(pm.ACT_CONTRACT, amax_a), pm.inside(pm.ACT_FP32, amax_a)
            assert contract and fp32      # post-normalisation values of order 1
            print(f"{mode} {kind} {norm} tile {tile}, x * 2^{e}: max|a| = {amax_a:.3g}")
            xb, wm, dyb = to_buf(x), master_weight(w, tr), to_buf(dy)
            ob = torch.full((Ho, Wo, cout), float("nan"), device="cuda")
            ops.conv_fwd(desc, xb, nd, wm, pad_vec(b), ob, 0, None)
            name = _last()
            _split_ran(name, mode)
            if tile == "patch":
                assert "igemm3p" in name, name
            got, truth = from_buf(ob, cout), pm.truth_fwd(tr, a64, w, b, s, p)
            _g2("fwd", got, pm.model_fwd(mode, tr, a, w, b, s, p), truth, k * k * cin)
            _g3("fwd", got, truth, mode, "f16", contract, fp32)
            for published in (False, True):
                d = _publish(dyb.clone()) if published else dyb
                gw = _run_wgrad(ops, desc, xb, nd, d, wm, shape, mode)
                am = float(dy.abs().max()) if published else None
                twg = pm.truth_wgrad(tr, a64, dy, wshape, s, p)
                _g2(f"wgrad (published {published})", gw, pm.model_wgrad(mode, tr, a, dy, wshape, s, p, am), twg, Ho * Wo)
                _g3(f"wgrad (published {published})", gw, twg, mode, "f16" if published else "bf16", True, published)
    finally:
        _select_tile("auto")

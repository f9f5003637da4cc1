"""tests/small_kernels_ref.py held to torch on the CPU, in float64: the reference that tests/test_hip_small_kernels.py compares the
kernels with must be right on its own.  Running statistics against F.batch_norm(training=True), SGD against torch.optim.SGD, the
sigmoid / tanh derivatives against autograd, the layout functions against permute / torch.cat.

The two run-time ulp budgets of the GPU file (sgan_sigmoid_fwd, sgan_add_act_fwd with tanh) are computed here as well, from the same
inputs and the same torch CPU fp32 evaluation, and must stay at or below 16 ulp: a broken reference cannot widen them silently.
Run with -s for the figures."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_kernels_ref as R


def cpu_f32_sigmoid(x):
    """The kernel's expression, 1 / (1 + exp(-x)), evaluated by torch on the CPU in float32."""
    t = torch.from_numpy(np.asarray(x, dtype=np.float32))
    return (1.0 / (1.0 + torch.exp(-t))).numpy()


def cpu_f32_add_tanh(a, b):
    """tanh(a + b) evaluated by torch on the CPU in float32."""
    return torch.tanh(torch.from_numpy(np.asarray(a, dtype=np.float32)) + torch.from_numpy(np.asarray(b, dtype=np.float32))).numpy()


# ---- layout -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,Cstore", [(1, 4), (3, 4), (4, 4), (5, 8), (8, 8), (1, 8)])
def test_to_nhwc_ref_is_permute_and_zero_pad(C, Cstore):
    rng = np.random.default_rng(C * 10 + Cstore)
    src = rng.standard_normal((C, 5, 7)).astype(np.float32)
    out = R.to_nhwc_ref(src, Cstore)
    want = torch.zeros(5, 7, Cstore)
    want[..., :C] = torch.from_numpy(src).permute(1, 2, 0)
    assert out.dtype == np.float32 and np.array_equal(out.view(np.int32), want.numpy().view(np.int32))


@pytest.mark.parametrize("Ca,Cb", [(1, 1), (1, 3), (3, 1), (2, 3), (4, 4), (3, 6)])
def test_concat_and_slice_ref_are_torch_cat_and_indexing(Ca, Cb):
    rng = np.random.default_rng(Ca * 10 + Cb)
    a = rng.standard_normal((4, 6, Ca + 2)).astype(np.float32)        # ld larger than the channel count
    b = rng.standard_normal((4, 6, Cb + 3)).astype(np.float32)
    Cs = (Ca + Cb + 3) // 4 * 4
    out = R.concat_ref(a, Ca, b, Cb, Cs)
    want = torch.cat((torch.from_numpy(a)[..., :Ca], torch.from_numpy(b)[..., :Cb], torch.zeros(4, 6, Cs - Ca - Cb)), dim=2).numpy()
    assert np.array_equal(out.view(np.int32), want.view(np.int32))
    for c0, Cn in ((0, Ca), (Ca, Cb), (1, Ca + Cb - 1)):
        sl = R.slice_ref(out, c0, Cn, Cn + 2)
        assert np.array_equal(sl[..., :Cn], out[..., c0: c0 + Cn]) and not sl[..., Cn:].view(np.int32).any()
    assert np.array_equal(R.slice_ref(out, 0, Ca, Ca), a[..., :Ca]) and np.array_equal(R.slice_ref(out, Ca, Cb, Cb), b[..., :Cb])


# ---- elementwise --------------------------------------------------------------------------------------------------------------
def test_sigmoid_and_tanh_refs_against_autograd_fp64():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(500) * 6.0, R.SIGMOID_PLANTED.astype(np.float64)[:11]])
    xt = torch.from_numpy(x).requires_grad_(True)
    p = torch.sigmoid(xt)
    dp = torch.from_numpy(rng.standard_normal(x.size))
    (gx,) = torch.autograd.grad(p, xt, dp)
    assert np.abs(R.sigmoid_ref(x) - p.detach().numpy()).max() <= 4 * np.finfo(np.float64).eps
    got = R.sigmoid_bwd_ref(dp.numpy(), p.detach().numpy())
    assert np.abs(got - gx.numpy()).max() <= 8 * np.finfo(np.float64).eps * np.abs(dp.numpy()).max()
    a, b = rng.standard_normal(500) * 2.0, rng.standard_normal(500) * 2.0
    at = torch.from_numpy(a).requires_grad_(True)
    y = torch.tanh(at + torch.from_numpy(b))
    dy = torch.from_numpy(rng.standard_normal(500))
    (ga,) = torch.autograd.grad(y, at, dy)
    assert np.abs(R.add_act_ref(a, b, True) - y.detach().numpy()).max() <= 4 * np.finfo(np.float64).eps
    assert np.array_equal(R.add_act_ref(a, b, False), a + b)
    assert np.abs(R.tanh_bwd_ref(dy.numpy(), y.detach().numpy()) - ga.numpy()).max() <= 8 * np.finfo(np.float64).eps * np.abs(dy.numpy()).max()
    # the far ends of float32 logits: no overflow warning, no NaN, exact limits
    ends = R.sigmoid_ref(np.array([-1e30, -800.0, 800.0, 1e30]))
    assert ends[0] == 0.0 and ends[1] == 0.0 and ends[2] == 1.0 and ends[3] == 1.0


# ---- BatchNorm running statistics ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W,momentum", [(8, 16, 16, 0.1), (3, 1, 2, 0.1), (5, 7, 9, 1.0), (4, 6, 5, 0.0), (257, 3, 4, 0.25)])
@pytest.mark.parametrize("replicas,sq_extra", [(1, 0), (4, 0), (8, 5)])
def test_bn_running_ref_against_batch_norm(C, H, W, momentum, replicas, sq_extra):
    rng = np.random.default_rng(C + H)
    x = rng.standard_normal((1, C, H, W)) * 2.0 + 1.0
    rm0, rv0 = rng.standard_normal(C), rng.uniform(0.5, 2.0, C)
    rm, rv = torch.from_numpy(rm0.copy()), torch.from_numpy(rv0.copy())
    F.batch_norm(torch.from_numpy(x), rm, rv, None, None, training=True, momentum=momentum)
    sq = C + sq_extra
    rep = 2 * sq + 3 if replicas > 1 else 0
    stats = np.zeros(max(replicas * rep, 2 * sq))
    w = rng.dirichlet(np.ones(replicas))            # the sums spread over the copies in unequal parts
    for r in range(replicas):
        stats[r * rep: r * rep + C] = w[r] * x.sum((0, 2, 3))
        stats[r * rep + sq: r * rep + sq + C] = w[r] * (x * x).sum((0, 2, 3))
    got_m, got_v, _, _ = R.bn_running_ref(stats, C, H * W, sq if sq_extra else 0, rep, replicas, rm0, rv0, momentum)
    assert np.abs(got_m - rm.numpy()).max() <= 1e-13 and np.abs(got_v - rv.numpy()).max() <= 1e-12


def test_bn_running_ref_count_one_and_clamp():
    """count == 1: torch refuses (it needs more than one value per channel); the kernel's rule is factor 1, variance 0.  The clamp:
    sumsq / count below mean^2 gives variance 0, not a negative number."""
    stats = np.array([3.0, -2.0, 9.0, 4.0])
    m, v, mean, var = R.bn_running_ref(stats, 2, 1, 0, 0, 1, np.zeros(2), np.ones(2), 0.5)
    assert np.array_equal(mean, [3.0, -2.0]) and np.array_equal(var, [0.0, 0.0]) and np.array_equal(v, [0.5, 0.5])
    stats = np.array([256 * 1e4, 256 * (1e8 - 100.0)])
    m, v, mean, var = R.bn_running_ref(stats, 1, 256, 0, 0, 1, np.zeros(1), np.ones(1), 1.0)
    assert mean[0] == 1e4 and var[0] == 0.0 and v[0] == 0.0


# ---- SGD ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mu", [0.0, 0.9])
def test_sgd_step_ref_against_torch_optim(mu):
    rng = np.random.default_rng(6)
    p0 = rng.standard_normal(1000)
    ref_p = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.SGD([ref_p], lr=0.05, momentum=mu)
    p, buf = p0.copy(), (np.zeros(1000) if mu else None)      # torch's first step sets buf = g: a zero buffer reproduces it
    for _ in range(5):
        g = rng.standard_normal(1000)
        ref_p.grad = torch.from_numpy(g.copy())
        opt.step()
        p, buf, _ = R.sgd_step_ref(p, g, buf, 0.05, mu)
        assert np.abs(p - ref_p.detach().numpy()).max() <= 1e-14
    if mu:
        assert np.abs(buf - opt.state[ref_p]["momentum_buffer"].numpy()).max() <= 1e-14


def test_sgd_step_ref_leaves_an_unused_buffer_alone():
    p, g, buf = np.ones(3), np.full(3, 2.0), np.full(3, 5.0)
    q, b, gg = R.sgd_step_ref(p, g, buf, 0.5, 0.0)
    assert b is buf and np.array_equal(q, [0.0, 0.0, 0.0]) and np.array_equal(gg, g)
    q, b, gg = R.sgd_step_ref(p, g, None, 0.5, 0.9)
    assert b is None and np.array_equal(q, [0.0, 0.0, 0.0])
    q, b, gg = R.sgd_step_ref(p, g, buf, 0.5, 0.5)
    assert np.array_equal(b, [4.5] * 3) and np.array_equal(q, [-1.25] * 3)


# ---- the run-time budgets -----------------------------------------------------------------------------------------------------
def test_ulp_error_counts_float32_ulps():
    one = np.float32(1.0)
    assert R.ulp_error(np.nextafter(one, np.float32(2)), 1.0).item() == 1.0
    assert R.ulp_error(np.float32(0), 1e-39).item() == 0.0                  # below one minimum normal: free
    assert R.ulp_error(np.float32(3e-38), 1e-38).item() > 1e5               # 2e-38 off: far outside


@pytest.mark.parametrize("npix", R.SIGMOID_NPIX)
def test_sigmoid_budget_stays_below_16_ulp(npix):
    x = R.sigmoid_inputs(npix)
    budget = R.ulp_budget(cpu_f32_sigmoid(x), R.sigmoid_ref(x))
    print(f"sigmoid npix={npix}: budget {budget:.2f} ulp")
    assert 2.0 <= budget <= 16.0


@pytest.mark.parametrize("n", R.EW_SIZES)
def test_add_tanh_budget_stays_below_16_ulp(n):
    a, b = R.add_tanh_inputs(n)
    budget = R.ulp_budget(cpu_f32_add_tanh(a, b), R.add_act_ref(a, b, True))
    print(f"add+tanh n={n}: budget {budget:.2f} ulp")
    assert 2.0 <= budget <= 16.0

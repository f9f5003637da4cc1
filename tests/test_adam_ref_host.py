"""The numpy optimizer reference (tests/adam_ref.py) against torch.optim on float64 CPU tensors and against the oracle's own Adam
-- no GPU.  The GPU tests (tests/test_hip_adam_pack.py, tests/test_hip_optim.py) hold the kernels to this reference, so it has to be
right on its own."""
import numpy as np
import pytest
import torch

import adam_ref as A

N, STEPS = 4099, 5
LR, BETAS, EPS = 2e-4, (0.5, 0.999), 1e-8


def _inputs(seed):
    """Parameters from N(0, 1), gradients of scale 10^(step - 3): what the GPU tests feed the kernels."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(N), [rng.standard_normal(N) * 10.0 ** (s - 3) for s in range(STEPS)]


def _close(a, b, tol):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max()) <= tol * float(np.abs(np.asarray(b)).max())


def test_adam_step_is_torch_adam_in_float64():
    p0, grads = _inputs(1)
    tp = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=LR, betas=BETAS, eps=EPS)
    p, m, v = p0, np.zeros(N), np.zeros(N)
    for t, g in enumerate(grads, 1):
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = A.adam_step(p, g, m, v, t, LR, *BETAS, EPS)
        st = opt.state[tp]
        assert p.dtype == np.float64 and int(st["step"]) == t
        assert _close(p, tp.detach().numpy(), 1e-12), t
        assert _close(m, st["exp_avg"].numpy(), 1e-12) and _close(v, st["exp_avg_sq"].numpy(), 1e-12), t
    assert float(np.abs(p - p0).max()) > 4 * LR          # the five steps moved the parameters (the first ones are sign-like: ~lr each)


def test_adam_step_leaves_its_arguments_alone():
    p0, grads = _inputs(2)
    p, g, m, v = p0.copy(), grads[0].copy(), np.full(N, 0.25), np.full(N, 0.5)
    A.adam_step(p, g, m, v, 3, LR, *BETAS, EPS)
    A.adam_step_f32(p.astype(np.float32), g, m, v, 3, LR, *BETAS, EPS)
    assert np.array_equal(p, p0) and np.array_equal(g, grads[0]) and (m == 0.25).all() and (v == 0.5).all()


def test_oracle_adam_fp32_is_within_the_fp32_yardstick():
    """sgan_oracle.Adam (torch fp32 on CPU, the form the kernels were written from) lands within the bound the kernels are held to:
    YARDSTICK_FACTOR x the deviation of adam_step_f32 from adam_step.  All three get the hyper-parameters rounded to float32, as a
    kernel would (adam_ref.as_f32); the inputs are float32 values, so every side starts from the same numbers."""
    import sgan_oracle as O
    lr, b1, b2, eps = A.as_f32(LR, *BETAS, EPS)
    p0, grads = _inputs(3)
    p0, grads = p0.astype(np.float32), [g.astype(np.float32) for g in grads]
    tp = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = O.Adam([tp], lr=lr, beta1=b1, beta2=b2, eps=eps)
    for g in grads:
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
    ref = A.adam_run(A.adam_step, p0.astype(np.float64), grads, lr, b1, b2, eps)
    f32 = A.adam_run(A.adam_step_f32, p0, grads, lr, b1, b2, eps)
    assert all(a.dtype == np.float32 for a in f32) and all(a.dtype == np.float64 for a in ref)
    dev, yard = A.assert_within_yardstick((tp.detach().numpy(), opt.m[0].numpy(), opt.v[0].numpy()), f32, ref, "oracle Adam")
    assert 0 < yard[0] < 2e-6 and 0 < yard[1] < 1e-6 and 0 < yard[2] < 1e-6      # the yardstick itself is fp32 rounding, nothing larger


def test_yardstick_tells_a_wrong_update_from_rounding():
    """What the bound is for: a skipped step, a doubled step and a step number off by one are each far outside 4 x the yardstick."""
    lr, b1, b2, eps = A.as_f32(LR, *BETAS, EPS)
    p0, grads = _inputs(4)
    p0, grads = p0.astype(np.float32), [g.astype(np.float32) for g in grads]
    ref = A.adam_run(A.adam_step, p0.astype(np.float64), grads, lr, b1, b2, eps)
    f32 = A.adam_run(A.adam_step_f32, p0, grads, lr, b1, b2, eps)
    wrong = {"skipped": A.adam_run(A.adam_step_f32, p0, grads[:-1], lr, b1, b2, eps),
             "doubled": A.adam_run(A.adam_step_f32, p0, grads + grads[-1:], lr, b1, b2, eps),
             "t + 1": A.adam_run(A.adam_step_f32, p0, grads, lr, b1, b2, eps, t0=1)}
    for what, got in wrong.items():
        with pytest.raises(AssertionError):
            A.assert_within_yardstick(got, f32, ref, what)
        assert A.deviation(got, ref)[0] > 50 * A.deviation(f32, ref)[0], what


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_sgd_step_is_torch_sgd_in_float64(momentum):
    p0, grads = _inputs(5)
    tp = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.SGD([tp], lr=0.05, momentum=momentum)
    p, buf = p0, None
    for t, g in enumerate(grads, 1):
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p, buf = A.sgd_step(p, g, buf, 0.05, momentum)
        assert _close(p, tp.detach().numpy(), 1e-12), t
        if momentum:
            assert _close(buf, opt.state[tp]["momentum_buffer"].numpy(), 1e-12), t
    f32 = A.sgd_run(A.sgd_step_f32, p0.astype(np.float32), [g.astype(np.float32) for g in grads], 0.05, momentum)
    assert f32[0].dtype == np.float32 and _close(f32[0], p, 1e-6)

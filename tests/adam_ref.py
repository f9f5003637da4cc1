"""Plain numpy reference of the optimizer updates (csrc/sgan_ew.hip: sg_adam_kernel, sg_adam_pack_kernel, sg_sgd_kernel), in the
torch.optim form the kernels state.  float64 throughout, no torch optimizer inside: the tests compare the kernels with this, never
the other way round (tests/test_adam_ref_host.py holds it to torch.optim on its own).

The *_f32 functions are the SAME formulas carried out in numpy float32, operation by operation as the kernels write them.  They are
no second implementation to test: their distance from the float64 result, on the very inputs of a GPU run, is the yardstick that says
how far a correct fp32 kernel may be from float64 (`deviation`, `assert_within_yardstick`)."""
import math

import numpy as np

YARDSTICK_FACTOR = 4.0      # FMA contraction, and division / square-root rounding that may differ from numpy's


def as_f32(*hyper):
    """Hyper-parameters as the kernels receive them: the C ABI takes `float`, so lr, the betas and eps arrive rounded to float32
    (0.999 becomes 0.99900001287...: 1 - b2 differs from 0.001 by 1.3e-5 relative, which v would show).  A comparison with a kernel
    feeds the reference these values, so that both sides compute the same operation."""
    return tuple(float(np.float32(h)) for h in hyper)


def bias_corrections(t, lr, b1, b2):
    """(lr / (1 - b1^t), 1 / sqrt(1 - b2^t)) in float64: the two scalars every Adam kernel derives from the step number."""
    return lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t)


def adam_step(p, g, m, v, t, lr, b1, b2, eps):
    """One Adam step, step number t (1-based), float64.  Returns the new (p, m, v); the arguments are left alone."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    step_size, inv_sqrt_bc2 = bias_corrections(t, lr, b1, b2)
    p = p - step_size * (m / (np.sqrt(v) * inv_sqrt_bc2 + eps))
    return p, m, v


def adam_step_f32(p, g, m, v, t, lr, b1, b2, eps):
    """adam_step in float32: the two bias-correction scalars formed in float64 and rounded once, every other operation rounded
    to float32 on its own (no FMA), in the order sg_adam1 writes them."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    b1, b2, eps = f(b1), f(b2), f(eps)
    step_size, inv_sqrt_bc2 = (f(x) for x in bias_corrections(t, float(lr), float(b1), float(b2)))
    m = b1 * m + (f(1) - b1) * g
    v = b2 * v + (f(1) - b2) * g * g
    p = p - step_size * (m / (np.sqrt(v) * inv_sqrt_bc2 + eps))
    assert p.dtype == m.dtype == v.dtype == f
    return p, m, v


def sgd_step(p, g, buf, lr, mu):
    """torch.optim.SGD (dampening 0, no Nesterov, no weight decay), float64: buf = mu * buf + g, p -= lr * buf; the buffer starts
    at zero (buf=None), which reproduces torch's first step (buf = g).  mu == 0: plain p -= lr * g.  Returns the new (p, buf)."""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    buf = np.zeros_like(p) if buf is None else np.asarray(buf, dtype=np.float64)
    buf = mu * buf + g
    return p - lr * buf, buf


def sgd_step_f32(p, g, buf, lr, mu):
    """sgd_step in float32 (the yardstick of the SGD kernel)."""
    f = np.float32
    p, g = np.asarray(p, dtype=f), np.asarray(g, dtype=f)
    buf = np.zeros_like(p) if buf is None else np.asarray(buf, dtype=f)
    buf = f(mu) * buf + g
    p = p - f(lr) * buf
    assert p.dtype == buf.dtype == f
    return p, buf


def adam_run(step, p0, grads, lr, b1, b2, eps, m0=None, v0=None, t0=0):
    """len(grads) steps of `step` (adam_step or adam_step_f32) from (p0, m0, v0) at step numbers t0 + 1, ...: the final (p, m, v)."""
    p = np.array(p0)
    m = np.zeros_like(p) if m0 is None else np.array(m0)
    v = np.zeros_like(p) if v0 is None else np.array(v0)
    for i, g in enumerate(grads):
        p, m, v = step(p, g, m, v, t0 + 1 + i, lr, b1, b2, eps)
    return p, m, v


def sgd_run(step, p0, grads, lr, mu):
    p, buf = np.array(p0), None
    for g in grads:
        p, buf = step(p, g, buf, lr, mu)
    return p, buf


def deviation(got, ref, sel=slice(None)):
    """How far the state `got` = (p, then moments) is from the float64 state `ref` over the elements `sel`: max |dp| (absolute),
    and for each moment max |d| relative to the reference's largest magnitude there."""
    out = []
    for i, (a, b) in enumerate(zip(got, ref)):
        a, b = np.asarray(a, dtype=np.float64)[sel], np.asarray(b, dtype=np.float64)[sel]
        d = float(np.abs(a - b).max())
        out.append(d if i == 0 else d / max(float(np.abs(b).max()), np.finfo(np.float64).tiny))
    return tuple(out)


def assert_within_yardstick(got, f32, ref, what, sel=slice(None)):
    """A kernel's state must stay within YARDSTICK_FACTOR x the deviation of the float32 restatement from float64, on the same
    inputs and the same elements; separately for p and for each moment.  There is no derivable elementwise ulp bound (m cancels to
    2e-4 relative on single elements when the gradient scale changes tenfold per step), hence a measured yardstick.  A skipped or
    doubled update is of the order of lr per step, tens of times above it.  Prints the figures, returns them."""
    dev, yard = deviation(got, ref, sel), deviation(f32, ref, sel)
    print(f"{what}: deviation from fp64 (p abs, moments rel) " + " ".join(f"{d:.3e}" for d in dev)
          + " | fp32 yardstick " + " ".join(f"{y:.3e}" for y in yard))
    for name, d, y in zip(("p", "m", "v"), dev, yard):
        assert np.isfinite(d) and d <= YARDSTICK_FACTOR * y, f"{what}: {name} is {d:.3e} from fp64, the fp32 yardstick is {y:.3e}"
    return dev, yard

"""What tests/test_loss_ref_host.py and tests/test_hip_loss_kernels.py share beside tests/loss_ref.py: the input sets of the device
tests, and torch's CPU fp32 evaluation of the kernels' own compositions -- the other fp32 implementation that the softmax /
cross-entropy budgets are measured on (loss_ref.budget) and that every BCE interval must contain."""
import numpy as np
import torch

import loss_ref as R

# ---- GAN term: input sets ------------------------------------------------------------------------------------------------------
# (h, w, seed) of every random map the device tests use; the seeds are those at which the reference's own interval of the summed loss
# stays inside GAN_MAX_HALF_WIDTH for all four targets (tests/test_loss_ref_host.py asserts it)
SINGLE_MAPS = ((1, 1, 1), (1, 1023, 1), (1, 1025, 1), (67, 67, 1))                       # around the 1024-thread sweep of the one-workgroup kernel
BWD_MAPS = ((130, 127, 1), (1, 16383, 1), (1, 16384, 1), (1, 16385, 1),                  # around one 16 * 256 * 4 = 16 384 sweep
            (1, 256 * 256 + 1, 1))                                                       # past the 256-workgroup cap of sgan_gan_loss_bwd
MULTI_MAPS = ((1, 1, 1), (67, 67, 1), (130, 127, 1), (2, 3, 1), (19, 21, 1), (67, 67, 2), (2, 3, 5), (19, 21, 2))
MULTI_LD = (1, 4, 4, 1, 4, 1, 4, 1)
MULTI_TARGETS = (1.0, 0.0, 0.9, 0.1, 1.0, 0.0, 0.9, 0.1)
MULTI_WEIGHTS = (0.5, -0.6, 2.0, 0.0, 1.0, 0.125, 3.0, 0.75)                             # a negative one and 0 among them


def random_gan_maps():
    seen = []
    for m in SINGLE_MAPS + BWD_MAPS + MULTI_MAPS:
        if m not in seen:
            seen.append(m)
    return seen


# ---- torch CPU fp32 compositions -----------------------------------------------------------------------------------------------
def f32_sigmoid(x):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return 1.0 / (1.0 + torch.exp(-t))


def f32_bce_term(p, t):
    t = torch.as_tensor(t, dtype=torch.float32)
    return -(t * torch.clamp(torch.log(p), min=-100.0) + (1.0 - t) * torch.clamp(torch.log1p(-p), min=-100.0))


def f32_bce_dterm(p, t):
    t = torch.as_tensor(t, dtype=torch.float32)
    return (p - t) / torch.clamp((1.0 - p) * p, min=1e-12)


def f32_gan_elem(x, target, scale):
    """(loss, gradient) per element in fp32, the kernels' expressions: d = dterm * go * ((1 - p) p)."""
    p = f32_sigmoid(x)
    go = torch.tensor(scale, dtype=torch.float32)
    return f32_bce_term(p, target).numpy(), (f32_bce_dterm(p, target) * go * ((1.0 - p) * p)).numpy()


def f32_bce01_elem(x, t, C):
    xs = torch.from_numpy(np.ascontiguousarray(x[:, :C], dtype=np.float32))
    ts = torch.from_numpy(np.ascontiguousarray(t[:, :C], dtype=np.float32))
    p, tg = (xs + 1.0) * 0.5, (ts + 1.0) * 0.5
    inv = torch.tensor(1.0 / xs.numel(), dtype=torch.float32)
    return f32_bce_term(p, tg).numpy(), (f32_bce_dterm(p, tg) * 0.5 * inv).numpy()


def _f32_lse(z):
    m = z.max(dim=1, keepdim=True).values
    return m + torch.log(torch.exp(z - m).sum(dim=1, keepdim=True))


def f32_softmax(z, C):
    zt = torch.from_numpy(np.ascontiguousarray(z[:, :C], dtype=np.float32))
    return torch.exp(zt - _f32_lse(zt)).numpy()


def f32_softmax_bwd(dp, p, C):
    d = torch.from_numpy(np.ascontiguousarray(dp[:, :C], dtype=np.float32))
    q = torch.from_numpy(np.ascontiguousarray(p[:, :C], dtype=np.float32))
    return (q * (d - (d * q).sum(dim=1, keepdim=True))).numpy()


def f32_ce(z, C, label, const_label, cw, gout):
    """(loss, gradient) of the kernels' composition in fp32, the two sums in float64 as the kernels keep them."""
    zt = torch.from_numpy(np.ascontiguousarray(z[:, :C], dtype=np.float32))
    n = zt.shape[0]
    y = np.full(n, int(const_label), dtype=np.int64) if label is None else np.asarray(label, dtype=np.int64)
    ok = (y >= 0) & (y < C)
    ys = torch.from_numpy(np.where(ok, y, 0))
    w = torch.from_numpy(np.where(ok, cw[np.where(ok, y, 0)] if cw is not None else np.float32(1.0), np.float32(0.0)).astype(np.float32))
    lse = _f32_lse(zt)
    zy = zt.gather(1, ys[:, None])
    den = float(w.double().sum())
    if den <= 0.0:
        return 0.0, np.zeros((n, C), np.float32)
    loss = float((w[:, None] * (lse - zy)).double().sum()) / den
    scale = torch.tensor(R.f32(gout) / den, dtype=torch.float32)
    onehot = torch.zeros(n, C).scatter_(1, ys[:, None], 1.0) * torch.from_numpy(ok.astype(np.float32))[:, None]
    return loss, ((w * scale)[:, None] * (torch.exp(zt - lse) - onehot)).numpy()


def softmax_bwd_inputs(z, C, seed):
    """(dp, p): an upstream gradient normal * 2 and the fp32 rounding of the float64 softmax, both [npix, C]."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((z.shape[0], C)) * 2.0).astype(np.float32), R.softmax_ref(z, C).astype(np.float32)

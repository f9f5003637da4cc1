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


def f32_ce(z, C, label, const_label, cw, gout, pixel_add=None):
    """(loss, gradient) of the kernels' composition in fp32, the two sums in float64 as the kernels keep them.  pixel_add: the
    pixel-weighted head's map, one fp32 addition to the weight of every pixel whose label is in range."""
    zt = torch.from_numpy(np.ascontiguousarray(z[:, :C], dtype=np.float32))
    n = zt.shape[0]
    y = np.full(n, int(const_label), dtype=np.int64) if label is None else np.asarray(label, dtype=np.int64)
    ok = (y >= 0) & (y < C)
    ys = torch.from_numpy(np.where(ok, y, 0))
    w = np.where(ok, cw[np.where(ok, y, 0)] if cw is not None else np.float32(1.0), np.float32(0.0)).astype(np.float32)
    if pixel_add is not None:
        w = np.where(ok, w + np.asarray(pixel_add, dtype=np.float32).reshape(-1), np.float32(0.0)).astype(np.float32)
    w = torch.from_numpy(w)
    lse = _f32_lse(zt)
    zy = zt.gather(1, ys[:, None])
    den = float(w.double().sum())
    if den <= 0.0:
        return 0.0, np.zeros((n, C), np.float32)
    loss = float((w[:, None] * (lse - zy)).double().sum()) / den
    scale = torch.tensor(R.f32(gout) / den, dtype=torch.float32)
    onehot = torch.zeros(n, C).scatter_(1, ys[:, None], 1.0) * torch.from_numpy(ok.astype(np.float32))[:, None]
    return loss, ((w * scale)[:, None] * (torch.exp(zt - lse) - onehot)).numpy()


# ---- the segmentation head, the --use_sigmoid_ss kernels, the factored loss (tests/test_hip_head_kernels.py) ----------------------
HEAD_PAIRS = ((1, 4), (3, 4), (2, 8), (12, 12), (16, 16), (5, 5))    # (C, ld): the 16-byte row forms 4 / 8 / 12 / 16 and a scalar one
HEAD_SMALL = ((5, 7), (257, 3))                                      # one partial workgroup; four workgroups, the last one partial
HEAD_LARGE = ((257, 256), (363, 362))                                # 257 workgroups: the slot sum's second trip; 514: past the 512 cap
HEAD_LARGE_PAIRS = ((3, 4), (16, 16), (5, 5))
BCEW_SHAPES = ((1, 16383), (1, 16384), (1, 16385), (130, 127))       # around the 64-workgroup sweep of sgan_bce_weighted_fwd
BCEW_PAIRS = ((1, 4, 4, 1), (3, 4, 8, 5), (2, 8, 4, 2), (5, 5, 8, 12))      # (C, ld of z / t, pld, dpld): ld != pld != dpld
BCEW_BWD_CAP_NPIX = 1024 * 256 + 3
SIGMOID_CAP_NPIX = 2048 * 256 + 3
HEAD_GOUT = 1.7


def head_shapes():
    """(H, W, C, ld) of every seg-head case."""
    return [(H, W, C, ld) for H, W in HEAD_SMALL for C, ld in HEAD_PAIRS] + [(H, W, C, ld) for H, W in HEAD_LARGE for C, ld in HEAD_LARGE_PAIRS]


def head_seed(H, W, C):
    return H * 1000 + W * 10 + C


def nw_of(which, C):
    return {"0": 0, "2": min(2, C), "1": 1, "C": C}[which]


def f32_bcew(p, t, C, cw, nw, gout, chain):
    """(weighted loss terms [npix, C], gradient [npix, C]) of the kernels' expressions in fp32 at the fp32 probabilities p."""
    p = torch.from_numpy(np.ascontiguousarray(np.asarray(p)[:, :C], dtype=np.float32))
    tt = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
    w = torch.ones(p.shape[0])
    for i in range(nw):
        w = w + tt[:, i] * (float(cw[i]) - 1.0)
    tc = tt[:, :C]
    go = torch.tensor(R.f32(gout), dtype=torch.float32) / torch.tensor(float(p.numel()), dtype=torch.float32)
    g = (w * go)[:, None] * (p - tc) / torch.clamp((1.0 - p) * p, min=1e-12)
    if chain:
        g = g * p * (1.0 - p)
    return (w[:, None] * f32_bce_term(p, tc)).numpy(), g.numpy()


def factd_composition(l1s, l2s, ups, targets, weights, mode, dtype, upstream=1.0):
    """(each, total, [dl1], [dl2], [pred], [padded upsampled map]) of the torch composition on the CPU in `dtype`: sigmoid ->
    F.interpolate(bilinear, align_corners=False) -> F.pad(reflect) -> product -> BCE / MSE -> backward()."""
    import torch.nn.functional as F
    sig1, sig2, mse = mode
    a = [torch.from_numpy(np.asarray(x)).to(dtype)[None, None].requires_grad_(True) for x in l1s]
    b = [torch.from_numpy(np.asarray(x)).to(dtype)[None, None].requires_grad_(True) for x in l2s]
    each, preds, qs = [], [], []
    for x, y, up, tg in zip(a, b, ups, targets):
        p1 = torch.sigmoid(x) if sig1 else x
        p2 = torch.sigmoid(y) if sig2 else y
        if up == 2:
            p1 = F.interpolate(p1, scale_factor=2, mode="bilinear", align_corners=False)
        pads = R.factd_pad_split(p2.shape[2] - p1.shape[2], p2.shape[3] - p1.shape[3])
        q = F.pad(p1, pads, mode="reflect") if any(pads) else p1
        pred = q * p2
        t = torch.full_like(pred, R.f32(tg))
        each.append(F.mse_loss(pred, t) if mse else F.binary_cross_entropy(pred, t))
        preds.append(pred.detach()[0, 0].numpy())
        qs.append(q.detach()[0, 0].numpy())
    total = sum(e * R.f32(w) for e, w in zip(each, weights))      # what the weights are once they have crossed the C ABI as floats
    (total * R.f32(upstream)).backward()
    return (np.array([float(e.detach()) for e in each]), float(total.detach()), [x.grad[0, 0].numpy() for x in a], [y.grad[0, 0].numpy() for y in b], preds, qs)


def factd_reference(shape, mode, target, weight, gout, seed):
    """(l1, l2, the loss_ref.factd_term dict, torch's fp32 composition): in BCE mode the candidate ulps of p and q are measured on
    that composition (loss_ref.candidate_ulps)."""
    l1, l2 = R.factd_logits(shape, seed)
    c32 = factd_composition([l1], [l2], [shape[2]], [target], [weight], mode, torch.float32, gout)
    kp = kq = None
    if not mode[2]:
        pt = R.factd_term(l1, l2, shape[2], target, mode, weight, gout)
        kp, kq = R.candidate_ulps(c32[4][0], pt["p"]), R.candidate_ulps(c32[5][0], pt["q"])
    ref = R.factd_term(l1, l2, shape[2], target, mode, weight, gout, kp, kq)
    ref["kp"], ref["kq"] = kp, kq
    return l1, l2, ref, c32


def softmax_bwd_inputs(z, C, seed):
    """(dp, p): an upstream gradient normal * 2 and the fp32 rounding of the float64 softmax, both [npix, C]."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((z.shape[0], C)) * 2.0).astype(np.float32), R.softmax_ref(z, C).astype(np.float32)

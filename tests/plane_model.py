"""CPU model of the 16-bit plane arithmetic of the conv kernels (SGAN_MATH_BF16X3 / SGAN_MATH_BF16X1), in fp64.

The kernels cut every fp32 operand into 16-bit planes hi = r16(x), lo = r16(x - hi) and form a_hi b_hi + a_hi b_lo + a_lo b_hi
(bf16x3) or a_hi b_hi alone (bf16x1) with fp32 accumulation:
  forward          fp16 planes of the prologue output (unscaled) x fp16 planes of w * 2^10, the accumulator times 2^-10;
  backward-data    bf16 planes of dY and w; with a published max|dY|: fp16 planes of dY * 2^s (s = sg_f16_shift) x fp16 planes of
                   w * 2^10, the accumulator times 2^(-10 - s);
  backward-weight  bf16 planes of dY and of the prologue output; with a published maximum fp16 planes of dY * 2^s and of the
                   (unscaled) prologue output, the accumulator times 2^-s.
model_* return the exact (fp64) sum of the plane products the kernel forms, magnitude_* the same sum over the planes' absolute
values (M = sum |a| |b| per result element, what a bound on fp32 accumulation error is stated in), truth_* the fp64 result of the
unrounded operands.  The operand domains the documentation states (include/sgan_hip.h) are the constants at the end;
tests/test_plane_range_host.py derives them from a sweep of this model."""
import math

import numpy as np
import torch
import torch.nn.functional as F

W_SHIFT = 10       # SGAN_F16_WEIGHT_SHIFT
MODES = ("bf16x3", "bf16x1")


def _f16(t, shift=0):
    """fp16 of t * 2^shift (round to nearest even, subnormals kept: v_cvt_pk_f16_f32), as a float64 tensor of the UNSCALED value."""
    return (t.float() * (2.0 ** shift)).half().double() / (2.0 ** shift)


def _bf16(t):
    return t.float().bfloat16().double()


def _shift(amax):
    """sg_f16_shift: 2^s brings max|dY| under 2^15."""
    e = int((np.float32(amax).view(np.uint32) >> 23) & 255)
    return max(-100, min(100, 141 - e)) if e else 0


def _prologue(x, st, gamma, beta, norm, act, count):
    """The kernels' normalise-on-load in fp32: mean / rstd from the fp64 sums (sg_mean_rstd), y = x * sc + sh, activation."""
    C = x.shape[1]
    y = x.float()
    if norm:
        Cs = st.numel() // 2
        s, q = st[:C].double().cpu(), st[Cs: Cs + C].double().cpu()
        m = s / count
        var = (q / count - m * m).clamp_min(0.0)
        mean, rstd = m.float(), (1.0 / torch.sqrt(var + 1e-5)).float()
        g = gamma.float() if gamma is not None else torch.ones(C)
        b = beta.float() if beta is not None else torch.zeros(C)
        sc = g * rstd
        sh = b - mean * sc
        y = y * sc.view(1, C, 1, 1) + sh.view(1, C, 1, 1)
    if act == 1:
        y = torch.clamp_min(y, 0.0)
    elif act == 2:
        y = torch.maximum(y, y * torch.tensor(0.2, dtype=torch.float32))
    return y


def _conv(tr, a, w, b, s, p):
    return F.conv_transpose2d(a, w, b, stride=s, padding=p) if tr else F.conv2d(a, w, b, stride=s, padding=p)


def _dgrad_ref(tr, dy, w, s, p, xshape):
    x = torch.zeros(xshape, dtype=torch.float64, requires_grad=True)
    (_conv(tr, x, w, None, s, p) * dy).sum().backward()
    return x.grad


def _wgrad_ref(tr, a, dy, wshape, s, p):
    w = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
    (_conv(tr, a, w, None, s, p) * dy).sum().backward()
    return w.grad


# ---- two-plane splits: float64 tensors of the UNSCALED planes (hi + lo ~ t) ----

def split_f16(t, shift=0):
    """fp16 planes of t * 2^shift as sg_split8<true> forms them: the scaling and the subtraction in fp32 (both exact while
    nothing overflows), each plane rounded to nearest even with fp16 subnormals kept."""
    xs = t.float() * (2.0 ** shift)
    hi = xs.half()
    lo = (xs - hi.float()).half()
    return hi.double() / (2.0 ** shift), lo.double() / (2.0 ** shift)


def split_bf16(t):
    x = t.float()
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    return hi.double(), lo.double()


def _pairs(mode, a, b):
    """The plane products a mode forms, as (a plane, b plane) pairs; a, b = (hi, lo)."""
    if mode == "bf16x3":
        return [(a[0], b[0]), (a[0], b[1]), (a[1], b[0])]
    if mode == "bf16x1":
        return [(a[0], b[0])]
    raise ValueError(mode)


def _bwd_planes(g, other, amax, other_shift):
    """Planes of a gradient and of the operand it meets: bf16 unless the gradient's maximum was published."""
    if amax is None:
        return split_bf16(g), split_bf16(other)
    return split_f16(g, _shift(amax)), split_f16(other, other_shift)


def _fwd(mode, tr, a, w, s, p, mag):
    f = torch.abs if mag else (lambda t: t)
    return sum(_conv(tr, f(pa), f(pw), None, s, p) for pa, pw in _pairs(mode, split_f16(a), split_f16(w, W_SHIFT)))


def _dgrad(mode, tr, dy, w, s, p, xshape, amax, mag):
    f = torch.abs if mag else (lambda t: t)
    pd, pw = _bwd_planes(dy, w, amax, W_SHIFT)
    return sum(_dgrad_ref(tr, f(d), f(ww), s, p, xshape) for d, ww in _pairs(mode, pd, pw))


def _wgrad(mode, tr, a, dy, wshape, s, p, amax, mag):
    f = torch.abs if mag else (lambda t: t)
    pd, pa = _bwd_planes(dy, a, amax, 0)
    return sum(_wgrad_ref(tr, f(aa), f(d), wshape, s, p) for d, aa in _pairs(mode, pd, pa))


def model_fwd(mode, tr, a, w, b, s, p):
    """a: the fp32 prologue output; b: bias or None (added in fp64)."""
    y = _fwd(mode, tr, a, w, s, p, False)
    return y if b is None else y + b.double().view(1, -1, 1, 1)


def model_dgrad(mode, tr, dy, w, s, p, xshape, amax=None):
    """The raw backward-data product (no epilogue); amax: the published max|dY| (fp16 planes) or None (bf16 planes)."""
    return _dgrad(mode, tr, dy, w, s, p, xshape, amax, False)


def model_wgrad(mode, tr, a, dy, wshape, s, p, amax=None):
    return _wgrad(mode, tr, a, dy, wshape, s, p, amax, False)


def magnitude_fwd(mode, tr, a, w, s, p):
    return _fwd(mode, tr, a, w, s, p, True)


def magnitude_dgrad(mode, tr, dy, w, s, p, xshape, amax=None):
    return _dgrad(mode, tr, dy, w, s, p, xshape, amax, True)


def magnitude_wgrad(mode, tr, a, dy, wshape, s, p, amax=None):
    return _wgrad(mode, tr, a, dy, wshape, s, p, amax, True)


def truth_fwd(tr, a, w, b, s, p):
    return _conv(tr, a.double(), w.double(), None if b is None else b.double(), s, p)


def truth_dgrad(tr, dy, w, s, p, xshape):
    return _dgrad_ref(tr, dy.double(), w.double(), s, p, xshape)


def truth_wgrad(tr, a, dy, wshape, s, p):
    return _wgrad_ref(tr, a.double(), dy.double(), wshape, s, p)


def rel_max(a, b):
    """max-norm relative error (hip_utils.rel, without its GPU imports)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def shift_restated(amax):
    """"amax * 2^s in [2^14, 2^15)" stated directly, with the kernel's clamp to +-100 and its answer 0 for zero / denormal maxima."""
    a = float(np.float32(amax))
    if a < 2.0 ** -126:
        return 0
    if math.isinf(a):
        return -100
    m, ex = math.frexp(a)          # a = m * 2^ex, m in [0.5, 1): a in [2^(ex-1), 2^ex)
    s = 15 - ex
    assert 2.0 ** 14 <= math.ldexp(a, s) < 2.0 ** 15
    return max(-100, min(100, s))


# ---- the layer of the host sweep and of shape A of tests/test_hip_plane_range.py, with the suite's operand distributions ----

A_SHAPE = ("conv", 4, 1, 2, 32, 64, 17, 19, None, 2)      # kind, k, s, p, cin, cout, H, W, norm, act


def shape_a_operands(seed=41):
    """x ~ 1.5 N(0,1) + 0.3, w ~ 0.05 N(0,1), b ~ 0.1 N(0,1), dY ~ N(0,1) at scale 1 (what every GPU parity test draws)."""
    kind, k, s, p, cin, cout, H, W, norm, act = A_SHAPE
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1, cin, H, W, generator=g) * 1.5 + 0.3
    w = torch.randn(cout, cin, k, k, generator=g) * 0.05
    b = torch.randn(cout, generator=g) * 0.1
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    dy = torch.randn(1, cout, Ho, Wo, generator=g)
    return x, w, b, dy


def pow2(t, e):
    """t * 2^e as an fp32 tensor (exact up to overflow / underflow of fp32)."""
    return (t.double() * 2.0 ** e).float()


# ---- the documented operand domains (include/sgan_hip.h): [low, high] of an operand's MAXIMUM MAGNITUDE ----
# All of it is model-derived: test_plane_range_host.py sweeps this model on the layer above and checks every low edge against the
# sweep (the last power of two that passes, moved inwards by one more); the high edges are fp16's largest finite value.
# "contract": the result stays within 1e-3 (max-norm, relative) of fp64 -- bf16x3 on either kind of plane, bf16x1 on fp16 planes
#             (bf16x1 on bf16 planes is 2^-9 per operand, ~2.5e-3 of the result at every scale: never inside).
# "fp32":     bf16x3 on fp16 planes is fp32-equivalent: the plane rounding stays under 1e-6 of the result, the exact-fp32 kernel's
#             own distance from fp64 (2e-7 .. 1.1e-6), so the sum stays under the suite's 3e-6 gate.
FP32_EQUIV = 1e-6
CONTRACT = 1e-3
ACT_OVERFLOW = 65504.0            # fp16 planes of the unscaled prologue output: larger magnitudes round to infinity
W_OVERFLOW = 64.0                 # fp16 planes of w * 2^10: |w| < 64
ACT_CONTRACT = (2.0 ** -11, ACT_OVERFLOW)      # fp16-plane paths: forward, backward-weight with a published maximum
ACT_FP32 = (2.0 ** -2, ACT_OVERFLOW)
W_CONTRACT = (2.0 ** -22, 2.0 ** 5)            # fp16 planes of w * 2^10 (forward, backward-data with a published maximum); 2^5: the
W_FP32 = (2.0 ** -12, 2.0 ** 5)                # last power of two under W_OVERFLOW
G_CONTRACT = (2.0 ** -112, 2.0 ** 115)         # max|dY|, published (fp16 planes of dY * 2^s; above 2^115 the clamp of s at -100 lets
G_FP32 = (2.0 ** -102, 2.0 ** 115)             # dY * 2^s pass 65504) or not (bf16 planes: contract only)


def inside(dom, amax):
    return dom[0] <= float(amax) <= dom[1]


def contract_applies(mode, planes):
    """planes: "f16" or "bf16"."""
    return mode == "bf16x3" or planes == "f16"

"""Plain numpy reference of the resampling kernels of csrc/sgan_ew.hip: the Gaussian pre-filter (sgan_gauss_down_*), the x2 bilinear
upsampling (sgan_bilinear_up2_*) and the label pyramid (sgan_avgpool_pyramid_*), each with its adjoint.  No torch, no GPU: the tests
compare the kernels with this, never the other way round (tests/test_resample_ref_host.py holds it to torch.nn.functional and
torch.autograd on its own).  Every function is written from the definition of the operation, none from a kernel.

Every function takes `out_dtype`.  np.float64 is the reference: the operation itself.  np.float32 is the YARDSTICK
(tests/pad_norm_ref.py): the same sum with every product and every partial sum rounded to float32, in the order `reverse` / `flat`
selects.  Every function has a `*_terms` companion: sum |terms| per output element in float64, the T of the a-priori bounds
|fp32 sum in any order - exact| <= gamma_n T that tests/test_hip_resample*.py impose (`bound_*` below state n per kernel).

Arrays are NHWC, [H, W, C].  The Gaussian functions take the LOGICAL channels only (C = Creal, taps [C, k, k]); what the kernels do
with the padding channels of a stored buffer is the tests' business."""
import numpy as np

U32 = 2.0 ** -24            # unit roundoff of float32


# ---- Gaussian pre-filter: depthwise strided correlation with zero padding -----------------------------------------------------------
def gauss_out_size(n, k, pad, s):
    return (n + 2 * pad - k) // s + 1


def _tap_order(k, reverse):
    order = [(ky, kx) for ky in range(k) for kx in range(k)]
    return order[::-1] if reverse else order


def _gauss_fwd(x, taps, k, pad, s, dtype, reverse):
    H, W, C = x.shape
    Ho, Wo = gauss_out_size(H, k, pad, s), gauss_out_size(W, k, pad, s)
    assert taps.shape == (C, k, k) and Ho >= 1 and Wo >= 1
    xp = np.zeros((H + 2 * pad, W + 2 * pad, C), dtype=dtype)
    xp[pad: pad + H, pad: pad + W] = x
    out = np.zeros((Ho, Wo, C), dtype=dtype)
    for ky, kx in _tap_order(k, reverse):      # out[oy, ox, c] = sum_{ky, kx} taps[c, ky, kx] * xp[oy s + ky, ox s + kx, c]
        out = out + taps[:, ky, kx] * xp[ky: ky + s * (Ho - 1) + 1: s, kx: kx + s * (Wo - 1) + 1: s]
    assert out.dtype == dtype
    return out


def gauss_down(x, taps, k, pad, s, out_dtype=np.float64, reverse=False):
    """out[Ho, Wo, C], Ho = (H + 2 pad - k) // s + 1: taps[c] correlated (not convolved) with channel c of the zero-padded image."""
    return _gauss_fwd(np.asarray(x, dtype=np.float32).astype(out_dtype), np.asarray(taps, dtype=np.float32).astype(out_dtype), k, pad, s,
                      out_dtype, reverse)


def gauss_down_terms(x, taps, k, pad, s):
    return _gauss_fwd(np.abs(np.asarray(x, dtype=np.float32).astype(np.float64)), np.abs(np.asarray(taps, dtype=np.float32).astype(np.float64)),
                      k, pad, s, np.float64, False)


def _gauss_adj(dout, taps, k, pad, s, H, W, dtype, reverse):
    Ho, Wo, C = dout.shape
    assert (Ho, Wo) == (gauss_out_size(H, k, pad, s), gauss_out_size(W, k, pad, s)) and taps.shape == (C, k, k)
    dp = np.zeros((H + 2 * pad, W + 2 * pad, C), dtype=dtype)
    for ky, kx in _tap_order(k, reverse):      # every (tap, output) pair adds to the one padded pixel it read; a pixel gets one term per tap
        dp[ky: ky + s * (Ho - 1) + 1: s, kx: kx + s * (Wo - 1) + 1: s] += taps[:, ky, kx] * dout
    assert dp.dtype == dtype
    return dp[pad: pad + H, pad: pad + W].copy()


def gauss_down_adj(dout, taps, k, pad, s, H, W, base=None, out_dtype=np.float64, reverse=False):
    """din[H, W, C] = (base +) the transpose of gauss_down applied to dout; rows / columns no output reads get exactly 0."""
    d = _gauss_adj(np.asarray(dout, dtype=np.float32).astype(out_dtype), np.asarray(taps, dtype=np.float32).astype(out_dtype), k, pad, s, H, W,
                   out_dtype, reverse)
    if base is not None:
        d = np.asarray(base, dtype=np.float32).astype(out_dtype) + d
    assert d.dtype == out_dtype
    return d


def gauss_down_adj_terms(dout, taps, k, pad, s, H, W, base=None):
    t = _gauss_adj(np.abs(np.asarray(dout, dtype=np.float32).astype(np.float64)), np.abs(np.asarray(taps, dtype=np.float32).astype(np.float64)),
                   k, pad, s, H, W, np.float64, False)
    return t if base is None else t + np.abs(np.asarray(base, dtype=np.float32).astype(np.float64))


def gauss_ring(Ho, Wo, pad, s):
    """Boolean [Ho, Wo]: the first and last ceil(pad / s) + 1 rows and columns (the outputs and gradients the zero padding shapes)."""
    r = -(-pad // s) + 1
    m = np.zeros((Ho, Wo), dtype=bool)
    m[:r] = m[-r:] = True
    m[:, :r] = m[:, -r:] = True
    return m


def bound_gauss_fwd(k, T):
    """k^2 products and k^2 - 1 additions in any order: gamma_{k^2} T <= (k^2 + 1) u T."""
    return (k * k + 1) * U32 * T


def bound_gauss_bwd(ks, T, base=False):
    """ks: the (k, s) of every job summed into the gradient.  n = sum ceil(k / s)^2 taps reach an image pixel (and the base is one
    more term): n products and n - 1 additions in any order, (n + 2) u T."""
    n = sum((-(-k // s)) ** 2 for k, s in ks) + (1 if base else 0)
    return (n + 2) * U32 * T


# ---- bilinear x2, align_corners = False -------------------------------------------------------------------------------------------
def _lin(n):
    """(i0, i1, w0, w1) for the 2 n outputs of one axis: source coordinate (o + 0.5) / 2 - 0.5 clamped at 0, i0 its floor, i1 = i0 + 1
    clamped to the last sample, w1 the fraction."""
    src = np.maximum((np.arange(2 * n) + 0.5) / 2.0 - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    w1 = src - i0
    return i0, i1, 1.0 - w1, w1


def _bil_terms(x, dtype):
    """The four (weight [2H, 2W, 1], value [2H, 2W, C]) terms of every output element."""
    H, W, _ = x.shape
    y0, y1, a0, a1 = _lin(H)
    x0, x1, b0, b1 = _lin(W)
    out = []
    for yi, wy in ((y0, a0), (y1, a1)):
        for xi, wx in ((x0, b0), (x1, b1)):
            w = (wy[:, None] * wx[None, :]).astype(dtype)[..., None]      # 9/16, 3/16, 1/16, 3/4, 1/4, 1, 0: exact in both types
            out.append((w, x[yi[:, None], xi[None, :], :]))
    return out


def bilinear_up2(x, out_dtype=np.float64, reverse=False):
    """out[2H, 2W, C] = sum of the four (1 - ly | ly) (1 - lx | lx) x[y0 | y1, x0 | x1] terms: four products, three additions."""
    x = np.asarray(x, dtype=np.float32).astype(out_dtype)
    terms = _bil_terms(x, out_dtype)
    out = None
    for w, v in (terms[::-1] if reverse else terms):
        out = w * v if out is None else out + w * v
    assert out.dtype == out_dtype
    return out


def bilinear_up2_terms(x):
    x = np.abs(np.asarray(x, dtype=np.float32).astype(np.float64))
    return sum(w * v for w, v in _bil_terms(x, np.float64))


def _scatter_axis0(d, n, dtype, reverse):
    """The transpose of the one-axis interpolation along axis 0: [2n, ...] -> [n, ...], each output row added to its two sources."""
    i0, i1, w0, w1 = _lin(n)
    out = np.zeros((n,) + d.shape[1:], dtype=dtype)
    rows = range(2 * n - 1, -1, -1) if reverse else range(2 * n)
    for o in rows:
        out[i0[o]] += dtype(w0[o]) * d[o]
        out[i1[o]] += dtype(w1[o]) * d[o]
    assert out.dtype == dtype
    return out


def _bil_adj(d, dtype, reverse):
    Ho, Wo, _ = d.shape
    t = _scatter_axis0(d, Ho // 2, dtype, reverse)
    return _scatter_axis0(t.transpose(1, 0, 2), Wo // 2, dtype, reverse).transpose(1, 0, 2).copy()


def bilinear_up2_adj(dout, out_dtype=np.float64, reverse=False):
    """din[H, W, C]: the transpose of bilinear_up2 (the interpolation is separable, so its transpose is too): up to 16 terms."""
    return _bil_adj(np.asarray(dout, dtype=np.float32).astype(out_dtype), out_dtype, reverse)


def bilinear_up2_adj_terms(dout):
    return _bil_adj(np.abs(np.asarray(dout, dtype=np.float32).astype(np.float64)), np.float64, False)


def ring1(H, W):
    """Boolean [H, W]: the outermost row and column on every side."""
    m = np.zeros((H, W), dtype=bool)
    m[0] = m[-1] = True
    m[:, 0] = m[:, -1] = True
    return m


def bound_bilinear_fwd(T):
    """Four products and three additions, with or without FMA contraction, nested or flat: gamma_7 T <= 8 u T."""
    return 8 * U32 * T


def bound_bilinear_bwd(T):
    """16 terms, each the product of two weights and a value, 15 additions in any order: (16 + 2 + 2) u T."""
    return 20 * U32 * T


# ---- label pyramid: level s = AvgPool2d(2^(s+1)) -------------------------------------------------------------------------------------
LEVELS = 6


def _blocks(x, b):
    H, W, C = x.shape
    return x.reshape(H // b, b, W // b, b, C).transpose(0, 2, 4, 1, 3).reshape(H // b, W // b, C, b * b)


def avgpool_pyramid(x, out_dtype=np.float64, flat=True):
    """[level 0 .. 5]; level s [H >> (s+1), W >> (s+1), C] is the mean over 2^(s+1) x 2^(s+1) squares.  flat: every level summed from
    the pixels and scaled once (the definition).  not flat: each level the 2 x 2 mean of the one before (another order of the same sum)."""
    x = np.asarray(x, dtype=np.float32).astype(out_dtype)
    out = []
    for s in range(LEVELS):
        if flat:
            b = 2 << s
            v = _blocks(x, b).sum(axis=-1, dtype=out_dtype) * out_dtype(1.0 / (b * b))
        else:
            p = x if s == 0 else out[-1]
            v = out_dtype(0.25) * ((p[0::2, 0::2] + p[0::2, 1::2]) + (p[1::2, 0::2] + p[1::2, 1::2]))
        assert v.dtype == out_dtype
        out.append(v)
    return out


def avgpool_pyramid_terms(x):
    return avgpool_pyramid(np.abs(np.asarray(x, dtype=np.float32)), np.float64, True)


def _spread(d, b, dtype):
    """dl[p >> log2 b] / b^2 for every pixel p."""
    return np.repeat(np.repeat(d, b, axis=0), b, axis=1) * dtype(1.0 / (b * b))


def avgpool_pyramid_adj(dlevels, H, W, base=None, out_dtype=np.float64, reverse=False):
    """dlabel[H, W, C] = (base +) sum over the levels given (None: absent) of dlevels[s][y >> (s+1), x >> (s+1)] / 4^(s+1)."""
    assert len(dlevels) == LEVELS
    C = next(d.shape[2] for d in dlevels if d is not None)
    acc = np.zeros((H, W, C), dtype=out_dtype) if base is None else np.asarray(base, dtype=np.float32).astype(out_dtype)
    order = range(LEVELS - 1, -1, -1) if reverse else range(LEVELS)
    for s in order:
        if dlevels[s] is not None:
            acc = acc + _spread(np.asarray(dlevels[s], dtype=np.float32).astype(out_dtype), 2 << s, out_dtype)
    assert acc.dtype == out_dtype
    return acc


def avgpool_pyramid_adj_terms(dlevels, H, W, base=None):
    return avgpool_pyramid_adj([None if d is None else np.abs(np.asarray(d, dtype=np.float32)) for d in dlevels], H, W,
                               None if base is None else np.abs(np.asarray(base, dtype=np.float32)))


def bound_pyramid_fwd(s, T):
    """Level s is a sum of 4^(s+1) terms taken as a tree of 2 x 2 sums: 2 (s + 1) additions deep, the scalings by 1/4 exact:
    gamma_{2(s+1)} T <= 3 (s + 1) u T.  (A flat running sum is not covered a priori; the host test measures it on the test data.)"""
    return 3 * (s + 1) * U32 * T


def bound_pyramid_bwd(T):
    """At most six levels and the base, the scalings by 4^-(s+1) exact: six additions, gamma_6 T <= 8 u T."""
    return 8 * U32 * T

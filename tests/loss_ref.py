"""Plain numpy float64 references of the loss kernels of csrc/sgan_ew.hip: the GAN term (sgan_gan_loss_fwd / _bwd / _multi_fwd /
_multi_bwd), the image losses (sgan_l1w_fwd, sgan_bce01_fwd), the class-weighted cross-entropy (sgan_ce_fwd / _bwd) and the channel
softmax (sgan_softmax_fwd / _bwd).  Neither torch nor the library is imported.  tests/test_loss_ref_host.py holds these functions to
torch's double autograd on the CPU; tests/test_hip_loss_kernels.py compares the kernels with them.

The BCE terms are references with an interval.  BCELoss(sigmoid(x), t) is ill-conditioned in the fp32 rounding of p = sigmoid(x): at
x = 12 one ulp of p moves log1p(-p) by 1 %, and near x = 17 p may or may not round to 1.  So the float64 formula is evaluated at every
fp32 value p32 + k ulp, k = -3 .. 3 (clipped to [0, 1]; p32 the fp32 rounding of the float64 sigmoid; 3 = the standalone sigmoid's
pinned 2.01 ulp, tests/test_hip_small_kernels.py, rounded up), the minimum and maximum are taken per element and widened by
ELEM_ROUNDINGS fp32 roundings of the value plus 2^-126 (`widen`).  A mean must lie in the mean of the intervals, widened by one
rounding of the result (`mean_interval`).

Also here, because the host test and the device test need the very same ones: the inputs (`gan_logits`, `image_inputs`, `ce_inputs`)
and the error measure of the softmax / cross-entropy budgets (`scaled_ulp_error`, `budget`)."""
import numpy as np

U = 2.0 ** -24                                   # one fp32 rounding (unit roundoff, round to nearest)
MIN_NORMAL = float(np.finfo(np.float32).tiny)    # 2^-126
P_ULPS = 3                                       # candidates p32 - 3 ulp .. p32 + 3 ulp
ELEM_ROUNDINGS = 4
CLAMP = float(np.float32(1e-12))                 # the kernels' 1e-12f: torch's clamp of p (1 - p), as an fp32 constant


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def f32(v):
    """What a Python float is once it has crossed the C ABI as a float."""
    return float(np.float32(v))


def widen(lo, hi, k=ELEM_ROUNDINGS):
    lo, hi = _f64(lo), _f64(hi)
    return lo - (k * U * np.abs(lo) + MIN_NORMAL), hi + (k * U * np.abs(hi) + MIN_NORMAL)


def inside(got, lo, hi):
    got = _f64(got)
    return (got >= lo) & (got <= hi)


def mean_interval(lo, hi, n=None):
    """The interval of a mean over `n` (default: all) elements with the given intervals, widened by one fp32 rounding of the result."""
    n = lo.size if n is None else n
    return widen(_f64(lo).sum() / n, _f64(hi).sum() / n, 1)


# ---- sigmoid and the BCE term --------------------------------------------------------------------------------------------------
def sigmoid64(x):
    x = _f64(x)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def p_candidates(p64, saturated_is_point=False, ulps=None):
    """[2 * ulps + 2, ...] float64 (ulps: P_ULPS unless given): the fp32 values p32 + k ulp around the fp32 rounding of p64, clipped to [0, 1], and one more
    row that holds 0 where p32 is below 2^-126 (x < -87.3: an fp32 division may flush a denormal quotient, as torch's CPU kernels
    do; the same allowance as the 2^-126 floor of `widen`, taken on p) and p32 elsewhere.  With
    saturated_is_point, an element whose p64 is exactly 0 or 1 has that value in every row (sgan_bce01_fwd at the planted x = -+1: its
    p = (x + 1) / 2 is one correctly rounded addition and an exact halving, so an exact 0 or 1 leaves no freedom)."""
    p64 = _f64(p64)
    p32 = p64.astype(np.float32)
    rows = [p32]
    up, dn = p32, p32
    for _ in range(P_ULPS if ulps is None else int(ulps)):
        up = np.nextafter(up, np.float32(2.0))
        dn = np.nextafter(dn, np.float32(-1.0))
        rows += [up, dn]
    rows.append(np.where(p32 < np.float32(MIN_NORMAL), np.float32(0.0), p32))      # a denormal p may be flushed to zero on either side
    c = np.clip(np.stack(rows).astype(np.float64), 0.0, 1.0)
    if saturated_is_point:
        c = np.where((p64 == 0.0) | (p64 == 1.0), p64, c)
    return c


def bce_term(p, t):
    """torch's BCELoss term, both logs clamped at -100."""
    p, t = _f64(p), _f64(t)
    with np.errstate(divide="ignore"):
        lp = np.maximum(np.log(p), -100.0)
        lq = np.maximum(np.log1p(-p), -100.0)
    return -(t * lp + (1.0 - t) * lq)


def bce_dterm(p, t):
    """torch's d BCE / d p = (p - t) / max(p (1 - p), 1e-12)."""
    p, t = _f64(p), _f64(t)
    return (p - t) / np.maximum(p * (1.0 - p), CLAMP)


def _minmax(v):
    return widen(v.min(axis=0), v.max(axis=0))


# ---- the GAN term --------------------------------------------------------------------------------------------------------------
def gan_loss_elem(x, target, mode):
    """(lo, hi) of every element's loss.  mode 0: BCELoss(sigmoid(x), t), the interval; mode 1: (x - t)^2, lo == hi, not widened."""
    x, t = _f64(x), f32(target)
    if mode == 1:
        v = (x - t) ** 2
        return v, v
    return _minmax(bce_term(p_candidates(sigmoid64(x)), t))


def gan_grad_elem(x, target, mode, scale):
    """(lo, hi) of d (scale * sum of the element losses) / d x.  mode 0: (p - t) / max(p (1 - p), 1e-12) * p (1 - p) * scale, the
    interval; mode 1: 2 (x - t) scale, lo == hi, not widened.  scale = weight / npix (times the upstream gradient), in float64."""
    x, t = _f64(x), f32(target)
    if mode == 1:
        v = 2.0 * (x - t) * scale
        return v, v
    p = p_candidates(sigmoid64(x))
    return _minmax(bce_dterm(p, t) * (p * (1.0 - p)) * scale)


GAN_BLOCKS = 16                                  # sg_gan_loss_multi_fwd_kernel: workgroups (and fp64 slots) per term


def gan_slot_of(npix):
    """Which of a term's GAN_BLOCKS fp64 slots element i is summed into: workgroup b takes i with (i mod 4096) // 256 == b."""
    return (np.arange(npix) % (GAN_BLOCKS * 256)) // 256


def gan_slot_intervals(lo, hi):
    """(lo, hi) [GAN_BLOCKS] of the slot partials: sums of the element intervals, widened by the float64 summation's n 2^-53."""
    lo, hi = _f64(lo).reshape(-1), _f64(hi).reshape(-1)
    s = gan_slot_of(lo.size)
    slo = np.array([lo[s == b].sum() for b in range(GAN_BLOCKS)])
    shi = np.array([hi[s == b].sum() for b in range(GAN_BLOCKS)])
    e = lo.size * 2.0 ** -53
    return slo - e * np.abs(slo), shi + e * np.abs(shi)


def weighted_total_interval(each_lo, each_hi, weights):
    """sum_i w_i each_i for each_i anywhere in its interval, widened by one fp32 rounding of the result."""
    w = _f64([f32(v) for v in weights])
    a, b = w * _f64(each_lo), w * _f64(each_hi)
    return widen(np.minimum(a, b).sum(), np.maximum(a, b).sum(), 1)


GAN_TARGETS = (1.0, 0.0, 0.9, 0.1)
GAN_PLANTED = (17.0, -17.0, 20.0, -20.0, 30.0, -30.0, 40.0, -40.0, 88.0, -88.0, 100.0, -100.0, 104.0, -104.0, 120.0, -120.0)
GAN_MAX_HALF_WIDTH = 2e-5      # of the summed loss of a random map: no interval may grow wide enough to hide a wrong sum


def gan_logits(h, w, seed=1):
    """[h, w] fp32 logits: normal * 3."""
    return (np.random.default_rng(seed).standard_normal((h, w)) * 3.0).astype(np.float32)


def gan_half_width(x, target):
    """Half-width of the reference's own interval of the summed mode-0 loss, relative to the loss."""
    lo, hi = gan_loss_elem(x, target, 0)
    return float((hi.sum() - lo.sum()) / (hi.sum() + lo.sum()))


# ---- image losses --------------------------------------------------------------------------------------------------------------
def l1w_weights(a, wts, nw):
    """(w, |w| bound, fp32 roundings in w) per pixel: the label form w = 1 + sum_i (a_i + 1) / 2 (wts_i - 1) (nw > 0), an explicit map
    a[..., 0] (nw == 0) or None."""
    if a is None:
        return None, None, 0
    a = _f64(a)
    if nw == 0:
        return a[..., 0], np.abs(a[..., 0]), 0
    terms = (a[..., :nw] + 1.0) * 0.5 * (_f64(wts)[:nw] - 1.0)
    return 1.0 + terms.sum(-1), 1.0 + np.abs(terms).sum(-1), 3 + nw        # each term: a + 1, wts - 1, their product; nw additions


def l1w_ref(x, y, C, a, wts, nw, lam):
    """lam * mean(|x - y| w) over npix * C and its gradient sign(x - y) w lam / (npix C), sign(0) = 0.  x, y: [npix, >= C].
    Returns (loss, grad [npix, C], loss bound, grad bound [npix, C]): |kernel - reference| may reach the bounds through fp32
    roundings alone -- per gradient element those of w (l1w_weights), then w * lam, the cast of 1 / (npix C) and the product with
    it, plus one for second-order terms: (kw + 4) u |w|bound lam / N; for the loss x - y, |d| * w, the roundings of w and the cast
    of the result: (kw + 3) u lam / N sum |d| |w|bound + u |loss|."""
    d = _f64(x)[:, :C] - _f64(y)[:, :C]
    N = d.size
    w, wabs, kw = l1w_weights(a, wts, nw)
    if w is None:
        w = wabs = np.ones(d.shape[0])
    w, wabs = w.reshape(-1, 1), wabs.reshape(-1, 1)
    lam = f32(lam)
    loss = lam * (np.abs(d) * w).sum() / N
    grad = np.sign(d) * w * lam / N
    loss_bound = (kw + 3) * U * abs(lam) / N * (np.abs(d) * wabs).sum() + U * abs(loss) + MIN_NORMAL
    grad_bound = (kw + 4) * U * np.abs(np.sign(d)) * wabs * abs(lam) / N + MIN_NORMAL
    return loss, grad, loss_bound, grad_bound


def bce01_ref(x, t, C):
    """BCELoss((x + 1) / 2, (t + 1) / 2), mean over npix * C, and d loss / d x = (p - t') / max(p (1 - p), 1e-12) / 2 / (npix C): the
    GAN interval scheme around p = (x + 1) / 2; t' is the fp32 value of (t + 1) / 2 (one correctly rounded addition, an exact halving).
    Returns ((loss lo, hi), (grad lo, hi) [npix, C])."""
    xs = np.asarray(x, dtype=np.float32)[:, :C]
    ts = np.asarray(t, dtype=np.float32)[:, :C]
    N = xs.size
    tg = ((ts + np.float32(1.0)) * np.float32(0.5)).astype(np.float64)
    p = p_candidates((xs.astype(np.float64) + 1.0) * 0.5, saturated_is_point=True)
    llo, lhi = _minmax(bce_term(p, tg))
    return mean_interval(llo, lhi, N), _minmax(bce_dterm(p, tg) * 0.5 / N)


def image_inputs(H, W, C, ld, seed):
    """(x, y, a, wts, wmap): x, y [H * W, ld] = tanh(normal) in the C logical channels with +-1 planted (BCE on (x + 1) / 2: p = 1 and
    p = 0, t' = 1 and 0), an exact x == y pair (sign(0)), NaN-free zeros behind; a [H * W, 4]: three label channels; wts: their
    weights; wmap [H * W, 1]: an explicit weight map."""
    rng = np.random.default_rng(seed)
    n = H * W
    x, y = np.zeros((n, ld), np.float32), np.zeros((n, ld), np.float32)
    x[:, :C] = np.tanh(rng.standard_normal((n, C))).astype(np.float32)
    y[:, :C] = np.tanh(rng.standard_normal((n, C))).astype(np.float32)
    x[0, 0], x[1 % n, C - 1] = 1.0, -1.0
    y[2 % n, 0], y[3 % n, C - 1] = 1.0, -1.0
    y[n - 1, 0] = x[n - 1, 0]
    a = np.zeros((n, 4), np.float32)
    a[:, :3] = np.tanh(rng.standard_normal((n, 3))).astype(np.float32)
    wts = np.array([2.0, 5.0, 0.5], dtype=np.float32)
    wmap = rng.uniform(0.5, 3.0, size=(n, 1)).astype(np.float32)
    return x, y, a, wts, wmap


# ---- cross-entropy and softmax -------------------------------------------------------------------------------------------------
def _lse(z):
    m = z.max(axis=1, keepdims=True)
    return m + np.log(np.exp(z - m).sum(axis=1, keepdims=True))


def softmax_ref(z, C):
    z = _f64(z)[:, :C]
    return np.exp(z - _lse(z))


def softmax_bwd_ref(dp, p, C):
    """(dz, magnitude): dz = p (dp - sum_c dp_c p_c) from the given p; magnitude = |p| (|dp| + sum_c |dp_c p_c|), what the roundings of
    the expression are relative to (the difference cancels)."""
    dp, p = _f64(dp)[:, :C], _f64(p)[:, :C]
    dot = (dp * p).sum(axis=1, keepdims=True)
    return p * (dp - dot), np.abs(p) * (np.abs(dp) + np.abs(dp * p).sum(axis=1, keepdims=True))


def ce_ref(z, C, label, const_label, cw, gout=1.0, pixel_add=None):
    """Weighted mean of lse - z_y over the pixels whose label is in [0, C) (every other label is skipped, torch's -100 among them; all
    skipped: loss 0 and an all-zero gradient, as the kernel documents).  z [npix, >= C]; label: int64 [npix] or None for const_label
    everywhere; cw: [>= C] class weights or None.  Returns (loss, grad [npix, C] = gout w_y (softmax - onehot) / sum w, sum w,
    loss magnitude, grad magnitude): the magnitudes are what fp32 roundings are relative to -- sum w_y (|lse| + |z_y|) / sum w for
    the loss, whose terms cancel where the pixel is classified well, and |scale| w_y (softmax + onehot) for the gradient.
    pixel_add [npix] (the pixel-weighted head): added to the weight of every pixel whose label is in range."""
    z = _f64(z)[:, :C]
    n = z.shape[0]
    y = np.full(n, int(const_label), dtype=np.int64) if label is None else np.asarray(label, dtype=np.int64).reshape(-1)
    ok = (y >= 0) & (y < C)
    ys = np.where(ok, y, 0)
    w = np.where(ok, (_f64(cw)[ys] if cw is not None else 1.0) + (_f64(pixel_add).reshape(-1) if pixel_add is not None else 0.0), 0.0)
    lse = _lse(z)[:, 0]
    zy = z[np.arange(n), ys]
    den = w.sum()
    if den <= 0.0:
        zero = np.zeros((n, C))
        return 0.0, zero, 0.0, 0.0, zero
    loss = (w * (lse - zy)).sum() / den
    onehot = (np.arange(C)[None, :] == ys[:, None]) & ok[:, None]
    p = np.exp(z - lse[:, None])
    scale = f32(gout) / den
    grad = scale * w[:, None] * (p - onehot)
    return loss, grad, den, (w * (np.abs(lse) + np.abs(zy))).sum() / den, abs(scale) * w[:, None] * (p + onehot)


CE_PAIRS = ((1, 4), (3, 4), (5, 8), (12, 12), (16, 16), (5, 5))      # (C, ld)
CE_SHAPES = ((10, 20), (70, 66), (363, 362))                        # one workgroup; several; 131 406 pixels, past the 512-workgroup cap
CE_BWD_CAP_NPIX = 1024 * 256 + 3                                    # 1025 workgroups' worth: past the 1024-workgroup cap of sgan_ce_bwd
BIG_LABELS = (2 ** 32 + 1, -(2 ** 32) + 2)                          # narrowed to 32 bits they would read 1 and 2


def ce_inputs(H, W, C, ld, seed):
    """(z [H * W, ld] fp32: normal * 2 in the C logical channels, zeros behind; label int64 [H * W] with -100, C, -1 and BIG_LABELS
    in it; cw [C] fp32 class weights in [0.5, 5))."""
    rng = np.random.default_rng(seed)
    n = H * W
    z = np.zeros((n, ld), np.float32)
    z[:, :C] = (rng.standard_normal((n, C)) * 2.0).astype(np.float32)
    lab = rng.integers(0, C, size=n).astype(np.int64)
    lab[:3] = -100
    lab[3], lab[4] = C, -1
    lab[5], lab[6] = BIG_LABELS
    lab[-2:] = (C, -100)
    lab[-4:-2] = BIG_LABELS
    cw = rng.uniform(0.5, 5.0, size=C).astype(np.float32)
    return z, lab, cw


def scaled_ulp_error(got, ref, mag=None):
    """|got - ref| in fp32 ulps of `mag` (default |ref|), elementwise, after the absolute floor of one minimum normal."""
    got, ref = _f64(got), _f64(ref)
    mag = np.abs(ref) if mag is None else _f64(mag)
    ulp = _f64(np.spacing(np.maximum(mag, MIN_NORMAL).astype(np.float32)))
    return np.maximum(np.abs(got - ref) - MIN_NORMAL, 0.0) / ulp


def budget(f32_eval, ref, mag=None):
    """4 x the largest scaled_ulp_error that another fp32 evaluation of the same expression (torch on the CPU) shows against the
    float64 reference on the same inputs; at least 2 ulp.  Computed from the reference side only."""
    return max(2.0, 4.0 * float(np.max(scaled_ulp_error(f32_eval, ref, mag))))


# ---- interval helpers of the head and factored-loss references -----------------------------------------------------------------
def imul(a, b):
    """Product of two intervals (lo, hi) of any sign."""
    c = np.stack([a[0] * b[0], a[0] * b[1], a[1] * b[0], a[1] * b[1]])
    return c.min(axis=0), c.max(axis=0)


def scale_interval(lo, hi, s, sabs, k):
    """[lo, hi] times a float64 factor s that the kernel holds in fp32 after k roundings relative to sabs >= |s|."""
    a, b = s * lo, s * hi
    e = k * U * sabs * np.maximum(np.abs(lo), np.abs(hi))
    return np.minimum(a, b) - e, np.maximum(a, b) + e


def ulps_off(f32_eval, ref):
    """Largest |f32_eval - ref| in ulps of the fp32 rounding of ref."""
    ref = _f64(ref)
    return float(np.max(np.abs(_f64(f32_eval) - ref) / _f64(np.spacing(np.maximum(np.abs(ref), MIN_NORMAL).astype(np.float32)))))


def candidate_ulps(f32_eval, ref):
    """k of a probability with more roundings behind it than one sigmoid: 4 x the largest deviation of another fp32 evaluation
    (torch on the CPU) from float64, in ulps, rounded up; never below P_ULPS."""
    return max(P_ULPS, int(np.ceil(4.0 * ulps_off(f32_eval, ref))))


# ---- the segmentation head (csrc/sgan_seghead.hip) and the --use_sigmoid_ss kernels (csrc/sgan_factd.hip) -----------------------
# Softmax mode is ce_ref (with pixel_add for the PW form) and softmax_ref.  The weight sums:
def weight_sum_ref(C, label, cw, pixel_add=None):
    """(sum, bound) of sgan_label_weight_sum / sgan_pixel_weight_sum: sum over the pixels with a label in [0, C) of cw[y] (1 without
    cw) + pixel_add.  The kernels add fp32 weights in fp64 and round the sum once: bound = u |sum| (+ u sum (|cw[y]| + |pixel_add|)
    for the PW form, whose weight is one fp32 addition per pixel) + n 2^-53 |sum| for the fp64 additions."""
    y = np.asarray(label, dtype=np.int64).reshape(-1)
    ok = (y >= 0) & (y < C)
    ys = np.where(ok, y, 0)
    base = np.where(ok, _f64(cw)[ys] if cw is not None else 1.0, 0.0)
    add = np.where(ok, _f64(pixel_add).reshape(-1), 0.0) if pixel_add is not None else np.zeros(y.size)
    s = (base + add).sum()
    bound = U * abs(s) + y.size * 2.0 ** -53 * abs(s) + MIN_NORMAL
    if pixel_add is not None:
        bound += U * (np.abs(base) + np.abs(add)).sum()
    return s, bound


def bcew_weights(t, cw, nw):
    """(w, |w| bound, fp32 roundings in w) per pixel: w = 1 + sum_{i < nw} t_i (cw_i - 1); each term cw - 1, the product, the addition."""
    t = _f64(t)
    if not nw:
        one = np.ones(t.shape[0])
        return one, one, 0
    terms = t[:, :nw] * (_f64(cw)[:nw] - 1.0)
    return 1.0 + terms.sum(1), 1.0 + np.abs(terms).sum(1), 3 * nw


def bcew_point(p, t, C, cw, nw, gout=1.0, chain=False):
    """(loss, gradient [npix, C]) at the float64 probabilities p themselves: loss = mean_{c, pix} w bce(p, t); gradient w.r.t. p
    (sgan_bce_weighted_bwd) = gout w / (C npix) (p - t) / max(p (1 - p), 1e-12), times p (1 - p) with `chain` (w.r.t. the logits:
    sgan_sigmoid_nhwc_bwd behind it, or the sigmoid mode of sgan_seg_head)."""
    p, t = _f64(p)[:, :C], _f64(t)
    w = bcew_weights(t, cw, nw)[0][:, None]
    g = f32(gout) * w / p.size * bce_dterm(p, t[:, :C])
    return (w * bce_term(p, t[:, :C])).mean(), g * (p * (1.0 - p)) if chain else g


def bcew_ref(p64, t, C, cw, nw, gout=1.0, chain=False, extra=0):
    """The interval form of bcew_point around the fp32 rounding of p64 [npix, >= C] (what a sigmoid kernel wrote, or what the kernel
    computes itself): candidates p32 +- P_ULPS.  Returns ((loss lo, hi), (grad lo, hi) [npix, C]).
    Loss: a pixel's sum over its C channels, each term widened by ELEM_ROUNDINGS, is C - 1 fp32 additions of terms of one sign;
    times w in fp64 (the roundings of w alone); the mean is rounded once.  Gradient: the element (ELEM_ROUNDINGS) times
    gout w / (C npix), which the kernels hold after the roundings of w, the quotient, the product with w and second-order terms
    (kw + 3), plus `extra` for a rescaling launch behind it."""
    t = _f64(t)
    p = p_candidates(_f64(p64)[:, :C])
    tc = t[:, :C]
    N = tc.size
    w, wabs, kw = bcew_weights(t, cw, nw)
    elo, ehi = _minmax(bce_term(p, tc))
    slo, shi = widen(elo.sum(1), ehi.sum(1), C - 1)
    tlo, thi = scale_interval(slo, shi, w, wabs, kw)
    d = bce_dterm(p, tc)
    if chain:
        d = d * (p * (1.0 - p))
    dlo, dhi = _minmax(d)
    g = f32(gout) / N
    return widen(tlo.sum() / N, thi.sum() / N, 1), scale_interval(dlo, dhi, g * w[:, None], abs(g) * wabs[:, None], kw + 3 + extra)


def wide_share(lo, hi, rel=1e-3):
    """Share of the elements whose interval half-width is above `rel` of the larger endpoint magnitude."""
    big = np.maximum(np.abs(lo), np.abs(hi))
    return float(np.mean((hi - lo) * 0.5 > rel * big))


def half_width(lo, hi):
    return float((hi - lo) / (abs(hi) + abs(lo)))


GRAD_MAX_WIDE_SHARE = 1e-3     # of a random map's gradient elements may have an interval half-width above 1e-3 of its larger endpoint


def head_inputs(H, W, C, seed):
    """(z [n, C] fp32 normal * 1.5, label int64 [n] -- the first image row -100 (the first three pixels of a one-row map), then C, -1
    and BIG_LABELS, and again at the end --, one-hot targets [n, C] of the labels before that, soft targets uniform [n, C] kept 0.01 off sigmoid(z),
    cw [C] in [0.5, 5), pixel_add [n]: zero on 70 % of the pixels, up to 10 elsewhere)."""
    rng = np.random.default_rng(seed)
    n = H * W
    z = (rng.standard_normal((n, C)) * 1.5).astype(np.float32)
    lab = rng.integers(0, C, size=n).astype(np.int64)
    hot = (np.arange(C)[None, :] == lab[:, None]).astype(np.float32)
    k = W if H > 1 else 3
    lab[:k] = -100
    lab[k], lab[k + 1] = C, -1
    lab[k + 2], lab[k + 3] = BIG_LABELS
    lab[-2:] = (C, -100)
    lab[-4:-2] = BIG_LABELS
    soft = rng.uniform(0.0, 1.0, size=(n, C))
    p = sigmoid64(z)      # a soft target within 0.01 of p is moved 0.02 off it: p - t cancels there and the gradient's interval grows wide
    soft = np.where(np.abs(soft - p) < 0.01, np.where(p < 0.5, p + 0.02, p - 0.02), soft).astype(np.float32)
    cw = rng.uniform(0.5, 5.0, size=C).astype(np.float32)
    add = (rng.uniform(0.0, 10.0, size=n) * (rng.uniform(size=n) > 0.7)).astype(np.float32)
    return z, lab, hot, soft, cw, add


# ---- the factored GAN loss (sgan_factd_loss_multi_fwd / _bwd) -------------------------------------------------------------------
def factd_pad_split(dH, dW):
    """(left, right, top, bottom): the left and the bottom take the floor of the half, the right and the top the remainder."""
    pl, pb = dW // 2, dH // 2
    return pl, dW - pl, dH - pb, pb


def up2_matrix(n):
    """[2n, n]: bilinear x2, align_corners=False: out[2i + a] = 0.75 in[i] + 0.25 in[clamp(i - 1 + 2a)]."""
    M = np.zeros((2 * n, n))
    for o in range(2 * n):
        i, a = divmod(o, 2)
        M[o, i] += 0.75
        M[o, min(max(i - 1 + 2 * a, 0), n - 1)] += 0.25
    return M


def reflect_matrix(n, before, after):
    """[before + n + after, n] of 0 / 1: row r reads source reflect(r - before), the border not repeated (every pad < n)."""
    assert before < n and after < n
    P = np.zeros((before + n + after, n))
    for r in range(before + n + after):
        s = r - before
        s = -s if s < 0 else (2 * (n - 1) - s if s >= n else s)
        P[r, s] = 1.0
    return P


def factd_maps(h1, w1, up, H2, W2):
    """(My [H2, h1], Mx [W2, w1]), both >= 0: q = My a1 Mx^T is pad(upsample(a1)), and the gradient arriving at a1 is its explicit
    adjoint My^T G Mx -- first the pad's (every mirrored position adds into its source), then the x2 taps'."""
    hu, wu = h1 * up, w1 * up
    pl, pr, pt, pb = factd_pad_split(H2 - hu, W2 - wu)
    Uy = up2_matrix(h1) if up == 2 else np.eye(h1)
    Ux = up2_matrix(w1) if up == 2 else np.eye(w1)
    return reflect_matrix(hu, pt, pb) @ Uy, reflect_matrix(wu, pl, pr) @ Ux


FACTD_Q_ROUNDINGS = 7          # the x2 taps of one output: four products and three additions (the pad copies)
FACTD_DL2_ROUNDINGS = 12       # p - t, 1 - p, (1 - p) p, the division; go = gout * w / np: 2; times go, times q; a2 (1 - a2): 2, times it; one spare
FACTD_DL1_ROUNDINGS = 40       # a gathered term: 8; <= 9 of them added, 4 + 4 tap products and additions twice over: relative to the sum of the absolute gathered terms


def factd_term(l1, l2, up, target, mode, weight=1.0, gout=1.0, kp=None, kq=None):
    """One term of the factored loss.  l1 [h1, w1], l2 [H2, W2] fp32 logits; mode (sig1, sig2, mse).  Returns a dict:
    p, q (the product and the padded upsampled map), each, dl1, dl2: the float64 point values -- a = sigmoid or identity, q = My a1 Mx^T,
    p = q a2, each = mean crit(p, target), dl2 = d / d l2, dl1 = (My^T (dcrit go a2) Mx) a1' with go = gout weight / pixels;
    qmag, each_mag, dl1_mag, dl2_mag: what fp32 roundings are relative to -- sum |tap| |operand| for q, (|p| + |t|)^2 for the MSE term,
    and the gradients with every difference replaced by the sum of its operands' magnitudes;
    with kp (BCE mode: the candidate ulps of p, and kq of q): each_iv, dl1_iv, dl2_iv, the intervals."""
    sig1, sig2, mse = mode
    x1, x2 = _f64(l1), _f64(l2)
    a1 = sigmoid64(x1) if sig1 else x1
    a2 = sigmoid64(x2) if sig2 else x2
    My, Mx = factd_maps(x1.shape[0], x1.shape[1], up, x2.shape[0], x2.shape[1])
    q = My @ a1 @ Mx.T
    qmag = My @ np.abs(a1) @ Mx.T
    p = q * a2
    tg = f32(target)
    go = f32(gout) * f32(weight) / p.size
    s1 = a1 * (1.0 - a1) if sig1 else np.ones_like(a1)
    s2 = a2 * (1.0 - a2) if sig2 else np.ones_like(a2)
    pmag = qmag * np.abs(a2) + abs(tg)
    if mse:
        crit, dcrit, dmag = (p - tg) ** 2, 2.0 * (p - tg), 2.0 * pmag
    else:
        crit, dcrit = bce_term(p, tg), bce_dterm(p, tg)
        dmag = np.abs(dcrit)
    out = dict(p=p, q=q, qmag=qmag, each=crit.mean(), each_mag=(pmag ** 2).mean() if mse else crit.mean(),
               dl2=dcrit * go * q * s2, dl2_mag=dmag * abs(go) * qmag * np.abs(s2),
               dl1=(My.T @ (dcrit * go * a2) @ Mx) * s1, dl1_mag=(My.T @ (dmag * abs(go) * np.abs(a2)) @ Mx) * np.abs(s1))
    if kp is not None:
        assert sig1 and sig2 and not mse
        pc = p_candidates(p, ulps=kp)
        out["each_iv"] = mean_interval(*_minmax(bce_term(pc, tg)))
        d = bce_dterm(pc, tg)
        D = (d.min(0), d.max(0))
        qc = p_candidates(q, ulps=kq)
        c2, c1 = p_candidates(a2), p_candidates(a1)
        S2, S1 = c2 * (1.0 - c2), c1 * (1.0 - c1)
        lo, hi = imul(imul(D, (qc.min(0), qc.max(0))), (S2.min(0), S2.max(0)))
        out["dl2_iv"] = scale_interval(lo, hi, go, abs(go), FACTD_DL2_ROUNDINGS)
        glo, ghi = imul(D, (c2.min(0), c2.max(0)))
        gath = (My.T @ glo @ Mx, My.T @ ghi @ Mx)                      # My, Mx >= 0: the adjoint is monotone
        gabs = My.T @ np.maximum(np.abs(glo), np.abs(ghi)) @ Mx
        lo, hi = imul(gath, (S1.min(0), S1.max(0)))
        e = FACTD_DL1_ROUNDINGS * U * abs(go) * gabs * S1.max(0) + MIN_NORMAL
        out["dl1_iv"] = (np.minimum(go * lo, go * hi) - e, np.maximum(go * lo, go * hi) + e)
    return out


# (h1, w1, up, H2, W2): tests/test_hip_factd.py's geometries, then a one-pixel map (both clamps of the x2 taps on the same pixel), pads
# of size - 1 on both axes, a large top remainder with an even width difference, 4489 pixels with no pad (past one 16 x 256 sweep)
FACTD_SHAPES = ((3, 5, 2, 9, 13), (4, 4, 2, 15, 15), (7, 7, 1, 7, 7), (5, 6, 1, 8, 9), (4, 6, 2, 8, 12), (11, 11, 2, 35, 35), (7, 7, 2, 19, 19),
                (19, 19, 2, 67, 67), (1, 1, 2, 2, 2), (1, 1, 2, 3, 3), (2, 3, 1, 3, 5), (3, 2, 2, 11, 7), (67, 67, 1, 67, 67))
FACTD_MODES = ((1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1))      # (sig1, sig2, mse)


def factd_logits(shape, seed):
    """(l1 [h1, w1], l2 [H2, W2]) fp32, normal * 1.5."""
    h1, w1, _, H2, W2 = shape
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((h1, w1)) * 1.5).astype(np.float32), (rng.standard_normal((H2, W2)) * 1.5).astype(np.float32)

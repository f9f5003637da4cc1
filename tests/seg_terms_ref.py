"""Plain numpy float64 reference of the Tversky / focal loss terms on the logits (csrc/sgan_segterms.hip: sg_seg_terms_fwd_kernel,
sg_seg_terms_bwd_kernel) WITH its error model, element by element and in the kernels' own composition.  Neither torch nor the library
is imported; the helpers of tests/loss_ref.py are used, not copied.  util.seg_terms_ref stays the point yardstick of the formulas;
tests/test_seg_terms_ref_host.py holds this file to it and to torch's double autograd, tests/test_hip_seg_terms_kernels.py holds the
kernels to this file.  u = 2^-24 (one fp32 rounding), eps = 2^-53 (one fp64 rounding), 1 ulp = 2 u resp. 2 eps of the binade.

Forward sums (`forward_intervals`).  TP, FP, FN of a listed class, the focal numerator and norm are sums over the pixels of a
per-pixel interval, then the fp64 accumulation 2 (npix + 2) eps of the sum (the counted term of tests/test_hip_seg_terms.py).
  softmax p     p64 +- bp ulp OF p ITSELF (+ 2^-126: a denormal may be flushed), bp = 4 x the largest error of torch's CPU fp32
                exp(z - m) / sum against float64 on the same logits, at least 2 (loss_ref.budget); clipped to [0, 1]
  sigmoid p     the fp32 candidates p32 - 3 .. p32 + 3 ulp of loss_ref.p_candidates (0 among them where p32 is denormal);
                p t, p (1 - t), (1 - p) t are monotone in p and taken at the two ends in fp64
  focal term    softmax: w (1 - pt)^g (-lp), 1 - pt the others' exponentials over the sum, lp = z_y - (m + log sum): budget in ulps of
                w (1 - pt)^g (|z_y| + |m| + |log sum|) -- lp is a difference and its roundings are relative to its operands;
                sigmoid: every channel term w (t q^g softplus(-z) + (1 - t) p^g softplus(z)), q = sigmoid(-z), is a sum of two
                non-negative products: budget in ulps of THE TERM; a pixel adds its C terms in fp32, C - 1 more roundings (u each)
                of the pixel's sum.  Both budgets by the same 4 x rule on torch's CPU fp32 evaluation of the very composition.
A sum whose reference is 0 has the interval [0, 0].

Derived state (`derived`).  D, TI, L_c, G(0), G(1), L_T, L_F are recomputed in float64 from the sums THE DEVICE wrote, in the order
((TP + a FP) + b FN) + s, and the device must agree to a counted number of fp64 roundings; the counts stand beside the constants
below.  The two pow calls cannot be counted: `pow_allowance` gives them 4 x the largest deviation of numpy's float64 pow from a
numpy.longdouble evaluation on the very (u, power) pairs, at least 2 fp64 ulp (the floor alone, POW_FLOOR_ONLY set, where
numpy.longdouble is no wider than float64).

Backward (`backward`), per element, in ulps of the magnitude with every difference replaced by the sum of its operands' magnitudes:
  softmax   dz_c = p_c (g_c - sum_j p_j g_j) + ws (onehot - p_c):  |p_c| (|g_c| + sum_j |p_j g_j|)  +  |w fscale| kmag (onehot + p_c),
            ws = w fscale k, k = -(1 - pt)^g + g pt (1 - pt)^(g - 1) lp (the product left out where g == 0 or 1 - pt == 0),
            kmag = (1 - pt)^g + g pt (1 - pt)^(g - 1) (|z_y| + |m| + |log sum|)
  sigmoid   dz_c = p q (g0 + t (g1 - g0)) + cw fscale (pos - neg):  p q (|g0| + |t| (|g1| + |g0|))  +  |cw fscale| (|pos| + |neg|)
g0, g1 = fp32(gout_t G(0)), fp32(gout_t G(1)), fscale = fp32(gout_f / norm) as the kernel forms them (`upstream`).  The joint
gradient is measured in ulps of the sum of the two magnitudes and gets one more ulp for the addition.  The budget is 4 x torch's CPU
fp32 evaluation of that composition, at least 2 ulp, the largest over the (mode, gamma) group of the test's inputs.  (a) from the
device's own state: the budget alone.  (b) end to end, against the reference state: the same magnitudes plus what the relative
error the sums' intervals allow on G and on the norm moves the element by (`g_slack`).
An element whose magnitude is 0 (ignored or out-of-range label, unlisted sigmoid channel, D == 0 or 1 - TI == 0 class, NULL or zero
upstream gradient) must be exactly 0."""
import itertools

import numpy as np

import loss_ref as R

U = R.U
EPS = 2.0 ** -53
SOFTMAX, SIGMOID = 0, 1


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def ulp_of(mag):
    """One fp32 ulp of `mag`, never below that of 2^-126 -- the unit of loss_ref.scaled_ulp_error."""
    return _f64(np.spacing(np.maximum(_f64(mag), R.MIN_NORMAL).astype(np.float32)))


def allowed(bud, mag):
    """The absolute error a budget of `bud` ulps of `mag` allows: the inverse of loss_ref.scaled_ulp_error."""
    return bud * ulp_of(mag) + R.MIN_NORMAL


def softplus64(x):
    x = _f64(x)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def _pow(b, e):
    """b ** e for b >= 0 with 0 ** 0 = 1 (C's pow) and 0 ** negative = 0: the callers leave that product out."""
    b = _f64(b)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((b == 0.0) & (e < 0.0), 0.0, np.power(b, e))


class Pixels:
    """The per-pixel float64 quantities both kernels form, from fp32 logits z [npix, >= C] and the label [npix] / target [npix, >= C]."""

    def __init__(self, z, lt, mode, C):
        z = _f64(np.asarray(z, dtype=np.float32))[:, :C]
        self.z, self.C, self.mode, self.npix = z, C, int(mode), z.shape[0]
        n = self.npix
        if self.mode == SOFTMAX:
            y = np.asarray(lt).reshape(n).astype(np.int64)
            self.ok = (y >= 0) & (y < C)                      # judged in 64 bits
            ys = np.where(self.ok, y, 0)
            self.ys = ys
            self.onehot = (np.arange(C)[None, :] == ys[:, None]) & self.ok[:, None]
            self.t = self.onehot.astype(np.float64)
            m = z.max(axis=1)
            e = np.exp(z - m[:, None])
            s = e.sum(axis=1)
            self.p = e / s[:, None]
            self.om = (e * ~self.onehot).sum(axis=1) / s      # 1 - pt: the others over the sum
            zy = z[np.arange(n), ys]
            self.lp = zy - (m + np.log(s))
            self.lmag = np.abs(zy) + np.abs(m) + np.abs(np.log(s))
            self.pt = self.p[np.arange(n), ys]
        else:
            self.ok = np.ones(n, dtype=bool)
            self.t = _f64(np.asarray(lt, dtype=np.float32)).reshape(n, -1)[:, :C]
            self.p, self.q = R.sigmoid64(z), R.sigmoid64(-z)
            self.spn, self.spp = softplus64(-z), softplus64(z)


def class_weights(C, cw, nw):
    """[C] float64: the first nw of cw, 1 behind them (softmax: nw == C or no weights at all)."""
    w = np.ones(C)
    if cw is not None and nw:
        w[:nw] = _f64(np.asarray(cw, dtype=np.float32))[:nw]
    return w


# ---- forward ----------------------------------------------------------------------------------------------------------------------
def focal_terms(px, gamma, w):
    """(term, magnitude): softmax [npix] (0 on a pixel without a valid label), sigmoid [npix, C] per channel (magnitude = term)."""
    if px.mode == SOFTMAX:
        wy = w[px.ys] * px.ok
        og = _pow(px.om, gamma)
        # one channel: exp(0) = 1, the sum 1, its log 0 and lp = z - (z + 0) = 0 are all exact in fp32: no roundings, no magnitude
        return wy * og * -px.lp, wy * og * (px.lmag if px.C > 1 else 0.0)
    term = w[None, :] * (px.t * _pow(px.q, gamma) * px.spn + (1.0 - px.t) * _pow(px.p, gamma) * px.spp)
    return term, term


def point_sums(px, classes, gamma, w):
    """(S [n, 3] = TP, FP, FN of every listed class, focal numerator, focal norm) at the float64 p; gamma None: both focal sums 0."""
    v = px.ok.astype(np.float64)
    S = np.zeros((len(classes), 3))
    for j, c in enumerate(classes):
        pc, tc = px.p[:, c], px.t[:, c]
        S[j] = (np.sum(pc * tc * v), np.sum(pc * (1.0 - tc) * v), np.sum((1.0 - pc) * tc * v))
    if gamma is None:
        return S, 0.0, 0.0
    term, _ = focal_terms(px, gamma, w)
    norm = float(np.sum(w[px.ys] * px.ok)) if px.mode == SOFTMAX else float(px.C) * float(px.npix)
    return S, float(term.sum()), norm


def acc_term(npix):
    """The fp64 accumulation of npix non-negative terms, on either side: 2 (npix + 2) eps of the sum."""
    return 2.0 * (npix + 2) * EPS


def forward_intervals(px, classes, gamma, w, bp, bt):
    """(lo [n, 3], hi [n, 3], (numerator lo, hi), (norm lo, hi)).  bp: the softmax p budget in ulps of p (unused in sigmoid mode);
    bt: the focal term budget in ulps of the magnitude focal_terms states."""
    v = px.ok.astype(np.float64)
    if px.mode == SOFTMAX:
        a = allowed(bp, px.p) if px.C > 1 else 0.0           # one channel: p = 1 / 1 is exact
        plo, phi = np.clip(px.p - a, 0.0, 1.0), np.clip(px.p + a, 0.0, 1.0)
    else:
        c = R.p_candidates(px.p)
        plo, phi = c.min(axis=0), c.max(axis=0)
    e = acc_term(px.npix)
    lo, hi = np.zeros((len(classes), 3)), np.zeros((len(classes), 3))
    for j, c in enumerate(classes):
        tc = px.t[:, c] * v
        fc = (1.0 - px.t[:, c]) * v
        lo[j] = (np.sum(plo[:, c] * tc), np.sum(plo[:, c] * fc), np.sum((1.0 - phi[:, c]) * tc))
        hi[j] = (np.sum(phi[:, c] * tc), np.sum(phi[:, c] * fc), np.sum((1.0 - plo[:, c]) * tc))
    # a structurally empty sum (no pixel of the class, a target that is 0 or 1 everywhere) is [0, 0] already: its terms are 0 * p
    lo, hi = lo * (1.0 - e), hi * (1.0 + e)
    if gamma is None:
        return lo, hi, (0.0, 0.0), (0.0, 0.0)
    term, mag = focal_terms(px, gamma, w)
    if px.mode == SOFTMAX:
        b = np.where(mag > 0.0, allowed(bt, mag), 0.0)
        norm = float(np.sum(w[px.ys] * px.ok))              # fp32 weights added in fp64: the accumulation alone
        nrm = (norm * (1.0 - e), norm * (1.0 + e))
    else:
        s = term.sum(axis=1)
        b = np.where(mag > 0.0, allowed(bt, mag), 0.0).sum(axis=1) + (px.C - 1) * U * s      # C - 1 fp32 additions of the pixel's sum
        term = s
        norm = float(px.C) * float(px.npix)                  # a product of two integers: exact
        nrm = (norm, norm)
    nlo, nhi = np.sum(np.maximum(term - b, 0.0)), np.sum(term + b)
    return lo, hi, (nlo * (1.0 - e), nhi * (1.0 + e)), nrm


# ---- the derived state ----------------------------------------------------------------------------------------------------------
ND = 6       # D = ((TP + a FP) + b FN) + s: two products and three additions of non-negative terms, one spare for a fused multiply-add
NTI = ND + 2     # TI = (TP + s) / D: the numerator's addition and the division on top of D's
NU = ND + 3      # u = 1 - TI <= 1: TI's and the subtraction, ABSOLUTE (relative to 1 >= TI)
NK = 3           # k = -(E / n) pow(u, E - 1): the division, the product, one spare
NG0 = 2 * ND + 5     # -(num a) / (D D): num, num a, D D on two D's, the division, the product with k
NG1 = 2 * ND + 8     # 1 / D - (num (1 - b)) / (D D): ND + 1 for the reciprocal, 1 - b, num, their product, D D on two D's, the division, the
#                      subtraction, the product with k -- relative to |k| (1 / D + num |1 - b| / D^2)
POW_FLOOR = 2.0      # fp64 ulp
POW_FLOOR_ONLY = np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps


def pow_allowance(pairs):
    """fp64 ulps allowed to one pow call: 4 x the largest deviation of numpy's float64 pow from numpy.longdouble's on `pairs` of
    (u, exponent), at least POW_FLOOR; the floor alone where longdouble is no wider than float64 on this host."""
    worst = 0.0
    if not POW_FLOOR_ONLY:
        for u, e in pairs:
            if u > 0.0 and e not in (0.0, 1.0):
                wide = np.power(np.longdouble(u), np.longdouble(e))
                worst = max(worst, float(abs(np.longdouble(np.power(u, e)) - wide) / np.longdouble(np.spacing(float(wide)))))
    return max(POW_FLOOR, 4.0 * worst)


def pow_pairs(S, tv):
    """The (u, power), (u, power - 1) pairs the state of sums S [n, 3] takes pow of."""
    a, b, s, E = tv
    out = []
    for TP, FP, FN in _f64(S).reshape(-1, 3):
        D = ((TP + a * FP) + b * FN) + s
        if D > 0.0:
            u = max(1.0 - (TP + s) / D, 0.0)
            out += [(u, E), (u, E - 1.0)]
    return out


def derived(S, tv, pow_ulps=POW_FLOOR):
    """(val [n, 5], bound [n, 5], L_T, its bound): D, TI, L_c, G(0), G(1) of every listed class from the sums S [n, 3] in float64, and
    the absolute error a device that computes the same expressions from the same sums in fp64 may show."""
    a, b, s, E = (float(x) for x in tv)
    S = _f64(S).reshape(-1, 3)
    n = S.shape[0]
    val, bound = np.zeros((n, 5)), np.zeros((n, 5))
    pw = lambda e: 0.0 if e in (0.0, 1.0) else 2.0 * pow_ulps * EPS      # noqa: E731  pow(u, 0) and pow(u, 1) are exact
    for j, (TP, FP, FN) in enumerate(S):
        D = ((TP + a * FP) + b * FN) + s
        if not D > 0.0:
            continue                                          # D == 0: every term is 0, the sum is exact, the class takes no part
        num = TP + s
        TI = num / D
        u = max(1.0 - TI, 0.0)
        bu = NU * EPS
        val[j, :2], bound[j, :2] = (D, TI), (ND * EPS * D, NTI * EPS * TI)
        if u <= 2.0 * bu:
            # 1 - TI is 0 or within its own roundings of it: the device may stand on either side; both sides' values are allowed
            if u > 0.0:
                k = -(E / n) * u ** (E - 1.0)
                val[j, 2:] = (u ** E, k * (-(num * a) / (D * D)), k * (1.0 / D - (num * (1.0 - b)) / (D * D)))
                bound[j, 2:] = np.abs(val[j, 2:]) * 4.0 + (3.0 * bu) ** E
            continue
        ru = bu / u
        Lc = u ** E
        k = -(E / n) * u ** (E - 1.0)
        rk = abs(E - 1.0) * ru + pw(E - 1.0) + NK * EPS
        G0 = k * (-(num * a) / (D * D))
        G1 = k * (1.0 / D - (num * (1.0 - b)) / (D * D))
        M1 = abs(k) * (1.0 / D + num * abs(1.0 - b) / (D * D))
        val[j, 2:] = (Lc, G0, G1)
        bound[j, 2:] = ((E * ru + pw(E) + EPS) * Lc, (rk + NG0 * EPS) * abs(G0), (rk + NG1 * EPS) * M1)
    LT = float(val[:, 2].sum() / n) if n else 0.0
    return val, bound, LT, (float(bound[:, 2].sum() / n) + (n + 1) * EPS * LT) if n else 0.0


def state_of(S, fnum, fnorm, tv, focal):
    """The 68 doubles the forward writes, from the given sums."""
    st = np.zeros(68)
    n = len(S)
    LT = 0.0
    if n:
        val, _, LT, _ = derived(S, tv)
        for j in range(n):
            st[8 * j:8 * j + 3] = S[j]
            st[8 * j + 3:8 * j + 8] = val[j]
    if focal:
        st[64], st[65] = fnum, fnorm
        st[67] = fnum / fnorm if fnorm > 0.0 else 0.0
    st[66] = LT
    return st


def reference_state(px, classes, tv, gamma, w):
    S, fnum, fnorm = point_sums(px, classes, gamma, w)
    return state_of(S, fnum, fnorm, tv if len(classes) else (0.5, 0.5, 1.0, 1.0), gamma is not None)


# ---- backward -------------------------------------------------------------------------------------------------------------------
def upstream(state, classes, C, gout_t, gout_f, focal, rounded=True):
    """(g0 [C], g1 [C], fscale) as the kernel forms them from a state: fp32(gout_t G) per listed channel (0 elsewhere; all 0 with
    gout_t None) and fp32(gout_f / norm) (0 with gout_f None, the focal term off or norm == 0).  rounded=False: in float64."""
    cast = (lambda v: float(np.float32(v))) if rounded else float
    g0, g1 = np.zeros(C), np.zeros(C)
    if gout_t is not None:
        up = R.f32(gout_t)
        for j, c in enumerate(classes):
            g0[c], g1[c] = cast(up * state[8 * j + 6]), cast(up * state[8 * j + 7])
    fscale = 0.0
    if focal and gout_f is not None and state[65] > 0.0:
        fscale = cast(R.f32(gout_f) / state[65])
    return g0, g1, fscale


def backward(px, g0, g1, fscale, gamma, w):
    """(dz, Tversky magnitude, focal magnitude), each [npix, C] float64, from per-channel g0, g1 (zeros: that part is off) and fscale
    (0: the focal part is off)."""
    C = px.C
    g0, g1 = _f64(g0)[None, :], _f64(g1)[None, :]
    zero = np.zeros((px.npix, C))
    dF = mF = zero
    if px.mode == SOFTMAX:
        v = px.ok[:, None]
        g = np.where(px.onehot, g1, g0)
        dT = px.p * (g - (px.p * g).sum(axis=1, keepdims=True)) * v
        mT = px.p * (np.abs(g) + np.abs(px.p * g).sum(axis=1, keepdims=True)) * v
        if fscale != 0.0 and gamma is not None:
            og = _pow(px.om, gamma)
            second = gamma * px.pt * _pow(px.om, gamma - 1.0) if gamma != 0.0 else np.zeros(px.npix)
            second = np.where(px.om != 0.0, second, 0.0)
            wy = w[px.ys] * px.ok
            k, kmag = -og + second * px.lp, og + second * px.lmag
            dF = (wy * fscale * k)[:, None] * (px.t - px.p) * v
            mF = (wy * abs(fscale) * kmag)[:, None] * (px.t + px.p) * v
    else:
        dT = px.p * px.q * (g0 + px.t * (g1 - g0))
        mT = px.p * px.q * (np.abs(g0) + np.abs(px.t) * (np.abs(g1) + np.abs(g0)))
        if fscale != 0.0 and gamma is not None:
            pos = (1.0 - px.t) * _pow(px.p, gamma) * (gamma * px.q * px.spp + px.p)
            neg = px.t * _pow(px.q, gamma) * (gamma * px.p * px.spn + px.q)
            dF = w[None, :] * fscale * (pos - neg)
            mF = np.abs(w[None, :] * fscale) * (np.abs(pos) + np.abs(neg))
    return dT + dF, mT, mF


def g_slack(lo, hi, tv, fnorm_iv, ref_state, classes, C):
    """(dg0 [C], dg1 [C], relative error of the norm): how far G(0), G(1) of a state computed from sums anywhere in [lo, hi] may lie
    from the reference state's -- the largest deviation over the 8 corners of every class's (TP, FP, FN) box, times 1.5 for the
    curvature inside a box whose sides are at most 2e-5 of the sums."""
    dg0, dg1 = np.zeros(C), np.zeros(C)
    n = len(classes)
    for j, c in enumerate(classes):
        for corner in itertools.product((0, 1), repeat=3):
            S = np.array([[(lo, hi)[k][j, i] for i, k in enumerate(corner)]])
            val = derived(S, tv)[0][0] / n                    # derived() divides by ITS n = 1
            dg0[c] = max(dg0[c], 1.5 * abs(val[3] - ref_state[8 * j + 6]))
            dg1[c] = max(dg1[c], 1.5 * abs(val[4] - ref_state[8 * j + 7]))
    nlo, nhi = fnorm_iv
    return dg0, dg1, (nhi - nlo) / (nhi + nlo) if nhi > 0.0 else 0.0


def slack_of(px, dg0, dg1, up_abs, rel_norm, mF):
    """The absolute amount the end-to-end element may move through the state: the Tversky expression at |gout_t| (dg0, dg1) with every
    difference as a sum, plus the focal magnitude times the norm's relative error."""
    d0, d1 = up_abs * _f64(dg0)[None, :], up_abs * _f64(dg1)[None, :]
    if px.mode == SOFTMAX:
        g = np.where(px.onehot, d1, d0)
        sT = px.p * (g + (px.p * g).sum(axis=1, keepdims=True)) * px.ok[:, None]
    else:
        sT = px.p * px.q * (d0 + np.abs(px.t) * (d1 + d0))
    return sT + 2.0 * rel_norm * mF


# ---- inputs --------------------------------------------------------------------------------------------------------------------
# Narrowed: the softmax cases read logits normal * 2 (loss_ref.ce_inputs' scale), the sigmoid cases the same normals * 3.  At normal * 3
# the p budget, which the pixel with the largest z - m sets for all, reached 78 ulp and the gamma = 8 focal term's 291 ulp, and the
# half-widths of FN and of the focal numerator 8.4e-5 and 3.1e-5 against the cap of 2e-5 (tests/test_seg_terms_ref_host.py).
SOFTMAX_SCALE = 2.0


def inputs(H, W, C, seed, absent=None):
    """dict: z [n, C] fp32 normal * 3 and zs, the same normals * SOFTMAX_SCALE; label int64 [n] (with -100, C, -1 and loss_ref.BIG_LABELS planted at both ends where the map has
    16 pixels or more; `absent`: that class never occurs); hot [n, C] the one-hot target of the label before the planting; soft
    [n, C] uniform(0, 1) (`absent`: 0 on that channel); cw [C] fp32 class weights in [0.5, 5)."""
    rng = np.random.default_rng(seed)
    n = H * W
    normal = rng.standard_normal((n, C))
    z = (normal * 3.0).astype(np.float32)
    zs = (normal * SOFTMAX_SCALE).astype(np.float32)
    lab = rng.integers(0, C, size=n).astype(np.int64)
    if absent is not None:
        lab[lab == absent] = (absent + 1) % C
    hot = (np.arange(C)[None, :] == lab[:, None]).astype(np.float32)
    if n >= 16:
        lab[:2] = -100
        lab[2], lab[3] = C, -1
        lab[4], lab[5] = R.BIG_LABELS
        lab[-2:] = (C, -100)
        lab[-4:-2] = R.BIG_LABELS
    soft = rng.uniform(0.0, 1.0, size=(n, C)).astype(np.float32)
    if absent is not None:
        soft[:, absent] = 0.0
    cw = rng.uniform(0.5, 5.0, size=C).astype(np.float32)
    return dict(z=z, zs=zs, label=lab, hot=hot, soft=soft, cw=cw)


def planted_inputs(C=3):
    """loss_ref.GAN_PLANTED on one channel against zeros elsewhere, each value four times: the label / target on the planted channel
    and off it, the planted channel moving with the pixel.  dict as `inputs`; `soft` holds 0 / 1 targets and 0.9 / 0.1 behind them."""
    vals = np.repeat(np.array(R.GAN_PLANTED, dtype=np.float32), 4)
    n = vals.size
    ch = np.arange(n) % C
    z = np.zeros((n, C), np.float32)
    z[np.arange(n), ch] = vals
    on = (np.arange(n) % 4) < 2
    lab = np.where(on, ch, (ch + 1 + (np.arange(n) // 4) % (C - 1)) % C).astype(np.int64)
    hot = (np.arange(C)[None, :] == lab[:, None]).astype(np.float32)
    soft = hot.copy()
    odd = np.arange(n) % 2 == 1
    soft[odd] = np.where(hot[odd] > 0.5, np.float32(0.9), np.float32(0.1))
    cw = np.array([3.0, 0.5, 1.5, 2.0][:C] + [1.0] * max(0, C - 4), dtype=np.float32)
    return dict(z=z, zs=z, label=lab, hot=hot, soft=soft, cw=cw)

"""Plain numpy float64 reference of the boundary / Hausdorff loss node on the logits (csrc/sgan_distloss.hip: sg_dist_loss_fwd_kernel,
sg_dist_loss_bwd_kernel) WITH its error model, element by element and in the kernels' own composition.  Neither torch nor the library
is imported; the helpers of tests/loss_ref.py and tests/seg_terms_ref.py are used, not copied.  util.dist_terms_ref stays the point
yardstick of the formulas; tests/test_dist_terms_kernels_ref_host.py holds this file to it and to torch's double autograd,
tests/test_hip_dist_terms_kernels.py holds the kernels to this file.  u = 2^-24, eps = 2^-53, 1 ulp = 2 u resp. 2 eps of the binade.

Per pixel (`Pixels`).  softmax: p of every channel and om = 1 - p_cls as the other channels' exponentials over the sum; sigmoid:
p = sigmoid(z_cls) and q = sigmoid(-z_cls); g = [y == cls] or target_cls; phi from the integer map as dl_phi (sqrt(s), 1 - sqrt(-s),
0); F as dl_field (|t|^(alpha/2) + |p|^(alpha/2), a zero map value adding 0, the exact integer |t| + |p| at alpha == 2).  A label
outside [0, C), judged in 64 bits, takes the pixel out of every sum and every gradient.

Forward sums (`forward_intervals`).  S_B = sum phi p and S_H = sum (p - g)^2 F are sums of per-pixel intervals:
  softmax p     p64 +- bp ulp OF p ITSELF (+ 2^-126: a denormal may be flushed), bp = 4 x the largest error of torch's CPU fp32
                exp(z - m) / sum against float64 on the same logits, at least 2 (loss_ref.budget); clipped to [0, 1]; one channel:
                p = 1 / 1 is exact
  sigmoid p     the fp32 candidates p32 - 3 .. p32 + 3 ulp of loss_ref.p_candidates
  phi p         monotone in p: taken at the two ends
  (p - g)^2 F   taken at the two ends of the p interval, and 0 where the interval contains g
then the fp64 accumulation 2 (npix + 2) eps of the sum of the terms' MAGNITUDES (the boundary sum is signed: its terms cancel, its
roundings do not), and on S_H `pow_allowance` for the two pow calls (4 x the largest deviation of numpy's float64 pow from
numpy.longdouble's on the map's own (value, alpha / 2) pairs, at least 2 fp64 ulp), relative to the terms.  A term that is switched
off has the interval [0, 0].

Derived state (`derived`).  state[2] == npix; state[3] == state[0] / npix and state[4] == state[1] / npix to the bit, recomputed in
float64 from the sums THE DEVICE wrote (one division each: nothing to count); both fp32 losses are the single roundings of those; a
switched-off term has exactly 0 in its sum and its loss.

Backward (`backward`), per element: G = ub phi + uh (p - g) F with ub = gout_B / N, uh = 2 gout_H / N; softmax dz_cls = G p om,
dz_c = -G p p_c; sigmoid dz_cls = G p q, every other channel 0.  The error is measured in ulps of the magnitude with every
difference replaced by the sum of its operands' magnitudes,
  M = (|ub| |phi| + |uh| (p + |g|) F) p w,     w = om (softmax, the class channel), p_c (softmax, the others), q (sigmoid),
against a budget of 4 x the largest error, in that unit, of torch's CPU fp32 evaluation of the very composition (fp32 softmax /
sigmoid, G in float64 from that fp32 p rounded once, then the fp32 products), at least 2 ulp, the largest over the (mode, alpha)
group of the test's inputs.  The backward kernel takes no state -- it reads the logits, the maps and the two upstream scalars --, so
"against the reference backward" and "end to end" are the same measurement here and one is made.  An element whose magnitude is 0
(ignored or out-of-range label, another sigmoid channel, both maps 0, a NULL or zero upstream gradient, one-channel softmax, a
padding channel) must be exactly 0."""
import numpy as np

import loss_ref as R
from seg_terms_ref import EPS, SIGMOID, SOFTMAX, acc_term, allowed, pow_allowance, ulp_of      # noqa: F401  (re-exported)

U = R.U
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def level_set(s):
    """dl_phi: the distance outside, 1 - the distance inside, 0 where the map is 0; the map is negated in float64."""
    s = np.asarray(s).astype(np.int64).astype(np.float64)
    return np.where(s > 0, np.sqrt(np.abs(s)), np.where(s < 0, 1.0 - np.sqrt(np.abs(s)), 0.0))


def field(t, p, alpha):
    """dl_field: |t|^(alpha / 2) + |p|^(alpha / 2), a zero value adding 0; at alpha == 2.0 the exact integer |t| + |p| < 2^32."""
    a = np.abs(np.asarray(t).astype(np.int64)).astype(np.float64)
    b = np.abs(np.asarray(p).astype(np.int64)).astype(np.float64)
    if alpha == 2.0:
        return a + b
    h = 0.5 * float(alpha)
    return np.where(a > 0.0, np.power(a, h), 0.0) + np.where(b > 0.0, np.power(b, h), 0.0)


def pow_pairs(t, p, alpha):
    """The (value, alpha / 2) pairs the map pair takes pow of: none at alpha == 2 or with the term off."""
    if alpha is None or alpha == 2.0:
        return []
    v = np.unique(np.abs(np.concatenate([np.asarray(t).reshape(-1), np.asarray(p).reshape(-1)]).astype(np.int64)))
    return [(float(x), 0.5 * float(alpha)) for x in v if x > 0]


class Pixels:
    """The per-pixel float64 quantities both kernels form.  z [npix, >= C] fp32 logits; lt: the label [npix] (softmax) or the target
    [npix, >= C] (sigmoid: only channel `cls` is read); tmap, pmap: integers [npix] (pmap None with alpha None); boundary: that
    term is on; alpha None: the Hausdorff term is off."""

    def __init__(self, z, lt, mode, C, cls, tmap, pmap, boundary, alpha):
        z = _f64(np.asarray(z, dtype=np.float32))[:, :C]
        self.z, self.C, self.mode, self.cls, self.npix = z, C, int(mode), int(cls), z.shape[0]
        self.boundary, self.alpha = bool(boundary), alpha
        n = self.npix
        hot = np.arange(C) == self.cls
        if self.mode == SOFTMAX:
            y = np.asarray(lt).reshape(n).astype(np.int64)
            self.ok = (y >= 0) & (y < C)                      # judged in 64 bits
            self.g = (y == self.cls).astype(np.float64)
            m = z.max(axis=1)
            e = np.exp(z - m[:, None])
            s = e.sum(axis=1)
            self.P = e / s[:, None]
            self.p = self.P[:, self.cls]
            self.om = (e * ~hot[None, :]).sum(axis=1) / s     # 1 - p: the others over the sum
            self.w = np.where(hot[None, :], self.om[:, None], self.P)
        else:
            self.ok = np.ones(n, dtype=bool)
            self.g = _f64(np.asarray(lt, dtype=np.float32)).reshape(n, -1)[:, self.cls]
            zc = z[:, self.cls]
            self.p, self.q = R.sigmoid64(zc), R.sigmoid64(-zc)
            self.w = np.where(hot[None, :], self.q[:, None], 0.0)
        self.tmap = np.asarray(tmap).reshape(n).astype(np.int64)
        self.phi = level_set(self.tmap) if self.boundary else np.zeros(n)
        if alpha is not None:
            self.pmap = np.asarray(pmap).reshape(n).astype(np.int64)
            self.F = field(self.tmap, self.pmap, alpha)
        else:
            self.pmap, self.F = None, np.zeros(n)


# ---- forward --------------------------------------------------------------------------------------------------------------------
def point_sums(px):
    """(S_B, S_H) at the float64 p."""
    v = px.ok.astype(np.float64)
    return float(np.sum(px.phi * px.p * v)), float(np.sum((px.p - px.g) ** 2 * px.F * v))


def p_interval(px, bp):
    """(lo, hi) [npix] of the class's p as the device may hold it."""
    if px.mode == SOFTMAX:
        a = allowed(bp, px.p) if px.C > 1 else 0.0           # one channel: p = 1 / 1 is exact
        return np.clip(px.p - a, 0.0, 1.0), np.clip(px.p + a, 0.0, 1.0)
    c = R.p_candidates(px.p)
    return c.min(axis=0), c.max(axis=0)


def forward_intervals(px, bp, pow_ulps=2.0):
    """((S_B lo, hi), (S_H lo, hi)).  bp: the softmax p budget in ulps of p (unused in sigmoid mode); pow_ulps: pow_allowance of
    the map's pairs."""
    v = px.ok.astype(np.float64)
    plo, phi = p_interval(px, bp)
    e = acc_term(px.npix)
    a, b = px.phi * plo * v, px.phi * phi * v                # monotone in p, of either sign
    mag = float(np.sum(np.maximum(np.abs(a), np.abs(b))))
    SB = (float(np.sum(np.minimum(a, b))) - e * mag, float(np.sum(np.maximum(a, b))) + e * mag)
    dlo, dhi = plo - px.g, phi - px.g
    far = np.maximum(dlo * dlo, dhi * dhi)
    near = np.where((dlo <= 0.0) & (dhi >= 0.0), 0.0, np.minimum(dlo * dlo, dhi * dhi))
    rel = e + (0.0 if px.alpha in (None, 2.0) else 2.0 * pow_ulps * EPS)
    SH = (float(np.sum(near * px.F * v)) * (1.0 - rel), float(np.sum(far * px.F * v)) * (1.0 + rel))
    return SB, SH


def derived(SB, SH, npix, boundary, hausdorff):
    """The five doubles of the state and the two fp32 losses from the given sums, as the last workgroup's thread 0 forms them."""
    n = float(npix)
    LB = SB / n if boundary else 0.0
    LH = SH / n if hausdorff else 0.0
    return np.array([SB, SH, n, LB, LH]), np.float32(LB), np.float32(LH)


# ---- backward -------------------------------------------------------------------------------------------------------------------
def upstream(npix, gout_b, gout_h, boundary, hausdorff):
    """(ub, uh) = (gout_B / N, 2 gout_H / N) from the fp32 upstream scalars; 0 for a NULL one or a term that is off."""
    ub = R.f32(gout_b) / float(npix) if boundary and gout_b is not None else 0.0
    uh = 2.0 * R.f32(gout_h) / float(npix) if hausdorff and gout_h is not None else 0.0
    return ub, uh


def g_of(px, ub, uh, p=None):
    """(G, its magnitude) [npix] at p (default: the float64 p)."""
    p = px.p if p is None else _f64(p)
    G = ub * px.phi + uh * (p - px.g) * px.F
    return G, abs(ub) * np.abs(px.phi) + abs(uh) * (p + np.abs(px.g)) * px.F


def backward(px, ub, uh):
    """(dz, magnitude), each [npix, C] float64."""
    G, Gm = g_of(px, ub, uh)
    v = px.ok.astype(np.float64)
    sign = np.where(np.arange(px.C) == px.cls, 1.0, -1.0)[None, :]
    with np.errstate(invalid="ignore"):
        dz = sign * (G * px.p * v)[:, None] * px.w
        mag = (Gm * px.p * v)[:, None] * px.w
    # 0 * inf cannot arise: G is finite for int32 maps at alpha <= 4 and fp32 upstream scalars over N
    return np.where(px.w == 0.0, 0.0, dz), np.where(px.w == 0.0, 0.0, mag)

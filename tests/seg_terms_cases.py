"""What tests/test_seg_terms_ref_host.py and tests/test_hip_seg_terms_kernels.py share beside tests/seg_terms_ref.py: the table of
cases, torch's CPU fp32 evaluation of the two kernels' own compositions -- the other fp32 implementation every budget is measured on
(loss_ref.budget) --, and the budgets per (mode, gamma) group, measured once per process."""
import collections
import functools

import numpy as np
import torch

import loss_ref as R
import seg_terms_ref as S

SOFTMAX, SIGMOID = S.SOFTMAX, S.SIGMOID
SMALL = ((1, 1), (5, 7), (257, 3))                # one pixel; one partial wave; four workgroups, the last one partial
LARGE = ((257, 256), (363, 362))                  # 257 workgroups: the slot loop's second trip; past the 512 cap: the grid-stride second trip
LARGE_PAIRS = ((3, 4), (16, 16))
TVERSKY = ((0.5, 0.5, 1.0, 1.0), (0.3, 0.7, 1.0, 0.75), (0.0, 1.0, 1.0, 2.0), (1.0, 0.0, 1.0, 4.0), (0.5, 0.5, 0.0, 1.0))
GAMMAS = (0.0, 0.5, 1.0, 2.0, 8.0)
GOUTS = ((0.5, 0.25), (-2.0, 3.0), (0.0, 1.0), (1e-30, 1e-30), (None, 0.25), (0.5, None))
EIGHT_OF_SIXTEEN = [13, 2, 7, 0, 15, 8, 5, 10]
LISTED = {1: ([0], []), 3: ([2, 0], [1], []), 5: ([4, 0, 2], [4, 0], [3]), 12: ([11, 0], [5], []), 16: (EIGHT_OF_SIXTEEN, [15, 0], [])}

# layout: "dense" (rows of ld); "view32" (C channels viewed inside rows of 32: scalar); "off1" (base one float into its allocation, ld 4);
# "tld8" (sigmoid: target rows of 8 beside logit rows of 4); "dld8" (gradient rows of 8 beside logit rows of 4)
Case = collections.namedtuple("Case", "H W C ld mode classes tv gamma nw gout kind layout")


def case_id(c):
    tv = "-" if c.tv is None else "a%gb%gs%gE%g" % c.tv
    return (f"{c.H}x{c.W}_C{c.C}ld{c.ld}_{'softmax' if c.mode == SOFTMAX else 'sigmoid'}_{'+'.join(map(str, c.classes)) or 'none'}_{tv}"
            f"_g{c.gamma}_nw{c.nw}_{c.gout[0]}_{c.gout[1]}_{c.kind}_{c.layout}")


def _grid():
    """Small maps x CE_PAIRS x both modes.  Every option is dealt by an index of its own in (mode mi, shape si, pair pi), so that no
    option is tied to a (C, ld) pair: over the three shapes a pair sees all its class lists, both parities of GOUTS, three Tversky sets
    and three gammas; tests/test_seg_terms_ref_host.py asserts the coverage."""
    out = []
    for mi, mode in enumerate((SOFTMAX, SIGMOID)):
        for si, (H, W) in enumerate(SMALL):
            for pi, (C, ld) in enumerate(R.CE_PAIRS):
                opts = LISTED[C]
                classes = opts[(si + pi + mi) % len(opts)]
                gamma = GAMMAS[(2 * si + pi + 3 * mi) % 5]
                if classes and (si + 2 * pi + mi) % 5 == 4:
                    gamma = None                                  # the Tversky term alone
                tv = TVERSKY[(si + 2 * pi + mi) % 5] if classes else None
                nw = (0, 1, C)[(si + pi) % 3] if mode == SIGMOID else (0 if (si + pi + mi) % 4 == 1 else C)
                out.append(Case(H, W, C, ld, mode, tuple(classes), tv, gamma, nw, GOUTS[(2 * si + pi + mi) % 6], "random", "dense"))
    return out


def _explicit():
    """What must not depend on the dealing, in both modes: for every (C, ld) the richest class list with both terms on and an ordinary
    upstream pair, at 35 pixels; for every (C, ld) no listed class (focal only: all 64 class slots of the state 0), at 771 pixels."""
    out = []
    for mi, mode in enumerate((SOFTMAX, SIGMOID)):
        for pi, (C, ld) in enumerate(R.CE_PAIRS):
            out.append(Case(5, 7, C, ld, mode, tuple(LISTED[C][0]), TVERSKY[(pi + mi) % 5], GAMMAS[1 + (pi + mi) % 4], C, GOUTS[(pi + mi) % 2], "random", "dense"))
            out.append(Case(257, 3, C, ld, mode, (), None, GAMMAS[(pi + 2 * mi) % 5], C if (pi + mi) % 2 else (0 if mode == SOFTMAX else 1), GOUTS[(1, 4, 0)[pi % 3]],
                            "random", "dense"))
    return out


def _large():
    out = []
    for k, (H, W) in enumerate(LARGE):
        for j, (C, ld) in enumerate(LARGE_PAIRS):
            for mode in (SOFTMAX, SIGMOID):
                classes = (2, 0) if C == 3 else tuple(EIGHT_OF_SIXTEEN)
                out.append(Case(H, W, C, ld, mode, classes, TVERSKY[1 + 2 * ((j + k) % 2)], (2.0, 8.0)[(j + k + mode) % 2], C, GOUTS[k], "random", "dense"))
    return out


def _layouts():
    out = []
    for H, W in SMALL:
        for mode in (SOFTMAX, SIGMOID):
            for layout in ("view32", "off1", "dld8") + (("tld8",) if mode == SIGMOID else ()):
                out.append(Case(H, W, 3, 4, mode, (2, 0), TVERSKY[1], 2.0, 3, GOUTS[0], "random", layout))
    return out


def _special():
    out = []
    for mode in (SOFTMAX, SIGMOID):
        # a listed class nobody has: alpha = 0, smooth = 0 makes its D exactly 0; alpha = 0, smooth = 1 makes its 1 - TI exactly 0
        out.append(Case(5, 7, 3, 4, mode, (1, 0), (0.0, 1.0, 0.0, 0.75), None, 0, (0.5, None), "absent", "dense"))
        out.append(Case(257, 3, 5, 8, mode, (1, 4), (0.0, 1.0, 1.0, 2.0), 1.0, 5, (0.5, 0.25), "absent", "dense"))
        out.append(Case(5, 7, 3, 4, mode, (1,), (0.0, 1.0, 0.0, 0.75), None, 0, (0.5, None), "absent", "dense"))      # alone: all of dz is 0
        out.append(Case(5, 7, 3, 4, mode, (2, 0), TVERSKY[0], 2.0, 3, (None, None), "random", "dense"))                # both NULL
        for gamma in (0.0, 0.5, 2.0, 8.0):
            out.append(Case(1, 64, 3, 4, mode, (2, 0), TVERSKY[1], gamma, 3, GOUTS[0], "planted", "dense"))
            out.append(Case(1, 64, 3, 4, mode, (2, 0), TVERSKY[1], gamma, 3, GOUTS[0], "planted_soft" if mode == SIGMOID else "planted", "dense"))
    seen = []
    for c in out:
        if c not in seen:
            seen.append(c)
    return seen


def _distinct(cases):
    seen = []
    for c in cases:
        if c not in seen:
            seen.append(c)
    return seen


CASES = _distinct(_grid() + _explicit() + _large() + _layouts() + _special())


@functools.lru_cache(maxsize=4)
def _inputs(H, W, C, kind):
    if kind.startswith("planted"):
        return S.planted_inputs(C)
    return S.inputs(H, W, C, 1000 * H + 10 * W + C, absent=1 if kind == "absent" else None)


def case_inputs(c):
    """(z [n, C], label [n] or target [n, C], cw [C] or None) of a case."""
    d = _inputs(c.H, c.W, c.C, c.kind)
    if c.mode == SOFTMAX:
        lt = d["label"]
    else:
        lt = d["soft"] if c.kind in ("random", "planted_soft") else d["hot"]
    return d["zs" if c.mode == SOFTMAX else "z"], lt, (d["cw"] if c.nw else None)


# ---- torch CPU fp32 compositions -----------------------------------------------------------------------------------------------------
def _t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _sp32(x):
    return torch.clamp(x, min=0.0) + torch.log1p(torch.exp(-torch.abs(x)))


def f32_sigmoid(z):
    zt = _t32(z)
    return (1.0 / (1.0 + torch.exp(-zt))).numpy()


def _softmax32(z, px):
    """(p, om, lp, onehot) in fp32, the kernel's composition: exp(z - m) times the reciprocal of their sum."""
    zt = _t32(z)
    m = zt.max(dim=1, keepdim=True).values
    e = torch.exp(zt - m)
    s = e.sum(dim=1, keepdim=True)
    inv = 1.0 / s
    hot = torch.from_numpy(px.onehot)
    om = (e * (~hot)).sum(dim=1, keepdim=True) * inv
    zy = (zt * hot).sum(dim=1, keepdim=True)
    lp = zy - (m + torch.log(s))
    return e * inv, om[:, 0], lp[:, 0], hot


def f32_forward(px, gamma, w):
    """(softmax p or None, the focal terms as seg_terms_ref.focal_terms shapes them, or None) in fp32."""
    g = None if gamma is None else torch.tensor(gamma, dtype=torch.float32)
    if px.mode == SOFTMAX:
        p, om, lp, _ = _softmax32(px.z, px)
        term = None
        if g is not None:
            wy = _t32(w[px.ys] * px.ok)
            term = (wy * (torch.pow(om, g) * -lp)).numpy()
        return p.numpy(), term
    if g is None:
        return None, None
    zt, t = _t32(px.z), _t32(px.t)
    pv, qv = 1.0 / (1.0 + torch.exp(-zt)), 1.0 / (1.0 + torch.exp(zt))
    return None, (_t32(w)[None, :] * (t * torch.pow(qv, g) * _sp32(-zt) + (1.0 - t) * torch.pow(pv, g) * _sp32(zt))).numpy()


def f32_backward(px, g0, g1, fscale, gamma, w):
    """dz [npix, C] of sg_seg_terms_bwd_kernel's expressions in torch fp32 from fp32 g0, g1 [C] and fscale."""
    g0, g1 = _t32(g0)[None, :], _t32(g1)[None, :]
    fs = torch.tensor(fscale, dtype=torch.float32)
    focal = gamma is not None and fscale != 0.0
    g = torch.tensor(0.0 if gamma is None else gamma, dtype=torch.float32)
    if px.mode == SOFTMAX:
        p, om, lp, hot = _softmax32(px.z, px)
        gg = torch.where(hot, g1, g0)
        d = p * (gg - (p * gg).sum(dim=1, keepdim=True))
        if focal:
            pt = (p * hot).sum(dim=1)
            k = -torch.pow(om, g)
            if gamma != 0.0:
                safe = torch.where(om != 0, om, torch.ones_like(om))
                k = k + torch.where(om != 0, g * pt * torch.pow(safe, g - 1.0) * lp, torch.zeros_like(om))
            ws = _t32(w[px.ys] * px.ok) * fs * k
            d = d + ws[:, None] * (hot.float() - p)
        return (d * torch.from_numpy(px.ok)[:, None]).numpy()
    zt, t = _t32(px.z), _t32(px.t)
    pv, qv = 1.0 / (1.0 + torch.exp(-zt)), 1.0 / (1.0 + torch.exp(zt))
    d = pv * qv * (g0 + t * (g1 - g0))
    if focal:
        neg = t * torch.pow(qv, g) * (g * pv * _sp32(-zt) + qv)
        pos = (1.0 - t) * torch.pow(pv, g) * (g * qv * _sp32(zt) + pv)
        d = d + _t32(w)[None, :] * fs * (pos - neg)
    return d.numpy()


# ---- one case's reference side ------------------------------------------------------------------------------------------------------
class Ref:
    """Everything about a case that needs no device: the pixels, the reference state, the fp32 compositions' errors."""

    def __init__(self, c):
        self.c = c
        z, lt, cw = case_inputs(c)
        self.z, self.lt, self.cw = z, lt, cw
        self.px = px = S.Pixels(z, lt, c.mode, c.C)
        self.w = S.class_weights(c.C, cw, c.nw)
        self.tv = c.tv if c.classes else (0.5, 0.5, 1.0, 1.0)
        self.state = S.reference_state(px, c.classes, self.tv, c.gamma, self.w)
        self.focal = c.gamma is not None
        # the fp32 compositions, each against float64 on the same inputs, in ulps of the stated magnitude
        p32, t32 = f32_forward(px, c.gamma, self.w)
        self.e_p = float(np.max(R.scaled_ulp_error(p32[px.ok], px.p[px.ok]))) if p32 is not None and px.ok.any() else 0.0
        self.e_t = 0.0
        if t32 is not None:
            term, mag = S.focal_terms(px, c.gamma, self.w)
            self.e_t = float(np.max(R.scaled_ulp_error(t32, term, mag)))
        self.g = S.upstream(self.state, c.classes, c.C, c.gout[0], c.gout[1], self.focal)
        self.dz, self.mT, self.mF = S.backward(px, *self.g, c.gamma, self.w)
        self.d32 = f32_backward(px, *self.g, c.gamma, self.w)
        self.e_d = float(np.max(R.scaled_ulp_error(self.d32, self.dz, self.mT + self.mF)))


@functools.lru_cache(maxsize=None)
def ref_of(c):
    return Ref(c)


def group_of(c):
    return (c.mode, c.gamma, c.kind.startswith("planted"))


@functools.lru_cache(maxsize=None)
def _p_budget(mode, planted):
    """The softmax p does not depend on gamma: its budget is measured over every case of the mode."""
    return max(2.0, 4.0 * max(ref_of(c).e_p for c in CASES if c.mode == mode and c.kind.startswith("planted") == planted))


@functools.lru_cache(maxsize=None)
def budgets(group):
    """(bp, bt, bd) in ulp for a (mode, gamma, planted) group: 4 x the largest error torch's CPU fp32 compositions show over every
    case of the group (the softmax p: of the (mode, planted) group), at least 2 -- the softmax p, the focal term, the gradient
    element (one more ulp where both parts are added)."""
    e = np.array([[r.e_t, r.e_d] for r in (ref_of(c) for c in CASES if group_of(c) == group)])
    return (_p_budget(group[0], group[2]),) + tuple(max(2.0, 4.0 * float(v)) for v in e.max(axis=0))


def grad_budget(c):
    joint = c.classes and c.gamma is not None and c.gout[0] is not None and c.gout[1] is not None
    return budgets(group_of(c))[2] + (1.0 if joint else 0.0)

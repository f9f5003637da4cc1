"""What tests/test_dist_terms_kernels_ref_host.py and tests/test_hip_dist_terms_kernels.py share beside tests/dist_terms_ref.py: the
table of cases, their inputs, torch's CPU fp32 evaluation of the two kernels' own compositions -- the other fp32 implementation every
budget is measured on (loss_ref.budget) --, and the budgets per (mode, alpha) group, measured once per process."""
import collections
import functools

import numpy as np
import torch

import dist_terms_ref as D
import loss_ref as R

SOFTMAX, SIGMOID = D.SOFTMAX, D.SIGMOID
SMALL = ((1, 1), (5, 7), (33, 31))                # one pixel; one partial wave; four workgroups, the last one partial
BLOB = (64, 64)                                   # the plane of the blob geometries: 16 full workgroups
LARGE = ((257, 256), (363, 362))                  # 257 workgroups: the slot loop's second trip; past the 512 cap: the grid-stride second trip
LARGE_PAIRS = ((3, 4), (16, 16))
ALPHAS = (0.5, 1.0, 1.5, 2.0, float(np.nextafter(2.0, 3.0)), 3.0, 4.0)
GEOMS = ("discs", "wall", "single", "synth")
GOUTS = ((0.5, 0.25), (-2.0, 3.0), (None, 0.25), (0.5, None), (0.0, 1.0), (1e-30, 1e-30), (None, None))
ORDINARY = GOUTS[:2]
BOTH, BOUNDARY_ALONE, HAUSDORFF_ALONE = 0, 1, 2
# (C, logit rows, gradient rows, layout).  layout: "dense"; "view32" (C channels viewed inside rows of 32: the scalar form of both
# kernels' loads); "off1" (every float operand's base one float into its allocation: the scalar form of vector-sized rows)
FORMS = (
    (1, 4, 4, "dense"), (2, 4, 4, "dense"), (3, 4, 4, "dense"), (4, 4, 4, "dense"), (12, 12, 12, "dense"), (16, 16, 16, "dense"),      # pad4(C)
    (1, 8, 8, "dense"), (3, 8, 8, "dense"), (4, 8, 8, "dense"), (2, 16, 16, "dense"), (12, 16, 16, "dense"),                           # rows of 8 and 16
    (3, 32, 4, "view32"), (3, 32, 32, "view32"), (3, 4, 4, "off1"),
    (3, 4, 3, "dense"), (3, 4, 5, "dense"), (3, 4, 8, "dense"), (3, 4, 20, "dense"), (3, 4, 32, "dense"), (16, 16, 20, "dense"),      # dl_store_row<0>, its trailing loop
    (4, 4, 5, "off1"), (3, 8, 4, "dense"),                                                # the last: sigmoid logits in rows of 8 beside vector gradient rows of 4
)

# tgt (sigmoid): "hot" one-hot of the label, "soft" uniform(0, 1).  kind: "random" logits 3 N(0, 1); "planted" loss_ref.GAN_PLANTED on
# pixels whose field is not zero; "saturated" +-40
Case = collections.namedtuple("Case", "H W C ld dld mode cls geom alpha boundary gout kind tgt layout")


def pad4(C):
    return (C + 3) // 4 * 4


def case_id(c):
    return (f"{c.H}x{c.W}_C{c.C}ld{c.ld}dld{c.dld}_{'softmax' if c.mode == SOFTMAX else 'sigmoid'}_cls{c.cls}_{c.geom}_a{c.alpha!r}_"
            f"{'B' if c.boundary else ''}{'H' if c.alpha is not None else ''}_{c.gout[0]}_{c.gout[1]}_{c.kind}_{c.tgt}_{c.layout}")


def _terms(which, alpha):
    """(alpha or None, boundary) of a term switch."""
    return (None, True) if which == BOUNDARY_ALONE else (alpha, which == BOTH)


def _grid():
    """Small planes x FORMS x both modes.  Every option is dealt by an index of its own in (mode mi, plane si, form fi), so that
    none is tied to a (C, ld, dld) form; tests/test_dist_terms_kernels_ref_host.py asserts the coverage."""
    out = []
    for mi, mode in enumerate((SOFTMAX, SIGMOID)):
        for si, (H, W) in enumerate(SMALL):
            for fi, (C, ld, dld, layout) in enumerate(FORMS):
                alpha, boundary = _terms((BOTH, BOUNDARY_ALONE, BOTH, HAUSDORFF_ALONE)[(fi + si + mi) % 4], ALPHAS[(fi + 2 * si + 3 * mi) % 7])
                out.append(Case(H, W, C, ld, dld, mode, (0, C - 1, C // 2)[(fi + si) % 3], GEOMS[(fi + 3 * si + mi) % 4], alpha, boundary,
                                GOUTS[(2 * fi + si + mi) % 7], "random", ("hot", "soft")[(fi + si + mi) % 2], layout))
    return out


def _explicit():
    """What must not depend on the dealing, in both modes: every form with both terms on under an ordinary upstream pair at 35 pixels."""
    out = []
    for mi, mode in enumerate((SOFTMAX, SIGMOID)):
        for fi, (C, ld, dld, layout) in enumerate(FORMS):
            out.append(Case(5, 7, C, ld, dld, mode, (C - 1, 0)[(fi + mi) % 2], GEOMS[(fi + mi) % 2], ALPHAS[(3 * fi + mi) % 7], True, ORDINARY[(fi + mi) % 2],
                            "random", ("soft", "hot")[fi % 2], layout))
    return out


def _blobs():
    """64 x 64: every geometry at every alpha and with the Hausdorff term off, in both modes."""
    out = []
    H, W = BLOB
    for mi, mode in enumerate((SOFTMAX, SIGMOID)):
        for ai, a in enumerate(ALPHAS + (None,)):
            for k in range(2):
                C, ld = ((3, 4), (4, 4), (12, 12), (2, 8))[(ai + k + mi) % 4]
                out.append(Case(H, W, C, ld, ld, mode, (ai + k) % C, GEOMS[(ai + 2 * k + mi) % 4], a, a is None or (ai + k) % 3 != 2,
                                ORDINARY[(ai + k) % 2], "random", ("hot", "soft")[(ai + k) % 2], "dense"))
        for gi, geom in enumerate(GEOMS):      # the measured setup: C = 3, both terms, every geometry at the two ends of alpha
            for a in (0.5, 4.0):
                out.append(Case(H, W, 3, 4, 4, mode, 0, geom, a, True, ORDINARY[0], "random", ("hot", "soft")[gi % 2], "dense"))
    return out


def _large():
    out = []
    for k, (H, W) in enumerate(LARGE):
        for j, (C, ld) in enumerate(LARGE_PAIRS):
            for mode in (SOFTMAX, SIGMOID):
                out.append(Case(H, W, C, ld, ld, mode, (0, C - 1)[(j + k) % 2], ("discs", "wall")[(j + k + mode) % 2], (4.0, 0.5, 1.5, 2.0)[(2 * j + k + mode) % 4],
                                True, ORDINARY[k], "random", ("soft", "hot")[(j + k) % 2], "dense"))
    return out


def _special():
    out = []
    for mode in (SOFTMAX, SIGMOID):
        for a in (None, 0.5, 2.0, 4.0):      # p next to 1 on a pixel with a field: om as others-over-sum, sigmoid(-z) for 1 - p
            out.append(Case(33, 31, 3, 4, 4, mode, 1, "discs", a, True, ORDINARY[0], "planted", "hot", "dense"))
            out.append(Case(33, 31, 3, 4, 4, mode, 1, "discs", a, True, ORDINARY[0], "planted", "soft", "dense"))
        for a in (1.0, 4.0):
            out.append(Case(5, 7, 3, 4, 4, mode, 0, "discs", a, True, ORDINARY[0], "saturated", "hot", "dense"))
        # maps at the edge of int32 at the upper end of alpha, each term alone and both
        for which in (BOTH, BOUNDARY_ALONE, HAUSDORFF_ALONE):
            a, b = _terms(which, 4.0)
            out.append(Case(5, 7, 3, 4, 4, mode, 2, "synth", a, b, ORDINARY[0], "random", "soft", "dense"))
        # a NULL upstream gradient beside a term that is on; both NULL
        for gout in ((None, 0.25), (0.5, None), (None, None)):
            out.append(Case(33, 31, 3, 4, 4, mode, 0, "discs", 3.0, True, gout, "random", "soft", "dense"))
    # one-channel softmax: om == 0, every dz exactly 0, L_B the mean of phi over the labelled pixels
    for geom in ("discs", "synth"):
        out.append(Case(33, 31, 1, 4, 4, SOFTMAX, 0, geom, 1.5, True, ORDINARY[0], "random", "hot", "dense"))
        out.append(Case(33, 31, 1, 4, 3, SOFTMAX, 0, geom, None, True, ORDINARY[1], "random", "hot", "dense"))
    return out


def _distinct(cases):
    seen, out = set(), []
    for c in cases:
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


CASES = _distinct(_grid() + _explicit() + _blobs() + _large() + _special())


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
SYNTH = (0, 1, -1, 2, -2, 2 ** 30, -2 ** 30, D.INT32_MAX, D.INT32_MIN, 5, -9, 1458, -225, 0, 3, -4)


def _disc(H, W, cy, cx, r):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy - cy) ** 2 + (xx - cx) ** 2 < r * r


def masks(H, W, geom):
    """(truth, prediction) bool [H, W] of a blob geometry.  discs: an open disc of radius 15/64 of the shorter side about
    (26/64 H, 26/64 W) and a smaller one (11/64) off its centre -- at 64 x 64 the radius-15 and radius-11 discs, maps -225 .. 1405; wall: one-pixel walls every 8th row and column with a gap
    per segment (cell_map of tests/test_hip_signed_edt.py) and the same walls moved by (2, 3); single: one inside pixel each."""
    s = min(H, W) / 64.0
    if geom == "discs":
        cy, cx = 26 * H // 64, 26 * W // 64
        return _disc(H, W, cy, cx, 15.0 * s), _disc(H, W, cy + int(round(5 * s)), cx + int(round(4 * s)), 11.0 * s)
    if geom == "wall":
        m = np.zeros((H, W), bool)
        m[::8, :] = True
        m[:, ::8] = True
        m[::8, 3::16] = False
        return m, np.roll(m, (2, 3), axis=(0, 1))
    assert geom == "single", geom
    t, p = np.zeros((H, W), bool), np.zeros((H, W), bool)
    t[H // 2, W // 2] = True
    p[(H // 2 + 3) % H, (W // 2 + 5) % W] = True
    return t, p


@functools.lru_cache(maxsize=None)
def maps(H, W, geom):
    """(t_sdsq, p_sdsq, truth mask) int32 [npix] x 2 and bool [npix]: util.signed_edt_sq of the masks, or -- the node reads its
    maps as numbers -- the integers of SYNTH dealt over the pixels, 0, +-1, +-2^30 and both ends of int32 among them."""
    n = H * W
    if geom == "synth":
        i = np.arange(n) + (H + W + 5) % 16
        t = np.array(SYNTH, dtype=np.int64)[i % 16].astype(np.int32)
        p = np.array(SYNTH, dtype=np.int64)[(7 * i + 3) % 16].astype(np.int32)
        return t, p, t < 0
    from supervised_gan_amd.util import signed_edt_sq
    truth, pred = masks(H, W, geom)
    return signed_edt_sq(truth).reshape(n), signed_edt_sq(pred).reshape(n), truth.reshape(n)


def planted_pixels(t_s, p_s, count):
    """The first `count` pixels on which the level set AND the Hausdorff field are non-zero (a map value of 0 or -1 has phi == 0)."""
    idx = np.flatnonzero((t_s != 0) & (t_s != -1))
    assert idx.size >= count
    return idx[:count]


@functools.lru_cache(maxsize=8)
def _inputs(H, W, C, cls, geom, kind):
    """dict: z [n, C] fp32; label int64 [n]: `cls` inside the truth mask, another class outside (C == 1: 0 everywhere), then -100,
    C, -1 and loss_ref.BIG_LABELS planted at both ends where the map has 16 pixels or more; hot [n, C]: the one-hot target of the
    label before the planting; soft [n, C] uniform(0, 1)."""
    rng = np.random.default_rng(1000 * H + 10 * W + C)
    n = H * W
    t_s, p_s, truth = maps(H, W, geom)
    z = (rng.standard_normal((n, C)) * 3.0).astype(np.float32)
    other = (cls + 1 + rng.integers(0, max(C - 1, 1), size=n)) % C
    lab = np.where(truth, cls, other).astype(np.int64)
    soft = rng.uniform(0.0, 1.0, size=(n, C)).astype(np.float32)
    if kind == "saturated":      # +-40: p reaches exactly 1.0 in fp32; every other pixel with the wrong class on top
        z = np.full((n, C), -40.0, np.float32)
        top = np.where(np.arange(n) % 2 == 0, lab, (lab + 1) % C)
        z[np.arange(n), top] = 40.0
    if kind == "planted":
        # every planted value four times: on the class's channel with the label / target on and off it, then on another channel
        idx = planted_pixels(t_s, p_s, 4 * len(R.GAN_PLANTED))
        k = np.arange(idx.size)
        ch = np.where(k % 4 < 2, cls, (cls + 1) % C)
        z[idx] = 0.0
        z[idx, ch] = np.repeat(np.array(R.GAN_PLANTED, dtype=np.float32), 4)
        lab[idx] = np.where(k % 2 == 0, cls, (cls + 2) % C)
        soft[idx] = np.where(k % 2 == 0, np.float32(0.9), np.float32(0.1))[:, None]
    hot = (np.arange(C)[None, :] == lab[:, None]).astype(np.float32)
    if n >= 16 and kind != "planted":
        lab[:2] = -100
        lab[2], lab[3] = C, -1
        lab[4], lab[5] = R.BIG_LABELS
        lab[-2:] = (C, -100)
        lab[-4:-2] = R.BIG_LABELS
    elif n >= 16:      # the planted pixels may stand at the front: the out-of-range labels go to the end alone
        lab[-6:] = (-100, -1) + tuple(R.BIG_LABELS) + (C, -100)
    return dict(z=z, label=lab, hot=hot, soft=soft)


def case_inputs(c):
    """(z [n, C], label [n] or target [n, C] with NaN in every channel but the class's, t_sdsq [n], p_sdsq [n])."""
    d = _inputs(c.H, c.W, c.C, c.cls, c.geom, c.kind)
    t_s, p_s, _ = maps(c.H, c.W, c.geom)
    if c.mode == SOFTMAX:
        return d["z"], d["label"], t_s, p_s
    t = np.full((c.H * c.W, c.C), np.nan, np.float32)
    t[:, c.cls] = d[c.tgt][:, c.cls]
    return d["z"], t, t_s, p_s


# ---- torch CPU fp32 compositions --------------------------------------------------------------------------------------------------
def _t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def f32_p(px):
    """(p [npix, C] or [npix], 1 - p [npix]) in fp32, the kernels' composition: exp(z - m) times the reciprocal of their sum and the
    others' share of it; 1 / (1 + exp(-z)) and 1 / (1 + exp(z))."""
    zt = _t32(px.z)
    if px.mode == SOFTMAX:
        m = zt.max(dim=1, keepdim=True).values
        e = torch.exp(zt - m)
        inv = 1.0 / e.sum(dim=1, keepdim=True)
        hot = torch.arange(px.C) == px.cls
        om = (e * (~hot)[None, :]).sum(dim=1, keepdim=True) * inv
        return (e * inv).numpy(), om[:, 0].numpy()
    zc = zt[:, px.cls]
    return (1.0 / (1.0 + torch.exp(-zc))).numpy(), (1.0 / (1.0 + torch.exp(zc))).numpy()


def f32_backward(px, ub, uh):
    """dz [npix, C] of sg_dist_loss_bwd_kernel's expressions: the fp32 p, G in float64 from it rounded once, the products in fp32."""
    p32, om32 = f32_p(px)
    pc = p32[:, px.cls] if px.mode == SOFTMAX else p32
    G32 = _t32(D.g_of(px, ub, uh, p=pc.astype(np.float64))[0].astype(np.float32))
    Gp = G32 * _t32(pc)
    hot = np.arange(px.C) == px.cls
    if px.mode == SOFTMAX:
        d = torch.where(torch.from_numpy(hot)[None, :], (Gp * _t32(om32))[:, None], -(Gp[:, None] * _t32(p32)))
    else:
        d = torch.where(torch.from_numpy(hot)[None, :], (Gp * _t32(om32))[:, None], torch.zeros(1))
    return (d * torch.from_numpy(px.ok)[:, None]).numpy()


# ---- one case's reference side ------------------------------------------------------------------------------------------------------
class Ref:
    """Everything about a case that needs no device: the pixels, the reference sums and gradient, the fp32 compositions' errors."""

    def __init__(self, c):
        self.c = c
        self.z, self.lt, self.t_s, self.p_s = case_inputs(c)
        self.hausdorff = c.alpha is not None
        self.px = px = D.Pixels(self.z, self.lt, c.mode, c.C, c.cls, self.t_s, self.p_s if self.hausdorff else None, c.boundary, c.alpha)
        self.SB, self.SH = D.point_sums(px)
        self.state, self.LB, self.LH = D.derived(self.SB, self.SH, px.npix, c.boundary, self.hausdorff)
        self.u = D.upstream(px.npix, c.gout[0], c.gout[1], c.boundary, self.hausdorff)
        self.dz, self.mag = D.backward(px, *self.u)
        self.p32 = f32_p(px)[0]
        self.pc32 = (self.p32[:, c.cls] if c.mode == SOFTMAX else self.p32).astype(np.float64)
        ok = px.ok
        self.e_p = float(np.max(R.scaled_ulp_error(self.p32[ok], px.P[ok]))) if c.mode == SOFTMAX and c.C > 1 and ok.any() else 0.0
        self.d32 = f32_backward(px, *self.u)
        self.e_d = float(np.max(R.scaled_ulp_error(self.d32, self.dz, self.mag)))
        self.pow_ulps = D.pow_allowance(D.pow_pairs(self.t_s, self.p_s, c.alpha))


@functools.lru_cache(maxsize=None)
def ref_of(c):
    return Ref(c)


def group_of(c):
    return (c.mode, c.alpha)


@functools.lru_cache(maxsize=None)
def p_budget(mode):
    """The softmax p does not depend on alpha: its budget is measured over every case of the mode."""
    return max(2.0, 4.0 * max(ref_of(c).e_p for c in CASES if c.mode == mode))


@functools.lru_cache(maxsize=None)
def grad_budget(group):
    """ulps of the stated magnitude for a (mode, alpha) group: 4 x the largest error torch's CPU fp32 composition shows over every
    case of the group, at least 2."""
    return max(2.0, 4.0 * max(ref_of(c).e_d for c in CASES if group_of(c) == group))

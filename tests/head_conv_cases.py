"""The case table of tests/test_hip_head_conv.py and tests/test_head_conv_host.py: the smallest shapes that reach every branch of the
three kernels of the one-channel stride-1 head (PatchGAN logits conv, CRN output conv) --
    sg_conv_head2_kernel<K,R>  (sgan_head.hip)   forward, thread = channel; variant "K4 R2 nrg1": taps, result rows per wave, row groups
    sg_conv_head_kernel<TH>    (sgan_igemm.hip)  forward through an LDS patch, what head2 declines; variant "TH4"
    sg_head_bwd_kernel<K>      (sgan_head.hip)   dX, dW, dbias and the two norm-backward sums; variant "K4 tiles<total> gy<grid.y>"
`kernel` / `variant` are what sgan_last_kernel() / sgan_last_variant() must report after the row's launch; fwd_dispatch and
bwd_dispatch restate sg_head_plan / sg_launch_head2 / sg_launch_head / sgan_conv_head_bwd for the host test.  Rows, operands, the
redraw away from activation kinks and the bounds are those of thin_conv_cases / thin_conv_ref.

Where the dispatch or the reference disagrees with a shape one would write down first, the row is the nearest shape that reaches
the branch:
  * sg_head_plan wants Ck % 32 == 0, so the partial channel chunk of head2 is Ck 96 / 160 / 320 (never a chunk cut inside a quad),
    and the backward kernel (which has no such rule) takes C 200 for its masked lanes;
  * a 1 x 1 map has no instance norm (x - mean = 0 sits on the activation's kink): the single-pixel rows read x plain;
  * a map one pixel wide has a result only with k4 p2 or k3 p1 (the backward kernel takes 2 pad <= k);
  * TH 8 by tile count would be a 256 x 256 map (8 MB); the table takes SGAN_HEAD_TH=8 on a 9 x 7 map instead, and k7 reaches TH 8
    through its 14 x 14 patch without a knob;
  * five rows sum more than thin_conv_ref.L_MAX products into a result and no nearer shape reaches their branch: the real head at Ck 512
    (16 x 512), the LDS-limit decline (no k, Ck with k^2 Ck <= L_MAX passes 64 KiB), and the 128 / 144 / 129-tile maps of the backward
    kernel's decline rule (16384 pixels per tap and more).  They are marked long: their bound carries thin_conv_ref.second_order(L + c)
    in the place of the constant 2 (LONG_ROWS; the host test pins the list and the term)."""
import functools
import zlib

import torch

import thin_conv_cases as K
import thin_conv_ref as R
from thin_conv_cases import cdiv
from thin_conv_ref import Layer, pad4

H2, HD, HB = "sg_conv_head2_kernel", "sg_conv_head_kernel", "sg_head_bwd_kernel"
HEAD_KERNELS = (H2, HD, HB)
R4, TH8, TH2, NO2 = {"SGAN_HEAD2_R": "4"}, {"SGAN_HEAD_TH": "8"}, {"SGAN_HEAD_TH": "2"}, {"SGAN_NO_HEAD2": "1"}
KNOBS = ("SGAN_HEAD2_R", "SGAN_HEAD_TH", "SGAN_NO_HEAD2")
MAX_TILES = 128      # sgan_conv_head_bwd: tiles per weight tensor past which the same-address atomics lose to the generic pair
EIGHT = [(1, 8), (2, 8), (7, 9), (8, 15), (9, 16), (11, 17), (17, 33), (8, 1)]


def hd(c, k=4, p=2):
    return Layer("conv", k, 1, p, c, 1)


class Fwd(K.Case):
    def __init__(self, name, kernel, variant, layer, sizes, norm=None, act=0, bias=False, tanh=False, env=None, long=False):
        super().__init__(name, "fwd", kernel, layer, sizes, norm, act, bias=bias, tanh=tanh, env=env, variant=variant)
        self.long = long


class Bwd(K.Case):
    """One backward pass of the head: the backward-data and the backward-weight job list over the same operands.  wt: backward-data
    reads the transposed weight copy; wj: a backward-weight list at all (False: dX and sums only, the raw entry point); bias: dbias
    wanted; sums: the two norm-backward sums wanted; own_dw: a dW / dbias per problem instead of one shared; rep: the sums go to
    SGAN_STAT_REPLICAS copies; wnorm: the normalisation the backward-weight list names (default: the same as backward-data);
    wide: the forward tensor sits in a buffer of twice its channels and the backward-data list names the pixel stride C all the same
    (only where x is read plain and the activation is none: dX does not depend on x then);
    expect: "launch", or "decline" (sgan_conv_head_bwd answers 1 and the generic pair runs)."""

    def __init__(self, name, variant, layer, sizes, norm=None, act=0, wt=True, wj=True, bias=True, sums=True, own_dw=False, rep=False, accum=False,
                 long=False, wnorm="same", wide=False, expect="launch"):
        super().__init__(name, "dgrad", HB, layer, sizes, norm, act, bias=bias, stats=sums and bool(norm), accum=accum, x=True, wt=wt)
        self.wj, self.own_dw, self.rep, self.long, self.wide, self.expect = wj, own_dw, rep, long, wide, expect
        self.wnorm = norm if wnorm == "same" else wnorm
        self.variant = variant


FWD2 = [
    # ---- head2 <4,2>: nrg 4 / 2 / 1, a partial chunk (96), an idle wave (192), two chunks for wave 0 (320); pads 0..3 ----
    Fwd("h2_k4p0_c64_1x1", H2, "K4 R2 nrg4", hd(64, 4, 0), [(4, 4)], bias=True),
    Fwd("h2_k4p1_c96_8x15_in_relu_tanh", H2, "K4 R2 nrg2", hd(96, 4, 1), [(9, 16)], "in", 1, tanh=True),
    Fwd("h2_k4p2_c128_4x16_bn_lrelu", H2, "K4 R2 nrg2", hd(128, 4, 2), [(3, 15)], "bn", 2, bias=True),
    Fwd("h2_k4p3_c192_7x17_relu_tanh", H2, "K4 R2 nrg1", hd(192, 4, 3), [(4, 14)], None, 1, bias=True, tanh=True),
    Fwd("h2_k4p2_c256_11x33_in_lrelu", H2, "K4 R2 nrg1", hd(256, 4, 2), [(10, 32)], "in", 2, bias=True),
    Fwd("h2_k4p0_c320_3x17_bn", H2, "K4 R2 nrg1", hd(320, 4, 0), [(6, 20)], "bn", 0),
    Fwd("h2_k4p1_c64_4x1_in", H2, "K4 R2 nrg4", hd(64, 4, 1), [(5, 2)], "in", 0),      # Hout 4 < R nrg = 8, Wout 1
    Fwd("h2_k4p2_c64_3prob_lrelu", H2, "K4 R2 nrg4", hd(64, 4, 2), [(66, 30), (9, 17), (1, 1)], None, 2, bias=True),
    Fwd("h2_k4p2_c128_8prob_in_relu", H2, "K4 R2 nrg2", hd(128, 4, 2), [(10, 12), (5, 5), (17, 3), (3, 33), (8, 8), (1, 20), (12, 1), (6, 40)],
        "in", 1, bias=True),
    # ---- head2 <3,2> ----
    Fwd("h2_k3p0_c64_1x1_bn_relu_tanh", H2, "K3 R2 nrg4", hd(64, 3, 0), [(3, 3)], "bn", 1, bias=True, tanh=True),
    Fwd("h2_k3p1_c160_21x19", H2, "K3 R2 nrg1", hd(160, 3, 1), [(21, 19)]),
    Fwd("h2_k3p2_c64_9x15_in_lrelu", H2, "K3 R2 nrg4", hd(64, 3, 2), [(7, 13)], "in", 2),
    # ---- SGAN_HEAD2_R=4: <4,4> and <3,4> (64 values per wave, no final pair shuffle), Hout 1 / 5 / 16 / 17 ----
    Fwd("h2r4_k4_c64_17x21_in_lrelu", H2, "K4 R4 nrg4", hd(64, 4, 2), [(16, 20)], "in", 2, bias=True, env=R4),
    Fwd("h2r4_k4_c256_5x18_relu", H2, "K4 R4 nrg1", hd(256, 4, 2), [(4, 17)], None, 1, env=R4),
    Fwd("h2r4_k4_c128_8x8_bn", H2, "K4 R4 nrg2", hd(128, 4, 1), [(9, 9)], "bn", 0, bias=True, env=R4),
    Fwd("h2r4_k3_c64_1x33_bn_lrelu_tanh", H2, "K3 R4 nrg4", hd(64, 3, 1), [(1, 33)], "bn", 2, bias=True, tanh=True, env=R4),
    Fwd("h2r4_k3_c192_16x16_in", H2, "K3 R4 nrg1", hd(192, 3, 1), [(16, 16)], "in", 0, env=R4),
]

FWD1 = [
    # ---- sg_conv_head_kernel <4>: Ck 32, k outside {3, 4}, pad >= k; Hp no multiple of 4, Wp 1 / 7 / 8 / 9 ----
    Fwd("hk_k4p2_c32_7x7_in_lrelu", HD, "TH4", hd(32, 4, 2), [(6, 6)], "in", 2, bias=True),
    Fwd("hk_k3p1_c32_5x8_relu", HD, "TH4", hd(32, 3, 1), [(5, 8)], None, 1),
    Fwd("hk_k5p2_c96_9x9_bn_lrelu_tanh", HD, "TH4", hd(96, 5, 2), [(9, 9)], "bn", 2, bias=True, tanh=True),      # ncb 3: the break
    Fwd("hk_k5p2_c64_3x1_in", HD, "TH4", hd(64, 5, 2), [(3, 1)], "in", 0),
    Fwd("hk_k4p4_c64_9x10_lrelu", HD, "TH4", hd(64, 4, 4), [(4, 5)], None, 2, bias=True),
    Fwd("hk_k2p0_c64_7x8_in_relu", HD, "TH4", hd(64, 2, 0), [(8, 9)], "in", 1),
    Fwd("hk_k3p1_c32_3prob", HD, "TH4", hd(32, 3, 1), [(13, 9), (2, 17), (6, 1)], bias=True),
    Fwd("hk_k4p1_c32_8prob_bn_relu", HD, "TH4", hd(32, 4, 1), [(10, 12), (5, 5), (17, 3), (3, 33), (8, 8), (2, 20), (12, 2), (6, 40)], "bn", 1),
    # ---- <8>: the 14 x 14 patch of k7; the knob on a small map (see the module docstring) ----
    Fwd("hk_k7p3_c32_11x9_in_lrelu_tanh", HD, "TH8", hd(32, 7, 3), [(11, 9)], "in", 2, bias=True, tanh=True),
    Fwd("hk_th8_k3p1_c32_9x7_lrelu", HD, "TH8", hd(32, 3, 1), [(9, 7)], None, 2, env=TH8),
    # ---- <2> ----
    Fwd("hk_th2_k4p2_c32_6x9_in_relu", HD, "TH2", hd(32, 4, 2), [(5, 8)], "in", 1, bias=True, env=TH2),
    # ---- SGAN_NO_HEAD2: the real head shape, two problems ----
    Fwd("hk_nohead2_k4p2_c256_2prob_in_lrelu", HD, "TH4", hd(256, 4, 2), [(10, 12), (17, 15)], "in", 2, bias=True, env=NO2),
    Fwd("hk_nohead2_k4p2_c512_2prob_in_lrelu", HD, "TH4", hd(512, 4, 2), [(9, 9), (14, 12)], "in", 2, bias=True, env=NO2, long=True),
    # ---- the LDS limit: 16 taps x 1024 channels of weights alone are 64 KiB -> sg_head_plan declines, the small-N kernel runs ----
    Fwd("hk_lds_decline_k4p2_c1024", K.SN64, "NR1 BKC1", hd(1024, 4, 2), [(7, 9)], "in", 2, bias=True, env=NO2, long=True),
]
FWD = FWD2 + FWD1

BWD = [
    # ---- one problem: k4 p 2 / 1 / 0, k3 p 1 / 0; C 64 .. 256; H 1 2 7 8 9 11 17, W 1 8 9 15 16 17 33; norm x act ----
    Bwd("hb_k4p2_c64_1x1", "K4 tiles1 gy1", hd(64, 4, 2), [(1, 1)]),
    Bwd("hb_k4p1_c96_2x8_in_relu", "K4 tiles1 gy2", hd(96, 4, 1), [(2, 8)], "in", 1),
    Bwd("hb_k4p0_c128_7x9_bn_lrelu", "K4 tiles1 gy2", hd(128, 4, 0), [(7, 9)], "bn", 2, wt=False),
    Bwd("hb_k4p2_c200_8x15_lrelu", "K4 tiles1 gy4", hd(200, 4, 2), [(8, 15)], None, 2),
    Bwd("hb_k4p2_c256_9x16_in_lrelu", "K4 tiles2 gy4", hd(256, 4, 2), [(9, 16)], "in", 2),
    Bwd("hb_k4p1_c64_11x17_bn", "K4 tiles4 gy1", hd(64, 4, 1), [(11, 17)], "bn", 0, wt=False),
    Bwd("hb_k4p2_c96_17x33_in", "K4 tiles9 gy2", hd(96, 4, 2), [(17, 33)], "in", 0),
    Bwd("hb_k3p1_c128_9x1_relu", "K3 tiles2 gy2", hd(128, 3, 1), [(9, 1)], None, 1),
    Bwd("hb_k3p0_c200_8x9_bn_relu", "K3 tiles1 gy4", hd(200, 3, 0), [(8, 9)], "bn", 1),
    Bwd("hb_k3p1_c256_2x16_in_lrelu", "K3 tiles1 gy4", hd(256, 3, 1), [(2, 16)], "in", 2, wt=False),
    # ---- operands left out ----
    Bwd("hb_dx_only_c128_2prob_in_lrelu", "K4 tiles5 gy2", hd(128, 4, 2), [(9, 17), (8, 8)], "in", 2, wj=False),
    Bwd("hb_no_dbias_k3_c64_11x15_bn_lrelu", "K3 tiles2 gy1", hd(64, 3, 1), [(11, 15)], "bn", 2, bias=False),
    Bwd("hb_no_sums_c96_7x9_in_relu", "K4 tiles1 gy2", hd(96, 4, 2), [(7, 9)], "in", 1, sums=False),
    # ---- problem lists: 3 and 8 of unequal size on one dW, and with a dW each; the replicated sums (9 tiles over 8 copies) ----
    Bwd("hb_3prob_c64_in_lrelu", "K4 tiles11 gy1", hd(64, 4, 2), [(17, 33), (7, 8), (1, 9)], "in", 2),
    Bwd("hb_8prob_c96_lrelu", "K4 tiles20 gy2", hd(96, 4, 2), [(1, 1)] + EIGHT[1:], None, 2),
    Bwd("hb_3prob_own_dw_k3_c128_bn_relu", "K3 tiles6 gy2", hd(128, 3, 1), [(9, 9), (2, 17), (11, 1)], "bn", 1, own_dw=True),
    Bwd("hb_8prob_own_dw_c64_in_lrelu", "K4 tiles20 gy1", hd(64, 4, 2), EIGHT, "in", 2, own_dw=True, wt=False),
    Bwd("hb_rep_sums_c256_17x33_in_lrelu", "K4 tiles9 gy4", hd(256, 4, 2), [(17, 33)], "in", 2, rep=True),
    # ---- the tile limit, accepted side: 8 x 16 tiles ----
    Bwd("hb_128tiles_c64_64x256_lrelu", "K4 tiles128 gy1", hd(64, 4, 2), [(64, 256)], None, 2, long=True),
]

DECLINED = [
    Bwd("hb_144tiles_c64_72x256_lrelu", None, hd(64, 4, 2), [(72, 256)], None, 2, long=True, expect="decline"),
    Bwd("hb_129tiles_c64_2prob_lrelu", None, hd(64, 4, 2), [(64, 256), (1, 1)], None, 2, long=True, expect="decline"),
    Bwd("hb_accumulate_c64_9x16_in_lrelu", None, hd(64, 4, 2), [(9, 16)], "in", 2, accum=True, expect="decline"),
    # the two lists read the forward tensor differently: backward-weight with the instance norm, backward-data plain ...
    Bwd("hb_norm_mismatch_c64_9x16_lrelu", None, hd(64, 4, 2), [(9, 16)], None, 2, wnorm="in", expect="decline"),
    # ... and with another pixel stride
    Bwd("hb_ld_mismatch_c64_9x16", None, hd(64, 4, 2), [(9, 16)], wide=True, expect="decline"),
]

ALL_BWD = BWD + DECLINED
LONG_ROWS = {"hk_nohead2_k4p2_c512_2prob_in_lrelu", "hk_lds_decline_k4p2_c1024", "hb_128tiles_c64_64x256_lrelu", "hb_144tiles_c64_72x256_lrelu",
             "hb_129tiles_c64_2prob_lrelu"}
IDS = K.IDS


# ---- operands and references ------------------------------------------------------------------------------------------------------------
def bwd_signs(row, d):
    """Both forms of the pre-activation value: xhat form (backward-data epilogue, the head kernel's backward-weight operand) and the
    prologue's x sc + sh (the generic backward-weight kernels)."""
    if row.act == 0:
        return []
    ys = [R.act_grad(p["x"], row.norm, row.act, d["gamma"], d["beta"])[2] for p in d["probs"]]
    ys += [R.prologue(p["x"], row.norm, row.act, d["gamma"], d["beta"])[2] for p in d["probs"]]
    if row.wnorm != row.norm:
        ys += [R.act_grad(p["x"], row.wnorm, row.act)[2] for p in d["probs"]] + [R.prologue(p["x"], row.wnorm, row.act)[2] for p in d["probs"]]
    return ys


@functools.lru_cache(maxsize=None)
def bwd_data(row):
    """thin_conv_cases.data() with the redraw rule applied to every tensor of bwd_signs."""
    seed = zlib.crc32(row.name.encode()) & 0xFFFFFF
    d = K._draw(row, seed)
    n = len(d["probs"])
    for attempt in range(1, 64):
        ys = bwd_signs(row, d)
        if all(R.margin(y) > R.MASK_MARGIN for y in ys):
            return d
        nxt = K._draw(row, seed + attempt)
        for i, y in enumerate(ys):
            p, q = d["probs"][i % n], nxt["probs"][i % n]
            near = y.abs() <= 4 * R.MASK_MARGIN * y.abs().max()
            p["x"] = torch.where(near, q["x"], p["x"])
    raise AssertionError(f"{row.name}: no draw keeps the activation margin")


@functools.lru_cache(maxsize=None)
def fwd_reference(case):
    d, L = K.data(case), case.layer
    return [R.op_forward(L, p["x"], d["w"], d["b"], norm=case.norm, act=case.act, gamma=d["gamma"], beta=d["beta"], tanh=case.tanh, long=case.long)
            for p in d["probs"]]


@functools.lru_cache(maxsize=None)
def bwd_reference(row):
    """(op_dgrad per problem, op_wgrad per dW).  Computed once, never modified."""
    d, L = bwd_data(row), row.layer
    dg = [R.op_dgrad(L, p["dy"], d["w"], p["H"], p["W"], x=p["x"], norm=row.norm, act=row.act, gamma=d["gamma"], beta=d["beta"], prev=p["prev"])
          for p in d["probs"]]
    tup = [(p["x"], p["dy"], row.wnorm, row.act, d["gamma"], d["beta"]) for p in d["probs"]]
    return dg, [R.op_wgrad(L, g, long=row.long) for g in ([[t] for t in tup] if row.own_dw else [tup])]


def head_dw_bound(row, ref):
    """sg_head_bwd_kernel forms the operand from xhat: C_PRO_XHAT in the place of C_PRO."""
    return ref["dw_bound"] + ((R.C_PRO_XHAT - R.C_PRO) * R.U * ref["MA"] if row.wnorm else 0.0)


def reduction_length(case):
    """The largest number of products summed into one element of any output of the row."""
    L = case.layer
    if case.op == "fwd":
        return L.k * L.k * pad4(L.cin)
    px = [H * W for H, W in case.sizes]
    return max(L.k * L.k * 4, max(px) if case.own_dw else sum(px))


# ---- the launchers, restated ------------------------------------------------------------------------------------------------------------
def fwd_dispatch(case):
    """(kernel, variant, tiles) of sg_dispatch_igemm for a one-channel stride-1 forward row."""
    L, env = case.layer, case.env
    ck, k, p = pad4(L.cin), L.k, L.p
    outs = [L.out_hw(H, W) for H, W in case.sizes]
    assert L.s == 1 and L.cout == 1 and not L.tr
    # sg_head_plan
    plan = ck % 32 == 0 and ck <= 1024 and 4 <= k * k <= 49 and "SGAN_NO_HEAD_KERNEL" not in env
    th = 8 if sum(cdiv(ho, 8) * cdiv(wo, 8) for ho, wo in outs) >= 1024 else 4
    if env.get("SGAN_HEAD_TH") in ("8", "4", "2"):
        th = int(env["SGAN_HEAD_TH"])
    pph, ppw = th + k - 1, 8 + k - 1
    if pph * ppw > 32 * th:
        th, pph = 8, 8 + k - 1
    lds = ((pph * ppw * 144 + 255) & ~255) + k * k * ck * 4 + 49 * 4 + 2 * ck * 4
    plan = plan and pph * ppw <= 256 and lds <= 64 * 1024
    if not plan:
        kt = k * k * ck
        return (K.SN64 if kt >= 2048 else K.SN16 if kt >= 256 else K.SN8), "NR1 BKC1", None
    # sg_launch_head2
    if "SGAN_NO_HEAD2" not in env and ck >= 64 and k in (3, 4) and p < k:
        nch = cdiv(ck, 64)
        nrg = 1 if nch >= 3 else 2 if nch == 2 else 4
        r = 4 if env.get("SGAN_HEAD2_R") == "4" else 2
        return H2, f"K{k} R{r} nrg{nrg}", sum(cdiv(wo, 16) * cdiv(ho, r * nrg) for ho, wo in outs)
    return HD, f"TH{th}", sum(cdiv(ho, th) * cdiv(wo, 8) for ho, wo in outs)


def bwd_tiles(row):
    return [cdiv(W, 16) * cdiv(H, 8) for H, W in row.sizes]


def bwd_dispatch(row):
    """("launch", variant) or ("decline", reason) of sgan_conv_head_bwd."""
    L, C, t = row.layer, pad4(row.layer.cin), bwd_tiles(row)
    if L.tr or L.s != 1 or L.k not in (3, 4) or L.cout != 1 or C < 64 or 2 * L.p > L.k:
        return "decline", "layer"
    if row.accum:
        return "decline", "accumulate"
    if row.wj and (row.wnorm != row.norm or row.wide):
        return "decline", "lists differ"
    if row.wj and (max(t) if row.own_dw else sum(t)) > MAX_TILES:
        return "decline", "tiles"
    return "launch", f"K{L.k} tiles{sum(t)} gy{cdiv(C, 64)}"

"""The case table of tests/test_hip_split_conv.py, tests/test_hip_split_wgrad.py, tests/test_hip_fused_bwd.py and
tests/test_split_conv_host.py: the smallest shapes that reach the branches of the split 16-bit-plane conv kernels (the default
arithmetic of training, SGAN_MATH_BF16X3, and SGAN_MATH_BF16X1 beside it) -- sg_igemm3_kernel, sg_igemm3p_kernel, sg_wgrad3_kernel,
sg_bwd_fused_kernel and, behind a K split, sg_splitk_epilogue_kernel.

Rows are thin_conv_cases.Case objects with two more fields: `mode` ("bf16x3" / "bf16x1", also the row's `math`) and `planes` (True:
the gradient tensor carries its published maximum, so backward-data / backward-weight form fp16 planes of dY * 2^s; False: bf16
planes; the forward pass always runs on fp16 planes).  Operands are thin_conv_cases.data's (x ~ 1.5 N + 0.3, w ~ 0.05 N, bias ~ 0.1 N,
dY ~ N, redrawn near an activation's kink until MASK_MARGIN holds).

`kernel` is what sgan_last_kernel() reports (names unchanged), `variant` what sgan_last_variant() reports:
    sg3_launch              "ks<k> PRO<0|1> F16<0|1>"  the K split that ran, the prologue, fp16 planes  (+ " noslab": a planned split
                            found no workspace and ran unsplit)
    sg3p_launch             "AIT<2|4|6> KW<1|2> PRO<0|1> F16<0|1>"  the patch form (<= 128 / <= 256 patch pixels / stride-2 parity
                            planes), the wave groups per workgroup
    sgw3_launch             "PRO<0|1> F16<0|1> per<c> nsplit a,b,.."  the 32-pixel chunks per workgroup the split aims at, the pixel
                            split of every problem
    sg_conv_bwd_fused_impl  "DV<n> WV<n> ks<k> F16<0|1> WPRO<0|1> nsplit a,b,.."  the two bodies, the K split of the backward-data
                            half, the planes it was ACTUALLY formed from (a published maximum on a plan other than 6 is re-planned
                            on bf16 planes and reads F160), the backward-weight prologue and pixel splits
The planners that decide them (sg_igemm3_eligible, sg3_pick_tile with the SGAN_TILE3 force rules, sg3p_plan / sg3p_wanted with the
SGAN_IGEMM3P force, the kw2 rule, sgw3_covers, sgw3_prepare, sg_igemm3_fuse_plan with the SGAN_FUSE_KS_WGS cap, sg_wgrad3_fuse_plan,
and wide_conv_cases.plan_ksplit for sg_plan_ksplit) are restated below with the library's default thresholds.
tests/test_split_conv_host.py holds every row to the restatement, the GPU tests hold the same strings to the library: a threshold that
moves turns a row red instead of taking it silently off its branch.

Only the knobs the library reads per call are used (SGAN_TILE3, SGAN_IGEMM3P).  Out of reach of an in-process test, because their
knob is read once per process: sg_igemm3_kernel<64,64,2,2> WITHOUT two k-tiles per barrier (SGAN_KB2=0; the default, KB2, is what
every <64,64,2,2> row runs), the XCD-contiguous order of the fused launch (wmode 1, SGAN_FUSED_WXCD), a patch launch past
SGAN_PATCH_KW_MAX workgroups, N = 32 on the patch kernel (SGAN_PATCH_N32).  All ten DV x WV pairs of sg_bwd_fused_kernel are reached: the patch plans (DV 1 / 2 / 5) need more than 32
result channels (Cin) and gathered channels (Cout) in multiples of 32, WV 2 needs 32 <= Cout < 64, so the patch x WV 2 rows are the layers
with Cout = 32 exactly; DV 6 needs Cin <= 32; DV 3 is every other layer.  DV 4 is retired (sgan_fused.hip).

The model a row is held to (reference()): the exact float64 sum of the plane products the kernel forms -- plane_model's split_f16 /
split_bf16 / _pairs / _shift put through the three loops of thin_conv_ref (which know output_padding and can leave out a tap) -- and
M, the same sum over magnitudes.  Gates, per element, none left out:
  strict rows (no prologue, or ReLU / LeakyReLU only, which the host reproduces bit for bit; every backward-data row: dY is read
  plain, and the epilogue's xhat / y are thin_conv_ref.act_grad's fp32 expressions):
      |gpu - model| <= K u M + K 2^-149 + c,   u = 2^-24, K = taps in bounds x stored channels (pixels for backward-weight),
  c = u |bias| and one more u M for the bias add (forward: G1 of test_hip_plane_range.py), (C0_DGRAD) u M for act' / accumulate /
  second order with |previous| in M (backward-data), u M for the atomic add into a prefilled dw.  The plane products are exact in
  fp32 (11 x 11 or 8 x 8 bit significands), so what is left is fp32 accumulation.
  normalised rows (InstanceNorm / BatchNorm on load): the kernel's a' may differ from the host's a by the C_PRO roundings,
  |a' - a| <= 6 u A (thin_conv_ref), and a changed a re-splits: with S(a) = hi + lo, |S(a) - a| <= r |a| + 2^-25, r = 2^-22 for fp16
  planes (11 + 11 bits; 2^-25 = half the spacing of fp16's subnormals covers every plane that goes subnormal, so nothing needs to be
  avoided but overflow, which is asserted), r = 2^-16 for bf16 planes (8 + 8 bits).  The kernel forms sum S(a') b_hi + a'_hi b_lo, the
  model sum S(a) b_hi + a_hi b_lo, |a'_hi - a_hi| <= 6 u A + 2 h |a| with h = 2^-11 (fp16) / 2^-8 (bf16) and |b_lo| <= h |b_hi|:
      extra = C_PRO u M_A + (2 r + 2 h^2) / u * u M + 2 * 2^-25 sum |b|   = 8 u M_A + 16 u M (fp16) / 1024 u M (bf16) + u sum |b| ...
  (2 r + 2 h^2 = 2^-21 + 2^-21 = 16 u; bf16: 2^-15 + 2^-15 = 1024 u).  bf16x1 forms a'_hi b_hi alone: extra = 8 u M_A + 2 h M
  (2^14 u M on fp16 planes, 2^17 u M on bf16 planes) + u sum |b|.  None of it is measured.
  every row: G3 of test_hip_plane_range.py -- max-norm distance from the fp64 result of the unrounded operands under 1e-3 where the
  contract applies (bf16x3, or fp16 planes), under 3e-6 for bf16x3 on fp16 planes."""
import functools

import torch

import plane_model as PM
import thin_conv_cases as K
import thin_conv_ref as R
import wide_conv_cases as W
from thin_conv_cases import Case, cdiv, ct, cv

U = R.U
MIN_PIXELS = 256      # SGAN_BF16X3_MIN_PIXELS


def IG3(tile, x1=False):
    return f"sg_igemm3_kernel<{tile}{',x1' if x1 else ''}>"


def IG3P(s2=False, x1=False):
    return f"sg_igemm3p_kernel<64{',s2' if s2 else ''}{',x1' if x1 else ''}>"


def WG3(tile, x1=False):
    return f"sg_wgrad3_kernel<{tile}{',x1' if x1 else ''}>"


T128x32, T64, T128x64, T128 = "128,32,4,1", "64,64,2,2", "128,64,2,2", "128,128,2,4"
W64, W32 = "64,64,2,2", "32,128,1,4"
NOPATCH, PATCH = {"SGAN_IGEMM3P": "0"}, {"SGAN_IGEMM3P": "1"}
F128x64, F128 = {"SGAN_TILE3": "128x64", "SGAN_IGEMM3P": "0"}, {"SGAN_TILE3": "128x128", "SGAN_IGEMM3P": "0"}
FUSED, FUSED_X1, FUSED_WX1 = "sg_bwd_fused_kernel", "sg_bwd_fused_kernel<x1>", "sg_bwd_fused_kernel<wgrad x1>"


def S(name, op, kernel, layer, sizes, norm=None, act=0, mode="bf16x3", planes=False, **kw):
    c = Case(name, op, kernel, layer, sizes, norm, act, math=mode, **kw)
    c.mode, c.planes = mode, bool(planes) or op == "fwd"
    return c


X1 = dict(mode="bf16x1")
_3P = [(16, 16), (17, 19), (20, 24)]

FWD = [
    # ---- sg_igemm3_kernel<128,32,4,1>: N <= 32 ----
    S("f_128x32_n24", "fwd", IG3(T128x32), cv(16, 24, 3, 1, 1), [(16, 17)], bias=True, variant="ks1 PRO0 F161"),
    S("f_128x32_n32_lrelu_stats", "fwd", IG3(T128x32), cv(16, 32, 3, 1, 1), [(17, 19)], None, 2, bias=True, stats=True, variant="ks1 PRO1 F161"),
    S("f_128x32_n24_bn_relu", "fwd", IG3(T128x32), cv(16, 24, 3, 1, 1), [(16, 17)], "bn", 1, bias=True, stats=True, variant="ks1 PRO1 F161"),
    S("f_128x32_n24_x1", "fwd", IG3(T128x32, True), cv(16, 24, 3, 1, 1), [(16, 17)], bias=True, variant="ks1 PRO0 F161", **X1),
    # ---- <64,64,2,2>: unsplit, split 8 into a workspace (and, without one, " noslab": test_hip_split_conv.NOSLAB) ----
    S("f_64x64_unsplit", "fwd", IG3(T64), cv(16, 64, 3, 1, 1), [(16, 17)], bias=True, variant="ks1 PRO0 F161"),
    S("f_64x64_split8", "fwd", IG3(T64), cv(64, 64, 4, 2, 1), [(32, 32)], None, 1, bias=True, stats=True, variant="ks8 PRO1 F161"),
    S("f_64x64_in_lrelu", "fwd", IG3(T64), cv(16, 64, 3, 1, 1), [(16, 18)], "in", 2, stats=True, variant="ks1 PRO1 F161"),
    S("f_64x64_x1_relu", "fwd", IG3(T64, True), cv(32, 64, 3, 1, 1), [(16, 17)], None, 1, env=NOPATCH, variant="ks1 PRO1 F161", **X1),
    # ConvT k3 s2 p1 op1: phases of 1 / 2 / 2 / 4 taps = 5 / 9 / 9 / 17 k-tiles, split 4 by the longest: the short phases' trailing
    # splits are empty and write slabs of zeros
    S("f_convT_k3_short_phases_split4", "fwd", IG3(T64), ct(136, 64, 3, 2, 1, 1), [(16, 16)], bias=True, stats=True, variant="ks4 PRO0 F161"),
    # ---- <128,64,2,2> and <128,128,2,4>, forced: N no multiple of the tile, pixels no multiple of 128, three problems ----
    S("f_128x64_n72", "fwd", IG3(T128x64), cv(16, 72, 3, 1, 1), [(17, 19)], bias=True, env=F128x64, variant="ks1 PRO0 F161"),
    S("f_128x64_n40_3prob_lrelu", "fwd", IG3(T128x64), cv(16, 40, 3, 1, 1), _3P, None, 2, stats=True, env=F128x64, variant="ks1 PRO1 F161"),
    S("f_128x128_n136", "fwd", IG3(T128), cv(16, 136, 3, 1, 1), [(17, 19)], bias=True, env=F128, variant="ks1 PRO0 F161"),
    S("f_128x128_n72_3prob", "fwd", IG3(T128), cv(24, 72, 3, 1, 1), _3P, bias=True, env=F128, variant="ks1 PRO0 F161"),
    # ---- sg_igemm3p_kernel: AIT 2 (k3, k4), AIT 4 (k7: 14 x 14 patch), AIT 6 (stride 2); KW 2 at 2 and 4 channel blocks, KW 1 at 3 ----
    S("p_ait2_k3_kw2_ncb2", "fwd", IG3P(), cv(64, 64, 3, 1, 1), [(17, 19)], bias=True, env=PATCH, variant="AIT2 KW2 PRO0 F161"),
    S("p_ait2_k4_kw2_ncb4_2prob_relu", "fwd", IG3P(), cv(128, 64, 4, 1, 2), [(16, 16), (17, 19)], None, 1, stats=True, env=PATCH, variant="AIT2 KW2 PRO1 F161"),
    S("p_ait2_kw1_ck96", "fwd", IG3P(), cv(96, 64, 3, 1, 1), [(17, 19)], bias=True, env=PATCH, variant="AIT2 KW1 PRO0 F161"),
    S("p_ait4_k7", "fwd", IG3P(), cv(32, 64, 7, 1, 3), [(16, 17)], bias=True, env=PATCH, variant="AIT4 KW1 PRO0 F161"),
    S("p_ait6_k4s2", "fwd", IG3P(True), cv(32, 64, 4, 2, 1), [(33, 35)], bias=True, env=PATCH, variant="AIT6 KW1 PRO0 F161"),
    S("p_ait6_k3s2_lrelu", "fwd", IG3P(True), cv(32, 72, 3, 2, 1), [(33, 35)], None, 2, env=PATCH, variant="AIT6 KW1 PRO1 F161"),
    S("p_ait2_in_relu", "fwd", IG3P(), cv(64, 64, 3, 1, 1), [(16, 18)], "in", 1, stats=True, env=PATCH, variant="AIT2 KW2 PRO1 F161"),
    S("p_ait2_x1", "fwd", IG3P(x1=True), cv(64, 64, 3, 1, 1), [(16, 16)], bias=True, env=PATCH, variant="AIT2 KW2 PRO0 F161", **X1),
]

_EPI = dict(x=True, stats=True)
DGRAD = [
    # ---- the raw product on <128,32,4,1> (N = Cin <= 32): bf16 planes, fp16 planes (published maximum), one plane ----
    S("d_128x32_raw_bf16", "dgrad", IG3(T128x32), cv(24, 32, 3, 1, 1), [(16, 17)], variant="ks1 PRO0 F160"),
    S("d_128x32_raw_f16", "dgrad", IG3(T128x32), cv(24, 32, 3, 1, 1), [(16, 17)], planes=True, variant="ks1 PRO0 F161"),
    S("d_128x32_raw_x1", "dgrad", IG3(T128x32, True), cv(24, 32, 3, 1, 1), [(16, 17)], variant="ks1 PRO0 F160", **X1),
    # ---- the epilogue act'(norm(x)) with both norm-backward sums: in the kernel, and in sg_splitk_epilogue_kernel; accumulate ----
    S("d_128x32_epi_bn_relu", "dgrad", IG3(T128x32), cv(24, 32, 3, 1, 1), [(16, 17)], "bn", 1, variant="ks1 PRO0 F160", **_EPI),
    S("d_128x32_accum_f16", "dgrad", IG3(T128x32), cv(24, 32, 3, 1, 1), [(16, 17)], planes=True, accum=True, variant="ks1 PRO0 F161"),
    S("d_64x64_split4_epi_in_lrelu", "dgrad", IG3(T64), cv(64, 128, 4, 2, 1), [(32, 32)], "in", 2, env=NOPATCH, variant="ks4 PRO0 F160", **_EPI),
    S("d_64x64_split4_accum_bn_relu", "dgrad", IG3(T64), cv(64, 128, 4, 2, 1), [(32, 32)], "bn", 1, accum=True, env=NOPATCH, variant="ks4 PRO0 F160", **_EPI),
    S("d_128x64_n40_3prob", "dgrad", IG3(T128x64), cv(40, 16, 3, 1, 1), _3P, env=F128x64, variant="ks1 PRO0 F160"),
    # ---- the patch kernel: a stride-2 Conv's four phases of 2 x 2 taps (AIT 2), a stride-2 ConvT's parity planes (s2, AIT 6) ----
    S("pd_conv_s2_phases", "dgrad", IG3P(), cv(64, 128, 4, 2, 1), [(32, 34)], env=PATCH, variant="AIT2 KW2 PRO0 F160"),
    S("pd_conv_s2_phases_f16_epi", "dgrad", IG3P(), cv(64, 128, 4, 2, 1), [(32, 34)], "in", 2, planes=True, env=PATCH, variant="AIT2 KW2 PRO0 F161", **_EPI),
    S("pd_convT_s2", "dgrad", IG3P(True), ct(64, 64), [(16, 17)], env=PATCH, variant="AIT6 KW1 PRO0 F160"),
    S("pd_k3_x1", "dgrad", IG3P(x1=True), cv(64, 96, 3, 1, 1), [(17, 19)], env=PATCH, variant="AIT2 KW1 PRO0 F160", **X1),
]

WGRAD = [
    # ---- <64,64,2,2>: Cout 64 and 72 (a ragged second row tile); taps x Cin = 144 no multiple of 64; pixels no multiple of 32 ----
    S("w_64x64_c64", "wgrad", WG3(W64), cv(16, 64, 3, 1, 1), [(17, 19)], bias=True, variant="PRO0 F160 per4 nsplit 3"),
    S("w_64x64_c72_f16", "wgrad", WG3(W64), cv(16, 72, 3, 1, 1), [(17, 19)], planes=True, bias=True, variant="PRO0 F161 per4 nsplit 3"),
    S("w_64x64_3prob_nsplit_prefill_lrelu", "wgrad", WG3(W64), cv(16, 64, 3, 1, 1), [(40, 40), (20, 20), (16, 16)], None, 2, bias=True, accum=True,
      variant="PRO1 F160 per4 nsplit 13,4,2"),
    S("w_64x64_in_lrelu", "wgrad", WG3(W64), cv(16, 64, 3, 1, 1), [(16, 18)], "in", 2, bias=True, variant="PRO1 F160 per4 nsplit 3"),
    S("w_64x64_x1", "wgrad", WG3(W64, True), cv(16, 64, 3, 1, 1), [(17, 19)], bias=True, variant="PRO0 F160 per4 nsplit 3", **X1),
    # ---- <32,128,1,4>: Cout 32, 40, 56 ----
    S("w_32x128_c32", "wgrad", WG3(W32), cv(16, 32, 3, 1, 1), [(17, 19)], bias=True, variant="PRO0 F160 per4 nsplit 3"),
    S("w_32x128_c40_relu_f16", "wgrad", WG3(W32), cv(24, 40, 3, 1, 1), [(17, 19)], None, 1, planes=True, bias=True, variant="PRO1 F161 per4 nsplit 3"),
    S("w_32x128_c56_convT_bn_relu", "wgrad", WG3(W32), ct(16, 56), [(16, 17)], "bn", 1, bias=True, variant="PRO1 F160 per4 nsplit 3"),
]
# A prefilled dw is bit-equal to plain + previous only where ONE workgroup owns the element.  No row of this size has such an element:
# a map of at least SGAN_BF16X3_MIN_PIXELS is 8 chunks, and sgw3_prepare aims at per = 4 chunks per workgroup until the launch has
# 448 k x Cout tiles (256 -> 512 channels at k4), so every dw element is the fp32 atomic sum of at least two workgroups; the prefilled row is
# therefore held to the bound with |previous| in M (one more rounding, c = 1), as are its prefilled bias gradients.

# ---- the fused launch: (name, backward-data half, backward-weight half, variant or None = refused, kernel, dgrad_math, workspace) ----
# Both halves are the same layer at the same sizes with their own operands (the C entry compares nothing else); the backward-weight
# half never carries a published maximum (the entry builds it with bf16 planes).
def _pair(name, layer, sizes, variant, kernel=FUSED, dplanes=False, wnorm=None, wact=0, dmode="bf16x3", wmode="bf16x3", env=None, ws=True, dkw=None):
    d = S(name + ":d", "dgrad", None, layer, sizes, mode=dmode, planes=dplanes, env=env, **(dkw or {}))
    w = S(name + ":w", "wgrad", None, layer, sizes, wnorm, wact, mode=wmode, bias=True, env=env)
    return name, d, w, variant, kernel, ws


_2P = [(16, 16), (17, 19)]
PAIRS = [
    _pair("fu_dv1_wv1", cv(64, 64, 3, 1, 1), _2P, "DV1 WV1 ks1 F160 WPRO0 nsplit 2,3", env=PATCH),
    _pair("fu_dv1_wv2", cv(64, 32, 3, 1, 1), _2P, "DV1 WV2 ks1 F160 WPRO1 nsplit 2,3", wact=2, env=PATCH),
    _pair("fu_dv2_wv1", cv(64, 64, 7, 1, 3), _2P, "DV2 WV1 ks1 F160 WPRO0 nsplit 2,3", env=PATCH),
    _pair("fu_dv2_wv2", cv(64, 32, 7, 1, 3), _2P, "DV2 WV2 ks1 F160 WPRO0 nsplit 2,3", env=PATCH),
    _pair("fu_dv3_wv1", cv(64, 72, 3, 1, 1), _2P, "DV3 WV1 ks1 F160 WPRO1 nsplit 2,3", wnorm="in", wact=2),
    _pair("fu_dv3_wv2", cv(72, 40, 3, 1, 1), _2P, "DV3 WV2 ks1 F160 WPRO0 nsplit 2,3"),
    _pair("fu_dv5_wv1", ct(64, 64), _2P, "DV5 WV1 ks1 F160 WPRO0 nsplit 2,3", env=PATCH),
    _pair("fu_dv5_wv2", ct(64, 32), _2P, "DV5 WV2 ks1 F160 WPRO0 nsplit 2,3", env=PATCH),
    _pair("fu_dv6_wv1_f16", cv(32, 64, 4, 1, 2), _2P, "DV6 WV1 ks1 F161 WPRO1 nsplit 3,3", dplanes=True, wact=2),
    _pair("fu_dv6_wv2", cv(24, 40, 3, 1, 1), _2P, "DV6 WV2 ks1 F160 WPRO0 nsplit 2,3"),
    # a published maximum on a plan other than 6: re-planned on bf16 planes, F160 -- the result meets the bf16-plane model and is
    # farther than the bound from the fp16-plane model.  The two models differ by the planes' residuals, sqrt(K) 2^-17 of a term,
    # against a bound of K u M: only a shallow sum tells them apart, so this is a 1 x 1 layer, K = 32 (the host test requires the
    # models more than two bounds apart: a result inside one bound of the bf16 model is then outside one bound of the other)
    _pair("fu_dv3_replanned_bf16", cv(64, 32, 1, 1, 0), _2P, "DV3 WV2 ks1 F160 WPRO0 nsplit 2,3", dplanes=True),
    # one problem: the split of the backward-data half stays inside the fused launch (slabs in the workspace).  16 tiles of 16 k-tiles
    # plan a split of 4, which the SGAN_FUSE_KS_WGS cap (128 // 16 = 8) leaves alone; 32 tiles of 32 k-tiles (the 256 -> 128 layer's
    # backward-data on a 16 x 16 map) plan 8, and the cap (128 // 32 = 4) moves it to 4
    _pair("fu_dv3_ks4_ws", cv(64, 128, 4, 2, 1), [(32, 32)], "DV3 WV1 ks4 F160 WPRO0 nsplit 2", env=NOPATCH,
          dkw=dict(norm="in", act=2, x=True, stats=True)),
    _pair("fu_dv3_ks_capped_8_to_4", cv(128, 256, 4, 2, 1), [(32, 32)], "DV3 WV1 ks4 F160 WPRO0 nsplit 2", env=NOPATCH),
    # one plane: both halves; backward-weight alone beside a split backward-data
    _pair("fu_x1_both", cv(64, 72, 3, 1, 1), _2P, "DV3 WV1 ks1 F160 WPRO0 nsplit 2,3", FUSED_X1, dmode="bf16x1", wmode="bf16x1"),
    _pair("fu_wx1_only", cv(64, 72, 3, 1, 1), _2P, "DV3 WV1 ks1 F160 WPRO0 nsplit 2,3", FUSED_WX1, wmode="bf16x1"),
    # ---- the refusals: the entry answers 1 and writes nothing ----
    _pair("refused_dx1_beside_split_wgrad", cv(64, 72, 3, 1, 1), _2P, None, dmode="bf16x1"),
    _pair("refused_skinny_dgrad", cv(4, 64, 3, 1, 1), _2P, None),
    _pair("refused_workspace_too_small", cv(64, 128, 4, 2, 1), [(32, 32)], None, env=NOPATCH, ws=False),
    _pair("refused_cout16_wgrad", cv(64, 16, 3, 1, 1), _2P, None),
]
# (the fifth refusal, a prologue on the backward-data job, cannot be expressed through sgan_conv_dgrad_job: the job has no in_norm
# field and sg_build_dgrad_params sets pro_act = NONE; sg_igemm3_fuse_plan's test is unreachable from the C ABI)

ALL = FWD + DGRAD + WGRAD + [c for p in PAIRS for c in p[1:3]]
IDS = K.IDS


def strict(case):
    return case.op == "dgrad" or not case.norm


# ---- the planners, restated (library defaults) ------------------------------------------------------------------------------------
gemm, phase_taps, max_k = W.gemm, W.phase_taps, W.max_k


def conv_form(case):
    return (not case.layer.tr) != (case.op == "dgrad")


def maps(case):
    """[(pixels of the forward input, of the forward output)] per problem."""
    return [(h * w, ho * wo) for h, w in case.sizes for ho, wo in [case.layer.out_hw(h, w)]]


def eligible(case):
    """sg_igemm3_eligible (the tests always pass packed weights; backward-data reads the transposed copy)."""
    Ck, N = gemm(case)
    return case.wt and Ck % 8 == 0 and Ck >= 16 and N >= 16 and all(min(m) >= MIN_PIXELS for m in maps(case))


def patch_plan(case):
    """sg3p_plan -> None or dict(a_it, tiles, waste, min_taps, s2, wgs)."""
    L, (Ck, N) = case.layer, gemm(case)
    cf = conv_form(case)
    is_ = L.s if cf else 1
    if (is_ != 1 and not (is_ == 2 and cf)) or Ck % 32 or N <= 32:
        return None
    maxpix, min_taps = 0, 1 << 30
    for a in range(1 if cf else L.s):
        for b in range(1 if cf else L.s):
            if cf:
                dys = dxs = [kk - L.p for kk in range(L.k)]
            else:
                dys = [(a + L.p - ky) // L.s for ky in range(L.k) if (a + L.p - ky) % L.s == 0]
                dxs = [(b + L.p - kx) // L.s for kx in range(L.k) if (b + L.p - kx) % L.s == 0]
            if not dys or not dxs:
                return None
            maxpix = max(maxpix, (7 * is_ + 1 + max(dys) - min(dys)) * (7 * is_ + 1 + max(dxs) - min(dxs)))
            min_taps = min(min_taps, len(dys) * len(dxs))
    if maxpix > (384 if is_ == 2 else 256):
        return None
    ph = [(hp, wp) for H, W_ in case.sizes for hp, wp, _ in K.phases(case, H, W_)]
    tiles, real = sum(cdiv(hp, 8) * cdiv(wp, 8) for hp, wp in ph), sum(hp * wp for hp, wp in ph)
    if real == 0:
        return None
    return dict(a_it=6 if is_ == 2 else 2 if maxpix <= 128 else 4, tiles=tiles, waste=tiles * 64 / real, min_taps=min_taps, s2=is_ == 2,
                wgs=tiles * cdiv(N, 64))


def patch_wanted(case, pl):
    if pl is None:
        return False
    if "SGAN_IGEMM3P" in case.env:
        return int(case.env["SGAN_IGEMM3P"]) != 0
    if pl["s2"] and pl["wgs"] < 100:
        return False
    if pl["min_taps"] >= 9:
        return pl["waste"] < 1.6
    return pl["min_taps"] >= 4 and pl["waste"] < 1.3


def pick_tile(case):
    """sg3_pick_tile with the force rules of SGAN_TILE3."""
    N = gemm(case)[1]
    force = case.env.get("SGAN_TILE3")
    if force:
        bm, bn = map(int, force.split("x"))
        if (bm, bn) == (128, 128) and N > 64:
            return 128, 128
        if (bm, bn) == (128, 64) and N > 32:
            return 128, 64
        if (bm, bn) == (64, 64) and N > 32:
            return 64, 64
    if N <= 32:
        return 128, 32
    if N > 64 and W.total_tiles(case, 128) * cdiv(N, 128) >= 192:
        return 128, 128
    if W.total_tiles(case, 128) * cdiv(N, 64) >= 384:
        return 128, 64
    return 64, 64


TILE_NAMES = {(128, 32): T128x32, (64, 64): T64, (128, 64): T128x64, (128, 128): T128}


def igemm3_plan(case, workspace=True):
    """(kernel, variant) of sg_launch_igemm3 for a forward / backward-data row; None where sg_igemm3_eligible says no."""
    if not eligible(case):
        return None
    x1 = case.mode == "bf16x1"
    pro = int(case.op == "fwd" and bool(case.norm or case.act))
    f16 = int(case.planes)
    pl = patch_plan(case)
    if patch_wanted(case, pl):
        ncb = gemm(case)[0] // 32
        kw = 2 if (pl["a_it"] == 2 and pl["wgs"] <= 256 and ncb % 2 == 0 and ncb >= 2) else 1
        return IG3P(pl["s2"], x1), f"AIT{pl['a_it']} KW{kw} PRO{pro} F16{f16}"
    BM, BN = pick_tile(case)
    ks = W.plan_ksplit(case, BM, BN)
    tail = ""
    if ks > 1 and not workspace:
        ks, tail = 1, " noslab"
    return IG3(TILE_NAMES[(BM, BN)], x1), f"ks{ks} PRO{pro} F16{f16}{tail}"


def wgrad3_covers(case):
    L = case.layer
    return L.cin % 8 == 0 and L.cout % 8 == 0 and L.cin >= 16 and L.cout >= 32 and all(min(m) >= MIN_PIXELS for m in maps(case))


def wgrad3_prepare(case):
    """(tile, BCO, BKC, per, [nsplit]) of sg_launch_wgrad3 / sgw3_prepare."""
    L = case.layer
    tile, BCO, BKC = (W32, 32, 128) if L.cout < 64 else (W64, 64, 64)
    tiles = cdiv(max_k(case), BKC) * cdiv(L.cout, BCO)
    nph = len(phase_taps(case))
    nchunk = [cdiv(max(hp * wp for hp, wp, _ in K.phases(case, H, W_)), 32) for H, W_ in case.sizes]
    per = max(4, int(sum(nchunk) * nph * tiles / 512.0 + 0.999))
    return tile, BCO, BKC, per, [min(max(cdiv(n, per), 1), 512) for n in nchunk]


def wgrad3_plan(case):
    if not wgrad3_covers(case):
        return None
    tile, _, _, per, nsplit = wgrad3_prepare(case)
    pro = int(bool(case.norm or case.act))
    return WG3(tile, case.mode == "bf16x1"), f"PRO{pro} F16{int(case.planes)} per{per} nsplit " + ",".join(map(str, nsplit))


def fuse_plan_dgrad(case):
    """(variant, ks) of sg_igemm3_fuse_plan; variant 0: not a body the fused kernel carries."""
    pl = patch_plan(case)
    if patch_wanted(case, pl):
        return {2: 1, 4: 2, 6: 5}[pl["a_it"]], 1
    BM, BN = pick_tile(case)
    if (BM, BN) == (128, 32) and W.plan_ksplit(case, 128, 32) == 1:
        return 6, 1
    if (BM, BN) != (64, 64):
        return 0, 1
    ks = W.plan_ksplit(case, 64, 64)
    if ks > 64:
        return 0, 1
    if ks > 1:
        cap = max(1, 128 // max(1, W.total_tiles(case, 64) * cdiv(gemm(case)[1], 64)))      # SGAN_FUSE_KS_WGS
        if ks > cap:
            nkt = cdiv(max_k(case), 32)
            ks = cdiv(nkt, cdiv(nkt, cap))
    return 3, ks


def fused_plan(d, w, workspace=True):
    """(kernel, variant) of sg_conv_bwd_fused_impl, or None where it answers 1."""
    dx1, wx1 = d.mode == "bf16x1", w.mode == "bf16x1"
    N = gemm(d)[1]
    skinny = N == 4 and not (d.x or d.stats or d.accum)
    if skinny or (dx1 and not wx1) or not eligible(d):
        return None
    dv, ks = fuse_plan_dgrad(d)
    if dv == 0 or not wgrad3_covers(w):
        return None
    if ks > 1 and not workspace:
        return None
    _, _, _, _, nsplit = wgrad3_prepare(w)
    wv = 2 if w.layer.cout < 64 else 1
    f16 = int(dv == 6 and d.planes)
    pro = int(bool(w.norm or w.act))
    kernel = FUSED_X1 if dx1 else FUSED_WX1 if wx1 else FUSED
    return kernel, f"DV{dv} WV{wv} ks{ks} F16{f16} WPRO{pro} nsplit " + ",".join(map(str, nsplit))


# ---- the plane model ----------------------------------------------------------------------------------------------------------------
def shift_of(dy):
    return PM._shift(float(dy.abs().max()))


def operand_planes(case, a, b, dy_is, f16=None):
    """((a_hi, a_lo), (b_hi, b_lo)) as float64.  fwd: a = prologue output, b = w.  dgrad: a = dY, b = w.  wgrad: a = prologue
    output, b = dY.  dy_is: "a" / "b" / None -- which operand is the gradient (scaled by its published maximum on fp16 planes).
    f16: override of the row's planes (the re-planned fused row is held to both models)."""
    f16 = case.planes if f16 is None else f16
    if case.op == "fwd":
        return PM.split_f16(a), PM.split_f16(b, PM.W_SHIFT)
    if not f16:
        return PM.split_bf16(a), PM.split_bf16(b)
    if case.op == "dgrad":
        return PM.split_f16(a, shift_of(a)), PM.split_f16(b, PM.W_SHIFT)
    return PM.split_f16(a), PM.split_f16(b, shift_of(b))


def pairs(mode, A, B, drop=None):
    """The plane products of a mode as (a plane, b plane); drop "lo_hi" / "hi_lo": that product left out (the host's mutation)."""
    if mode == "bf16x1":
        return [(A[0], B[0])]
    out = [("hi_hi", A[0], B[0]), ("hi_lo", A[0], B[1]), ("lo_hi", A[1], B[0])]
    return [(a, b) for n, a, b in out if n != drop]


def _sum(f, prs, mag):
    g = torch.abs if mag else (lambda t: t)
    return sum(f(g(a), g(b)) for a, b in prs)


def model_fwd(case, a, w, mag=False, drop=None, only=None, f16=None):
    A, B = operand_planes(case, a, w, None, f16)
    return _sum(lambda pa, pw: R.forward(case.layer, pa, pw, only=only), pairs(case.mode, A, B, drop), mag)


def model_dgrad(case, dy, w, H, W_, mag=False, drop=None, only=None, f16=None):
    A, B = operand_planes(case, dy, w, "a", f16)
    return _sum(lambda pd, pw: R.dgrad(case.layer, pd, pw, H, W_, only=only), pairs(case.mode, A, B, drop), mag)


def model_wgrad(case, a, dy, mag=False, drop=None, f16=None):
    A, B = operand_planes(case, a, dy, "b", f16)
    return _sum(lambda pa, pd: R.wgrad(case.layer, pa, pd), pairs(case.mode, A, B, drop), mag)


def extra_terms(case):
    """(c_M, planes' h) of a normalised row: the multiple of u M the re-split of a changed `a` adds (module docstring)."""
    f16 = case.planes
    h = 2.0 ** -11 if f16 else 2.0 ** -8
    if case.mode == "bf16x1":
        return 2 * h / U
    r = 2.0 ** -22 if f16 else 2.0 ** -16
    return (2 * r + 2 * h * h) / U


def g3_limits(case):
    """(limit or None) of G3: the documented contract."""
    planes = "f16" if case.planes else "bf16"
    if case.mode == "bf16x3" and planes == "f16":
        return 3e-6
    return 1e-3 if PM.contract_applies(case.mode, planes) else None


@functools.lru_cache(maxsize=None)
def reference(case, f16=None):
    """fwd / dgrad: per problem dict(ref, bound, M, K, truth, ...); wgrad: one dict.  Computed once, never modified."""
    d, L = K.data(case), case.layer
    w = d["w"].double()
    n = dict(norm=case.norm, act=case.act, gamma=d["gamma"], beta=d["beta"])
    tiny = 2.0 ** -149
    if case.op == "fwd":
        out = []
        for p in d["probs"]:
            a, A, y = R.prologue(p["x"], **n)
            assert float(a.abs().max()) < PM.ACT_OVERFLOW and float(w.abs().max()) < PM.W_OVERFLOW
            Kc = R.count_fwd(L, p["H"], p["W"])
            pre, M = model_fwd(case, a, w), model_fwd(case, a, w, mag=True)
            truth = R.forward(L, a, w)
            bound = (Kc + 1) * U * M + (Kc + 1) * tiny
            if case.bias:
                b = d["b"].double().view(-1, 1, 1)
                pre, truth, bound = pre + b, truth + b, bound + U * b.abs()
            if not strict(case):
                MA = R.forward(L, A, PM.split_f16(w, PM.W_SHIFT)[0].abs())
                bound = bound + R.C_PRO * U * MA + extra_terms(case) * U * M + U * R.forward(L, torch.ones_like(a), w.abs())
            r = dict(pre=pre, pre_bound=bound, ref=pre, bound=bound, M=M, K=Kc, truth=truth, a=a, y=y)
            out.append(r)
        return out
    if case.op == "dgrad":
        out = []
        for p in d["probs"]:
            dy, H, W_ = p["dy"].double(), p["H"], p["W"]
            Kc = R.count_dgrad(L, H, W_)
            ref, M = model_dgrad(case, dy, w, H, W_, f16=f16), model_dgrad(case, dy, w, H, W_, mag=True, f16=f16)
            truth = R.dgrad(L, dy, w, H, W_)
            r = dict(xhat=None, y=None, f=1.0)
            c = 0
            if case.x:
                r["f"], r["xhat"], r["y"] = R.act_grad(p["x"], case.norm, case.act, d["gamma"], d["beta"])
                ref, M, truth, c = ref * r["f"], M * r["f"], truth * r["f"], R.C0_DGRAD
            r["own"], r["own_bound"], r["own_truth"] = ref, (Kc + c) * U * M + Kc * tiny, truth
            if p["prev"] is not None:
                ref, M, truth, c = ref + p["prev"].double(), M + p["prev"].double().abs(), truth + p["prev"].double(), R.C0_DGRAD
            r.update(ref=ref, bound=(Kc + c) * U * M + Kc * tiny, M=M, K=Kc, truth=truth)
            out.append(r)
        return out
    dw = M = MA = Kc = truth = ones = db = Mb = Kb = 0
    ys = []
    for p in d["probs"]:
        a, A, y = R.prologue(p["x"], **n)
        ys.append(y)
        assert float(a.abs().max()) < PM.ACT_OVERFLOW
        dy = p["dy"].double()
        dw, M = dw + model_wgrad(case, a, dy), M + model_wgrad(case, a, dy, mag=True)
        truth, Kc = truth + R.wgrad(L, a, dy), Kc + R.count_wgrad(L, p["H"], p["W"])
        if not strict(case):
            MA = MA + R.wgrad(L, A, dy.abs())
            ones = ones + R.wgrad(L, torch.ones_like(a), dy.abs())
        db, Mb, Kb = db + dy.sum((1, 2)), Mb + dy.abs().sum((1, 2)), Kb + dy.shape[1] * dy.shape[2]
    c = 0
    if case.accum:
        pw, pb = d["prev_w"].double(), d["prev_b"].double()
        dw, M, truth, c = dw + pw, M + pw.abs(), truth + pw, 1
        db, Mb = db + pb, Mb + pb.abs()
    bound = (Kc + c) * U * M + Kc * tiny
    if not strict(case):
        bound = bound + R.C_PRO * U * MA + extra_terms(case) * U * M + U * ones
    return dict(dw=dw, dw_bound=bound, db=db, db_bound=(Kb + R.C0_DBIAS) * U * Mb, M=M, K=Kc, truth=truth, ys=ys)

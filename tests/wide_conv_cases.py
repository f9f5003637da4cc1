"""The case table of tests/test_hip_wide_conv.py, tests/test_hip_wide_wgrad.py and tests/test_wide_conv_host.py: the smallest shapes
that reach every branch of the exact-fp32 MFMA conv kernels -- sg_igemm_kernel in its five tile shapes (both weight layouts, with
and without the normalise-on-load prologue, one or two wave groups, split-K), sg_splitk_epilogue_kernel and sg_wgrad_kernel in its
three shapes.  The rows are thin_conv_cases.Case objects: operands (thin_conv_cases.data) and the float64 reference with its
per-element bound (thin_conv_cases.reference -> thin_conv_ref.op_*) are the ones of the 4-channel-side table, unchanged.

`kernel` is the name the launcher reports through sgan_last_kernel(), `variant` what it reports through sgan_last_variant():
    sg_launch_igemm   "ks<k> KW<1|2> PRO<0|1>"  the K split that ran (1: none), the wave groups per workgroup, the prologue
                      (+ " noslab" when a planned split found no workspace and ran unsplit)
    sg_launch_wgrad   "PRO<0|1> per<c> nsplit a,b,.."  the prologue, the 32-pixel chunks per workgroup the split aims at, the pixel
                      split of every problem
The planners that decide them (sg_pick_tile, the half-tile rule of sg_dispatch_igemm, sg_plan_ksplit with its mid-grid branch and
sg_time_model, kw2 of sg_launch_igemm, per / nsplit of sg_launch_wgrad) are restated below with the library's default thresholds;
tests/test_wide_conv_host.py holds every row's kernel / variant to the restatement, the GPU tests hold them to the library -- a
threshold that moves turns a row red instead of silently taking it off its branch.  igemm_shares and wgrad_ranges restate the
kernels' own index arithmetic (which k-tiles a split and a wave group walk, which chunks a pixel split) for the host test, which
proves from them that the "empty trailing split", "uneven share" and "partial k-tile" rows are what they claim.

All rows run in the f32 mode except the three FALLBACK rows, which run in the default bf16x3 mode and must still land on the fp32
kernel (gathered channels below 16 or no multiple of 8; a map under 256 pixels).  Every row keeps L + c <= L_MAX (thin_conv_ref):
at most 16 taps x 352 stored channels (9 x 464 in the uneven-share row), 5780 pixels for backward-weight.  Not in the table: the
<128,64,2,2> tile, which no shape reaches -- sg_pick_tile selects it only through the SGAN_MIN128 tuning knob, read once per process."""
import thin_conv_cases as K
from thin_conv_cases import Case, cdiv, ct, cv
from thin_conv_ref import pad4

TILES = {(128, 16): "128,16,4,1", (128, 32): "128,32,4,1", (64, 32): "64,32,2,2", (64, 64): "64,64,2,2"}


def IG(bm, bn, bkc=True):
    return f"sg_igemm_kernel<{TILES[(bm, bn)]},{'true' if bkc else 'false'}>"


WG16, WG32, WG64 = "sg_wgrad_kernel<16,128,1,4>", "sg_wgrad_kernel<32,64,1,4>", "sg_wgrad_kernel<64,64,2,2>"
F32 = dict(math="f32")

FWD = [
    # ---- <128,16>: N <= 16 ----
    Case("f_128x16_in_noact_stats", "fwd", IG(128, 16), cv(16, 8, 3, 1, 1), [(12, 12)], "in", 0, stats=True, variant="ks1 KW1 PRO1", **F32),
    # 72 k-tiles in one block would split, but 256 % (12 / 4) != 0: the split-K epilogue cannot take N = 12
    Case("f_128x16_n12_deep_refused", "fwd", IG(128, 16), cv(256, 10, 3, 1, 1), [(8, 8)], bias=True, variant="ks1 KW1 PRO0", **F32),
    # a 4-channel result WITH statistics: sg_use_small_n declines it
    Case("f_128x16_n4_stats", "fwd", IG(128, 16), cv(24, 3, 3, 1, 1), [(9, 11)], bias=True, stats=True, variant="ks1 KW1 PRO0", **F32),
    # ---- <128,32>: 16 < N <= 32 ----
    Case("f_128x32_split8", "fwd", IG(128, 32), cv(64, 32, 4, 2, 1), [(16, 16)], bias=True, stats=True, variant="ks8 KW1 PRO0", **F32),
    Case("f_128x32_n20_ragged_tanh", "fwd", IG(128, 32), cv(12, 20, 3, 1, 1), [(37, 41)], None, 2, bias=True, tanh=True, variant="ks1 KW1 PRO1", **F32),
    # ---- <64,32>: the half tile (short reductions on small grids, no split planned) ----
    Case("f_64x32_half_kw1", "fwd", IG(64, 32), cv(16, 64, 3, 1, 1), [(20, 20)], bias=True, variant="ks1 KW1 PRO0", **F32),
    Case("f_64x32_half_kw2_bn_relu", "fwd", IG(64, 32), cv(16, 64, 4, 2, 1), [(18, 22)], "bn", 1, stats=True, variant="ks1 KW2 PRO1", **F32),
    Case("f_64x32_n48_deep_refused", "fwd", IG(64, 32), cv(128, 48, 4, 1, 1), [(6, 6)], bias=True, variant="ks1 KW2 PRO0", **F32),
    # ---- <64,64> ----
    Case("f_64x64_split16_kw1", "fwd", IG(64, 64), cv(128, 64, 4, 2, 1), [(8, 8)], "in", 2, bias=True, stats=True, variant="ks16 KW1 PRO1", **F32),
    Case("f_64x64_split8_kw2", "fwd", IG(64, 64), cv(128, 128, 4, 1, 1), [(46, 46)], bias=True, tanh=True, variant="ks8 KW2 PRO0", **F32),
    # two problems (never split), 131 k-tiles (past the half tile's 128): wave group 1 walks 65 of its 66 iterations on zeros
    Case("f_64x64_kw2_uneven_2prob", "fwd", IG(64, 64), cv(464, 64, 3, 1, 1), [(6, 7), (5, 5)], "in", 2, stats=True, variant="ks1 KW2 PRO1", **F32),
    # the mid-grid branch: 196 blocks x 128 k-tiles, sg_time_model picks 6 splits
    Case("f_64x64_mid_grid", "fwd", IG(64, 64), cv(256, 128, 4, 1, 1), [(80, 80)], bias=True, variant="ks6 KW1 PRO0", **F32),
    # ConvT k3 s2 p1 op1: phases of 1 / 2 / 2 / 4 taps = 5 / 9 / 9 / 17 k-tiles; the plan follows the longest, so the fourth
    # split of the three short phases is empty and writes a slab of zeros
    Case("f_convT_k3_short_phases_split4", "fwd", IG(64, 64), ct(136, 64, 3, 2, 1, 1), [(6, 6)], bias=True, stats=True, variant="ks4 KW1 PRO0", **F32),
    Case("f_convT_k4_bn_relu_bias_tanh", "fwd", IG(128, 32), ct(40, 20), [(9, 15)], "bn", 1, bias=True, tanh=True, variant="ks1 KW1 PRO1", **F32),
]

# the default mode's way back to the fp32 kernels (sg_igemm3_eligible)
FALLBACK = [
    Case("fb_ck12", "fwd", IG(128, 32), cv(12, 32, 3, 1, 1), [(17, 17)], bias=True, variant="ks1 KW1 PRO0", math="bf16x3"),
    Case("fb_ck20", "fwd", IG(64, 32), cv(20, 64, 3, 1, 1), [(17, 17)], "in", 2, variant="ks1 KW1 PRO1", math="bf16x3"),
    Case("fb_15x15_64to64", "fwd", IG(64, 64), cv(64, 64, 3, 1, 1), [(15, 15)], bias=True, stats=True, variant="ks4 KW1 PRO0", math="bf16x3"),
]

DGRAD = [
    # BKC = false: the n-contiguous master weights, K = 9 taps x 12 channels = 3 k-tiles and 12 elements
    Case("d_master_weights_k108", "dgrad", IG(128, 32, False), cv(24, 12, 3, 1, 1), [(10, 11)], wt=False, variant="ks1 KW1 PRO0", **F32),
    # the transposed copy with act'(IN(x)) and the two norm-backward sums: in the kernel's own epilogue, and in the split-K one
    Case("d_xnorm_in_lrelu_unsplit", "dgrad", IG(64, 32), cv(64, 32, 4, 2, 1), [(16, 16)], "in", 2, x=True, stats=True, variant="ks1 KW1 PRO0", **F32),
    Case("d_xnorm_in_lrelu_split4", "dgrad", IG(64, 64), cv(64, 128, 4, 2, 1), [(16, 16)], "in", 2, x=True, stats=True, variant="ks4 KW1 PRO0", **F32),
    Case("d_accum_bn_relu_split4", "dgrad", IG(64, 64), cv(64, 128, 4, 2, 1), [(16, 16)], "bn", 1, x=True, stats=True, accum=True, variant="ks4 KW1 PRO0", **F32),
    Case("d_accum_convT_unsplit", "dgrad", IG(128, 32), ct(20, 24), [(7, 5)], accum=True, variant="ks1 KW1 PRO0", **F32),
    # no forward tensor; N = 72 is two full half tiles and a ragged third
    Case("d_plain_n72_kw2", "dgrad", IG(64, 32), cv(72, 40, 3, 1, 1), [(9, 9)], variant="ks1 KW2 PRO0", **F32),
]

WGRAD = [
    Case("w_16x128_c8_in_lrelu", "wgrad", WG16, cv(12, 8, 3, 1, 1), [(9, 11)], "in", 2, bias=True, variant="PRO1 per4 nsplit 1", **F32),
    Case("w_16x128_c12_convT_bn_relu_prefill", "wgrad", WG16, ct(24, 10), [(5, 7)], "bn", 1, bias=True, accum=True, variant="PRO1 per4 nsplit 1", **F32),
    Case("w_32x64_c20", "wgrad", WG32, cv(20, 20, 4, 2, 1), [(13, 15)], bias=True, variant="PRO0 per4 nsplit 1", **F32),
    Case("w_64x64_c72_ragged", "wgrad", WG64, cv(24, 72, 3, 1, 1), [(10, 10)], bias=True, variant="PRO0 per4 nsplit 1", **F32),
    Case("w_64x64_3prob_nsplit_prefill", "wgrad", WG64, cv(16, 64, 3, 1, 1), [(40, 40), (20, 20), (5, 7)], None, 2, bias=True, accum=True,
         variant="PRO1 per4 nsplit 13,4,1", **F32),
]

ALL = FWD + FALLBACK + DGRAD + WGRAD
IDS = K.IDS


# ---- the launchers, restated (library defaults) -----------------------------------------------------------------------------------
def gemm(case):
    """(Ck, N): stored channels of the gathered tensor and of the result."""
    L, dg = case.layer, case.op == "dgrad"
    return pad4(L.cout if dg else L.cin), pad4(L.cin if dg else L.cout)


def phase_taps(case):
    """[[(ky, kx)] per phase] in the order sg_build_phases lays a phase's taps along k."""
    L, dg = case.layer, case.op == "dgrad"
    if (not L.tr) != dg:
        return [[(ky, kx) for ky in range(L.k) for kx in range(L.k)]]
    return [[(ky, kx) for ky in range(L.k) if (a + L.p - ky) % L.s == 0 for kx in range(L.k) if (b + L.p - kx) % L.s == 0]
            for a in range(L.s) for b in range(L.s)]


def total_tiles(case, BM):
    return sum(cdiv(hp * wp, BM) for H, W in case.sizes for hp, wp, _ in K.phases(case, H, W))


def max_k(case):
    return max(len(t) for t in phase_taps(case)) * gemm(case)[0]


def time_model(wgs, nkt_wg):
    """sg_time_model"""
    return nkt_wg * max(1.1, ((wgs + 255) // 256) * 0.69)


def plan_ksplit(case, BM, BN):
    """sg_plan_ksplit (every leading dimension of the tests' tensors is a multiple of 4)."""
    N = gemm(case)[1]
    NQ = N // 4
    if len(case.sizes) != 1 or NQ <= 0 or 256 % NQ != 0:
        return 1
    blocks = total_tiles(case, BM) * cdiv(N, BN)
    nkt = cdiv(max_k(case), 32)
    min_nkt = 16 if blocks <= 32 else 32 if blocks <= 96 else 64 if blocks <= 192 else 1 << 30
    if 192 < blocks <= 768 and nkt >= 128:
        H, W = case.sizes[0]
        Ho, Wo = (H, W) if case.op == "dgrad" else case.layer.out_hw(H, W)
        slab_us = Ho * Wo * N * 8.0 / 4e6
        best, best_cost = 1, time_model(blocks, nkt)
        for c in (2, 3, 4, 6, 8):
            if nkt // c < 16:
                break
            cost = time_model(blocks * c, cdiv(nkt, c)) + c * slab_us + 12.0
            if cost < 0.95 * best_cost:
                best, best_cost = c, cost
        return cdiv(nkt, cdiv(nkt, best)) if best > 1 else 1
    if nkt < min_nkt:
        return 1
    ks = min(cdiv(512, blocks), nkt // 4, 32)
    return cdiv(nkt, cdiv(nkt, ks)) if ks >= 2 else 1


def pick_tile(case):
    """sg_pick_tile and the half-tile rule of sg_dispatch_igemm."""
    N = gemm(case)[1]
    if N <= 16:
        return 128, 16
    if N <= 32:
        return 128, 32
    blocks, nkt = total_tiles(case, 64) * cdiv(N, 64), cdiv(max_k(case), 32)
    one_wave = 620 <= blocks <= 768
    if not one_wave and blocks <= 1024 and nkt <= 128 and plan_ksplit(case, 64, 64) == 1:
        return 64, 32
    return 64, 64


def igemm_plan(case):
    """(kernel, variant, ks, kw) of sg_dispatch_igemm / sg_launch_igemm for a row of the fp32 MFMA kernels."""
    BM, BN = pick_tile(case)
    N = gemm(case)[1]
    bkc = case.op != "dgrad" or case.wt
    ks = plan_ksplit(case, BM, BN)
    wgs = total_tiles(case, BM) * cdiv(N, BN) * ks
    nkt_wg = cdiv(cdiv(max_k(case), 32), ks)
    kw = 2 if (BM == 64 and bkc and wgs <= 512 and nkt_wg >= 8) else 1
    pro = int(case.op == "fwd" and bool(case.norm or case.act))
    return IG(BM, BN, bkc), f"ks{ks} KW{kw} PRO{pro}", ks, kw


def igemm_shares(case):
    """[[[(first k-tile, k-tiles walked, iterations run) per wave group] per split] per phase]: the k-tile ranges of sg_igemm_body."""
    _, _, ks, kw = igemm_plan(case)
    Ck = gemm(case)[0]
    out = []
    for taps in phase_taps(case):
        nkt_total = cdiv(len(taps) * Ck, 32)
        kt_per = cdiv(nkt_total, ks)
        ph = []
        for split in range(ks):
            wg_kt0 = split * kt_per
            wg_nkt = max(min(nkt_total, wg_kt0 + kt_per) - wg_kt0, 0)
            nkt = cdiv(wg_nkt, kw)
            ph.append([(wg_kt0 + kg * nkt, min(max(wg_nkt - kg * nkt, 0), nkt), nkt) for kg in range(kw)])
        out.append(ph)
    return out


def wgrad_plan(case):
    """(kernel, variant, per, [nsplit per problem]) of sgan_conv_wgrad_grouped / sg_launch_wgrad."""
    L = case.layer
    Cin, Cout = pad4(L.cin), pad4(L.cout)
    BCO, BKC, kernel = (16, 128, WG16) if Cout <= 16 else (32, 64, WG32) if Cout <= 32 else (64, 64, WG64)
    tiles = cdiv(max_k(case), BKC) * cdiv(Cout, BCO)
    nph = len(phase_taps(case))
    nchunk = [cdiv(max(hp * wp for hp, wp, _ in K.phases(case, H, W)), 32) for H, W in case.sizes]
    per = max(4, int(sum(nchunk) * nph * tiles / 512.0 + 0.999))
    nsplit = [min(max(cdiv(n, per), 1), 512) for n in nchunk]
    pro = int(bool(case.norm or case.act))
    return kernel, f"PRO{pro} per{per} nsplit " + ",".join(map(str, nsplit)), per, nsplit


def wgrad_ranges(case):
    """[[[(first chunk, end chunk) per split] per phase] per problem]: the 32-pixel chunk ranges of sg_wgrad_kernel."""
    nsplit = wgrad_plan(case)[3]
    out = []
    for (H, W), ns in zip(case.sizes, nsplit):
        prob = []
        for hp, wp, _ in K.phases(case, H, W):
            n = cdiv(hp * wp, 32)
            per = cdiv(n, ns)
            prob.append([(s * per, min(n, s * per + per)) for s in range(ns)])
        out.append(prob)
    return out


def ktile_terms(case, phase, kt):
    """[(ky, kx, c0, c1)]: the (tap, stored-channel range) pieces of k-tile kt of a phase."""
    Ck, taps = gemm(case)[0], phase_taps(case)[phase]
    out, k, end = [], kt * 32, min(kt * 32 + 32, len(taps) * Ck)
    while k < end:
        t, c = divmod(k, Ck)
        n = min(end - k, Ck - c)
        out.append(taps[t] + (c, c + n))
        k += n
    return out

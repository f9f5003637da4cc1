"""The case table of tests/test_hip_thin_conv.py, tests/test_hip_thin_wgrad.py and tests/test_thin_conv_ref_host.py: the smallest
shapes that reach every branch of the kernels with a 4-stored-channel side.  `kernel` is where the dispatch code sends the row
(sg_dispatch_igemm, sg_use_c4, sg_use_scatter4, sgan_conv_wgrad_grouped, sgan_conv_bwd_thin_pair); the GPU tests assert it through
sgan_last_kernel().  What that name does not tell (NB / RB of sg_conv_c4_kernel, NR and the weight layout of sg_conv_small_n_kernel,
the pixel split of sg_wgrad_thin_kernel, the halves of the pair) is the row's `variant`: the GPU tests compare it with what the
library reports through sgan_last_variant(), so a launcher whose thresholds move turns the row red instead of silently leaving its
branch.  c4_variant and thin_ranges restate the launchers for the host test only (which waves a split leaves empty or cuts mid-step).

Operands are drawn as everywhere in the suite (x ~ 1.5 N + 0.3, w ~ 0.05 N, bias ~ 0.1 N, dY ~ N); the elements of a
case that sit near an activation's kink are redrawn from the next seed, deterministically, until every tensor whose sign an
activation reads keeps min |y| > MASK_MARGIN max |y| (thin_conv_ref)."""
import functools
import zlib

import torch

import thin_conv_ref as R
from thin_conv_ref import Layer, pad4

S4, C4, PAIR = "sg_conv_scatter4_kernel", "sg_conv_c4_kernel", "sg_bwd_thin_pair_kernel"
SN8, SN16, SN64 = "sg_conv_small_n_kernel<8>", "sg_conv_small_n_kernel<16>", "sg_conv_small_n_kernel<64>"


def THIN(mb, form):
    return f"sg_wgrad_thin_kernel<{mb},{form}>"


class Case:
    """op: fwd / dgrad / wgrad.  norm, act: the prologue (fwd, wgrad) or the forward tensor's norm of the backward-data epilogue
    (dgrad, with x=True); stats: result statistics (fwd) or the two norm-backward sums (dgrad); accum: pre-filled output (dgrad) /
    pre-filled dw and dbias (wgrad); wt: backward-data reads the transposed weight copy; env: per-call knobs; math: the arithmetic
    mode the row is launched in (None: whatever is current -- the kernels of this table do not read it)."""

    def __init__(self, name, op, kernel, layer, sizes, norm=None, act=0, bias=False, tanh=False, stats=False, accum=False, x=False,
                 wt=True, env=None, variant=None, math=None):
        self.name, self.op, self.kernel, self.layer, self.sizes = name, op, kernel, layer, sizes
        self.norm, self.act, self.bias, self.tanh, self.stats, self.accum, self.x, self.wt = norm, act, bias, tanh, stats, accum, x, wt
        self.env, self.variant, self.math = env or {}, variant, math

    def __repr__(self):
        return self.name


def ct(cin, cout, k=4, s=2, p=1, op=0):
    return Layer("convT", k, s, p, cin, cout, op)


def cv(cin, cout, k=4, s=2, p=2):
    return Layer("conv", k, s, p, cin, cout)


SPLIT3 = {"SGAN_THIN_MINPIX": "16", "SGAN_THIN_WANT": "3"}
SPLIT6 = {"SGAN_THIN_MINPIX": "16", "SGAN_THIN_WANT": "6"}

FWD = [
    # ---- scatter4: ConvT k4 s2 p1 to 4 stored channels; phase extents = the input size ----
    Case("s4_fwd_ck16_1x2", "fwd", S4, ct(16, 2), [(1, 2)], bias=True),
    Case("s4_fwd_ck48_2x7_in_lrelu_tanh", "fwd", S4, ct(48, 3), [(2, 7)], "in", 2, tanh=True),
    Case("s4_fwd_ck16_6x31_bn_relu_tanh", "fwd", S4, ct(16, 2), [(6, 31)], "bn", 1, bias=True, tanh=True),
    Case("s4_fwd_ck16_7x30_relu", "fwd", S4, ct(16, 4), [(7, 30)], None, 1),
    Case("s4_fwd_ck512_6x7_in_lrelu", "fwd", S4, ct(512, 2), [(6, 7)], "in", 2, bias=True),
    Case("s4_fwd_ck16_3prob", "fwd", S4, ct(16, 1), [(61, 30), (7, 31), (2, 6)], "bn", 1, bias=True, tanh=True),
    Case("s4_fwd_ck32_31x61", "fwd", S4, ct(32, 2), [(31, 61)]),
    # ---- scatter4 declined: Ck < 16, Ck % 16 != 0 -> the small-N kernel by its reduction length (4 taps x Ck) ----
    Case("s4_declined_ck8", "fwd", SN8, ct(8, 2), [(6, 7)], "in", 2, bias=True, variant="NR2 BKC1"),
    Case("s4_declined_ck520", "fwd", SN64, ct(520, 2), [(6, 7)], bias=True, variant="NR2 BKC1"),
    # ---- c4, plain: 4 gathered channels, 16 < N <= 64, bias / tanh only ----
    Case("c4_k4s2p1_n20", "fwd", C4, cv(2, 20, 4, 2, 1), [(37, 41)], bias=True, variant="NB2 RB2"),
    Case("c4_k4s2p2_n32", "fwd", C4, cv(3, 32), [(9, 7)], variant="NB2 RB2"),
    Case("c4_k3s1p1_n36", "fwd", C4, cv(4, 36, 3, 1, 1), [(5, 7)], bias=True, variant="NB3 RB2"),
    Case("c4_k4s1p2_n48", "fwd", C4, cv(1, 48, 4, 1, 2), [(6, 5)], bias=True, variant="NB3 RB2"),
    Case("c4_k4s2p2_n52_2prob", "fwd", C4, cv(2, 52), [(21, 19), (8, 30)], variant="NB4 RB2"),
    Case("c4_k4s1p0_n64_w1_tanh", "fwd", C4, cv(3, 64, 4, 1, 0), [(9, 4)], bias=True, tanh=True, variant="NB4 RB2"),
    Case("c4_plain_rb4_n20", "fwd", C4, cv(2, 20), [(640, 640)], bias=True, variant="NB2 RB4"),
    # ---- c4, full epilogue, forward: the statistics of the result; N = 36 is a second grid.y block of four columns ----
    Case("c4e_fwd_stats_n36", "fwd", C4, cv(2, 36), [(21, 19)], bias=True, stats=True, variant="NB2 RB2 EPI gy2"),
    # ---- small_n: one per lanes-per-pixel form (ktot < 256, 256 .. 2047, >= 2048) ----
    Case("sn8_convT_k3s2op1_16to3", "fwd", SN8, ct(16, 3, 3, 2, 1, 1), [(9, 7)], "in", 2, bias=True, variant="NR4 BKC1"),
    Case("sn16_k7_8to1_tanh", "fwd", SN16, cv(8, 1, 7, 1, 3), [(16, 16)], bias=True, tanh=True, variant="NR1 BKC1"),
]

DGRAD = [
    # ---- scatter4: image gradient of conv k4 s2 from <= 4 channels; phase extents ceil((H - a) / 2) ----
    Case("s4_dgrad_p2_13x61", "dgrad", S4, cv(2, 16), [(13, 61)]),
    Case("s4_dgrad_p1_3x122", "dgrad", S4, cv(3, 48, 4, 2, 1), [(3, 122)]),
    Case("s4_dgrad_3prob", "dgrad", S4, cv(1, 16), [(13, 61), (61, 3), (1, 2)]),
    # ---- c4 plain through backward-data (ConvT to 4 stored channels, no forward tensor) ----
    Case("c4_dgrad_convT_n36", "dgrad", C4, ct(36, 2), [(5, 6)], variant="NB3 RB2"),
    # ---- c4, full epilogue ----
    Case("c4e_tail_dgrad_n32_bn_relu", "dgrad", C4, ct(32, 2), [(9, 11)], "bn", 1, x=True, stats=True, variant="NB2 RB2 EPI gy1"),
    Case("c4e_logits_dgrad_n64_in_lrelu", "dgrad", C4, cv(64, 1, 4, 1, 2), [(10, 12)], "in", 2, x=True, stats=True, variant="NB2 RB2 EPI gy2"),
    Case("c4e_logits_dgrad_n256_in_lrelu", "dgrad", C4, cv(256, 1, 4, 1, 2), [(7, 9)], "in", 2, x=True, stats=True, variant="NB2 RB2 EPI gy8"),
    Case("c4e_accum_n32_bn_relu", "dgrad", C4, ct(32, 2), [(9, 11)], "bn", 1, x=True, stats=True, accum=True, variant="NB2 RB2 EPI gy1"),
    Case("c4e_accum_plain_n20", "dgrad", C4, ct(20, 2), [(7, 5)], accum=True, variant="NB2 RB2 EPI gy1"),
    Case("c4e_rb4_n32_bn_relu", "dgrad", C4, ct(32, 2), [(321, 321)], "bn", 1, x=True, stats=True, variant="NB2 RB4 EPI gy1"),
    # ---- small_n, n-contiguous weights (the master copy), 16 taps x 128 channels = 2048 ----
    Case("sn64_dgrad_k4s1_128to2", "dgrad", SN64, cv(2, 128, 4, 1, 1), [(9, 10)], wt=False, variant="NR2 BKC0"),
]

WGRAD = [
    Case("w_cin4_mb1_c8_th1", "wgrad", THIN(1, "cin4"), cv(1, 8), [(9, 11)], bias=True, variant="nsplit 1"),
    Case("w_cin4_mb1_c16_th3_pro", "wgrad", THIN(1, "cin4"), cv(3, 16, 3, 1, 1), [(12, 9)], "in", 2, bias=True, variant="nsplit 1"),
    Case("w_cin4_mb2_c20_th2_3prob_prefill", "wgrad", THIN(2, "cin4"), cv(2, 20, 4, 2, 1), [(20, 22), (9, 9), (5, 30)], bias=True, accum=True, variant="nsplit 1,1,1"),
    Case("w_cin4_mb2_c32_th4_pro", "wgrad", THIN(2, "cin4"), cv(4, 32, 4, 1, 2), [(10, 11)], "bn", 1, variant="nsplit 1"),
    Case("w_cin4_mb4_c64_th2_split", "wgrad", THIN(4, "cin4"), cv(2, 64), [(37, 41)], bias=True, env=SPLIT3, variant="nsplit 3"),
    Case("w_cin4_mb4_c64_th3_pro", "wgrad", THIN(4, "cin4"), cv(3, 64), [(13, 14)], None, 2, variant="nsplit 1"),
    Case("w_cout4_mb2_c16_th2_pro", "wgrad", THIN(2, "cout4"), ct(16, 2), [(9, 11)], "bn", 1, bias=True, variant="nsplit 1"),
    Case("w_cout4_mb2_c32_th1", "wgrad", THIN(2, "cout4"), cv(32, 1, 3, 1, 1), [(11, 8)], bias=True, variant="nsplit 1"),
    Case("w_cout4_mb4_c48_th3_pro_2prob", "wgrad", THIN(4, "cout4"), cv(48, 3, 4, 1, 2), [(8, 9), (5, 6)], "in", 2, bias=True, variant="nsplit 1,1"),
    Case("w_cout4_mb4_c128_th4_split_prefill", "wgrad", THIN(4, "cout4"), ct(128, 4), [(21, 19)], bias=True, accum=True, env=SPLIT6, variant="nsplit 3"),
]

# ---- the pair: (name, backward-data half, backward-weight half, what conv_bwd_grouped returns, kernel named last, its variant) ----
# The two job lists of a pair are independent (the C entry compares kind / Cin / Cout of the first descriptors only), so each half has
# its own operands, and pair_c4_cout4_rb4 puts a 321 x 321 backward-data job (RB 4 needs > 400 tiles) beside a 30 x 34
# backward-weight job (the table keeps backward-weight within 4096 pixels); its 1020 pixels are also the pair's row with nsplit > 1.
_D1, _D3 = [(13, 61)], [(13, 61), (34, 34), (7, 30)]
_T1, _T3 = [(9, 11)], [(9, 11), (20, 6), (3, 17)]
PAIRS = [
    ("pair_s4_cin4_1prob", Case("p1d", "dgrad", S4, cv(2, 32), _D1), Case("p1w", "wgrad", None, cv(2, 32), _D1, bias=True), True, PAIR, "DK1 RB0 nsplit 1"),
    ("pair_s4_cin4_3prob_pro", Case("p2d", "dgrad", S4, cv(2, 32), _D3), Case("p2w", "wgrad", None, cv(2, 32), _D3, None, 2, bias=True), True, PAIR, "DK1 RB0 nsplit 1,1,1"),
    ("pair_c4_cout4_1prob_pro", Case("p3d", "dgrad", C4, ct(32, 2), _T1, "bn", 1, x=True, stats=True),
     Case("p3w", "wgrad", None, ct(32, 2), _T1, "bn", 1, bias=True), True, PAIR, "DK0 RB2 nsplit 1"),
    ("pair_c4_cout4_3prob", Case("p4d", "dgrad", C4, ct(20, 2), _T3, accum=True), Case("p4w", "wgrad", None, ct(20, 2), _T3, bias=True), True, PAIR, "DK0 RB2 nsplit 1,1,1"),
    ("pair_c4_cout4_rb4", Case("p5d", "dgrad", C4, ct(32, 2), [(321, 321)], "bn", 1, x=True, stats=True, variant="NB2 RB4 EPI gy1"),
     Case("p5w", "wgrad", None, ct(32, 2), [(30, 34)], "bn", 1, bias=True), True, PAIR, "DK0 RB4 nsplit 3"),
    # the documented refusals: sgan_conv_bwd_thin_pair answers 1 and the two grouped launches run
    ("refused_cin4_cout64", Case("r1d", "dgrad", S4, cv(2, 64), _D1), Case("r1w", "wgrad", THIN(4, "cin4"), cv(2, 64), _D1, bias=True, variant="nsplit 1"), False, S4, None),
    ("refused_cout4_cin48", Case("r2d", "dgrad", C4, ct(48, 2), _T1, "bn", 1, x=True, stats=True),
     Case("r2w", "wgrad", THIN(4, "cout4"), ct(48, 2), _T1, "bn", 1, bias=True, variant="nsplit 1"), False, C4, "NB2 RB2 EPI gy2"),
    ("refused_mismatched_lists", Case("r3d", "dgrad", S4, cv(2, 32), _D3[:2]), Case("r3w", "wgrad", THIN(2, "cin4"), cv(2, 32), _D1, bias=True, variant="nsplit 1"), False, S4, None),
]

ALL = FWD + DGRAD + WGRAD + [c for p in PAIRS for c in p[1:3]]
IDS = lambda c: c.name      # noqa: E731


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def _draw(case, seed):
    L = case.layer
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    d = dict(w=rn(*L.wshape()) * 0.05, b=rn(L.cout) * 0.1 if case.bias else None, probs=[])
    d["gamma"] = 1 + 0.2 * rn(L.cin) if case.norm == "bn" else None
    d["beta"] = 0.1 * rn(L.cin) if case.norm == "bn" else None
    for H, W in case.sizes:
        Ho, Wo = L.out_hw(H, W)
        p = dict(H=H, W=W, Ho=Ho, Wo=Wo, x=rn(L.cin, H, W) * 1.5 + 0.3, dy=rn(L.cout, Ho, Wo))
        p["prev"] = rn(L.cin, H, W) if (case.accum and case.op == "dgrad") else None
        d["probs"].append(p)
    if case.accum and case.op == "wgrad":
        d["prev_w"], d["prev_b"] = rn(*L.wshape()) * 0.5, rn(L.cout)
    return d


def signs(case, d):
    """The fp32 tensors whose sign an activation of this case reads."""
    if case.act == 0 or (case.op == "dgrad" and not case.x):
        return []
    if case.op == "dgrad":
        return [R.act_grad(p["x"], case.norm, case.act, d["gamma"], d["beta"])[2] for p in d["probs"]]
    return [R.prologue(p["x"], case.norm, case.act, d["gamma"], d["beta"])[2] for p in d["probs"]]


@functools.lru_cache(maxsize=None)
def data(case):
    seed = zlib.crc32(case.name.encode()) & 0xFFFFFF
    d = _draw(case, seed)
    for attempt in range(1, 64):
        ys = signs(case, d)
        if all(R.margin(y) > R.MASK_MARGIN for y in ys):
            return d
        # redraw, from the next seed, the elements that sit too close to the activation's kink (a whole-tensor redraw never ends
        # at the two large shapes: 3 10^6 values, each inside the margin with probability 4 10^-5)
        nxt = _draw(case, seed + attempt)
        for p, q, y in zip(d["probs"], nxt["probs"], ys):
            near = y.abs() <= 4 * R.MASK_MARGIN * y.abs().max()
            p["x"] = torch.where(near, q["x"], p["x"])
    raise AssertionError(f"{case.name}: no draw keeps the activation margin")


@functools.lru_cache(maxsize=None)
def reference(case):
    """Per problem the dict of thin_conv_ref.op_forward / op_dgrad; for wgrad one dict of op_wgrad.  Computed once, never modified."""
    d, L = data(case), case.layer
    n = dict(norm=case.norm, act=case.act, gamma=d["gamma"], beta=d["beta"])
    if case.op == "fwd":
        return [R.op_forward(L, p["x"], d["w"], d["b"], tanh=case.tanh, **n) for p in d["probs"]]
    if case.op == "dgrad":
        return [R.op_dgrad(L, p["dy"], d["w"], p["H"], p["W"], x=p["x"] if case.x else None, prev=p["prev"], **n) for p in d["probs"]]
    return R.op_wgrad(L, [(p["x"], p["dy"], case.norm, case.act, d["gamma"], d["beta"]) for p in d["probs"]], d.get("prev_w"), d.get("prev_b"))


# ---- the launchers, restated ----------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def phases(case, H, W):
    """[(Hp, Wp, taps)] of sg_build_phases for the result grid of the case's operation."""
    L, dg = case.layer, case.op == "dgrad"
    Hg, Wg = (H, W) if dg else L.out_hw(H, W)
    if (not L.tr) != dg:      # conv form: one phase
        return [(Hg, Wg, L.k * L.k)]
    out = []
    for a in range(L.s):
        for b in range(L.s):
            nt = sum(1 for ky in range(L.k) for kx in range(L.k) if (a + L.p - ky) % L.s == 0 and (b + L.p - kx) % L.s == 0)
            out.append((cdiv(Hg - a, L.s) if Hg > a else 0, cdiv(Wg - b, L.s) if Wg > b else 0, nt))
    return out


def ktot(case):
    ck = pad4(case.layer.cout if case.op == "dgrad" else case.layer.cin)
    return max(t for _, _, t in phases(case, *case.sizes[0])) * ck


def c4_variant(case):
    """NB / RB / EPI / grid.y of sg_launch_c4 (sg_c4_pick_rb: four row blocks per wave past 400 tiles of 256 result pixels)."""
    N = pad4(case.layer.cin if case.op == "dgrad" else case.layer.cout)
    tiles = sum(cdiv(hp * wp, 256) for H, W in case.sizes for hp, wp, _ in phases(case, H, W))
    rb = 4 if tiles > 400 else 2
    if case.stats or case.x or case.accum:
        return f"NB2 RB{rb} EPI gy{cdiv(N, 32)}"
    return f"NB{2 if N <= 32 else 3 if N <= 48 else 4} RB{rb}"


def thin_ranges(case, want=256.0, nw=8):
    """[[(m_begin, m_end) per wave] per workgroup] per problem, from sg_thin_plan and sg_wgrad_thin_body (nw waves per workgroup,
    want = SGAN_THIN_WANT; the pair launches nw = 4, want = 512)."""
    L = case.layer
    swap = pad4(L.cout) == 4 and pad4(L.cin) >= 16
    rows = pad4(L.cin if swap else L.cout)
    mb = int(case.kernel.split("<")[1][0]) if case.kernel else 2
    nrb = cdiv(rows, 16 * mb)
    min_pix = int(case.env.get("SGAN_THIN_MINPIX", 256))
    want = float(case.env.get("SGAN_THIN_WANT", want)) / nrb
    Ms = [(H * W) if swap else (lambda o: o[0] * o[1])(L.out_hw(H, W)) for H, W in case.sizes]
    out = []
    for M in Ms:
        nsplit = max(1, min(int(want * (M / sum(Ms)) + 0.5), M // min_pix, 1024))
        per_wg = cdiv(cdiv(M, nsplit), 4 * nw) * (4 * nw)
        per_wave = per_wg // nw
        out.append([[(sp * per_wg + w * per_wave, min(M, sp * per_wg + (w + 1) * per_wave)) for w in range(nw)] for sp in range(nsplit)])
    return out

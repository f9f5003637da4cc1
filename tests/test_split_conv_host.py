"""CPU checks of tests/split_conv_cases.py, the table of the split 16-bit-plane conv kernels (no GPU):
  * the planners restated there (sg_igemm3_eligible, sg3_pick_tile with the SGAN_TILE3 force rules, sg3p_plan / sg3p_wanted with patch
    extents, a_it, waste and the 100 workgroups of stride 2, kw2, sgw3_covers, sgw3_prepare's per / nsplit, sg_igemm3_fuse_plan with the
    SGAN_FUSE_KS_WGS cap, sg_wgrad3_fuse_plan, and wide_conv_cases.plan_ksplit) reproduce every row's kernel and variant -- the GPU
    tests hold the same strings to the library -- and the rows are what they claim (every tile, every patch form, KW 1 forced by an odd
    block count, an empty trailing split, ks moved by the cap, every DV x WV pair, a strict row on every branch);
  * the plane model of every row (plane_model's planes through thin_conv_ref's loops) equals plane_model.model_* where that exists
    (no output_padding), and lies within its own plane-rounding distance -- computed from the planes' residuals, nothing assumed --
    of the float64 result of the unrounded operands, which is held to torch's conv2d / conv_transpose2d and autograd; activation
    margins (MASK_MARGIN) hold on every row; the largest reference stays under a second;
  * the bound has teeth.  For every strict row, leaving out of the reference, in turn, one tap, one 32-wide k-tile (backward-weight:
    one 32-pixel chunk), the last (ragged) 32-channel block, one problem's last tile, moves at least one element past that row's bound;
    the normalised rows pass the tap / k-tile / chunk proof on their wider bounds too.  Leaving out a_lo b_hi, then a_hi b_lo, moves an
    element of EVERY strict bf16x3 row past its bound, the deepest included (a lo plane is 2^-12 (fp16) or 2^-9 (bf16) of its operand
    with a random sign, so the lost product is about sqrt(K) of that against a bound of K u M: the margin shrinks with depth -- 1.16
    bounds at K = 1568 on fp16 planes, the k7 patch row -- and the printed ratios say by how much).  The normalised rows' wider
    bounds (16 u M or 1024 u M more) do not show a lost plane product; the strict row of the same branch carries that proof."""
import time

import pytest
import torch
import torch.nn.functional as F

import plane_model as PM
import split_conv_cases as S
import thin_conv_cases as K
import thin_conv_ref as R
import wide_conv_cases as W

IGEMM = S.FWD + S.DGRAD
HALVES = [c for p in S.PAIRS if p[3] is not None for c in p[1:3]]
MODEL_ROWS = IGEMM + S.WGRAD + HALVES
STRICT = [c for c in MODEL_ROWS if S.strict(c)]


# ---- the planners -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", IGEMM, ids=S.IDS)
def test_igemm3_rows_reach_the_kernel_and_variant_they_name(case):
    assert S.igemm3_plan(case) == (case.kernel, case.variant)
    assert case.mode == case.math and (case.op == "dgrad" or case.planes)
    Ck, N = S.gemm(case)
    assert Ck >= 16 and Ck % 8 == 0 and all(min(m) >= S.MIN_PIXELS for m in S.maps(case))
    assert set(case.env) <= {"SGAN_TILE3", "SGAN_IGEMM3P"}


@pytest.mark.parametrize("case", S.WGRAD, ids=S.IDS)
def test_wgrad3_rows_reach_the_kernel_and_variant_they_name(case):
    assert S.wgrad3_plan(case) == (case.kernel, case.variant) and not case.env


@pytest.mark.parametrize("pair", S.PAIRS, ids=lambda p: p[0])
def test_fused_rows_reach_the_variant_they_name(pair):
    name, d, w, variant, kernel, ws = pair
    assert S.fused_plan(d, w, ws) == ((kernel, variant) if variant else None)
    assert not w.planes and d.layer is w.layer and d.sizes == w.sizes


def test_rows_are_what_they_claim():
    by = {c.name: c for c in S.ALL}
    tiles = {c.kernel for c in IGEMM}
    assert tiles >= {S.IG3(t) for t in (S.T128x32, S.T64, S.T128x64, S.T128)} | {S.IG3P(), S.IG3P(True), S.IG3P(x1=True), S.IG3(S.T64, True)}
    v = {(c.kernel, c.variant) for c in IGEMM}
    assert {x[1][:4] for x in v if x[0] == S.IG3P()} == {"AIT2", "AIT4"} and all(x[1][:4] == "AIT6" for x in v if x[0] == S.IG3P(True))
    # KW 2 at an even channel-block count of 2 and of 4, KW 1 forced by an odd one
    kw = {(S.gemm(c)[0] // 32, c.variant.split()[1]) for c in IGEMM if c.kernel.startswith("sg_igemm3p") and c.variant.startswith("AIT2")}
    assert kw >= {(2, "KW2"), (4, "KW2"), (3, "KW1")}
    # N no multiple of the forced tiles, pixels no multiple of 128, three problems of different sizes
    for t, bn in ((S.T128x64, 64), (S.T128, 128)):
        rows = [c for c in IGEMM if c.kernel == S.IG3(t)]
        assert any(S.gemm(c)[1] % bn for c in rows) and any(len(c.sizes) == 3 and len(set(c.sizes)) == 3 for c in rows)
        assert any((hp * wp) % 128 for c in rows for H, W_ in c.sizes for hp, wp, _ in K.phases(c, H, W_))
    assert {S.gemm(c)[1] for c in IGEMM if c.kernel == S.IG3(S.T128x32)} >= {24, 32}
    # the ConvT k3 s2 op1 row: the trailing splits of the 1- and 2-tap phases are empty
    c = by["f_convT_k3_short_phases_split4"]
    nkt = [K.cdiv(len(t) * S.gemm(c)[0], 32) for t in S.phase_taps(c)]
    per = K.cdiv(max(nkt), 4)
    assert nkt == [5, 9, 9, 17] and [sum(1 for s in range(4) if s * per >= n) for n in nkt] == [3, 2, 2, 0]
    # split-K: forward with statistics, backward-data with act'(norm(x)) and both sums, accumulate; the same epilogue unsplit
    sp = [c for c in IGEMM if c.variant.startswith("ks") and not c.variant.startswith("ks1 ")]
    assert any(c.op == "fwd" and c.stats for c in sp) and any(c.op == "dgrad" and c.x and c.stats for c in sp) and any(c.accum for c in sp)
    assert any(c.x and c.stats and c.variant.startswith("ks1 ") for c in S.DGRAD) and any(c.accum and c.variant.startswith("ks1 ") for c in S.DGRAD)
    # the patch kernel's backward-data: a stride-2 Conv (four phases of 2 x 2 taps), a stride-2 ConvT (s2)
    assert [len(t) for t in S.phase_taps(by["pd_conv_s2_phases"])] == [4, 4, 4, 4] and by["pd_convT_s2"].kernel == S.IG3P(True)
    # maps that are no multiples of 8 in either direction on the patch kernel
    assert any(h % 8 and w % 8 for c in IGEMM if "igemm3p" in c.kernel for H, W_ in c.sizes for h, w, _ in K.phases(c, H, W_))
    # backward-weight: both tiles, Cout 64 / 72 and 32 / 40 / 56, K and pixel tails, three splits in one launch, both planes, x1
    assert {c.layer.cout for c in S.WGRAD if c.kernel == S.WG3(S.W64)} >= {64, 72} and {c.layer.cout for c in S.WGRAD if c.kernel == S.WG3(S.W32)} >= {32, 40, 56}
    assert all(S.max_k(c) % S.wgrad3_prepare(c)[2] for c in S.WGRAD) and any(len(set(S.wgrad3_prepare(c)[4])) == 3 for c in S.WGRAD)
    assert any((hp * wp) % 32 for c in S.WGRAD for H, W_ in c.sizes for hp, wp, _ in K.phases(c, H, W_))
    assert {(c.norm, c.act) for c in S.WGRAD} >= {("in", 2), ("bn", 1), (None, 0)} and any(c.accum for c in S.WGRAD) and all(c.bias for c in S.WGRAD)
    assert {c.planes for c in S.WGRAD} == {True, False} and any(c.mode == "bf16x1" for c in S.WGRAD)
    # the fused launch: all ten pairs, a split that stays, a split the cap moves, fp16 planes on 6, the re-plan, the one-plane mixes
    fv = {p[3][:7] for p in S.PAIRS if p[3]}
    assert fv == {f"DV{d} WV{w}" for d in (1, 2, 3, 5, 6) for w in (1, 2)}
    capped = next(p for p in S.PAIRS if p[0] == "fu_dv3_ks_capped_8_to_4")
    assert W.plan_ksplit(capped[1], 64, 64) == 8 and S.fuse_plan_dgrad(capped[1]) == (3, 4)
    stays = next(p for p in S.PAIRS if p[0] == "fu_dv3_ks4_ws")
    assert W.plan_ksplit(stays[1], 64, 64) == 4 and S.fuse_plan_dgrad(stays[1]) == (3, 4)
    assert any("DV6" in p[3] and "F161" in p[3] for p in S.PAIRS if p[3]) and any(p[1].planes and "F160" in p[3] for p in S.PAIRS if p[3])
    assert {p[4] for p in S.PAIRS if p[3]} == {S.FUSED, S.FUSED_X1, S.FUSED_WX1} and {("WPRO1" in p[3]) for p in S.PAIRS if p[3]} == {True, False}
    assert len([p for p in S.PAIRS if p[3] is None]) == 4
    # the re-planned row: its bf16-plane and fp16-plane models are more than two bounds apart in every problem
    rp = next(p for p in S.PAIRS if p[0] == "fu_dv3_replanned_bf16")[1]
    for b16, f16 in zip(S.reference(rp, False), S.reference(rp, True)):
        assert float(((b16["own"] - f16["own"]).abs() / torch.maximum(b16["own_bound"], f16["own_bound"])).max()) > 2.0
    # every branch has a strict row
    for kernel in tiles | {c.kernel for c in S.WGRAD}:
        assert any(S.strict(c) for c in IGEMM + S.WGRAD if c.kernel == kernel), kernel


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def _torch_truth(case, p, d, a):
    L = case.layer
    w = d["w"].double()
    conv = (lambda t, ww: F.conv_transpose2d(t, ww, None, L.s, L.p, output_padding=L.op)) if L.tr else (lambda t, ww: F.conv2d(t, ww, None, L.s, L.p))
    if case.op == "fwd":
        return conv(a[None], w)[0]
    if case.op == "dgrad":
        x = torch.zeros(1, L.cin, p["H"], p["W"], dtype=torch.float64, requires_grad=True)
        (conv(x, w)[0] * p["dy"].double()).sum().backward()
        return x.grad[0]
    ww = torch.zeros_like(w, requires_grad=True)
    (conv(a[None], ww)[0] * p["dy"].double()).sum().backward()
    return ww.grad


def _operands(case, p, d):
    """(first operand, second operand) of the row's product in problem p, float64."""
    if case.op == "dgrad":
        return p["dy"].double(), d["w"].double()
    a = R.prologue(p["x"], case.norm, case.act, d["gamma"], d["beta"])[0]
    return (a, d["w"].double()) if case.op == "fwd" else (a, p["dy"].double())


def _apply(case, p, a, b, only=None):
    L = case.layer
    if case.op == "fwd":
        return R.forward(L, a, b, only=only)
    if case.op == "dgrad":
        return R.dgrad(L, a, b, p["H"], p["W"], only=only)
    return R.wgrad(L, a, b)


@pytest.mark.parametrize("case", MODEL_ROWS, ids=S.IDS)
def test_model_matches_plane_model_and_torch_within_its_plane_rounding(case):
    d, L = K.data(case), case.layer
    for y in K.signs(case, d):
        assert R.margin(y) > R.MASK_MARGIN
    for p in d["probs"]:
        a, b = _operands(case, p, d)
        A, B = S.operand_planes(case, a, b, None)
        model = sum(_apply(case, p, pa, pb) for pa, pb in S.pairs(case.mode, A, B))
        truth = _apply(case, p, a, b)
        tt = _torch_truth(case, p, d, a)
        assert float((truth - tt).abs().max()) <= 1e-12 * float(tt.abs().max())
        # the model's own plane-rounding distance, from the planes' residuals
        if case.mode == "bf16x3":
            dist = _apply(case, p, (A[0] + A[1] - a).abs(), b.abs()) + _apply(case, p, (A[0] + A[1]).abs(), (B[0] + B[1] - b).abs()) + _apply(case, p, A[1].abs(), B[1].abs())
        else:
            dist = _apply(case, p, (A[0] - a).abs(), b.abs()) + _apply(case, p, A[0].abs(), (B[0] - b).abs())
        assert bool(((model - truth).abs() <= dist * (1 + 1e-9) + 1e-300).all())
        # and the residuals are what the formats promise: 11 + 11 bits (fp16, 2^-25 where a plane is subnormal), 8 + 8 bits (bf16)
        for t, P_ in ((a, A), (b, B)):
            f16 = case.op == "fwd" or case.planes
            r = (P_[0] + P_[1] - t).abs()
            if f16:
                # planes of t * 2^s (s = 0, 10, or the gradient's shift, which puts its maximum at 2^14 or above): the subnormal floor
                # 2^-25 is in scaled units, at most 2^-25 in unscaled ones when s >= 0, max|t| 2^-39 for a gradient
                floor = max(2.0 ** -25, 2.0 ** -39 * float(t.abs().max()))
                assert bool((r <= 2.0 ** -22 * t.abs() + floor).all())
            else:
                assert bool((r <= 2.0 ** -16 * t.abs() + 1e-300).all())
        if L.op == 0:
            tr, s, pd = L.tr, L.s, L.p
            if case.op == "fwd":
                pmod = PM.model_fwd(case.mode, tr, a[None], d["w"], None, s, pd)[0]
            elif case.op == "dgrad":
                pmod = PM.model_dgrad(case.mode, tr, p["dy"][None], d["w"], s, pd, (1, L.cin, p["H"], p["W"]), float(p["dy"].abs().max()) if case.planes else None)[0]
            else:
                pmod = PM.model_wgrad(case.mode, tr, a[None], p["dy"][None], L.wshape(), s, pd, float(p["dy"].abs().max()) if case.planes else None)
            assert float((model - pmod).abs().max()) <= 1e-12 * float(model.abs().max())


def test_the_largest_reference_stays_under_a_second():
    big = [c for c in S.ALL if c.name.startswith("fu_dv3_ks_capped_8_to_4")]
    assert {(c.layer.cin, c.layer.cout, c.layer.k) for c in big} == {(128, 256, 4)}      # backward-data: 256 -> 128 on a 16 x 16 map
    for c in big:
        S.reference.cache_clear()
        K.data(c)
        t = time.perf_counter()
        S.reference(c)
        assert time.perf_counter() - t < 1.0


# ---- the bound has teeth ------------------------------------------------------------------------------------------------------------
def _bounds(case):
    ref = S.reference(case)
    if case.op == "wgrad":
        return [ref["dw_bound"]]
    return [r["pre_bound"] if case.op == "fwd" else r["own_bound"] for r in ref]


def _factor(case, i):
    return S.reference(case)[i]["f"] if case.op == "dgrad" else 1.0


def _planes(case, p, d):
    a, b = _operands(case, p, d)
    return S.operand_planes(case, a, b, None)


def _piece(case, p, A, B, only=None, c0=None, c1=None, drop=None):
    """The model's contribution restricted to one tap and / or the gathered channels [c0, c1)."""
    L = case.layer
    if c0 is not None:
        if case.op == "fwd":
            A = tuple(t[c0:c1] for t in A)
            B = tuple(t.narrow(0 if L.tr else 1, c0, c1 - c0) for t in B)
        else:
            A = tuple(t[c0:c1] for t in A)
            B = tuple(t.narrow(1 if L.tr else 0, c0, c1 - c0) for t in B)
    return sum(_apply(case, p, pa, pb, only=only) for pa, pb in S.pairs(case.mode, A, B, drop))


@pytest.mark.parametrize("case", [c for c in MODEL_ROWS if c.op != "wgrad"], ids=S.IDS)
def test_a_dropped_tap_k_tile_channel_block_or_last_tile_is_visible(case):
    d, L = K.data(case), case.layer
    Ck = S.gemm(case)[0]
    worst = dict(tap={}, ktile={}, block={}, tile={})
    for i, p in enumerate(d["probs"]):
        A, B = _planes(case, p, d)
        bound, f = _bounds(case)[i].clamp_min(1e-300), _factor(case, i)
        vis = lambda c: float(((c * f).abs() / bound).max())      # noqa: E731
        for ky, kx, _i, _o in L.taps(p["H"], p["W"]):
            worst["tap"][(i, ky, kx)] = vis(_piece(case, p, A, B, only=(ky, kx)))
        for ph, taps in enumerate(S.phase_taps(case)):
            for kt in range(K.cdiv(len(taps) * Ck, 32)):
                c = sum(_piece(case, p, A, B, only=(ky, kx), c0=c0, c1=c1) for ky, kx, c0, c1 in W.ktile_terms(case, ph, kt))
                if torch.is_tensor(c) and float(c.abs().max()) > 0:      # (a tap that reaches no pixel of this problem)
                    worst["ktile"][(i, ph, kt)] = vis(c)
        c0 = (Ck - 1) // 32 * 32
        worst["block"][i] = vis(_piece(case, p, A, B, c0=c0, c1=Ck))
        # the last tile of the problem: the last pixels, row-major, of its last phase
        ref = S.reference(case)[i]["pre" if case.op == "fwd" else "own"]
        hp, wp, _ = K.phases(case, p["H"], p["W"])[-1]
        n = min(64, hp * wp)
        m = torch.arange(hp * wp - n, hp * wp)
        os_ = L.s if len(S.phase_taps(case)) > 1 else 1
        oa = ob = os_ - 1
        worst["tile"][i] = float((ref.abs() / bound)[:, (m // wp) * os_ + oa, (m % wp) * os_ + ob].max())
    print(f"{case.name}: least visible " + ", ".join(f"{k} {min(v.values()):.1f}" for k, v in worst.items()) + " bounds")
    kinds = worst if S.strict(case) else {k: worst[k] for k in ("tap", "ktile")}
    for k, v in kinds.items():
        assert min(v.values()) > 1.0, (k, min(v.items(), key=lambda kv: kv[1]))


@pytest.mark.parametrize("case", [c for c in MODEL_ROWS if c.op == "wgrad"], ids=S.IDS)
def test_a_dropped_chunk_tap_or_channel_block_is_visible(case):
    """One 32-pixel chunk of sg_wgrad3_kernel's pixel walk (phase by phase, row-major inside the phase), one tap of dw, the last
    32-channel block of the activations left out."""
    d, L = K.data(case), case.layer
    bound, worst = _bounds(case)[0].clamp_min(1e-300), {}
    os_ = L.s if L.tr else 1
    for i, p in enumerate(d["probs"]):
        A, B = _planes(case, p, d)
        for ph, (hp, wp, _) in enumerate(K.phases(case, p["H"], p["W"])):
            oa, ob = (ph // L.s, ph % L.s) if L.tr else (0, 0)
            for ch in range(K.cdiv(hp * wp, 32)):
                m = torch.arange(ch * 32, min(ch * 32 + 32, hp * wp))
                mask = torch.zeros(p["Ho"], p["Wo"], dtype=torch.float64)
                mask[(m // wp) * os_ + oa, (m % wp) * os_ + ob] = 1.0
                c = sum(R.wgrad(L, pa, pb * mask) for pa, pb in S.pairs(case.mode, A, B))
                worst[(i, ph, ch)] = float((c.abs() / bound).max())
    print(f"{case.name}: least visible chunk {min(worst.values()):.1f} bounds ({len(worst)} chunks)")
    assert min(worst.values()) > 1.0, min(worst.items(), key=lambda kv: kv[1])
    if S.strict(case):      # a whole tap of dw, a 32-channel block of its rows: the values themselves against their bounds
        dw = S.reference(case)["dw"] - (K.data(case)["prev_w"].double() if case.accum else 0.0)
        r = dw.abs() / bound
        assert float(r.amax((0, 1)).min()) > 1.0
        cin_dim = 0 if L.tr else 1
        c0 = (L.cin - 1) // 32 * 32
        assert float(r.narrow(cin_dim, c0, L.cin - c0).max()) > 1.0


def _plane_ratios(case):
    d = K.data(case)
    out = {}
    for drop in ("lo_hi", "hi_lo"):
        w = 0.0
        if case.op == "wgrad":
            c = sum(_piece(case, p, *_planes(case, p, d)) - _piece(case, p, *_planes(case, p, d), drop=drop) for p in d["probs"])
            w = float((c.abs() / _bounds(case)[0].clamp_min(1e-300)).max())
        else:
            for i, p in enumerate(d["probs"]):
                A, B = _planes(case, p, d)
                c = (_piece(case, p, A, B) - _piece(case, p, A, B, drop=drop)) * _factor(case, i)
                w = max(w, float((c.abs() / _bounds(case)[i].clamp_min(1e-300)).max()))
        out[drop] = w
    return out


def _kmax(case):
    ref = S.reference(case)
    return float(ref["K"].max()) if case.op == "wgrad" else max(float(r["K"].max()) for r in ref)


X3_STRICT = [c for c in STRICT if c.mode == "bf16x3"]


@pytest.mark.parametrize("case", X3_STRICT, ids=S.IDS)
def test_a_lost_plane_product_is_visible(case):
    r, Kc = _plane_ratios(case), _kmax(case)
    f16 = case.op == "fwd" or case.planes
    print(f"{case.name}: K {Kc:.0f}, {'fp16' if f16 else 'bf16'} planes: without a_lo b_hi {r['lo_hi']:.2f} bounds, without a_hi b_lo {r['hi_lo']:.2f} bounds")
    assert min(r.values()) > 1.0, r

"""CPU checks of tests/wide_conv_cases.py, the table of the exact-fp32 MFMA conv kernels (no GPU):
  * the three loops of tests/thin_conv_ref.py against torch's conv2d / conv_transpose2d and autograd in float64 at every row's layer and
    size, an fp32 restatement inside every bound, the activation margin (the checks of tests/test_thin_conv_ref_host.py, run on
    these rows), and L + c <= L_MAX;
  * the planners restated in wide_conv_cases (sg_pick_tile, the half-tile rule, sg_plan_ksplit with sg_time_model, kw2, the
    backward-weight per / nsplit) reproduce every row's kernel and variant -- the GPU tests hold the same strings to the library --
    and the kernels' own index arithmetic, restated, shows which splits and wave groups come out empty or short: the rows that claim
    an empty trailing split, an uneven share, a partial k-tile or differing pixel splits provably have them;
  * sensitivity, from the reference alone: dropping any single tap moves an element of the outermost two rows / columns by more than
    its bound; dropping one 32-wide k-tile, or (backward-weight) one 32-pixel chunk, moves some element by more than its bound.  A
    kernel that loses a border product, a k-tile at a split seam or a chunk at a pixel-split seam cannot stay inside the bounds."""
import pytest
import torch

import test_thin_conv_ref_host as H
import thin_conv_cases as K
import thin_conv_ref as R
import wide_conv_cases as W
from thin_conv_ref import pad4

IGEMM = W.FWD + W.FALLBACK + W.DGRAD


@pytest.mark.parametrize("case", W.ALL, ids=W.IDS)
def test_reference_matches_torch_and_fp32_is_inside_the_bound(case):
    H.test_reference_matches_torch_and_fp32_is_inside_the_bound(case)


@pytest.mark.parametrize("case", W.ALL, ids=W.IDS)
def test_mask_margin_and_prologue(case):
    H.test_mask_margin_and_prologue(case)


@pytest.mark.parametrize("case", W.ALL, ids=W.IDS)
def test_sum_length_within_l_max(case):
    L = case.layer
    for H_, W_ in case.sizes:
        if case.op == "fwd":
            assert float(R.count_fwd(L, H_, W_).max()) + R.CA_FWD + R.C_PRO <= R.L_MAX
        elif case.op == "dgrad":
            assert float(R.count_dgrad(L, H_, W_).max()) + R.C0_DGRAD <= R.L_MAX
    if case.op == "wgrad":
        assert float(K.reference(case)["L"].max()) + R.CA_WGRAD + R.C_PRO <= R.L_MAX
    assert len(W.phase_taps(case)[0]) <= 16 and max(W.gemm(case)) <= 464 and W.max_k(case) + 9 <= R.L_MAX


# ---- the planners -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", IGEMM, ids=W.IDS)
def test_igemm_rows_reach_the_kernel_and_variant_they_name(case):
    kernel, variant, ks, kw = W.igemm_plan(case)
    assert (kernel, variant) == (case.kernel, case.variant)
    Ck, N = W.gemm(case)
    # not a shape of the direct kernels: sg_use_small_n wants N = 4 without statistics / forward tensor / accumulate, sg_use_c4 Ck = 4
    assert Ck != 4 and (N != 4 or case.stats or case.x or case.accum)
    if case.math == "bf16x3":      # sg_igemm3_eligible says no
        pix = min(min(h * w, ho * wo) for h, w in case.sizes for ho, wo in [case.layer.out_hw(h, w)])
        assert Ck < 16 or Ck % 8 or N < 16 or pix < 256
    else:
        assert case.math == "f32"
    # the k-tile ranges of every phase: disjoint, in order, covering [0, nkt) once; a wave group never walks past its iterations
    shares = W.igemm_shares(case)
    for taps, ph in zip(W.phase_taps(case), shares):
        nkt_total = K.cdiv(len(taps) * Ck, 32)
        walked = [(k0, n) for split in ph for k0, n, _ in split if n > 0]
        assert walked[0][0] == 0 and sum(n for _, n in walked) == nkt_total
        assert all(a[0] + a[1] == b[0] for a, b in zip(walked, walked[1:]))
        assert all(n <= it for split in ph for _, n, it in split) and len(ph) == ks and all(len(s) == kw for s in ph)
    empty = [(p, s) for p, ph in enumerate(shares) for s, split in enumerate(ph) if sum(n for _, n, _ in split) == 0]
    short = [(p, s, g) for p, ph in enumerate(shares) for s, split in enumerate(ph) for g, (_, n, it) in enumerate(split) if 0 < n < it or (n == 0 and it > 0)]
    partial = [p for p, taps in enumerate(W.phase_taps(case)) if len(taps) * Ck % 32]
    print(f"{case.name}: {kernel} {variant}; k-tiles per phase {[K.cdiv(len(t) * Ck, 32) for t in W.phase_taps(case)]}; "
          f"empty (phase, split) {empty}; short (phase, split, group) {short}; phases with a partial last k-tile {partial}")
    CLAIMS[case.name] = dict(empty=empty, short=short, partial=partial, ks=ks, kw=kw)


CLAIMS = {}


def test_rows_are_what_they_claim():
    for c in IGEMM:
        if c.name not in CLAIMS:
            test_igemm_rows_reach_the_kernel_and_variant_they_name(c)
    C = CLAIMS
    # the empty trailing split: the fourth split of the 1- and 2-tap phases, not of the 4-tap phase
    assert C["f_convT_k3_short_phases_split4"]["empty"] == [(0, 3), (1, 3), (2, 3)]
    assert all(not v["empty"] for k, v in C.items() if k != "f_convT_k3_short_phases_split4")
    # the uneven hand-off: wave group 1 of the only split walks fewer k-tiles than it runs iterations
    assert C["f_64x64_kw2_uneven_2prob"]["short"] == [(0, 0, 1)] and C["f_64x64_kw2_uneven_2prob"]["partial"] == [0]
    assert C["d_master_weights_k108"]["partial"] == [0] and not W.DGRAD[0].wt and W.DGRAD[0].kernel == W.IG(128, 32, False)
    assert W.igemm_shares(W.FWD[9])[0][0] == [(0, 4, 4), (4, 4, 4)]      # f_64x64_split8_kw2: 8 k-tiles per workgroup, 4 per group
    # every tile shape, both weight layouts, split-K on each of the three tiles that take it, and every (KW, PRO) instantiation
    assert {c.kernel for c in IGEMM} == {W.IG(128, 16), W.IG(128, 32), W.IG(128, 32, False), W.IG(64, 32), W.IG(64, 64)}
    assert {c.kernel for c in IGEMM if C[c.name]["ks"] > 1} == {W.IG(128, 32), W.IG(64, 64)}
    assert {c.variant[4:] for c in IGEMM if c.kernel in (W.IG(64, 32), W.IG(64, 64)) and C[c.name]["ks"] == 1} >= {"KW1 PRO0", "KW1 PRO1", "KW2 PRO0", "KW2 PRO1"}
    assert {c.variant.split()[1:] == ["KW2", "PRO0"] for c in IGEMM if C[c.name]["ks"] > 1} == {True, False}
    # the refusals: deep enough to split, were it not for 256 % (N / 4)
    for name in ("f_128x16_n12_deep_refused", "f_64x32_n48_deep_refused"):
        c = next(c for c in W.FWD if c.name == name)
        assert 256 % (W.gemm(c)[1] // 4) != 0 and K.cdiv(W.max_k(c), 32) >= 64 and W.total_tiles(c, 64) <= 32
    # the mid-grid branch is the one that decides its row
    c = next(c for c in W.FWD if c.name == "f_64x64_mid_grid")
    assert 192 < W.total_tiles(c, 64) * 2 <= 768 and K.cdiv(W.max_k(c), 32) >= 128
    # split-K epilogue: forward with bias + statistics, with tanh, backward-data with the norm of the forward tensor, with accumulate
    sp = [c for c in IGEMM if C[c.name]["ks"] > 1]
    assert any(c.tanh for c in sp) and any(c.stats and c.op == "fwd" for c in sp) and any(c.x and c.norm and c.stats for c in sp if c.op == "dgrad")
    assert any(c.accum for c in sp) and any(c.accum for c in W.DGRAD if C[c.name]["ks"] == 1) and any(not c.x for c in W.DGRAD)
    # some M that is no multiple of the tile height, some N that is no multiple of the tile width
    assert any((h * w) % 64 for c in IGEMM for H_, W_ in c.sizes for h, w, _ in K.phases(c, H_, W_))
    assert {W.gemm(c)[1] for c in IGEMM} >= {4, 8, 12, 20, 48, 72}


@pytest.mark.parametrize("case", W.WGRAD, ids=W.IDS)
def test_wgrad_rows_reach_the_kernel_and_variant_they_name(case):
    kernel, variant, per, nsplit = W.wgrad_plan(case)
    assert (kernel, variant) == (case.kernel, case.variant) and case.math == "f32"
    assert pad4(case.layer.cin) != 4 and pad4(case.layer.cout) != 4      # not a thin layer
    for prob, (H_, W_) in zip(W.wgrad_ranges(case), case.sizes):
        for ranges, (hp, wp, _) in zip(prob, K.phases(case, H_, W_)):
            live = [r for r in ranges if r[1] > r[0]]
            assert live[0][0] == 0 and live[-1][1] == K.cdiv(hp * wp, 32) and all(a[1] == b[0] for a, b in zip(live, live[1:]))
            print(f"{case.name}: {hp}x{wp} pixels, chunk ranges {ranges}")


def test_wgrad_rows_are_what_they_claim():
    stored = {pad4(c.layer.cout): c.kernel for c in W.WGRAD}
    assert stored[8] == stored[12] == W.WG16 and stored[20] == W.WG32 and stored[72] == W.WG64
    assert any(c.layer.cout % 4 for c in W.WGRAD)      # logical rows short of the stored ones
    bkc = {W.WG16: 128, W.WG32: 64, W.WG64: 64}
    assert all(W.max_k(c) % bkc[c.kernel] for c in W.WGRAD if c.name != "w_32x64_c20")      # K tails
    assert all(any((hp * wp) % 32 for H_, W_ in c.sizes for hp, wp, _ in K.phases(c, H_, W_)) for c in W.WGRAD)      # pixel tails
    assert any(c.layer.tr and len(W.phase_taps(c)) == 4 for c in W.WGRAD)
    assert len(set(W.wgrad_plan(W.WGRAD[-1])[3])) == 3 and len(W.WGRAD[-1].sizes) == 3
    assert {(c.norm, c.act) for c in W.WGRAD} >= {("in", 2), ("bn", 1), (None, 0)}
    assert any(c.accum for c in W.WGRAD) and all(c.bias for c in W.WGRAD)


# ---- sensitivity ------------------------------------------------------------------------------------------------------------------
def _sub(L, c0, c1, gathered_is_cout):
    """The layer restricted to channels [c0, c1) of the gathered side, and the slicer of its torch-layout weight."""
    dim = (1 if L.tr else 0) if gathered_is_cout else (0 if L.tr else 1)
    return lambda w: w.narrow(dim, c0, c1 - c0)


def _ktile(case, d, ref_i, p, phase, kt):
    """The contribution of one 32-wide k-tile to the result of problem p, from the reference's loops."""
    L, tot = case.layer, 0.0
    for ky, kx, c0, c1 in W.ktile_terms(case, phase, kt):
        if case.op == "fwd":
            c1 = min(c1, L.cin)
            if c1 > c0:
                tot = tot + R.forward(L, ref_i["a"][c0:c1], _sub(L, c0, c1, False)(d["w"].double()), only=(ky, kx))
        else:
            c1 = min(c1, L.cout)
            if c1 > c0:
                tot = tot + R.dgrad(L, p["dy"].double()[c0:c1], _sub(L, c0, c1, True)(d["w"].double()), p["H"], p["W"], only=(ky, kx))
    return tot


def _tiles_to_drop(case):
    """(phase, k-tile): every k-tile of every phase, the seams between splits and wave groups and the partial last tile among them."""
    return [(ph, kt) for ph, taps in enumerate(W.phase_taps(case)) for kt in range(K.cdiv(len(taps) * W.gemm(case)[0], 32))]


@pytest.mark.parametrize("case", IGEMM, ids=W.IDS)
def test_a_dropped_tap_or_k_tile_is_visible(case):
    d, ref, L = K.data(case), K.reference(case), case.layer
    worst_tap, worst_kt = {}, {}
    for i, p in enumerate(d["probs"]):
        if case.op == "fwd":
            f, bound, ring = 1.0, ref[i]["pre_bound"], torch.from_numpy(R.ring2(p["Ho"], p["Wo"]))
        else:
            f = R.act_grad(p["x"], case.norm, case.act, d["gamma"], d["beta"])[0] if case.x else 1.0
            bound, ring = ref[i]["bound"], torch.from_numpy(R.ring2(p["H"], p["W"]))
        bound = bound.clamp_min(1e-300)
        for ky, kx, _i, _o in L.taps(p["H"], p["W"]):
            if case.op == "fwd":
                c = R.forward(L, ref[i]["a"], d["w"].double(), only=(ky, kx))
            else:
                c = R.dgrad(L, p["dy"].double(), d["w"].double(), p["H"], p["W"], only=(ky, kx)) * f
            worst_tap[(i, ky, kx)] = float((c.abs() / bound)[:, ring].max())
        for ph, kt in _tiles_to_drop(case):
            c = _ktile(case, d, ref[i], p, ph, kt)
            if torch.is_tensor(c):      # (a phase without pixels in this problem contributes nothing and is never launched)
                worst_kt[(i, ph, kt)] = float(((c * f).abs() / bound).max())
    print(f"{case.name}: least visible tap {min(worst_tap.values()):.1f} bounds on the outer ring, least visible k-tile "
          f"{min(worst_kt.values()):.1f} bounds ({len(worst_kt)} k-tiles dropped)")
    assert min(worst_tap.values()) > 1.0, min(worst_tap.items(), key=lambda kv: kv[1])
    assert min(worst_kt.values()) > 1.0, min(worst_kt.items(), key=lambda kv: kv[1])


@pytest.mark.parametrize("case", W.WGRAD, ids=W.IDS)
def test_a_dropped_chunk_is_visible(case):
    """One 32-pixel chunk of sg_wgrad_kernel's pixel walk (phase by phase, row-major inside the phase) left out of dw."""
    d, ref, L = K.data(case), K.reference(case), case.layer
    bound, worst = ref["dw_bound"].clamp_min(1e-300), {}
    os_ = L.s if L.tr else 1
    for i, p in enumerate(d["probs"]):
        a = R.prologue(p["x"], case.norm, case.act, d["gamma"], d["beta"])[0]
        for ph, (hp, wp, _) in enumerate(K.phases(case, p["H"], p["W"])):
            oa, ob = (ph // L.s, ph % L.s) if L.tr else (0, 0)
            for ch in range(K.cdiv(hp * wp, 32)):
                m = torch.arange(ch * 32, min(ch * 32 + 32, hp * wp))
                mask = torch.zeros(p["Ho"], p["Wo"], dtype=torch.float64)
                mask[(m // wp) * os_ + oa, (m % wp) * os_ + ob] = 1.0
                worst[(i, ph, ch)] = float((R.wgrad(L, a, p["dy"].double() * mask).abs() / bound).max())
    assert sum(K.cdiv(hp * wp, 32) for p in d["probs"] for hp, wp, _ in K.phases(case, p["H"], p["W"])) == len(worst)
    print(f"{case.name}: least visible chunk {min(worst.values()):.1f} bounds ({len(worst)} chunks)")
    assert min(worst.values()) > 1.0, min(worst.items(), key=lambda kv: kv[1])

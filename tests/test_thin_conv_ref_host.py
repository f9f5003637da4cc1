"""CPU checks of tests/thin_conv_ref.py and tests/thin_conv_cases.py: the float64 reference against torch's conv2d /
conv_transpose2d and autograd for every row of the table, M and L against direct loops, an fp32 restatement inside every bound, the
activation margin, the bound's power to see one dropped term, and the launch variants the table claims for its rows."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import thin_conv_cases as K
import thin_conv_ref as R

CASES = K.ALL


def _conv(L, a, w, b=None):
    if L.tr:
        return F.conv_transpose2d(a[None], w, b, stride=L.s, padding=L.p, output_padding=L.op)[0]
    return F.conv2d(a[None], w, b, stride=L.s, padding=L.p)[0]


def _torch_ops(case, dt):
    """forward / backward-data / backward-weight of every problem by torch and autograd in dtype dt, from the prologue's output."""
    d, L = K.data(case), case.layer
    out = []
    for p in d["probs"]:
        a = R.prologue(p["x"], case.norm, case.act, d["gamma"], d["beta"])[0].to(dt).clone().requires_grad_(True)
        w = d["w"].to(dt).clone().requires_grad_(True)
        y = _conv(L, a, w, d["b"].to(dt) if d["b"] is not None else None)
        (y * p["dy"].to(dt)).sum().backward()
        out.append((y.detach(), a.grad, w.grad))
    return out


def _close(a, b, what):
    assert float((a.double() - b.double()).abs().max()) <= 1e-12 * (1.0 + float(b.double().abs().max())), what


@pytest.mark.parametrize("case", CASES, ids=K.IDS)
def test_reference_matches_torch_and_fp32_is_inside_the_bound(case):
    d, ref = K.data(case), K.reference(case)
    t64, t32 = _torch_ops(case, torch.float64), _torch_ops(case, torch.float32)
    dw64, dw32 = sum(t[2] for t in t64), sum(t[2] for t in t32)
    for i, p in enumerate(d["probs"]):
        if case.op == "fwd":
            _close(ref[i]["pre"], t64[i][0], "forward")
            r32 = torch.tanh(t32[i][0]) if case.tanh else t32[i][0]
            assert bool(((r32.double() - ref[i]["ref"]).abs() <= ref[i]["bound"]).all())
        elif case.op == "dgrad":
            f = R.act_grad(p["x"], case.norm, case.act, d["gamma"], d["beta"])[0] if case.x else 1.0
            prev = p["prev"] if p["prev"] is not None else 0.0
            _close(ref[i]["ref"], t64[i][1] * f + prev, "backward-data")
            r32 = t32[i][1] * (f.float() if case.x else 1.0) + (p["prev"] if p["prev"] is not None else 0.0)
            assert bool(((r32.double() - ref[i]["ref"]).abs() <= ref[i]["bound"]).all())
    if case.op == "wgrad":
        pw, pb = d.get("prev_w"), d.get("prev_b")
        _close(ref["dw"], dw64 + (pw if pw is not None else 0.0), "backward-weight")
        db = sum(p["dy"].double().sum((1, 2)) for p in d["probs"]) + (pb if pb is not None else 0.0)
        _close(ref["db"], db, "bias gradient")
        r32 = dw32 + (pw if pw is not None else 0.0)
        assert bool(((r32.double() - ref["dw"]).abs() <= ref["dw_bound"]).all())
        b32 = sum(p["dy"].sum((1, 2)) for p in d["probs"]) + (pb if pb is not None else 0.0)
        assert bool(((b32.double() - ref["db"]).abs() <= ref["db_bound"]).all())


@pytest.mark.parametrize("case", CASES, ids=K.IDS)
def test_mask_margin_and_prologue(case):
    d = K.data(case)
    for y in K.signs(case, d):
        assert R.margin(y) > R.MASK_MARGIN
    if case.norm and case.op != "dgrad":
        for p in d["probs"]:      # the magnitude companion's scale / shift are the ones plane_model._prologue applies
            a, A, y = R.prologue(p["x"], case.norm, case.act, d["gamma"], d["beta"])
            _, _, sc, sh = R.scale_shift(p["x"], R.stats_of(p["x"]), d["gamma"], d["beta"])
            y2 = p["x"] * sc.view(-1, 1, 1) + sh.view(-1, 1, 1)
            assert torch.equal(y2, y) and bool((A * (1 + 4 * R.U) >= a.abs()).all())      # (a is rounded to fp32, A is not)
            # no rounding of sh or y can change the sign of y: 4 u A' stays under |y| / 2, element by element
            Ap = R.prologue_terms(p["x"], R.stats_of(p["x"]), d["gamma"], d["beta"])
            assert bool((4 * R.U * Ap < 0.5 * y.double().abs()).all())


@pytest.mark.parametrize("case", CASES, ids=K.IDS)
def test_a_dropped_term_is_visible(case):
    """Removing any single in-bounds contribution moves at least one element by more than its bound: the bound is tight enough to see
    one missing term.  A contribution is a whole (ky, kx) tap over the tensor for forward and backward-data, and one output pixel
    (through all its taps) for backward-weight; that EVERY element sees the loss of a single product is not claimed -- one product
    can be arbitrarily small."""
    d, ref, L = K.data(case), K.reference(case), case.layer
    if case.op == "wgrad":
        best = []
        for p in d["probs"]:
            dy, a = p["dy"], R.prologue(p["x"], case.norm, case.act, d["gamma"], d["beta"])[0].abs()
            vis = torch.zeros(p["Ho"], p["Wo"], dtype=torch.float64)
            for ky, kx, i, o in L.taps(p["H"], p["W"]):
                bt = L.tap(ref["dw_bound"], ky, kx)      # [cout, cin]
                r = (dy.double().abs()[:, None, o[0], o[1]] * a[None, :, i[0], i[1]] / bt[:, :, None, None]).amax((0, 1))
                vis[o[0], o[1]] = torch.maximum(vis[o[0], o[1]], r)
            best.append(float(vis.min()))
        assert min(best) > 1.0, best
        return
    worst = {}
    for i, p in enumerate(d["probs"]):
        for ky, kx, _i, _o in L.taps(p["H"], p["W"]):
            if case.op == "fwd":
                c, bound = R.forward(L, ref[i]["a"], d["w"].double(), only=(ky, kx)), ref[i]["pre_bound"]
            else:
                c = R.dgrad(L, p["dy"].double(), d["w"].double(), p["H"], p["W"], only=(ky, kx))
                f = R.act_grad(p["x"], case.norm, case.act, d["gamma"], d["beta"])[0] if case.x else 1.0
                c, bound = c * f, ref[i]["bound"]
            worst[(i, ky, kx)] = float((c.abs() / bound.clamp_min(1e-300)).max())
    assert min(worst.values()) > 1.0, min(worst.items(), key=lambda kv: kv[1])


def test_counts_and_magnitudes_against_direct_loops():
    g = torch.Generator().manual_seed(5)
    for L, H, W in ((R.Layer("conv", 3, 2, 1, 2, 3), 5, 4), (R.Layer("convT", 3, 2, 1, 2, 3, op=1), 3, 2), (R.Layer("convT", 4, 2, 1, 3, 2), 2, 3)):
        Ho, Wo = L.out_hw(H, W)
        x, w, dy = torch.randn(L.cin, H, W, generator=g), torch.randn(*L.wshape(), generator=g), torch.randn(L.cout, Ho, Wo, generator=g)
        Mf, Lf = np.zeros((L.cout, Ho, Wo)), np.zeros((Ho, Wo))
        Md, Ld = np.zeros((L.cin, H, W)), np.zeros((H, W))
        Mw, Lw = np.zeros(L.wshape()), np.zeros((L.k, L.k))
        for oy in range(Ho):
            for ox in range(Wo):
                for iy in range(H):
                    for ix in range(W):
                        ky, kx = (oy - iy * L.s + L.p, ox - ix * L.s + L.p) if L.tr else (iy - oy * L.s + L.p, ix - ox * L.s + L.p)
                        if not (0 <= ky < L.k and 0 <= kx < L.k):
                            continue
                        Lf[oy, ox] += 4
                        Ld[iy, ix] += 4
                        Lw[ky, kx] += 1
                        for co in range(L.cout):
                            for ci in range(L.cin):
                                wv = abs(float(w[ci, co, ky, kx] if L.tr else w[co, ci, ky, kx]))
                                Mf[co, oy, ox] += abs(float(x[ci, iy, ix])) * wv
                                Md[ci, iy, ix] += abs(float(dy[co, oy, ox])) * wv
                                Mw[(ci, co, ky, kx) if L.tr else (co, ci, ky, kx)] += abs(float(x[ci, iy, ix])) * abs(float(dy[co, oy, ox]))
        assert np.array_equal(R.count_fwd(L, H, W)[0].numpy(), Lf) and np.array_equal(R.count_dgrad(L, H, W)[0].numpy(), Ld)
        assert np.array_equal(R.count_wgrad(L, H, W)[0, 0].numpy(), Lw)
        assert np.allclose(R.op_forward(L, x, w)["M"].numpy(), Mf, rtol=1e-12, atol=0)
        assert np.allclose(R.op_dgrad(L, dy, w, H, W)["M"].numpy(), Md, rtol=1e-12, atol=0)
        r = R.op_wgrad(L, [(x, dy, None, 0, None, None)])
        assert np.allclose(r["M"].numpy(), Mw, rtol=1e-12, atol=0) and np.array_equal(r["L"][0, 0].numpy(), Lw)
        assert np.allclose(r["dw_bound"].numpy(), (Lw + R.CA_WGRAD + R.C_PRO) * R.U * Mw, rtol=1e-12, atol=0)      # plain read: M_A = M_a


def test_rows_reach_the_variants_they_name():
    for c in K.FWD + K.DGRAD + [p[1] for p in K.PAIRS]:
        if c.kernel == K.C4:
            N, ck = (c.layer.cin, c.layer.cout) if c.op == "dgrad" else (c.layer.cout, c.layer.cin)
            assert R.pad4(ck) == 4 and R.pad4(N) > 16 and (c.op == "dgrad" or (c.act == 0 and not c.norm)), c
            if c.variant:
                assert K.c4_variant(c) == c.variant, (c, K.c4_variant(c))
        if c.kernel in (K.SN8, K.SN16, K.SN64):
            kt = K.ktot(c)
            assert c.kernel == (K.SN64 if kt >= 2048 else K.SN16 if kt >= 256 else K.SN8), (c, kt)
        if c.kernel == K.S4 and c.op in ("fwd", "dgrad"):
            ck = R.pad4(c.layer.cout if c.op == "dgrad" else c.layer.cin)
            assert ck % 16 == 0 and 16 <= ck <= 512 and all(t == 4 for H, W in c.sizes for _, _, t in K.phases(c, H, W))
    # the phase extents the tile seams of sg_conv_scatter4 need, in either direction
    ext = [set(), set()]
    for c in K.FWD + K.DGRAD:
        if c.kernel == K.S4:
            for H, W in c.sizes:
                for hp, wp, _ in K.phases(c, H, W):
                    ext[0].add(hp), ext[1].add(wp)
    assert all({1, 2, 6, 7, 30, 31, 61} <= e for e in ext), ext
    assert {R.pad4(c.layer.cout if c.op == "dgrad" else c.layer.cin) for c in K.FWD + K.DGRAD if c.kernel == K.S4} >= {16, 48, 512}
    assert {R.pad4(c.layer.cout) for c in K.FWD if c.kernel == K.C4 and not c.stats} >= {20, 32, 36, 48, 52, 64}
    assert sum("RB4" in (c.variant or "") for c in K.FWD + K.DGRAD) == 2
    # thin backward-weight: every problem within 4096 pixels; the split rows have an empty wave, a range that ends mid-step and
    # an M that is no multiple of 4
    for c in K.WGRAD + [p[2] for p in K.PAIRS]:
        for H, W in c.sizes:
            assert max(H * W, np.prod(c.layer.out_hw(H, W))) <= 4096, c
    for c in K.WGRAD:
        assert c.variant == "nsplit " + ",".join(str(len(wgs)) for wgs in K.thin_ranges(c)), c
    for _n, dc, wc, ok, _k, v in K.PAIRS:
        if ok:
            assert v.endswith("nsplit " + ",".join(str(len(wgs)) for wgs in K.thin_ranges(wc, want=512.0, nw=4))), (wc, v)
            assert v.startswith("DK1 RB0") if dc.kernel == K.S4 else v.startswith("DK0 " + K.c4_variant(dc).split()[1]), (dc, v)
    for c in (c for c in K.WGRAD if c.env):
        wgs = K.thin_ranges(c)[0]
        waves = [r for wg in wgs for r in wg]
        assert len(wgs) == 3 and waves[-1][1] % 4 != 0
        assert any(e <= b for b, e in waves) and any(0 < e - b and (e - b) % 4 for b, e in waves)
        covered = sorted((b, e) for b, e in waves if e > b)
        assert covered[0][0] == 0 and all(covered[i][1] == covered[i + 1][0] for i in range(len(covered) - 1))
    assert all(len(wg) == 1 for c in K.WGRAD if not c.env for wg in [K.thin_ranges(c)[0]])

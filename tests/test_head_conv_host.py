"""CPU checks of tests/head_conv_cases.py: the float64 reference of every row against torch's conv2d and autograd, an fp32
restatement inside every bound, the activation margin (both forms of the pre-activation value), the launchers restated (kernel,
variant, decline rules), the reduction lengths, and the two extensions of thin_conv_ref this table needs (second_order for the long
rows, the fp32 runs of bound_sum)."""
import math
from fractions import Fraction

import pytest
import torch
import torch.nn.functional as F

import head_conv_cases as HC
import thin_conv_cases as K
import thin_conv_ref as R
from thin_conv_ref import pad4


def _close(a, b, what):
    assert float((a.double() - b.double()).abs().max()) <= 1e-12 * (1.0 + float(b.double().abs().max())), what


def _torch_ops(L, d, norm, act, dt):
    """(y, da, dw) per problem by torch and autograd in dtype dt, from the prologue's output."""
    out = []
    for p in d["probs"]:
        a = R.prologue(p["x"], norm, act, d["gamma"], d["beta"])[0].to(dt).clone().requires_grad_(True)
        w = d["w"].to(dt).clone().requires_grad_(True)
        y = F.conv2d(a[None], w, d["b"].to(dt) if d["b"] is not None else None, stride=1, padding=L.p)[0]
        (y * p["dy"].to(dt)).sum().backward()
        out.append((y.detach(), a.grad, w.grad))
    return out


@pytest.mark.parametrize("case", HC.FWD, ids=HC.IDS)
def test_forward_reference_matches_torch_and_fp32_is_inside_the_bound(case):
    d, ref = K.data(case), HC.fwd_reference(case)
    t64, t32 = (_torch_ops(case.layer, d, case.norm, case.act, dt) for dt in (torch.float64, torch.float32))
    for i in range(len(d["probs"])):
        _close(ref[i]["pre"], t64[i][0], "forward")
        r32 = torch.tanh(t32[i][0]) if case.tanh else t32[i][0]
        assert bool(((r32.double() - ref[i]["ref"]).abs() <= ref[i]["bound"]).all())


@pytest.mark.parametrize("row", HC.ALL_BWD, ids=HC.IDS)
def test_backward_reference_matches_torch_and_fp32_is_inside_the_bound(row):
    d, (dg, wg) = HC.bwd_data(row), HC.bwd_reference(row)
    t64, t32 = (_torch_ops(row.layer, d, row.norm, row.act, dt) for dt in (torch.float64, torch.float32))
    for i, p in enumerate(d["probs"]):
        f = R.act_grad(p["x"], row.norm, row.act, d["gamma"], d["beta"])[0]
        prev = p["prev"] if p["prev"] is not None else 0.0
        _close(dg[i]["ref"], t64[i][1] * f + prev, "backward-data")
        assert bool((((t32[i][1] * f.float() + prev).double() - dg[i]["ref"]).abs() <= dg[i]["bound"]).all())
    if row.wnorm != row.norm:
        t64, t32 = (_torch_ops(row.layer, d, row.wnorm, row.act, dt) for dt in (torch.float64, torch.float32))
    groups = [[i] for i in range(len(t64))] if row.own_dw else [list(range(len(t64)))]
    for g, ref in zip(groups, wg):
        _close(ref["dw"], sum(t64[i][2] for i in g), "backward-weight")
        _close(ref["db"], sum(d["probs"][i]["dy"].double().sum((1, 2)) for i in g), "bias gradient")
        assert bool(((sum(t32[i][2] for i in g).double() - ref["dw"]).abs() <= ref["dw_bound"]).all())
        assert bool((HC.head_dw_bound(row, ref) >= ref["dw_bound"]).all())
        assert bool(((sum(d["probs"][i]["dy"].sum((1, 2)) for i in g).double() - ref["db"]).abs() <= ref["db_bound"]).all())


def test_the_head_kernels_xhat_form_is_inside_its_bound():
    """y = gamma ((x - mean) rstd) + beta against x sc + sh, in fp32: the distance the 9 of C_PRO_XHAT pays for, element by element."""
    for row in (r for r in HC.ALL_BWD if r.wnorm):
        d = HC.bwd_data(row)
        for p in d["probs"]:
            y1 = R.act_grad(p["x"], row.wnorm, 0, d["gamma"], d["beta"])[2].double()
            y2 = R.prologue(p["x"], row.wnorm, 0, d["gamma"], d["beta"])[2].double()
            Ap = R.prologue_terms(p["x"], R.stats_of(p["x"]), d["gamma"], d["beta"])
            assert bool(((y1 - y2).abs() <= 7 * R.U * Ap).all()), row


@pytest.mark.parametrize("case", HC.FWD + HC.ALL_BWD, ids=HC.IDS)
def test_mask_margin(case):
    bwd = isinstance(case, HC.Bwd)
    d = HC.bwd_data(case) if bwd else K.data(case)
    for y in (HC.bwd_signs(case, d) if bwd else K.signs(case, d)):
        assert R.margin(y) > R.MASK_MARGIN
    for norm in {case.norm, case.wnorm if bwd else case.norm} - {None}:
        if case.act:
            for p in d["probs"]:      # no rounding of either form can change the sign of y
                Ap = R.prologue_terms(p["x"], R.stats_of(p["x"]), d["gamma"], d["beta"])
                for y in (R.prologue(p["x"], norm, 0, d["gamma"], d["beta"])[2], R.act_grad(p["x"], norm, 0, d["gamma"], d["beta"])[2]):
                    assert bool((7 * R.U * Ap < 0.5 * y.double().abs()).all())


def test_rows_reach_the_kernels_and_variants_they_name():
    for c in HC.FWD:
        kernel, variant, tiles = HC.fwd_dispatch(c)
        assert (kernel, variant) == (c.kernel, c.variant), (c, kernel, variant)
        assert tiles is None or tiles >= 1
    for r in HC.ALL_BWD:
        what, v = HC.bwd_dispatch(r)
        assert what == r.expect and (what == "decline" or v == r.variant), (r, what, v)
    # every instantiation and every row-group layout
    v2 = {c.variant for c in HC.FWD if c.kernel == HC.H2}
    assert {v[:5] for v in v2} == {"K4 R2", "K4 R4", "K3 R2", "K3 R4"} and {v[-4:] for v in v2} == {"nrg1", "nrg2", "nrg4"}
    assert all({f"K4 R{r} nrg1", f"K4 R{r} nrg4", f"K3 R{r} nrg1", f"K3 R{r} nrg4"} <= v2 for r in (2, 4))
    assert {c.variant for c in HC.FWD if c.kernel == HC.HD} == {"TH2", "TH4", "TH8"}
    assert {r.layer.k for r in HC.BWD} == {3, 4}
    # head2: chunks per wave, pads, result extents
    h2 = [c for c in HC.FWD if c.kernel == HC.H2]
    assert {pad4(c.layer.cin) for c in h2 if c.layer.k == 4 and not c.env} >= {64, 96, 128, 192, 256, 320}
    assert {pad4(c.layer.cin) for c in h2 if c.layer.k == 3 and not c.env} >= {64, 160}
    assert {c.layer.p for c in h2 if c.layer.k == 4} == {0, 1, 2, 3} and {c.layer.p for c in h2 if c.layer.k == 3} == {0, 1, 2}
    outs = [c.layer.out_hw(H, W) for c in h2 for H, W in c.sizes]
    assert (1, 1) in outs and {1, 15, 16, 17, 33} <= {wo for _, wo in outs}
    assert {1, 5, 16, 17} <= {c.layer.out_hw(*c.sizes[0])[0] for c in h2 if c.env}
    assert any(c.layer.out_hw(*c.sizes[0])[0] < 2 * int(c.variant[-1]) for c in h2 if not c.env)
    # the patch kernel: Ck 32, k outside {3, 4}, pad >= k, an odd number of channel blocks, ragged tiles
    hk = [c for c in HC.FWD if c.kernel == HC.HD]
    assert {c.layer.k for c in hk} >= {2, 3, 4, 5, 7} and any(c.layer.p >= c.layer.k for c in hk) and any((pad4(c.layer.cin) // 32) % 2 for c in hk)
    assert {1, 7, 8, 9} <= {c.layer.out_hw(H, W)[1] for c in hk for H, W in c.sizes}
    assert any(c.layer.out_hw(*c.sizes[0])[0] % int(c.variant[2:]) for c in hk)
    assert {pad4(c.layer.cin) for c in hk if "SGAN_NO_HEAD2" in c.env} == {256, 512}
    # 3 and 8 (SG_MAX_PROB) problems of unequal size for each kernel
    for rows in (h2, hk, HC.BWD):
        assert {3, 8} <= {len(set(c.sizes)) for c in rows}
    # the backward kernel: masked lanes, maps, operands, lists
    B = HC.BWD
    assert {pad4(r.layer.cin) for r in B} >= {64, 96, 128, 200, 256}
    assert {(r.layer.k, r.layer.p) for r in B} == {(4, 0), (4, 1), (4, 2), (3, 0), (3, 1)}
    assert {H for r in B for H, _ in r.sizes} >= {1, 2, 7, 8, 9, 11, 17} and {W for r in B for _, W in r.sizes} >= {1, 8, 9, 15, 16, 17, 33}
    assert {(r.norm, r.act) for r in B} == {(n, a) for n in (None, "in", "bn") for a in (0, 1, 2)}
    assert {r.wt for r in B} == {True, False} and any(not r.wj for r in B) and any(not r.bias for r in B)
    assert any(r.norm and not r.stats for r in B) and any(r.rep and sum(HC.bwd_tiles(r)) > 8 for r in B)
    assert {(len(r.sizes), r.own_dw) for r in B} >= {(1, False), (3, False), (8, False), (3, True), (8, True)}
    assert [sum(HC.bwd_tiles(r)) for r in B if r.long] == [HC.MAX_TILES]
    assert sorted(sum(HC.bwd_tiles(r)) for r in HC.DECLINED if r.long) == [HC.MAX_TILES + 1, 144]
    assert {HC.bwd_dispatch(r)[1] for r in HC.DECLINED} == {"tiles", "accumulate", "lists differ"}


def test_reduction_lengths():
    """Every row stays within L_MAX, where the second-order term of the bounds is the constant 2 -- but for the long rows, whose branch
    no shorter reduction reaches: they carry second_order(L + c)."""
    rows = HC.FWD + HC.ALL_BWD
    assert {c.name for c in rows if c.long} == HC.LONG_ROWS
    assert max(HC.reduction_length(c) for c in rows if not c.long) + R.CA_WGRAD + R.C_PRO_XHAT <= R.L_MAX
    assert all(HC.reduction_length(c) > R.L_MAX for c in rows if c.long)
    # the LDS-limit decline cannot be short: 4 bytes per weight alone pass 64 KiB - (patch <= 256 pixels) only past L_MAX products
    for k in range(2, 8):
        for ck in range(32, 1025, 32):
            if k * k * ck + R.CA_FWD + R.C_PRO <= R.L_MAX:
                c = HC.Fwd("probe", None, None, HC.hd(ck, k, k // 2), [(9, 9)], env=HC.NO2)
                assert HC.fwd_dispatch(c)[0] == HC.HD, (k, ck)


def test_second_order_term_and_fp32_runs():
    u = Fraction(1, 2 ** 24)
    for n in (2, 100, R.L_MAX, 8201, 16393, 16396, 18444):
        c = R.second_order(n)
        assert (1 + u) ** n - 1 <= (n + c) * u, n                      # exact rational arithmetic
        assert (1 + u) ** n - 1 > (n + c - 2) * u or c <= 1, n         # and not loose by more than the ceiling
    assert R.second_order(R.L_MAX) <= 2 and R.second_order(8201) == 3 and R.second_order(16393) == 9
    # long=False is the formula as it was; long=True adds (second_order - 2) u on the larger magnitude
    M, MA = torch.tensor([3.0]), torch.tensor([5.0])
    Lc = torch.tensor([16384.0])
    base = (Lc + 1) * R.U * M + 8 * R.U * MA
    assert torch.equal(R._bound(Lc, 1, M, 8, MA, long=True), base + (R.second_order(16393) - 2) * R.U * MA)
    assert torch.equal(R._bound(Lc, 4, M, long=True), (Lc + 4) * R.U * M + (R.second_order(16388) - 2) * R.U * M)
    assert torch.equal(R._bound(torch.tensor([100.0]), 1, M, 8, MA, long=True), R._bound(torch.tensor([100.0]), 1, M, 8, MA))
    with pytest.raises(AssertionError):
        R._bound(Lc, 1, M, 8, MA)
    # runs of 8 fp32 additions before the fp64 sum: summing in fp32 by rows of 8 stays inside bound_sum(run=8) with exact elements
    g = torch.Generator().manual_seed(3)
    v = torch.randn(5, 6, 8, generator=g)
    xh = torch.randn(5, 6, 8, generator=g)
    zero = torch.zeros(5, 6, 8, dtype=torch.float64)

    def runs(t):
        acc = torch.zeros(5, 6)
        for i in range(8):
            acc = acc + t[..., i]
        return acc.double().sum(1)
    assert bool(((runs(v) - v.double().sum((1, 2))).abs() <= R.bound_sum(v.double(), zero, run=8)).all())
    assert bool(((runs(v * xh) - (v.double() * xh.double()).sum((1, 2))).abs() <= R.bound_sum(v.double(), zero, xh.double(), run=8)).all())
    assert math.isclose(float(R.bound_sum(v.double(), zero, run=8)[0] / v.double().abs().sum((1, 2))[0]), 7 * R.U + 48 * 2.0 ** -53, rel_tol=1e-9)
    assert torch.equal(R.bound_sum(v.double(), zero + 1e-9, run=1), R.bound_sum(v.double(), zero + 1e-9))

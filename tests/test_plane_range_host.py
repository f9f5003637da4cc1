"""The operand domain of the 16-bit plane conv modes, from the CPU model of their documented arithmetic (plane_model.py): no GPU.

The layer is shape A of test_hip_plane_range.py (conv k4 s1 p2, 32 -> 64 on 17 x 19, LeakyReLU on load, no norm) with the suite's
operand distributions times 2^e; the error is max-norm relative to fp64 of the unrounded operands (forward without its bias, which
does not scale with the operands and would hide the rounding).  The sweeps print their table and pin the edges that
include/sgan_hip.h and DESIGN.md R2.1 state: every low edge is the smallest maximum magnitude from which all larger ones pass,
moved inwards by one power of two and rounded inwards to a power of two; the high edges are fp16's largest finite value."""
import math

import numpy as np
import pytest
import torch

import plane_model as pm

KIND, K, S, P, CIN, COUT, H, W, NORM, ACT = pm.A_SHAPE


def _act(x):
    return pm._prologue(x, None, None, None, None, ACT, H * W)


@pytest.fixture(scope="module")
def base():
    x, w, b, dy = pm.shape_a_operands()
    return x, w, dy


def _edge(rows, col, gate):
    """rows: (e, log2 of the operand's maximum, errors...) by ascending e.  The documented low edge, as a power of two: the first e
    from which every finite row passes, one step inwards, the maximum there rounded up to a power of two."""
    ok = None
    for i in range(len(rows) - 1, -1, -1):
        if not (rows[i][col] < gate):
            break
        ok = i
    assert ok is not None and 0 < ok < len(rows) - 1, "the sweep does not bracket the edge"
    return math.ceil(rows[ok + 1][1] - 1e-9)


def _print(title, head, rows, keep):
    print("\n" + title)
    print("  " + "  ".join(f"{h:>14s}" for h in head))
    for r in rows:
        if r[0] in keep:
            print("  " + "  ".join(f"{v:14.3g}" if isinstance(v, float) else f"{v:14d}" for v in r))


def test_activation_scale_sweep(base):
    """x * 2^e: forward (fp16 planes of the unscaled prologue output) and backward-weight, published (fp16) and not (bf16)."""
    x, w, dy = base
    wshape, am = tuple(w.shape), float(dy.abs().max())
    rows = []
    for e in range(-26, 16):
        a = _act(pm.pow2(x, e))
        t, tw = pm.truth_fwd(False, a, w, None, S, P), pm.truth_wgrad(False, a, dy, wshape, S, P)
        r = [e, math.log2(float(a.abs().max()))]
        for m in pm.MODES:
            r += [pm.rel_max(pm.model_fwd(m, False, a, w, None, S, P), t),
                  pm.rel_max(pm.model_wgrad(m, False, a, dy, wshape, S, P, am), tw),
                  pm.rel_max(pm.model_wgrad(m, False, a, dy, wshape, S, P, None), tw)]
        rows.append(r)
    _print("activation x * 2^e (model, max-norm relative to fp64)",
           ["e", "log2 max|a|", "x3 fwd", "x3 wgrad f16", "x3 wgrad bf16", "x1 fwd", "x1 wgrad f16", "x1 wgrad bf16"], rows,
           (-24, -20, -16, -12, -8, -4, 0, 8, 13, 14))
    finite = [r for r in rows if r[0] <= 13]
    # fp16 overflow: e = 13 (max 49.6e3) is the last finite scale; the bf16-plane backward-weight does not care
    assert all(math.isfinite(v) for r in finite for v in r) and all(not math.isfinite(r[2]) and not math.isfinite(r[5]) for r in rows if r[0] >= 14)
    assert all(math.isfinite(r[4]) and math.isfinite(r[7]) for r in rows)
    lo_contract = max(_edge(finite, c, pm.CONTRACT) for c in (2, 3, 5, 6))       # both modes, both fp16-plane paths
    lo_fp32 = max(_edge(finite, c, pm.FP32_EQUIV) for c in (2, 3))               # bf16x3 on fp16 planes
    print(f"documented: 1e-3 contract from max|a| = 2^{lo_contract}, fp32-equivalent from 2^{lo_fp32}, up to {pm.ACT_OVERFLOW:g}")
    assert pm.ACT_CONTRACT == (2.0 ** lo_contract, pm.ACT_OVERFLOW) and pm.ACT_FP32 == (2.0 ** lo_fp32, pm.ACT_OVERFLOW)
    for r in finite:
        amax = 2.0 ** r[1]
        if pm.inside(pm.ACT_CONTRACT, amax):
            assert max(r[2], r[3], r[5], r[6]) < pm.CONTRACT, r
        if pm.inside(pm.ACT_FP32, amax):
            assert max(r[2], r[3]) < pm.FP32_EQUIV, r
        # bf16 planes carry the fp32 exponent: the same error at every scale; the one-plane mode on them is never inside 1e-3
        assert r[4] < 1e-5 and pm.CONTRACT < r[7] < 4e-3, r
    # the domain is not stated wider than it is: three powers of two under an edge the gate is missed
    assert all(r[2] > pm.CONTRACT for r in finite if 2.0 ** r[1] < pm.ACT_CONTRACT[0] / 8)
    assert all(r[2] > pm.FP32_EQUIV for r in finite if 2.0 ** r[1] < pm.ACT_FP32[0] / 8)


def test_activation_overflow_edge():
    """65504 is the last magnitude whose hi plane is finite (65520 rounds to infinity)."""
    hi, lo = pm.split_f16(torch.tensor([65504.0, 65519.0, 65520.0, -65520.0]))
    assert hi[0] == 65504.0 and lo[0] == 0 and hi[1] == 65504.0 and lo[1] == 15.0
    assert torch.isinf(hi[2:]).all()


def test_weight_scale_sweep(base):
    """max|w| = 2^e: forward and published backward-data (fp16 planes of w * 2^10), unpublished backward-data (bf16 planes)."""
    x, w, dy = base
    a, am, w1 = _act(x), float(dy.abs().max()), w / w.abs().max()
    rows = []
    for e in range(-28, 8):
        ws = pm.pow2(w1, e)
        t, td = pm.truth_fwd(False, a, ws, None, S, P), pm.truth_dgrad(False, dy, ws, S, P, x.shape)
        r = [e, float(e)]
        for m in pm.MODES:
            r += [pm.rel_max(pm.model_fwd(m, False, a, ws, None, S, P), t),
                  pm.rel_max(pm.model_dgrad(m, False, dy, ws, S, P, x.shape, am), td),
                  pm.rel_max(pm.model_dgrad(m, False, dy, ws, S, P, x.shape, None), td)]
        rows.append(r)
    _print("weights, max|w| = 2^e (model, max-norm relative to fp64)",
           ["e", "log2 max|w|", "x3 fwd", "x3 dgrad f16", "x3 dgrad bf16", "x1 fwd", "x1 dgrad f16", "x1 dgrad bf16"], rows,
           (-28, -24, -22, -20, -16, -12, -10, 0, 5, 6))
    finite = [r for r in rows if r[0] <= 5]
    assert all(math.isfinite(v) for r in finite for v in r) and all(not math.isfinite(r[2]) for r in rows if r[0] >= 6)      # |w| < 64
    lo_contract = max(_edge(finite, c, pm.CONTRACT) for c in (2, 3, 5, 6))
    lo_fp32 = max(_edge(finite, c, pm.FP32_EQUIV) for c in (2, 3))
    print(f"documented: 1e-3 contract from max|w| = 2^{lo_contract}, fp32-equivalent from 2^{lo_fp32}, |w| < {pm.W_OVERFLOW:g}")
    assert pm.W_CONTRACT == (2.0 ** lo_contract, 2.0 ** 5) and pm.W_FP32 == (2.0 ** lo_fp32, 2.0 ** 5)
    for r in finite:
        if pm.inside(pm.W_CONTRACT, 2.0 ** r[0]):
            assert max(r[2], r[3], r[5], r[6]) < pm.CONTRACT, r
        if pm.inside(pm.W_FP32, 2.0 ** r[0]):
            assert max(r[2], r[3]) < pm.FP32_EQUIV, r
        assert r[4] < 1e-5 and pm.CONTRACT < r[7] < 4e-3, r
    assert all(r[2] > pm.CONTRACT for r in finite if 2.0 ** r[0] < pm.W_CONTRACT[0] / 8)
    hi, _ = pm.split_f16(torch.tensor([63.96875, 64.0]), pm.W_SHIFT)      # 65504 / 2^10 and the first weight that overflows
    assert hi[0] == 63.96875 and torch.isinf(hi[1])


def test_gradient_scale_sweep(base):
    """dY * 2^e: backward-data and backward-weight, published (fp16 planes of dY * 2^s, s clamped to +-100) and not (bf16 planes)."""
    x, w, dy = base
    a, wshape = _act(x), tuple(w.shape)
    rows = []
    for e in list(range(-126, -94)) + [-60, -30, 0, 30, 60] + list(range(94, 126)):
        d = pm.pow2(dy, e)
        am = float(d.abs().max())
        td, tw = pm.truth_dgrad(False, d, w, S, P, x.shape), pm.truth_wgrad(False, a, d, wshape, S, P)
        r = [e, math.log2(am)]
        for m in pm.MODES:
            r += [pm.rel_max(pm.model_dgrad(m, False, d, w, S, P, x.shape, am), td),
                  pm.rel_max(pm.model_dgrad(m, False, d, w, S, P, x.shape, None), td),
                  pm.rel_max(pm.model_wgrad(m, False, a, d, wshape, S, P, am), tw),
                  pm.rel_max(pm.model_wgrad(m, False, a, d, wshape, S, P, None), tw)]
        rows.append(r)
    _print("gradient dY * 2^e (model, max-norm relative to fp64)",
           ["e", "log2 max|dY|", "x3 dgrad f16", "x3 dgrad bf16", "x3 wgrad f16", "x3 wgrad bf16", "x1 dgrad f16", "x1 dgrad bf16",
            "x1 wgrad f16", "x1 wgrad bf16"], rows, (-120, -115, -110, -105, -100, -30, 0, 30, 100, 110, 114, 115, 120))
    finite = [r for r in rows if 2.0 ** r[1] <= pm.G_CONTRACT[1]]
    assert all(math.isfinite(v) for r in finite for v in r)
    # above 65504 * 2^100 the clamp of s lets the hi plane of dY * 2^s overflow; the bf16 planes do not care (the model accumulates
    # in fp64: the kernels' fp32 accumulator sets its own limit on the RESULT, which is the layer's business)
    assert all(not math.isfinite(r[2]) for r in rows if 2.0 ** r[1] > 65504.0 * 2.0 ** 100)
    assert all(math.isfinite(r[3]) and math.isfinite(r[5]) for r in rows)
    lo_contract = max(_edge(finite, c, pm.CONTRACT) for c in (2, 3, 4, 5, 6, 8))
    lo_fp32 = max(_edge(finite, c, pm.FP32_EQUIV) for c in (2, 4))
    print(f"documented: 1e-3 contract from max|dY| = 2^{lo_contract}, fp32-equivalent (published) from 2^{lo_fp32}, up to 2^115")
    assert pm.G_CONTRACT == (2.0 ** lo_contract, 2.0 ** 115) and pm.G_FP32 == (2.0 ** lo_fp32, 2.0 ** 115)
    for r in finite:
        if pm.inside(pm.G_CONTRACT, 2.0 ** r[1]):
            assert max(r[2], r[3], r[4], r[5], r[6], r[8]) < pm.CONTRACT, r
            assert max(r[3], r[5]) < 1e-5 and pm.CONTRACT < min(r[7], r[9]) and max(r[7], r[9]) < 4e-3, r
        if pm.inside(pm.G_FP32, 2.0 ** r[1]):
            assert max(r[2], r[4]) < pm.FP32_EQUIV, r
    assert all(r[2] > pm.CONTRACT for r in rows if 2.0 ** r[1] < pm.G_CONTRACT[0] / 8)


def test_shift_matches_its_statement():
    """sg_f16_shift (the test suite's _shift) against "amax * 2^s in [2^14, 2^15)", clamped to +-100, 0 for zero / denormal maxima."""
    f32 = np.float32
    cases = []
    for k in (-126, -30, 0, 15, 100):
        cases += [f32(2.0 ** k), np.nextafter(f32(2.0 ** k), f32(0))]
    cases += [f32(0), f32(1e-45), f32(1e-40), f32(np.inf)]
    want = {2.0 ** -126: 100, 2.0 ** -30: 44, 1.0: 14, 2.0 ** 15: -1, 2.0 ** 100: -86, 0.0: 0, float("inf"): -100}
    for a in cases:
        s = pm._shift(a)
        assert s == pm.shift_restated(a), (a, s, pm.shift_restated(a))
        if float(a) in want:
            assert s == want[float(a)], (a, s)
        if 2.0 ** -86 <= float(a) < 2.0 ** 115:      # where the clamp is idle
            assert 2.0 ** 14 <= float(a) * 2.0 ** s < 2.0 ** 15, (a, s)
    assert pm._shift(np.nextafter(f32(1), f32(0))) == 15 and pm._shift(np.nextafter(f32(2.0 ** -126), f32(0))) == 0

"""tests/resample_ref.py held to torch on the CPU, in float64: the reference the GPU parity tests (tests/test_hip_resample.py,
tests/test_hip_resample_gauss.py) compare the kernels with must be right on its own.  Gaussian against F.conv2d(groups=C) with the
case's own per-channel taps, bilinear against F.interpolate(align_corners=False), pyramid against F.avg_pool2d; every adjoint
against torch.autograd.grad and against <A x, r> == <x, A^T r>; the float32 restatement (the yardstick) against every a-priori bound
the GPU tests impose, in two summation orders; and the refusals that are decided before any HIP call.  Run with -s for the figures.

Largest ratio of |float32 restatement - float64| to the bound, over all cases and both orders (the reference alone, no kernel):
    Gaussian forward  (k k + 1) u T   0.29      Gaussian backward  (n + 2) u T    0.45
    bilinear forward  8 u T           0.34      bilinear backward  20 u T         0.11
    pyramid forward   3 (s + 1) u T   0.58 hierarchical, 0.78 flat               pyramid backward  8 u T   0.48
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resample_cases as K
import resample_ref as R

ULPS = 64 * 2.0 ** -53          # "a few ulps of float64" relative to sum |terms|: torch sums in another order


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64))).permute(2, 0, 1).unsqueeze(0).contiguous()


def _nhwc(t):
    return t.detach()[0].permute(1, 2, 0).numpy()


def _close(got, want, T, what):
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    assert (err <= ULPS * T + 1e-300).all(), f"{what}: {float((err / np.maximum(T, 1e-300)).max()):.3e} of sum |terms|"


def _ratio(a32, ref64, bound):
    assert a32.dtype == np.float32
    r = np.abs(a32.astype(np.float64) - ref64) / np.maximum(bound, 1e-300)
    return float(r.max())


def _adjoint(Ax, r, x, ATr, what):
    lhs, rhs = float((Ax * r).sum()), float((x * ATr).sum())
    scale = float((np.abs(Ax) * np.abs(r)).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(scale, 1e-300), f"{what}: <A x, r> = {lhs!r}, <x, A^T r> = {rhs!r}"


WORST = {}


def _note(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert ratio <= 1.0, f"{key}: the float32 restatement is at {ratio:.3f} of the bound"


# ---- Gaussian ------------------------------------------------------------------------------------------------------------------------
GAUSS_ALL = K.GAUSS + [K.GAUSS_GRID, K.GAUSS_GRID_MULTI_FWD] + [j for m in K.MULTI for j in m.jobs]


@pytest.mark.parametrize("case", GAUSS_ALL, ids=[f"{i}-{c.name}" for i, c in enumerate(GAUSS_ALL)])
def test_gauss_reference(case):
    k, pad, s, Cr = case.k, case.pad, case.s, case.Creal
    x, g = case.x[..., :Cr], case.R[..., :Cr]
    assert not np.array_equal(case.taps, case.taps.transpose(0, 2, 1)) and not np.array_equal(case.taps, case.taps[:, ::-1])
    assert not np.array_equal(case.taps, case.taps[:, :, ::-1]) and (Cr == 1 or not np.array_equal(case.taps[0], case.taps[1]))
    ref, T = R.gauss_down(x, case.taps, k, pad, s), R.gauss_down_terms(x, case.taps, k, pad, s)
    assert ref.shape == (case.Ho, case.Wo, Cr)
    xt = _nchw(x).requires_grad_(True)
    y = F.conv2d(xt, torch.from_numpy(case.taps.astype(np.float64)).unsqueeze(1), padding=pad, groups=Cr)[:, :, ::s, ::s]
    assert tuple(y.shape[2:]) == (case.Ho, case.Wo)
    _close(_nhwc(y), ref, T, "gauss_down")
    base = case.base[..., :Cr] if case.acc and case.base is not None else None
    adj = R.gauss_down_adj(g, case.taps, k, pad, s, case.H, case.W, base)
    Ta = R.gauss_down_adj_terms(g, case.taps, k, pad, s, case.H, case.W, base)
    gx, = torch.autograd.grad(y, xt, _nchw(g))
    _close(_nhwc(gx) + (0.0 if base is None else base.astype(np.float64)), adj, Ta, "gauss_down_adj")
    plain = R.gauss_down_adj(g, case.taps, k, pad, s, case.H, case.W)
    _adjoint(ref, g.astype(np.float64), x.astype(np.float64), plain, "gauss")
    if pad == 0:      # rows / columns beyond the last window: no output reads them
        hr, wr = s * (case.Ho - 1) + k, s * (case.Wo - 1) + k
        assert (hr < case.H or wr < case.W) and not plain[hr:].any() and not plain[:, wr:].any()      # 37 x 41: a column; 20 x 20: both
        assert (case.H, case.W) != (20, 20) or (hr < case.H and wr < case.W)
    if case.grid:
        return
    for rev in (False, True):
        _note("gauss fwd", _ratio(R.gauss_down(x, case.taps, k, pad, s, np.float32, rev), ref, R.bound_gauss_fwd(k, T)))
        _note("gauss bwd", _ratio(R.gauss_down_adj(g, case.taps, k, pad, s, case.H, case.W, base, np.float32, rev), adj,
                                  R.bound_gauss_bwd([(k, s)], Ta, base is not None)))


def test_gauss_case_table_reaches_its_edges():
    """What the issue names: image smaller than the padding with Ho = 1, H and W no multiples of s, s odd, k > 9, C > 4, the channel
    cross, both tap layouts, both buffer layouts, accumulate on and off; a multi-job set of every size 1 .. 5."""
    assert any(c.H <= c.pad and c.Ho == 1 for c in K.GAUSS) and any(c.H % c.s and c.W % c.s for c in K.GAUSS)
    assert any(c.s % 2 for c in K.GAUSS) and any(c.k > 9 for c in K.GAUSS_MULTI_OK) and any(c.k % 2 == 0 for c in K.GAUSS)
    assert {(c.C, c.Creal) for c in K.GAUSS} == set(K.CHANS.values())
    assert {(c.k, c.pad, c.s) for c in K.GAUSS} == set(K.GEOMS.values())
    for geom in K.GEOMS.values():
        mine = [c for c in K.GAUSS if (c.k, c.pad, c.s) == geom]
        assert {c.dense for c in mine} == {False, True} and {c.acc for c in mine} == {False, True}, geom
    assert {c.sliced for c in K.GAUSS} == {False, True}
    assert sorted({len(m.jobs) for m in K.MULTI}) == [1, 2, 3, 4, 5]
    for m in K.MULTI:
        assert len({(j.k, j.pad, j.s) for j in m.jobs}) == len(m.jobs) and all(j.k <= 3 * j.s for j in m.jobs)
    w, gcs = K.dense_weight(K.GAUSS[1].taps)
    assert np.isnan(w).sum() == w.size - K.GAUSS[1].taps.size and gcs == (K.GAUSS[1].Creal + 1) * K.GAUSS[1].k ** 2
    # the grid cases are just past cap * 256 work items
    assert K.GAUSS_GRID.Ho * K.GAUSS_GRID.Wo * 256 > 4096 * 256 >= (K.GAUSS_GRID.Ho - 1) * K.GAUSS_GRID.Wo * 256
    assert K.GAUSS_GRID_MULTI_FWD.Ho * K.GAUSS_GRID_MULTI_FWD.Wo * 256 > 2048 * 256 >= (K.GAUSS_GRID_MULTI_FWD.Ho - 1) * 65 * 256
    assert K.BIL_GRID_FWD.H * K.BIL_GRID_FWD.W * 4 * 256 > 2048 * 1024 >= (K.BIL_GRID_FWD.H - 1) * 65 * 4 * 256
    assert K.BIL_GRID_BWD.H * K.BIL_GRID_BWD.W * 256 > 4096 * 256 >= (K.BIL_GRID_BWD.H - 1) * 65 * 256
    assert K.PYR_GRID_BWD.H * K.PYR_GRID_BWD.W > 4096 * 256 >= K.PYR_GRID_BWD.H * (K.PYR_GRID_BWD.W - 64)


@pytest.mark.parametrize("m", K.MULTI, ids=[m.name for m in K.MULTI])
def test_gauss_multi_sum_of_adjoints(m):
    """The multi backward is the sum of the jobs' adjoints (plus the base): the restatement in job order stays inside its bound."""
    Cr = m.Creal
    for base in (None, m.base[..., :Cr]):
        ref = sum(R.gauss_down_adj(j.R[..., :Cr], j.taps, j.k, j.pad, j.s, m.H, m.W) for j in m.jobs)
        T = sum(R.gauss_down_adj_terms(j.R[..., :Cr], j.taps, j.k, j.pad, j.s, m.H, m.W) for j in m.jobs)
        a32 = np.zeros_like(ref, dtype=np.float32) if base is None else base.copy()
        if base is not None:
            ref, T = ref + base.astype(np.float64), T + np.abs(base.astype(np.float64))
        for j in m.jobs:
            a32 = a32 + R.gauss_down_adj(j.R[..., :Cr], j.taps, j.k, j.pad, j.s, m.H, m.W, out_dtype=np.float32)
        _note("gauss bwd", _ratio(a32, ref, R.bound_gauss_bwd([(j.k, j.s) for j in m.jobs], T, base is not None)))


# ---- bilinear ------------------------------------------------------------------------------------------------------------------------
BIL_ALL = K.BIL_BWD + [K.BIL_GRID_FWD, K.BIL_GRID_BWD]


@pytest.mark.parametrize("case", BIL_ALL, ids=[c.name for c in BIL_ALL])
def test_bilinear_reference(case):
    ref, T = R.bilinear_up2(case.x), R.bilinear_up2_terms(case.x)
    xt = _nchw(case.x).requires_grad_(True)
    y = F.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=False)
    _close(_nhwc(y), ref, T, "bilinear_up2")
    adj, Ta = R.bilinear_up2_adj(case.R), R.bilinear_up2_adj_terms(case.R)
    gx, = torch.autograd.grad(y, xt, _nchw(case.R))
    _close(_nhwc(gx), adj, Ta, "bilinear_up2_adj")
    _adjoint(ref, case.R.astype(np.float64), case.x.astype(np.float64), adj, "bilinear")
    if case.grid:
        return
    for rev in (False, True):
        _note("bilinear fwd", _ratio(R.bilinear_up2(case.x, np.float32, rev), ref, R.bound_bilinear_fwd(T)))
        _note("bilinear bwd", _ratio(R.bilinear_up2_adj(case.R, np.float32, rev), adj, R.bound_bilinear_bwd(Ta)))


def test_bilinear_case_table_reaches_its_edges():
    assert {(c.H, c.W) for c in K.BIL if c.C != 1024} == {(1, 1), (1, 5), (6, 1), (2, 3), (5, 7)}
    for hw in ((1, 1), (1, 5), (6, 1), (2, 3), (5, 7)):
        assert {c.C for c in K.BIL if (c.H, c.W) == hw} == {4, 8, 64}
    assert any(c.C == 1024 and (c.H, c.W) == (2, 2) for c in K.BIL) and any(c.C == 12 for c in K.BIL_BWD)
    assert {c.stats for c in K.BIL} == {"none", "plain", "sliced"} and {c.sliced for c in K.BIL} == {False, True}
    assert all(np.abs(c.stats0).min() > 0 for c in K.BIL if c.stats0 is not None)


# ---- pyramid -------------------------------------------------------------------------------------------------------------------------
PYR_ALL = K.PYR + [K.PYR_GRID_BWD]


@pytest.mark.parametrize("case", PYR_ALL, ids=[c.name for c in PYR_ALL])
def test_pyramid_reference(case):
    H, W = case.H, case.W
    ref, T = R.avgpool_pyramid(case.x), R.avgpool_pyramid_terms(case.x)
    xt = _nchw(case.x).requires_grad_(True)
    ys = [F.avg_pool2d(xt, 2 << s) for s in range(R.LEVELS)]
    for s in range(R.LEVELS):
        assert ref[s].shape == (H >> (s + 1), W >> (s + 1), 4)
        _close(_nhwc(ys[s]), ref[s], T[s], f"pyramid level {s}")
    x64 = case.x.astype(np.float64)
    for name, (present, acc) in K.PYR_BWD.items():
        dl = K.pyr_levels(case, present)
        base = case.base if acc else None
        adj, Ta = R.avgpool_pyramid_adj(dl, H, W, base), R.avgpool_pyramid_adj_terms(dl, H, W, base)
        gx, = torch.autograd.grad([ys[s] for s in present], xt, [_nchw(case.dl[s]) for s in present], retain_graph=True)
        _close(_nhwc(gx) + (0.0 if base is None else base.astype(np.float64)), adj, Ta, f"pyramid adjoint {name}")
        plain = R.avgpool_pyramid_adj(dl, H, W)
        lhs = sum(float((ref[s] * case.dl[s].astype(np.float64)).sum()) for s in present)
        scale = sum(float((np.abs(ref[s]) * np.abs(case.dl[s].astype(np.float64))).sum()) for s in present)
        assert abs(lhs - float((x64 * plain).sum())) <= 1e-12 * scale
        if not case.grid:
            for rev in (False, True):
                _note("pyramid bwd", _ratio(R.avgpool_pyramid_adj(dl, H, W, base, np.float32, rev), adj, R.bound_pyramid_bwd(Ta)))
    if case.grid:
        return
    for flat in (False, True):
        a32 = R.avgpool_pyramid(case.x, np.float32, flat)
        for s in range(R.LEVELS):
            _note("pyramid fwd " + ("flat" if flat else "hierarchical"), _ratio(a32[s], ref[s], R.bound_pyramid_fwd(s, T[s])))
    if case.onehot:      # every level is a multiple of 4^-(s+1) in [0, 1]: representable, and every order of the float32 sum is exact
        for s in range(R.LEVELS):
            q = ref[s] * 4.0 ** (s + 1)
            assert np.array_equal(q, np.round(q)) and np.array_equal(ref[s].astype(np.float32).astype(np.float64), ref[s])
            assert all(np.array_equal(R.avgpool_pyramid(case.x, np.float32, f)[s], ref[s].astype(np.float32)) for f in (False, True))


def test_pyramid_case_table_reaches_its_edges():
    assert {(c.H, c.W) for c in K.PYR} == {(64, 64), (64, 128), (128, 64)}
    for hw in ((64, 64), (64, 128), (128, 64)):
        assert {(c.sliced, c.onehot) for c in K.PYR if (c.H, c.W) == hw} in ({(False, False), (True, True)}, {(True, False), (False, True)})
    assert {(c.sliced, c.onehot) for c in K.PYR} == {(False, False), (True, True), (True, False), (False, True)}
    assert len(set(K.LEVEL_LD)) >= 4 and all(o + 4 <= ld for o, ld in zip(K.LEVEL_OFF, K.LEVEL_LD))
    assert K.PYR_BWD["only5-acc"] == ((5,), True)


def test_worst_ratios_are_reported():
    """Runs after the parametrised tests of this module (file order): prints what the docstring records."""
    for key in sorted(WORST):
        print(f"{key}: float32 restatement at most {WORST[key]:.3f} of the bound")


# ---- refusals that are decided before any HIP call -------------------------------------------------------------------------------------
def test_gauss_fwd_refuses_an_index_past_31_bits(built_lib):
    """Ho Wo C/4 >= 2^31: SGAN_ERR_UNSUPPORTED, `too large` -- the 32-bit index of sg_gauss_fwd_kernel is host-checked, as its
    comment says.  The pointers are never dereferenced on the host and nothing is launched."""
    from supervised_gan_amd import _lib
    l = _lib.lib()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    H, W, C = 46341, 46341, 4          # k = 1, pad = 0, s = 1: Ho Wo = 46341^2 = 2147488281 >= 2^31, every int32 argument in range
    assert H * W * (C >> 2) >= 2 ** 31 and H * W < 2 ** 32
    rc = l.sgan_gauss_down_fwd(p, C, H, W, C, C, p, 1, 1, 0, 1, p, C, H, W, None)
    assert rc == -2 and b"too large" in l.sgan_last_error()
    # the multi-job path always refused it
    job = _lib.GaussJob(p.value, C, H, W, p.value, C, H, W, p.value, 1, 1, 0, 1)
    assert l.sgan_gauss_down_multi_fwd((_lib.GaussJob * 1)(job), 1, C, C, None) == -2 and b"too large" in l.sgan_last_error()


def test_wrappers_refuse_mismatched_shapes_before_any_pointer_is_taken(built_lib):
    from supervised_gan_amd import ops
    from supervised_gan_amd._lib import SganError
    z = lambda *s, **kw: torch.zeros(*s, **kw)
    for call, word in (
            (lambda: ops.bilinear_up2_fwd(z(3, 5, 8), z(6, 9, 8)), "6x10"),                     # out too narrow
            (lambda: ops.bilinear_up2_fwd(z(3, 5, 8), z(10, 6, 8)), "6x10"),                    # out transposed: same pixel count
            (lambda: ops.bilinear_up2_fwd(z(3, 5, 8), z(6, 10, 4)), "6x10x8"),                  # too few channels
            (lambda: ops.bilinear_up2_fwd(z(3, 5, 8), z(6, 10, 16)[..., ::2]), None),           # channel stride 2
            (lambda: ops.bilinear_up2_bwd(z(6, 9, 8), z(3, 5, 8)), "6x10"),
            (lambda: ops.bilinear_up2_bwd(z(6, 10, 4), z(3, 5, 8)), "6x10x8"),
    ):
        with pytest.raises((SganError, AssertionError)) as e:
            call()
        assert word is None or (isinstance(e.value, SganError) and word in str(e.value)), str(e.value)
    H, W = 64, 128
    good = lambda: [z(H >> (s + 1), W >> (s + 1), 4) for s in range(6)]

    def bad(s, t):
        lv = good()
        lv[s] = t
        return lv
    wrong = [bad(0, z(32, 32, 4)), bad(5, z(2, 1, 4)), bad(3, z(4, 8, 3)), bad(2, z(8, 16, 4, dtype=torch.float64)),
             bad(1, z(16, 32, 8)[..., ::2]), good()[:5]]
    for lv in wrong:
        with pytest.raises(SganError, match="nothing was launched"):
            ops.avgpool_pyramid_fwd(z(H, W, 4), lv)
        with pytest.raises(SganError, match="nothing was launched"):
            ops.avgpool_pyramid_bwd(lv, z(H, W, 4))
    with pytest.raises(SganError, match="nothing was launched"):
        ops.avgpool_pyramid_bwd([None] * 5 + [z(1, 1, 4)], z(H, W, 4), accumulate=True)      # level 5 of 64 x 128 is 1 x 2
    with pytest.raises(SganError, match="all six"):
        ops.avgpool_pyramid_fwd(z(H, W, 4), bad(2, None))

"""tests/pad_norm_ref.py held to torch on the CPU, in float64: the reference the GPU parity tests (tests/test_hip_pad_reflect.py,
tests/test_hip_norm_bwd.py) compare the kernels with must be right on its own.  Forward against F.pad(mode="reflect") of
mask * act(norm(x)); backward against torch.autograd.grad; the fold against a brute-force count; the float32 restatement (the
yardstick) against the float64 reference on every case of the shared table.  Run with -s for the figures."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pad_norm_cases as K
import pad_norm_ref as R

EPS, SLOPE = K.EPS, K.SLOPE


def _nchw(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).permute(2, 0, 1).unsqueeze(0).contiguous()


def _nhwc(t):
    return t.detach()[0].permute(1, 2, 0).numpy()


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-300))


def _torch_fwd(x, norm, act, gamma, beta, mask, pad):
    """pad(mask * act(norm(x))) in torch float64 on NCHW tensors."""
    y = x
    if norm == "in":
        y = F.instance_norm(x, eps=EPS)
    elif norm == "bn":
        y = F.batch_norm(x, None, None, gamma, beta, training=True, eps=EPS)
    if act == "relu":
        y = F.relu(y)
    elif act == "lrelu":
        y = F.leaky_relu(y, SLOPE)
    if mask is not None:
        y = y * mask
    return F.pad(y, (pad, pad, pad, pad), mode="reflect") if pad else y


def _small(norm, act, mask, H=7, W=9, C=6, pad=3, seed=0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((H, W, C)) * 1.5 + 0.3).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32) if norm == "bn" else None
    beta = (rng.standard_normal(C) * 0.3).astype(np.float32) if norm == "bn" else None
    m = (rng.integers(0, 2, (H, W, C)) * 2).astype(np.float32) if mask else None
    Rr = rng.standard_normal((H + 2 * pad, W + 2 * pad, C)).astype(np.float32)
    stats = R.stats_of(x) if norm != "none" else None
    return x, gamma, beta, m, Rr, stats


COMBOS = [(n, a, m) for n in ("none", "in", "bn") for a in ("none", "relu", "lrelu") for m in (False, True)]


@pytest.mark.parametrize("norm,act,mask", COMBOS)
@pytest.mark.parametrize("H,W,pad", [(7, 9, 3), (3, 4, 1), (5, 7, 0)])
def test_forward_is_reflection_pad_of_masked_activation(norm, act, mask, H, W, pad):
    x, gamma, beta, m, _, stats = _small(norm, act, mask, H, W, 6, pad)
    out = R.pad_reflect_fwd(x, pad, stats, gamma, beta, H * W, EPS, act, SLOPE, m)
    ref = _torch_fwd(_nchw(x), norm, act, None if gamma is None else torch.from_numpy(gamma).double(),
                     None if beta is None else torch.from_numpy(beta).double(), None if m is None else _nchw(m), pad)
    assert out.dtype == np.float64 and out.shape == (H + 2 * pad, W + 2 * pad, 6)
    assert _rel(out, _nhwc(ref)) < 1e-12


@pytest.mark.parametrize("norm,act,mask", [c for c in COMBOS if c[0] != "none"])
@pytest.mark.parametrize("H,W,pad", [(7, 9, 3), (3, 4, 1), (5, 7, 0)])
def test_backward_with_norm_backward_is_autograd(norm, act, mask, H, W, pad):
    """pad_reflect_bwd followed by norm_bwd == the gradient of <pad(mask * act(norm(x))), R> with respect to x, gamma and beta."""
    x, gamma, beta, m, Rr, stats = _small(norm, act, mask, H, W, 6, pad, seed=1)
    xt = _nchw(x).requires_grad_(True)
    gt = torch.from_numpy(gamma).double().requires_grad_(True) if gamma is not None else None
    bt = torch.from_numpy(beta).double().requires_grad_(True) if beta is not None else None
    loss = (_torch_fwd(xt, norm, act, gt, bt, None if m is None else _nchw(m), pad) * _nchw(Rr)).sum()
    grads = torch.autograd.grad(loss, [xt] + ([gt, bt] if gt is not None else []))
    d, s1, s2, _ = R.pad_reflect_bwd(Rr, pad, x, stats, gamma, beta, H * W, EPS, act, SLOPE, m)
    dx, dgamma, dbeta = R.norm_bwd(d, x, stats, gamma, H * W, EPS, s1, s2)
    assert dx.dtype == np.float64 and _rel(dx, _nhwc(grads[0])) < 1e-10
    if gt is not None:
        assert _rel(dgamma, grads[1].numpy()) < 1e-10 and _rel(dbeta, grads[2].numpy()) < 1e-10


def test_norm_bwd_on_fp32_inputs_is_autograd():
    """norm_bwd on inputs that ARE fp32 values (what the kernel is given) is the autograd gradient of <BN(x), d> to 1e-10."""
    rng = np.random.default_rng(5)
    H, W, C = 6, 5, 8
    x, d = (rng.standard_normal((H, W, C)) * 2 + 1).astype(np.float32), rng.standard_normal((H, W, C)).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    wide = R.stats_of(x, width=24, offset=8)                       # statistics as a slice of a wider arena
    xt, gt = _nchw(x).requires_grad_(True), torch.from_numpy(gamma).double().requires_grad_(True)
    bt = torch.zeros(C, dtype=torch.float64, requires_grad=True)
    gx, gg, gb = torch.autograd.grad((F.batch_norm(xt, None, None, gt, bt, training=True, eps=EPS) * _nchw(d)).sum(), [xt, gt, bt])
    mean, rstd = R.mean_rstd(wide[8:], H * W, EPS, C, sq_stride=24, out_dtype=np.float64)
    xhat = (x.astype(np.float64) - mean) * rstd
    s1, s2 = d.astype(np.float64).sum((0, 1)), (d * xhat).sum((0, 1))
    dx, dgamma, dbeta = R.norm_bwd(d, x, wide[8:], gamma, H * W, EPS, s1, s2, sq_stride=24)
    assert _rel(dx, _nhwc(gx)) < 1e-10 and _rel(dgamma, gg.numpy()) < 1e-10 and _rel(dbeta, gb.numpy()) < 1e-10


def test_mean_rstd_restates_the_kernel_helper():
    rng = np.random.default_rng(2)
    x = (rng.standard_normal((5, 4, 8)) * 3 + 2).astype(np.float32)
    st = R.stats_of(x)
    m32, r32 = R.mean_rstd(st, 20, EPS, 8)
    assert m32.dtype == r32.dtype == np.float32
    x64 = x.astype(np.float64)
    assert _rel(m32, x64.mean((0, 1))) < 2 ** -23 and _rel(r32, 1 / np.sqrt(x64.var((0, 1)) + EPS)) < 2 ** -23
    # replicas that add up to the plain array, and a wider arena: the same pair, to fp64 rounding of the split
    parts = rng.standard_normal((3, 48))
    wide = np.zeros((4, 48))
    wide[:3] = parts
    plain = R.stats_of(x, width=24, offset=4)
    wide[3] = plain - parts.sum(0)
    m, r = R.mean_rstd(wide.reshape(-1)[4:], 20, EPS, 8, sq_stride=24, rep=48, replicas=4, out_dtype=np.float64)
    m0, r0 = R.mean_rstd(st, 20, EPS, 8, out_dtype=np.float64)
    assert _rel(m, m0) < 1e-13 and _rel(r, r0) < 1e-12
    # a constant channel: the variance clamps at zero instead of going negative
    c = np.full((5, 4, 4), 1.1, dtype=np.float32)
    _, r = R.mean_rstd(R.stats_of(c), 20, EPS, 4, out_dtype=np.float64)
    assert np.isfinite(r).all() and (r <= 1 / np.sqrt(EPS) * (1 + 1e-12)).all()


@pytest.mark.parametrize("H,W,pad", [(7, 9, 3), (3, 4, 1), (8, 12, 3), (5, 7, 0)])
def test_pure_fold_is_the_adjoint_of_the_pad(H, W, pad):
    rng = np.random.default_rng(3)
    x, Rr = rng.standard_normal((H, W, 4)).astype(np.float32), rng.standard_normal((H + 2 * pad, W + 2 * pad, 4)).astype(np.float32)
    d, s1, s2, terms = R.pad_reflect_bwd(Rr, pad)
    assert s1 is None and s2 is None
    xt = _nchw(x).requires_grad_(True)
    padded = F.pad(xt, (pad, pad, pad, pad), mode="reflect") if pad else xt
    g, = torch.autograd.grad((padded * _nchw(Rr)).sum(), xt)
    assert _rel(d, _nhwc(g)) < 1e-12
    lhs = float((R.pad_reflect_fwd(x, pad) * Rr.astype(np.float64)).sum())
    rhs = float((x.astype(np.float64) * d).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((np.abs(R.pad_reflect_fwd(x, pad)) * np.abs(Rr)).sum())
    assert (terms >= np.abs(d) - 1e-12).all()


def _brute_count(H, W, pad):
    """How many padded positions mirror each interior pixel, by walking every padded position."""
    cnt = np.zeros((H, W), dtype=np.int64)
    for py in range(H + 2 * pad):
        for px in range(W + 2 * pad):
            i, j = py - pad, px - pad
            i = -i if i < 0 else (2 * (H - 1) - i if i >= H else i)
            j = -j if j < 0 else (2 * (W - 1) - j if j >= W else j)
            cnt[i, j] += 1
    return cnt


@pytest.mark.parametrize("H,W", [(7, 9), (7, 7)])
def test_edge_map_centre_collects_both_mirrors(H, W):
    """H = 2 pad + 1: the centre row collects three padded rows, the centre column (W = 7) three padded columns."""
    pad = 3
    ones = np.ones((H + 2 * pad, W + 2 * pad, 4), dtype=np.float32)
    d, _, _, terms = R.pad_reflect_bwd(ones, pad)
    cnt = _brute_count(H, W, pad)
    assert np.array_equal(d[..., 0], cnt.astype(np.float64)) and np.array_equal(terms[..., 0], cnt.astype(np.float64))
    assert cnt.sum() == (H + 2 * pad) * (W + 2 * pad)
    rows = np.array([1, 2, 2, 3, 2, 2, 1])                          # padded rows that land on each of the 7 interior rows
    assert np.array_equal(cnt[:, 0], rows * 1) and cnt[3, 1] == 6 and cnt[0, 0] == 1
    if W == 7:
        assert cnt[3, 3] == 9 and np.array_equal(cnt, np.outer(rows, rows))
    else:
        assert cnt[3, 3] == 6 and cnt[3, 4] == 3                    # 9 columns: column 3 is mirrored on the left only


def test_case_table_keeps_clear_of_the_kink():
    assert 30 <= len(K.CASES) <= 48 and len({c.name for c in K.CASES}) == len(K.CASES)
    assert {c.shape for c in K.CASES} == set(K.SHAPES)
    for i, c in enumerate(K.CASES):
        assert c.x.size <= 5e4 and 1000 * (i + 1) <= c.seed < 1000 * (i + 1) + 16
        assert float(np.abs(c.x).max()) < 8.5
        if c.act != "none":
            assert c.margin is not None and c.margin >= K.KINK, (c.name, c.margin)
            full = R.kink_margin(c.x[..., :c.Cl], None if c.stats is None else R.stats_of(c.x[..., :c.Cl]),
                                 None if c.gamma is None else c.gamma[:c.Cl], None if c.beta is None else c.beta[:c.Cl], c.count, K.EPS)
            assert full == c.margin
        if c.Cl < c.C:                                              # padding channels: zero input, zero statistics, zero affine
            assert not c.x[..., c.Cl:].any() and (c.stats is None or not c.stats.reshape(2, c.C)[:, c.Cl:].any())
        if c.m is not None:
            assert set(np.unique(c.m)) == {0.0, 2.0}
        if c.gamma is not None:
            sc = np.abs(c.gamma[:c.Cl]) * R.mean_rstd(c.stats, c.count, K.EPS, c.C, out_dtype=np.float64)[1][:c.Cl]
            assert float(sc.max()) < 2.0, (c.name, float(sc.max()))


@pytest.mark.parametrize("case", K.CASES, ids=[c.name for c in K.CASES])
def test_fp32_restatement_stays_near_the_reference(case):
    """The yardstick is neither absurdly loose nor tight: within 1e-5 (relative to the largest magnitude) of float64."""
    kw64, kw32 = K.norm_args(case, np.float64), K.norm_args(case, np.float32)
    o64, o32 = R.pad_reflect_fwd(case.x, case.pad, **kw64), R.pad_reflect_fwd(case.x, case.pad, **kw32)
    assert o32.dtype == np.float32
    figs = [("out", _rel(o32, o64))]
    if 2 * case.pad < min(case.H, case.W):
        xin = case.x if case.norm != "none" else None
        d64, s1, s2, _ = R.pad_reflect_bwd(case.R, case.pad, xin, **kw64)
        d32, t1, t2, _ = R.pad_reflect_bwd(case.R, case.pad, xin, **kw32)
        assert d32.dtype == np.float32
        figs.append(("din", _rel(d32, d64)))
        if case.norm in ("in", "bn"):
            # the sums cancel (random signs): relative to the sum of magnitudes is the figure that has a meaning
            scale = float(np.abs(d64).sum((0, 1)).max())
            figs += [("s1", float(np.abs(t1 - s1).max()) / scale), ("s2", float(np.abs(t2 - s2).max()) / scale)]
            x64, _, _ = R.norm_bwd(d64, case.x, case.stats, case.gamma, case.count, K.EPS, s1, s2)
            x32, _, _ = R.norm_bwd(d32, case.x, case.stats, case.gamma, case.count, K.EPS, t1, t2, dtype=np.float32)
            assert x32.dtype == np.float32
            figs.append(("dx", _rel(x32, x64)))
    print(f"{case.name} (seed {case.seed}): fp32 restatement vs fp64 " + " ".join(f"{n} {v:.2e}" for n, v in figs))
    for n, v in figs:
        assert v < 1e-5, (case.name, n, v)


def test_norm_apply_and_residual_tail_references():
    rng = np.random.default_rng(7)
    H, W, C = 5, 6, 12
    u, res = rng.standard_normal((H, W, C)).astype(np.float32), rng.standard_normal((H, W, C)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    st = R.stats_of(u)
    t = R.norm_apply_fwd(u, st, gamma, beta, H * W, EPS, noise=res, sigma=1.0)
    ref = _nchw(res) + F.batch_norm(_nchw(u), None, None, torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(),
                                    training=True, eps=EPS)
    assert _rel(t, _nhwc(ref)) < 1e-12
    m = (rng.integers(0, 2, (H, W, C)) * 2).astype(np.float32)
    dm, s1, s2, a1, a2 = R.norm_apply_bwd_sums(res, u, st, H * W, EPS, mask=m)
    xhat = _nhwc(F.instance_norm(_nchw(u), eps=EPS))
    assert np.array_equal(dm, res.astype(np.float64) * m) and _rel(s1, dm.sum((0, 1))) < 1e-12
    assert _rel(s2, (dm * xhat).sum((0, 1))) < 1e-12 and (a1 >= np.abs(s1)).all() and (a2 >= np.abs(s2) - 1e-12).all()
    a, b = _nchw(u).requires_grad_(True), _nchw(res).requires_grad_(True)
    y = torch.tanh(a + b)
    ga, gb = torch.autograd.grad((y * _nchw(m)).sum(), [a, b])
    out = R.add_act(u, res, True)
    assert _rel(out, _nhwc(y)) < 1e-12 and np.array_equal(R.add_act(u, res, False), u.astype(np.float64) + res)
    assert _rel(R.tanh_bwd(m, out), _nhwc(ga)) < 1e-12 and torch.equal(ga, gb)

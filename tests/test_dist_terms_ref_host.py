"""CPU tests of the host yardsticks of the distance-map loss terms: util.signed_edt_sq against scipy's Euclidean distance transform
on both sides of the mask, the level set of util.dist_terms_ref against Kervadec's published composition, and util.dist_terms_ref
against torch float64 autograd of the plain formulas with both distance fields as constants."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy.ndimage import distance_transform_edt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, W, C = 9, 7, 3


def masks():
    rng = np.random.default_rng(11)
    out = {"d%g" % d: rng.random((33, 31)) < d for d in (0.02, 0.5, 0.98)}
    out["empty"] = np.zeros((5, 7), bool)
    out["full"] = np.ones((5, 7), bool)
    one = np.zeros((5, 7), bool)
    one[2, 3] = True
    out["one_inside"], out["one_outside"] = one, ~one
    out["one_pixel_plane_in"], out["one_pixel_plane_out"] = np.ones((1, 1), bool), np.zeros((1, 1), bool)
    out["row"] = rng.random((1, 40)) < 0.3
    out["column"] = rng.random((40, 1)) < 0.3
    return out


def scipy_signed_sq(m):
    """+ the squared distance to the nearest inside pixel outside, - the squared distance to the nearest outside pixel inside, from
    scipy's transform (distance to the nearest zero) squared and rounded to integers; 0 for an empty or full mask."""
    if not m.any() or m.all():
        return np.zeros(m.shape, np.int32)
    out = np.rint(distance_transform_edt(~m) ** 2).astype(np.int64)
    ins = np.rint(distance_transform_edt(m) ** 2).astype(np.int64)
    return np.where(m, -ins, out).astype(np.int32)


@pytest.mark.parametrize("name", sorted(masks()))
def test_signed_edt_sq_equals_scipy_on_both_sides(name):
    from supervised_gan_amd.util import signed_edt_sq
    m = masks()[name]
    got = signed_edt_sq(m)
    assert got.dtype == np.int32 and got.shape == m.shape
    assert np.array_equal(got, scipy_signed_sq(m)), name
    if m.any() and not m.all():
        assert (got[m] <= -1).all() and (got[~m] >= 1).all()
    else:
        assert not got.any()


def test_signed_edt_sq_threshold():
    from supervised_gan_amd.util import signed_edt_sq
    f = np.zeros((5, 7), np.float32)
    f[2, 3], f[0, 0], f[4, 6] = 1.0, np.nan, 0.5      # a NaN and an exact 0.5 are outside
    b = np.zeros((5, 7), bool)
    b[2, 3] = True
    assert np.array_equal(signed_edt_sq(f), signed_edt_sq(b))


def test_level_set_is_kervadecs_composition():
    """one_hot2dist of the boundary-loss paper: negdis * negmask - (posdis - 1) * posmask, posmask the object, posdis the distance
    inside it, negdis the distance outside; an absent (or full) class has an all-zero map."""
    from supervised_gan_amd.util import dist_level_set, signed_edt_sq
    for name, m in masks().items():
        phi = dist_level_set(signed_edt_sq(m))
        if m.any() and not m.all():
            pos, neg = m, ~m
            want = distance_transform_edt(neg) * neg - (distance_transform_edt(pos) - 1) * pos
        else:
            want = np.zeros(m.shape)
        assert np.allclose(phi, want, rtol=0, atol=1e-12), name


def case(mode, kind, seed=0):
    """(z [npix, C] fp32, label or target, truth mask, prediction mask) of the class 0 of a 9 x 7 map."""
    rng = np.random.default_rng(seed)
    npix = H * W
    z = (3.0 * rng.standard_normal((npix, C))).astype(np.float32)
    y = rng.integers(0, C, npix)
    if kind == "absent":
        y[y == 0] = 1
    if kind == "full":
        y[:] = 0
    truth = (y == 0).reshape(H, W)
    if kind == "ignored":
        y.reshape(H, W)[:, 0] = -100
    pred = np.zeros((H, W), bool) if kind == "absent" else rng.random((H, W)) < 0.4
    if mode == 0:
        return z, y.astype(np.int64), truth, pred
    t = rng.random((npix, C)).astype(np.float32)
    if kind in ("absent", "full"):
        t[:, 0] = 0.0 if kind == "absent" else 1.0
    return z, t, truth, pred


def plain_dist_losses(zt, lt, mode, cls, t_s, p_s, alpha):
    """(L_B, L_H) of the logits zt [npix, C] by the plain formulas in torch ops of zt's dtype and device, the fields as constants;
    lt: the int64 label tensor or the target tensor; t_s, p_s: integer tensors [npix]; alpha None: L_H = 0 and p_s is not read."""
    npix, Cn = zt.shape
    dtype = zt.dtype
    if mode == 0:
        valid = ((lt >= 0) & (lt < Cn)).to(dtype)
        p = torch.softmax(zt, dim=1)[:, cls]
        g = (lt == cls).to(dtype)
    else:
        valid = torch.ones(npix, dtype=dtype, device=zt.device)
        p = torch.sigmoid(zt[:, cls])
        g = lt[:, cls].to(dtype)
    s = t_s.to(dtype)
    d = s.abs().sqrt()
    phi = torch.where(s > 0, d, torch.where(s < 0, 1 - d, torch.zeros_like(d)))
    LB = (phi * p * valid).sum() / npix
    LH = zt.sum() * 0
    if alpha is not None:
        F = s.abs() ** (alpha / 2) + p_s.to(dtype).abs() ** (alpha / 2)
        LH = ((p - g) ** 2 * F * valid).sum() / npix
    return LB, LH


def torch_dist_terms(z, lt, mode, cls, t_s, p_s, alpha, dtype=torch.float64):
    """plain_dist_losses with autograd on the CPU: (L_B, L_H, dL_B/dz, dL_H/dz) as Python floats and float64 arrays."""
    zt = torch.tensor(z, dtype=dtype, requires_grad=True)
    LB, LH = plain_dist_losses(zt, torch.tensor(lt), mode, cls, torch.tensor(np.asarray(t_s).reshape(-1).astype(np.int64)),
                               None if p_s is None else torch.tensor(np.asarray(p_s).reshape(-1).astype(np.int64)), alpha)
    gB = torch.autograd.grad(LB, zt, retain_graph=True)[0].double().numpy()
    gH = torch.autograd.grad(LH, zt)[0].double().numpy()
    return float(LB.detach()), float(LH.detach()), gB, gH


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / (np.max(np.abs(b)) + 1e-12))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("kind", ["random", "absent", "full", "ignored"])
@pytest.mark.parametrize("alpha", [2.0, 1.0])
def test_ref_equals_torch_float64_autograd(mode, kind, alpha):
    from supervised_gan_amd.util import dist_terms_ref, signed_edt_sq
    z, lt, truth, pred = case(mode, kind, seed=3 + mode)
    t_s, p_s = signed_edt_sq(truth), signed_edt_sq(pred)
    LB, LH, state, dB, dH = dist_terms_ref(z, lt, mode, 0, t_s, p_s, True, alpha)
    rLB, rLH, rB, rH = torch_dist_terms(z, lt, mode, 0, t_s, p_s, alpha)
    assert abs(LB - rLB) <= 1e-12 * max(1.0, abs(rLB)) and abs(LH - rLH) <= 1e-12 * max(1.0, abs(rLH)), (LB, rLB, LH, rLH)
    assert rel(dB, rB) <= 1e-10 and rel(dH, rH) <= 1e-10, (rel(dB, rB), rel(dH, rH))
    assert state[2] == H * W and state[3] == LB and state[4] == LH and state[0] / (H * W) == LB and state[1] / (H * W) == LH
    # exact zeros
    if kind in ("absent", "full"):      # the truth's map is 0 everywhere: no boundary term; absent: the prediction's too
        assert not t_s.any() and LB == 0.0 and not dB.any()
        if kind == "absent":
            assert LH == 0.0 and not dH.any()
    if kind == "ignored" and mode == 0:
        rows = np.arange(H * W).reshape(H, W)[:, 0]
        assert not dB[rows].any() and not dH[rows].any()
    if mode == 1:
        assert not dB[:, 1:].any() and not dH[:, 1:].any()      # the other sigmoid channels
    # a term that is off
    off = dist_terms_ref(z, lt, mode, 0, t_s, None, True, None)
    assert off[0] == LB and off[1] == 0.0 and not off[4].any() and np.array_equal(off[3], dB)
    off = dist_terms_ref(z, lt, mode, 0, t_s, p_s, False, alpha)
    assert off[0] == 0.0 and off[1] == LH and not off[3].any() and np.array_equal(off[4], dH)

"""tests/dist_terms_ref.py against the point yardstick util.dist_terms_ref and against torch's double autograd of the plain formulas
(tests/test_dist_terms_ref_host.torch_dist_terms), to 1e-12, at every shape, mode and parameter set
tests/test_hip_dist_terms_kernels.py uses, and the conditions the reference side alone must meet:
  * torch's CPU fp32 evaluation of the backward composition lies inside its budget on every element, and the sums of its fp32 p inside
    both forward intervals;
  * the planted pixels have a non-zero level set and field and a p within a few ulp of 1 (sigmoid: exactly 1 for the larger values);
  * the case table covers what it is there for, so that a later edit cannot drop a form, a size, an exponent or a map value silently.
Every case is held to both, the maps at the edge of int32 included.  torch's autograd forms 1 - p by subtraction, so it is compared
in units of |G| p, the yardstick (others over the sum, sigmoid(-z)) in units of the element's own magnitude.  No GPU, no library."""
import numpy as np
import pytest

import dist_terms_cases as K
import dist_terms_ref as D
import loss_ref as R
from test_dist_terms_ref_host import torch_dist_terms

TOL = 1e-12


def _close(a, b, scale, tol=TOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool((np.abs(a - b) <= tol * np.maximum(scale, 1e-300)).all())


def _unique(cases):
    """One case per (inputs, mode, class, terms): the layouts, row widths and upstream gradients share a reference."""
    seen, out = set(), []
    for c in cases:
        key = (c.H, c.W, c.C, c.mode, c.cls, c.geom, c.alpha, c.boundary, c.kind, c.tgt if c.mode == K.SIGMOID else "")
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def _dense_target(r):
    """The sigmoid target with its unread channels (NaN) set to 0 for a yardstick that reads whole rows."""
    return r.lt if r.c.mode == K.SOFTMAX else np.nan_to_num(r.lt, nan=0.0)


@pytest.mark.parametrize("c", _unique(K.CASES), ids=K.case_id)
def test_point_values_against_the_yardstick_and_double_autograd(c):
    from supervised_gan_amd.util import dist_terms_ref
    r = K.ref_of(c)
    px = r.px
    lt = _dense_target(r)
    yLB, yLH, ystate, yB, yH = dist_terms_ref(r.z, lt, c.mode, c.cls, r.t_s, r.p_s if r.hausdorff else None, c.boundary, c.alpha)
    # the sums against the sum of their terms' magnitudes (the boundary sum is signed), everything else against itself
    v = px.ok.astype(np.float64)
    magB = float(np.sum(np.abs(px.phi) * px.p * v))
    assert _close(r.SB, ystate[0], magB) and _close(r.SH, ystate[1], abs(ystate[1])), (r.SB, r.SH, ystate)
    assert r.state[2] == ystate[2] == c.H * c.W
    assert _close(r.state[3], yLB, magB / px.npix) and _close(r.state[4], yLH, abs(yLH))
    dB, mB = D.backward(px, 1.0 / px.npix if c.boundary else 0.0, 0.0)
    dH, mH = D.backward(px, 0.0, 2.0 / px.npix if r.hausdorff else 0.0)
    assert _close(dB, yB, mB) and _close(dH, yH, mH)
    gB = (D.g_of(px, 1.0 / px.npix if c.boundary else 0.0, 0.0)[1] * px.p)[:, None]
    gH = (D.g_of(px, 0.0, 2.0 / px.npix if r.hausdorff else 0.0)[1] * px.p)[:, None]
    tLB, tLH, tB, tH = torch_dist_terms(r.z, lt, c.mode, c.cls, r.t_s, r.p_s if r.hausdorff else None, c.alpha)
    if c.boundary:
        assert _close(r.state[3], tLB, magB / px.npix), (r.state[3], tLB)
        assert _close(dB, tB, gB), float(np.abs(dB - tB).max())
    if r.hausdorff:
        assert _close(r.state[4], tLH, abs(tLH)), (r.state[4], tLH)
        assert _close(dH, tH, gH), float(np.abs(dH - tH).max())
    # the gradient the kernels are held to is that of the upstream pair
    ub, uh = r.u
    assert _close(r.dz, ub * px.npix * yB + 0.5 * uh * px.npix * yH, r.mag)
    # structural zeros
    assert not r.dz[~px.ok].any() and not r.mag[~px.ok].any()
    if c.mode == K.SIGMOID:
        others = [k for k in range(c.C) if k != c.cls]
        assert not r.dz[:, others].any() and not r.mag[:, others].any()
    if c.mode == K.SOFTMAX and c.C == 1:
        assert not r.mag.any() and r.SH == 0.0
        assert (px.p == 1.0).all() and r.SB == float(np.sum(px.phi * v))                    # L_B is the mean of phi over the labelled pixels
    if c.gout == (None, None) or (c.gout[0] in (None, 0.0) and not r.hausdorff) or (c.gout[1] is None and not c.boundary):
        assert not r.dz.any() and not r.mag.any()
    both_zero = (px.tmap == 0) & ((px.pmap == 0) if r.hausdorff else True)
    assert not r.mag[both_zero].any()
    if not c.boundary:
        assert r.SB == 0.0 and r.state[3] == 0.0 and r.LB == 0.0
    if not r.hausdorff:
        assert r.SH == 0.0 and r.state[4] == 0.0 and r.LH == 0.0


@pytest.mark.parametrize("c", _unique(K.CASES), ids=K.case_id)
def test_reference_side_conditions(c):
    r = K.ref_of(c)
    px = r.px
    bp, bd = K.p_budget(c.mode), K.grad_budget(K.group_of(c))
    assert r.e_p <= bp and r.e_d <= bd, (r.e_p, bp, r.e_d, bd)
    (blo, bhi), (hlo, hhi) = D.forward_intervals(px, bp, r.pow_ulps)
    assert blo <= r.SB <= bhi and hlo <= r.SH <= hhi
    # the forward with torch's fp32 p, everything behind it in float64 as in the kernel
    v = px.ok.astype(np.float64)
    gotB, gotH = float(np.sum(px.phi * r.pc32 * v)), float(np.sum((r.pc32 - px.g) ** 2 * px.F * v))
    assert blo <= gotB <= bhi and hlo <= gotH <= hhi, (gotB, blo, bhi, gotH, hlo, hhi)
    if not c.boundary:
        assert blo == 0.0 and bhi == 0.0
    if not r.hausdorff:
        assert hlo == 0.0 and hhi == 0.0
    magB = float(np.sum(np.abs(px.phi) * px.p * v))
    print(f"{K.case_id(c)}: budgets p {bp:.2f} dz {bd:.2f} ulp (fp32 composition {r.e_d:.2f}); half-width of S_B {(bhi - blo) / (2 * magB) if magB else 0:.3e} "
          f"of its terms' magnitudes, of S_H {R.half_width(hlo, hhi) if hhi > 0 else 0:.3e}; pow allowance {r.pow_ulps:.2f} fp64 ulp")
    assert 2.0 <= r.pow_ulps <= 16.0


def test_planted_pixels_have_a_field_and_p_next_to_one():
    """What the planted cases are there for: p within a few ulp of 1 on a pixel whose level set and field are not zero, where 1 - p
    by subtraction has lost every digit that om and sigmoid(-z) keep."""
    seen = 0
    for c in K.CASES:
        if c.kind != "planted":
            continue
        r = K.ref_of(c)
        px = r.px
        idx = K.planted_pixels(r.t_s, r.p_s, 4 * len(R.GAN_PLANTED))
        assert (px.phi[idx] != 0.0).all() and (r.hausdorff is False or (px.F[idx] > 0.0).all())
        on = idx[np.arange(idx.size) % 4 < 2][np.repeat(np.array(R.GAN_PLANTED) > 0, 2)]      # the class's channel holds +17 .. +120
        assert on.size == len(R.GAN_PLANTED) and (1.0 - px.p[on] <= 3.0 * 2.0 ** -24).all() and (px.p[on] < 1.0).any()
        w = px.om[on] if c.mode == K.SOFTMAX else px.q[on]
        assert (w > 0.0).all() and (w < 2.0 ** -23).all()
        assert (r.mag[on, c.cls] > 0.0).all()
        if c.mode == K.SOFTMAX:
            assert px.ok[idx].all() and {0.0, 1.0} == set(px.g[on])      # the label on and off the planted channel
        else:
            assert {float(np.float32(0.9)), float(np.float32(0.1))} == set(px.g[on]) or {0.0, 1.0} == set(px.g[on])
        seen += 1
    assert seen == 16


def test_case_table_covers_what_the_issue_lists():
    """No option may be tied to a (C, ld, dld) form by the way the table is dealt, and nothing the table is there for may drop out."""
    assert {f[0] for f in K.FORMS} == {1, 2, 3, 4, 12, 16}
    assert {(C, ld) for C, ld, dld, lay in K.FORMS if lay == "dense" and ld == dld} >= {(C, K.pad4(C)) for C in (1, 2, 3, 4, 12, 16)} | {(3, 8), (12, 16)}
    assert {dld for C, ld, dld, lay in K.FORMS if C == 3 and ld == 4 and lay == "dense"} >= {3, 4, 5, 8, 20, 32}
    assert (3, 32, 4, "view32") in K.FORMS and (3, 4, 4, "off1") in K.FORMS and (3, 8, 4, "dense") in K.FORMS and (16, 16, 20, "dense") in K.FORMS
    for mode in (K.SOFTMAX, K.SIGMOID):
        mine = [c for c in K.CASES if c.mode == mode]
        small = [c for c in mine if (c.H, c.W) in K.SMALL and c.kind == "random"]
        for form in K.FORMS:
            has = [c for c in small if (c.C, c.ld, c.dld, c.layout) == form]
            assert {(c.H, c.W) for c in has} == set(K.SMALL), (mode, form)
            assert any(c.boundary and c.alpha is not None and c.gout in K.ORDINARY for c in has), (mode, form, "joint backward")
            assert len({c.gout for c in has}) >= 3 and len({c.alpha for c in has}) >= 3, (mode, form)
        assert {c.alpha for c in small} == set(K.ALPHAS) | {None}
        assert {c.gout for c in small} == set(K.GOUTS)
        assert {(c.boundary, c.alpha is not None) for c in small} == {(True, True), (True, False), (False, True)}
        assert any(c.cls != 0 for c in small) and any(c.cls == 0 for c in small)
        blob = [c for c in mine if (c.H, c.W) == K.BLOB]
        assert {c.geom for c in blob} == set(K.GEOMS) and {c.alpha for c in blob} == set(K.ALPHAS) | {None}
        for geom in K.GEOMS:
            assert {0.5, 4.0} <= {c.alpha for c in blob if c.geom == geom and c.C == 3 and c.boundary}, (mode, geom)
        big = [c for c in mine if (c.H, c.W) in K.LARGE]
        assert {(c.H, c.W, c.C, c.ld) for c in big} == {(H, W, C, ld) for H, W in K.LARGE for C, ld in K.LARGE_PAIRS}
        assert all(c.boundary and c.alpha is not None and c.gout in K.ORDINARY for c in big)
        assert {c.alpha for c in mine if c.kind == "planted"} == {None, 0.5, 2.0, 4.0} and any(c.kind == "saturated" for c in mine)
        assert any(c.geom == "synth" and c.alpha == 4.0 and c.boundary for c in mine) and any(c.geom == "synth" and c.alpha == 4.0 and not c.boundary for c in mine)
        if mode == K.SIGMOID:
            assert {c.tgt for c in small} == {"hot", "soft"}
            assert any(c.ld == 8 and c.dld == 4 for c in small)      # the vector backward with logit rows of another width
    assert any(c.mode == K.SOFTMAX and c.C == 1 and c.geom != "synth" and c.alpha is not None for c in K.CASES)
    # map values: 0, +-1, +-2^30 and both ends of int32 reach a kernel, at least one beyond +-2^30 at alpha 4; real maps reach four digits
    assert {0, 1, -1, 2 ** 30, -2 ** 30, D.INT32_MIN, D.INT32_MAX} <= set(K.SYNTH)
    t_s, p_s, _ = K.maps(5, 7, "synth")
    assert {D.INT32_MIN, D.INT32_MAX} <= set(t_s.tolist()) | set(p_s.tolist()) and np.abs(t_s.astype(np.int64)).max() > 2 ** 30
    t_s, p_s, _ = K.maps(64, 64, "discs")
    assert t_s.min() == -225 and t_s.max() == 1405 and (t_s != 0).all()
    # out-of-range labels, the two that differ from a valid label in their upper 32 bits alone among them
    for c in K.CASES:
        if c.mode == K.SOFTMAX and c.H * c.W >= 16:
            lab = set(K.ref_of(c).lt.tolist())
            assert {-100, c.C, -1} | set(R.BIG_LABELS) <= lab, K.case_id(c)
        if c.mode == K.SIGMOID:
            t = K.ref_of(c).lt
            assert np.isnan(np.delete(t, c.cls, axis=1)).all() and np.isfinite(t[:, c.cls]).all()
    assert 2.0 < K.ALPHAS[4] < 2.0 + 1e-15

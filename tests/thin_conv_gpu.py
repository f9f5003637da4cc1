"""What tests/test_hip_thin_conv.py, tests/test_hip_thin_wgrad.py, tests/test_hip_wide_conv.py and tests/test_hip_wide_wgrad.py share:
the rows of tests/thin_conv_cases.py and tests/wide_conv_cases.py turned into job lists in NaN-guarded storage, and the checks of what a
launch left behind against tests/thin_conv_ref.py."""
import numpy as np
import torch

import thin_conv_cases as K
import thin_conv_ref as R
from hip_utils import _guard_intact, _guarded, from_buf, from_master, master_weight, pad_vec, to_buf
from thin_conv_ref import pad4

NAN = float("nan")
WORST = {}      # kernel -> worst ratio to the bound over the run (printed by the test modules)


class Guards:
    """Every operand goes through here: a copy whose storage ends in a NaN guard (hip_utils._guarded)."""

    def __init__(self):
        self.guards = []

    def __call__(self, t):
        v, g = _guarded(t.cuda())
        self.guards.append(g)
        return v

    def broken(self):
        return [i for i, g in enumerate(self.guards) if not _guard_intact(g)]


def last_kernel():
    from supervised_gan_amd import _lib
    return _lib.lib().sgan_last_kernel().decode()


def last_variant():
    from supervised_gan_amd import _lib
    return _lib.lib().sgan_last_variant().decode()


def launched(kernel, variant=None):
    """The last launch was `kernel`, in the variant the table names (None: the name says it all)."""
    assert last_kernel() == kernel, (last_kernel(), kernel)
    assert variant is None or last_variant() == variant, (last_variant(), variant)


def weights(ops, w, tr, G):
    """(master copy, transposed copy) of a torch-layout weight, guarded, tagged with guarded 16-bit copies as the networks' are."""
    wm0 = master_weight(w, tr)
    wm, wt = G(wm0), G(wm0._sgan_wt)
    ops.with_packed(wm, G(wm0._sgan_pk))
    ops.with_packed(wt, G(wm0._sgan_wt._sgan_pk), G(wm0._sgan_wt._sgan_pk16))
    return wm, wt


def _desc(ops, L, p):
    return ops.conv_desc(1 if L.tr else 0, L.k, L.s, L.p, p["H"], p["W"], pad4(L.cin), p["Ho"], p["Wo"], pad4(L.cout), L.cin, L.cout)


def _norm(ops, case, d, p, G, gam, bet):
    if not case.norm and not case.act:
        return None
    st = G(R.stats_of(p["x"])) if case.norm else None
    return ops.norm_desc(st, gam, bet, p["H"] * p["W"], 1e-5, case.act, R.SLOPE)


def _affine(case, d, G):
    return (G(pad_vec(d["gamma"])), G(pad_vec(d["beta"]))) if case.norm == "bn" else (None, None)


def held(got, ref, bound, what, key):
    """Every element within its bound; the worst ratio over the whole [C, H, W] output and over its outermost two rows / columns."""
    err = (got.double() - ref).abs()
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    ratio = err / bound.clamp_min(1e-300)
    ring = torch.from_numpy(R.ring2(*got.shape[-2:])) if got.dim() == 3 else None
    r, rr = float(ratio.max()), (float(ratio[:, ring].max()) if ring is not None else float("nan"))
    print(f"{what}: worst |kernel - fp64| / bound = {r:.3f} (outer two rows / columns {rr:.3f})")
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert bool((err <= bound).all()), f"{what}: {r:.3f} of the bound at {np.unravel_index(int(ratio.argmax()), ratio.shape)}"


def sums_held(st, C, refs, bounds, what, key):
    """double[2 Cs] statistics against the reference's two sums."""
    Cs, st = st.numel() // 2, st.cpu()
    for name, got, ref, b in (("sum", st[:C], refs[0], bounds[0]), ("second sum", st[Cs: Cs + C], refs[1], bounds[1])):
        err = (got - ref).abs()
        r = float((err / b.clamp_min(1e-300)).max())
        print(f"{what} {name}: worst ratio {r:.3f}")
        WORST[key + " sums"] = max(WORST.get(key + " sums", 0.0), r)
        assert bool((err <= b).all()), f"{what} {name}: {r:.3f} of the bound"
    assert float(st[C: Cs].abs().max() if Cs > C else 0.0) == 0.0 and float(st[Cs + C:].abs().max() if Cs > C else 0.0) == 0.0


# ---- forward --------------------------------------------------------------------------------------------------------------------------
def build_fwd(ops, case, G, key=None):
    """key: what the worst ratios are filed under (default: the row's kernel)."""
    d, L, key = K.data(case), case.layer, key or case.kernel
    wm, _ = weights(ops, d["w"], L.tr, G)
    bb = G(pad_vec(d["b"])) if case.bias else None
    gam, bet = _affine(case, d, G)
    jobs, outs = [], []
    for p in d["probs"]:
        ob = G(torch.full((p["Ho"], p["Wo"], pad4(L.cout)), NAN))
        ost = G(torch.zeros(2 * pad4(L.cout), dtype=torch.float64)) if case.stats else None
        jobs.append((_desc(ops, L, p), G(to_buf(p["x"][None])), _norm(ops, case, d, p, G, gam, bet), wm, bb, ob, ost, 0, 0))
        outs.append((ob, ost))

    def check():
        for i, ((ob, ost), ref) in enumerate(zip(outs, K.reference(case))):
            held(from_buf(ob, L.cout)[0], ref["ref"], ref["bound"], f"{case.name}[{i}] forward", key)
            assert pad4(L.cout) == L.cout or float(ob[..., L.cout:].abs().max()) == 0.0, "padded channels must stay exactly zero"
            if ost is not None:
                v, b = ref["pre"], ref["pre_bound"]
                sums_held(ost, L.cout, (v.sum((1, 2)), (v * v).sum((1, 2))), (R.bound_sum(v, b), R.bound_sumsq(v, b)), f"{case.name}[{i}] statistics",
                          key)
    return jobs, check


# ---- backward-data --------------------------------------------------------------------------------------------------------------------
def build_dgrad(ops, case, G, accum=None, key=None):
    """accum=False: the same jobs without accumulate into NaN-filled outputs (the accumulate rows run both)."""
    d, L, key = K.data(case), case.layer, key or case.kernel
    acc = case.accum if accum is None else accum
    wm, wt = weights(ops, d["w"], L.tr, G)
    gam, bet = _affine(case, d, G) if case.x else (None, None)
    jobs, outs = [], []
    for p in d["probs"]:
        din = G(to_buf(p["prev"][None])) if acc else G(torch.full((p["H"], p["W"], pad4(L.cin)), NAN))
        xb = G(to_buf(p["x"][None])) if case.x else None
        nd = _norm(ops, case, d, p, G, gam, bet) if case.x else None
        sums = G(torch.zeros(2 * pad4(L.cin), dtype=torch.float64)) if case.stats else None
        jobs.append((_desc(ops, L, p), G(to_buf(p["dy"][None])), wt if case.wt else wm, din, xb, nd, sums, 0, acc, case.wt, 0))
        outs.append((din, sums))

    def check():
        for i, ((din, sums), ref) in enumerate(zip(outs, K.reference(case))):
            r, b = (ref["ref"], ref["bound"]) if acc else (ref["own"], ref["own_bound"])
            held(from_buf(din, L.cin)[0], r, b, f"{case.name}[{i}] backward-data" + ("" if acc == case.accum else " (no accumulate)"), key)
            assert pad4(L.cin) == L.cin or float(din[..., L.cin:].abs().max()) == 0.0, "padded channels must stay exactly zero"
            if sums is not None:
                v, vb, xh = ref["own"], ref["own_bound"], ref["xhat"]
                sums_held(sums, L.cin, (v.sum((1, 2)), (v * xh).sum((1, 2))), (R.bound_sum(v, vb), R.bound_sum(v, vb, xh)),
                          f"{case.name}[{i}] norm-backward", key)
    return jobs, check, outs


# ---- backward-weight ------------------------------------------------------------------------------------------------------------------
def build_wgrad(ops, case, G, key=None):
    d, L = K.data(case), case.layer
    zero_w = torch.zeros(L.wshape())
    dw = G(master_weight(d["prev_w"] if case.accum else zero_w, L.tr).clone())
    db = G(pad_vec(d["prev_b"]) if case.accum else torch.zeros(pad4(L.cout))) if case.bias else None
    gam, bet = _affine(case, d, G)
    jobs = [(_desc(ops, L, p), G(to_buf(p["x"][None])), _norm(ops, case, d, p, G, gam, bet), G(to_buf(p["dy"][None])), dw, db) for p in d["probs"]]

    def check():
        ref, key_ = K.reference(case), key or case.kernel or K.PAIR + " dw"
        assert bool(torch.isfinite(dw).all())
        held(from_master(dw, L.k, L.cin, L.cout, L.tr).double(), ref["dw"], ref["dw_bound"], f"{case.name} backward-weight", key_)
        m = dw.detach().cpu().view(L.k, L.k, pad4(L.cout), pad4(L.cin))
        assert float(m[:, :, L.cout:].abs().max() if pad4(L.cout) > L.cout else 0.0) == 0.0, "padded rows of dw must stay exactly zero"
        assert float(m[..., L.cin:].abs().max() if pad4(L.cin) > L.cin else 0.0) == 0.0, "padded columns of dw must stay exactly zero"
        if db is not None:
            held(db.cpu()[: L.cout].double(), ref["db"], ref["db_bound"], f"{case.name} bias gradient", key_ + " dbias")
            assert pad4(L.cout) == L.cout or float(db[L.cout:].abs().max()) == 0.0
    return jobs, check

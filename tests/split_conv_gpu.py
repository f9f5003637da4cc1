"""What tests/test_hip_split_conv.py, tests/test_hip_split_wgrad.py and tests/test_hip_fused_bwd.py share: the rows of
tests/split_conv_cases.py turned into job lists in NaN-guarded storage (thin_conv_gpu's Guards / weights / descriptors), the two
per-call knobs of a row set for its launch, and the checks of what a launch left behind against split_conv_cases.reference: every
element within its bound (thin_conv_gpu.held prints and files the worst ratio), padded channels zero, sums within bound_sum, and G3
(distance from the fp64 result of the unrounded operands)."""
import os

import torch

import plane_model as PM
import split_conv_cases as S
import thin_conv_gpu as T
import thin_conv_ref as R
from hip_utils import from_buf, from_master, master_weight, pad_vec, to_buf
from thin_conv_ref import pad4

KNOBS = ("SGAN_TILE3", "SGAN_IGEMM3P")
NAN = float("nan")


def clear_knobs():
    for k in KNOBS:
        os.environ.pop(k, None)


class knobs:
    """The row's per-call knobs for the launches inside; both popped on the way out."""

    def __init__(self, case):
        self.env = case.env

    def __enter__(self):
        clear_knobs()
        os.environ.update(self.env)

    def __exit__(self, *exc):
        clear_knobs()
        return False


def publish(buf):
    buf._sgan_amax = buf.abs().max().reshape(1).float()
    return buf


def g3(what, got, truth, limit):
    e = PM.rel_max(got, truth)
    print(f"{what}: max-norm distance from fp64 {e:.3g} (limit {limit})")
    assert limit is None or e < limit, (what, e, limit)


def build_fwd(ops, case, G):
    d, L = T.K.data(case), case.layer
    wm, _ = T.weights(ops, d["w"], L.tr, G)
    bb = G(pad_vec(d["b"])) if case.bias else None
    gam, bet = T._affine(case, d, G)
    jobs, outs = [], []
    for p in d["probs"]:
        ob = G(torch.full((p["Ho"], p["Wo"], pad4(L.cout)), NAN))
        ost = G(torch.zeros(2 * pad4(L.cout), dtype=torch.float64)) if case.stats else None
        jobs.append((T._desc(ops, L, p), G(to_buf(p["x"][None])), T._norm(ops, case, d, p, G, gam, bet), wm, bb, ob, ost, 0, 0))
        outs.append((ob, ost))

    def check(key):
        for i, ((ob, ost), ref) in enumerate(zip(outs, S.reference(case))):
            got = from_buf(ob, L.cout)[0]
            T.held(got, ref["ref"], ref["bound"], f"{case.name}[{i}] forward", key)
            g3(f"{case.name}[{i}] forward", got, ref["truth"], S.g3_limits(case))
            assert pad4(L.cout) == L.cout or float(ob[..., L.cout:].abs().max()) == 0.0, "padded channels must stay exactly zero"
            if ost is not None:
                v, b = ref["pre"], ref["pre_bound"]
                T.sums_held(ost, L.cout, (v.sum((1, 2)), (v * v).sum((1, 2))), (R.bound_sum(v, b), R.bound_sumsq(v, b)), f"{case.name}[{i}] statistics", key)
    return jobs, check


def build_dgrad(ops, case, G, accum=None, planes=None, sentinel=None):
    """accum=False: the same jobs without accumulate into NaN-filled outputs; planes: whether dY carries its maximum (default: the
    row's); sentinel: outputs prefilled with it (the refusals)."""
    d, L = T.K.data(case), case.layer
    acc = case.accum if accum is None else accum
    pub = case.planes if planes is None else planes
    _, wt = T.weights(ops, d["w"], L.tr, G)
    gam, bet = T._affine(case, d, G) if case.x else (None, None)
    jobs, outs = [], []
    for p in d["probs"]:
        fill = NAN if sentinel is None else sentinel
        din = G(to_buf(p["prev"][None])) if acc else G(torch.full((p["H"], p["W"], pad4(L.cin)), fill))
        xb = G(to_buf(p["x"][None])) if case.x else None
        nd = T._norm(ops, case, d, p, G, gam, bet) if case.x else None
        sums = G(torch.full((2 * pad4(L.cin),), 0.0 if sentinel is None else sentinel, dtype=torch.float64)) if case.stats else None
        dyb = G(to_buf(p["dy"][None]))
        jobs.append((T._desc(ops, L, p), publish(dyb) if pub else dyb, wt, din, xb, nd, sums, 0, acc, True, 0))
        outs.append((din, sums))

    def check(key, f16=None, limit="row"):
        for i, ((din, sums), ref) in enumerate(zip(outs, S.reference(case, f16))):
            r, b, t = (ref["ref"], ref["bound"], ref["truth"]) if acc else (ref["own"], ref["own_bound"], ref["own_truth"])
            got = from_buf(din, L.cin)[0]
            T.held(got, r, b, f"{case.name}[{i}] backward-data", key)
            g3(f"{case.name}[{i}] backward-data", got, t, S.g3_limits(case) if limit == "row" else limit)
            assert pad4(L.cin) == L.cin or float(din[..., L.cin:].abs().max()) == 0.0, "padded channels must stay exactly zero"
            if sums is not None:
                v, vb, xh = ref["own"], ref["own_bound"], ref["xhat"]
                T.sums_held(sums, L.cin, (v.sum((1, 2)), (v * xh).sum((1, 2))), (R.bound_sum(v, vb), R.bound_sum(v, vb, xh)),
                            f"{case.name}[{i}] norm-backward", key)
    return jobs, check, outs


def build_wgrad(ops, case, G, sentinel=None):
    d, L = T.K.data(case), case.layer
    zero_w = torch.zeros(L.wshape()) if sentinel is None else torch.full(L.wshape(), sentinel)
    dw = G(master_weight(d["prev_w"] if case.accum else zero_w, L.tr).clone())
    db = G(pad_vec(d["prev_b"]) if case.accum else torch.full((pad4(L.cout),), 0.0 if sentinel is None else sentinel)) if case.bias else None
    gam, bet = T._affine(case, d, G)
    jobs = []
    for p in d["probs"]:
        dyb = G(to_buf(p["dy"][None]))
        jobs.append((T._desc(ops, L, p), G(to_buf(p["x"][None])), T._norm(ops, case, d, p, G, gam, bet), publish(dyb) if case.planes else dyb, dw, db))

    def check(key):
        ref = S.reference(case)
        got = from_master(dw, L.k, L.cin, L.cout, L.tr).double()
        T.held(got, ref["dw"], ref["dw_bound"], f"{case.name} backward-weight", key)
        g3(f"{case.name} backward-weight", got, ref["truth"], S.g3_limits(case))
        if db is not None:
            T.held(db.cpu()[: L.cout].double(), ref["db"], ref["db_bound"], f"{case.name} bias gradient", key + " dbias")
    return jobs, check, (dw, db)

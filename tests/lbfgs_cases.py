"""The case table of tests/test_hip_lbfgs_kernel.py and tests/test_lbfgs_ref_host.py: snapshots of sg_lbfgs_advance_kernel's state and
buffers built on the host (tests/lbfgs_ref.py has the layout), torch's CPU evaluation of the same launch (lbfgs._advance_one, fp32 for
the budgets and float64 for the reference's own check) and the budgets.  DESIGN.md R39.

A case is ONE launch: J snapshots of the same n and history_cap (history_size is a field of each state), the row strides of x and
grad, and the offset of their bases into their allocations.  Two kinds:
  * planted decisions: one non-zero element (index 65 of 67: the second wave), powers of two or single fp32 numbers, so every sum is
    exact and a comparison can be put just below, exactly at and just above its threshold (`nextafter`).  `want` holds the exit code
    and whether a pair goes into the ring, derived by hand: the reference is held to it on the host.
  * random snapshots for the arithmetic: a history Y = A S of an SPD A = Q D Q (Q a Householder reflection, D log-uniform in
    [1, cond], cond = 100; 1.05 for the 1024-pair ring of 8 unknowns, where 1024 factors (I - rho y s') of norm (cond + 1) / (2
    sqrt(cond)) each multiply up), the current pair y = g - pg = A (d t) as well, so that ys is far above 1e-10 and g.d far
    below -tolerance_change.  Ring slots outside the live pairs, d and prev_grad at n_iter == 1 and the slots behind history_size hold
    NaN: a launch that reads one of them turns its result NaN.
"""
import functools

import numpy as np
import torch

import lbfgs_ref as R
from supervised_gan_amd import lbfgs as LB

F32, F64 = np.float32, np.float64
NAN = float("nan")
RESERVED0 = 0x5A5A5A5A
RESERVED = [0x5A5A5A50 + i for i in range(8)]
NS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096, 4097, 5000)
JS = (1, 2, 5, 8)
PADS = (0, 1, 13)       # x_ld - n, g_ld - n
# (history_size, history_cap, hist_len, hist_head)
GEOMS = ((5, 5, 0, 0), (5, 5, 1, 0), (5, 5, 2, 3), (5, 5, 4, 2), (5, 5, 5, 0), (5, 5, 5, 2), (5, 5, 5, 4), (1, 1, 0, 0), (1, 1, 1, 0),
         (3, 7, 3, 1), (3, 7, 2, 2), (100, 128, 100, 57), (100, 128, 99, 0), (100, 100, 17, 0))
BIG_RING = (1024, 1024, 1024, 500)      # n = 8: more pairs than threads
TRIPLE = ("below", "at", "above")


def f32(v):
    return float(F32(v))


def new_state(**kw):
    st = dict(lr=f32(0.1), tolerance_grad=f32(1e-7), tolerance_change=1e-9, max_iter=20, max_eval=25, history_size=5, n_steps=5,
              func_evals=10, n_iter=9, steps=1, phase=R.PHASE_AFTER_MOVE, done=0, iter_in_step=2, evals_in_step=3, hist_len=0,
              hist_head=0, last_exit=R.EXIT_MAX_ITER, n_skipped=1, reserved0=RESERVED0, t=f32(0.1), h_diag=f32(0.77), prev_loss=2.0,
              reserved=list(RESERVED))
    assert set(kw) <= set(st), set(kw) - set(st)
    st.update(kw)
    return st


def _nan(*shape):
    return np.full(shape, NAN, F32)


def blank(n, cap, **state):
    """A snapshot with NaN in every buffer the launch could read."""
    return dict(state=new_state(**state), n=n, x=np.ones(n, F32), grad=np.zeros(n, F32), loss=F32(4.0), d=_nan(n), prev_grad=_nan(n),
                S=_nan(cap, n), Y=_nan(cap, n), rho=_nan(cap))


def case(name, snaps, pad_x=0, pad_g=0, off=0, want=None, triple=None, formats=False):
    n, cap = snaps[0]["n"], snaps[0]["rho"].shape[0]
    assert all(s["n"] == n and s["rho"].shape[0] == cap for s in snaps)
    return dict(name=name, snaps=snaps, J=len(snaps), n=n, cap=cap, x_ld=n + pad_x, g_ld=n + pad_g, off=off, want=want, triple=triple,
                formats=formats)


# ---- planted decisions ---------------------------------------------------------------------------------------------------------------
PN, PI = 67, 65


def _planted(g=1.0, d=1.0, n=PN, idx=PI, **state):
    """After a move: one non-zero element each in grad and d, prev_grad 0, t = lr = 1, an empty ring of 3.  y.s = g d."""
    kw = dict(lr=1.0, t=1.0, tolerance_grad=0.0, tolerance_change=2.0 ** -80, history_size=3, prev_loss=8.0, h_diag=0.5)
    kw.update(state)
    s = blank(n, 3, **kw)
    s["grad"][min(idx, n - 1)] = g
    s["d"] = np.zeros(n, F32)
    s["d"][min(idx, n - 1)] = d
    s["prev_grad"] = np.zeros(n, F32)
    return s


def _start(g, n=PN, idx=PI, cap=3, **state):
    """A fresh optimizer's first evaluation: n_iter 0, d and prev_grad never written."""
    kw = dict(lr=1.0, tolerance_grad=0.0, tolerance_change=2.0 ** -80, history_size=3, phase=R.PHASE_START, n_iter=0, func_evals=0, steps=0,
              iter_in_step=0, evals_in_step=0, last_exit=0, n_skipped=0, t=0.0, h_diag=1.0, prev_loss=0.0)
    kw.update(state)
    s = blank(n, cap, **kw)
    s["grad"][min(idx, n - 1)] = g
    return s


def _near(v, pos, dtype=F32):
    v = dtype(v)
    return float({"below": np.nextafter(v, dtype(0)), "at": v, "above": np.nextafter(v, dtype(np.inf))}[pos])


def planted_cases():
    out = []
    add = lambda *a, **k: out.append(case(*a, **k))
    for pos in TRIPLE:
        hit = pos != "above"
        # max|g| <= tolerance_grad, both phases; the element is negative: |g| is what is compared
        add(f"gmax_start_{pos}", [_start(-_near(0.75, pos), tolerance_grad=0.75)], triple=("gmax_start", pos),
            want=(R.EXIT_OPT_START if hit else 0, False))
        add(f"gmax_after_{pos}", [_planted(g=-_near(0.75, pos), d=-1.0, tolerance_grad=0.75)], triple=("gmax_after", pos),
            want=(R.EXIT_OPT_COND if hit else 0, not hit))
        # max|d t| <= (float)tolerance_change: the element moves past a fixed tolerance, and the tolerance past fl(3 * 0.1f)
        add(f"dt_value_{pos}", [_planted(d=_near(2.0 ** -20, pos), tolerance_change=2.0 ** -20, g=4.0)], triple=("dt_value", pos),
            want=(R.EXIT_SMALL_STEP if hit else 0, not hit))
        p = float(F32(3.0) * F32(0.1))
        inv = {"below": "above", "at": "at", "above": "below"}[pos]      # the tolerance just above <=> the quantity just below
        add(f"dt_product_{pos}", [_planted(d=3.0, t=f32(0.1), g=4.0, tolerance_change=_near(p, inv))], triple=("dt_product", pos),
            want=(R.EXIT_SMALL_STEP if hit else 0, not hit))
        # |loss - prev_loss| < tolerance_change in double: 2^-10 against the doubles next to 2^-10 (their fp32 form is 2^-10 all three)
        s = _planted(tolerance_change=_near(2.0 ** -10, inv, F64), prev_loss=1.0)
        s["loss"] = F32(1.0 + 2.0 ** -10)
        add(f"loss_{pos}", [s], triple=("loss", pos), want=(R.EXIT_NO_PROGRESS if pos == "below" else 0, pos != "below"))
        # ys > 1e-10f: update against skip
        add(f"ys_{pos}", [_planted(g=_near(1e-10, pos))], triple=("ys", pos), want=(0, pos == "above"))
        # g.d > -(float)tolerance_change at n_iter == 1: g.d = -2^-20 exactly
        add(f"gtd_{pos}", [_start(2.0 ** -10, tolerance_change=_near(2.0 ** -20, pos))], triple=("gtd", pos),
            want=(R.EXIT_GTD if pos == "above" else 0, False))
    # a tolerance_change that is no fp32 number; the quantity lies between its two forms, so the form decides
    add("formats_dt", [_planted(d=2.0 ** -20, g=4.0, tolerance_change=2.0 ** -20 * (1 - 2.0 ** -30))], formats=True, want=(R.EXIT_SMALL_STEP, False))
    add("formats_gtd", [_start(2.0 ** -10, tolerance_change=2.0 ** -20 * (1 + 2.0 ** -30))], formats=True, want=(0, False))
    s = _planted(tolerance_change=2.0 ** -20 * (1 + 2.0 ** -30), prev_loss=2.0 ** -20 * (1 + 2.0 ** -31))
    s["loss"] = F32(0.0)
    add("formats_loss", [s], formats=True, want=(R.EXIT_NO_PROGRESS, False))
    # counter-driven exits: the order of the chain
    add("max_eval_with_opt_cond", [_planted(g=0.5, tolerance_grad=0.75, evals_in_step=24, max_eval=25)], want=(R.EXIT_MAX_EVAL, False))
    add("max_iter_before_max_eval", [_planted(g=0.5, tolerance_grad=0.75, evals_in_step=24, max_eval=25, iter_in_step=20)], want=(R.EXIT_MAX_ITER, False))
    add("max_iter_at_move_last_step", [_planted(iter_in_step=19, steps=4)], want=(R.EXIT_MAX_ITER, True))
    add("max_iter_at_move", [_planted(iter_in_step=19, steps=2)], want=(R.EXIT_MAX_ITER, True))
    add("max_iter_at_first_move", [_start(0.5, max_iter=1, n_steps=1)], want=(R.EXIT_MAX_ITER, False))
    add("one_unknown", [_planted(n=1)], want=(0, True))
    # frozen problems: every bit stays
    add("frozen_done", [_planted(done=1)], want=(0, False))
    add("frozen_history_0", [_planted(history_size=0)], want=(0, False))
    add("frozen_history_above_cap", [_planted(history_size=4)], want=(0, False))
    return out


# ---- random snapshots ----------------------------------------------------------------------------------------------------------------
def _spd(n, rng, cond):
    v = rng.standard_normal(n)
    v /= np.linalg.norm(v)
    dd = np.exp(rng.uniform(0.0, np.log(cond), n))
    refl = lambda s: s - 2.0 * v * float(v @ s)
    return lambda s: refl(dd * refl(s))


def random_snap(n, geom, seed, skip=False, t=0.1, cond=100.0):
    """phase AFTER_MOVE, n_iter >= 2: the launch forms a pair (skip: y.s < 0, none), runs the recursion over the ring and moves."""
    hs, cap, length, head = geom
    rng = np.random.default_rng(seed)
    A = _spd(n, rng, cond)
    s = blank(n, cap, history_size=hs, hist_len=length, hist_head=head, n_iter=length + 4, t=f32(t))
    for k in R.ring_slots(head, length, hs):
        sk = (rng.standard_normal(n) * 0.1).astype(F32)
        yk = A(sk.astype(F64)).astype(F32)
        s["S"][k], s["Y"][k] = sk, yk
        s["rho"][k] = F32(1.0) / F32(float(sk.astype(F64) @ yk.astype(F64)))
    pg = rng.standard_normal(n).astype(F32)
    d = rng.standard_normal(n).astype(F32)
    step = A(d.astype(F64) * f32(t))
    s["grad"] = (pg.astype(F64) + (-1e-3 * step if skip else step)).astype(F32)
    s["prev_grad"], s["d"] = pg, d
    s["x"] = rng.standard_normal(n).astype(F32)
    s["loss"] = F32(1.5)
    return s


def first_snap(n, seed, l1, cap=3, hs=3):
    """n_iter == 1 with |g|_1 = l1 (about): below 1 the first step length is lr, above 1 it is lr / |g|_1.  A stale ring position."""
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(n)
    g *= l1 / np.abs(g).sum()
    s = _start(0.0, n=n, cap=cap, history_size=hs, lr=f32(0.1), tolerance_grad=f32(1e-7), tolerance_change=1e-9, hist_len=2, hist_head=1)
    s["grad"] = g.astype(F32)
    s["x"] = rng.standard_normal(n).astype(F32)
    return s


def done_snap(n, geom, seed):
    s = random_snap(n, geom, seed)
    s["state"]["done"] = 1
    return s


def random_cases():
    out = []
    i = 0
    for n in NS:
        for g in (GEOMS[i % len(GEOMS)], GEOMS[(i + 5) % len(GEOMS)]):
            out.append(case(f"rand_n{n}_h{g[0]}of{g[1]}_len{g[2]}_head{g[3]}", [random_snap(n, g, 100 + i)], PADS[i % 3], PADS[(i // 3) % 3], i % 2))
            i += 1
        for l1 in (0.25, 3.0):
            out.append(case(f"first_n{n}_l1_{l1}", [first_snap(n, 200 + i, l1)], PADS[(i + 1) % 3], PADS[i % 3], (i + 1) % 2))
            i += 1
    for g in GEOMS:     # every ring geometry at two waves, the second one partial
        out.append(case(f"rand_n65_h{g[0]}of{g[1]}_len{g[2]}_head{g[3]}", [random_snap(65, g, 300 + i)], PADS[i % 3], PADS[(i + 1) % 3], i % 2))
        i += 1
    for length in range(3, 19):     # the lengths a run of 18 iterations passes through
        g = (100, 100, length, 0)
        out.append(case(f"rand_n64_h100_len{length}", [random_snap(64, g, 400 + i)]))
        i += 1
    out.append(case("rand_n8_h1024_len1024", [random_snap(8, BIG_RING, 500, cond=1.05)], 1, 13, 1))
    out.append(case("rand_n8_h1024_len1023", [random_snap(8, (1024, 1024, 1023, 0), 501, cond=1.05)]))
    out.append(case("rand_skip_n65_len2", [random_snap(65, (5, 5, 2, 3), 502, skip=True)], 13, 1, 1))
    out.append(case("rand_skip_n4097_full", [random_snap(4097, (5, 5, 5, 2), 503, skip=True)]))
    out.append(case("rand_t_n257", [random_snap(257, (5, 5, 5, 4), 504, t=0.037)], 1, 0, 1))
    # launches whose problems take different branches
    full, wrap = (5, 7, 5, 2), (5, 7, 5, 4)
    out.append(case("multi_J2_n65", [random_snap(65, wrap, 600), done_snap(65, full, 601)], 13, 1, 1))
    out.append(case("multi_J2_n4097", [done_snap(4097, full, 602), random_snap(4097, wrap, 603)], 1, 13, 1))

    def hs_of(s, hs):
        s["state"]["history_size"] = hs
        return s

    def mixed(n, seed, J):
        ps = [done_snap(n, full, seed), first_snap(n, seed + 1, 0.25, 7, 5), random_snap(n, (5, 7, 2, 1), seed + 2, skip=True), random_snap(n, wrap, seed + 3),
              random_snap(n, (5, 7, 2, 3), seed + 4), first_snap(n, seed + 5, 3.0, 7, 7), hs_of(random_snap(n, full, seed + 6), 8),
              random_snap(n, (3, 7, 3, 1), seed + 7)]
        return ps[:J]

    out.append(case("multi_J5_n257", mixed(257, 610, 5), 13, 13, 1))
    out.append(case("multi_J8_n1000", mixed(1000, 620, 8), 1, 1, 0))
    out.append(case("multi_J8_n63", mixed(63, 630, 8), 0, 13, 1))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(planted_cases() + random_cases())


def case_id(c):
    return c["name"]


# ---- torch's evaluation of the same launch ----------------------------------------------------------------------------------------
def to_torch(snap, dtype):
    """(ReferenceState, loss, grad, x) of lbfgs._advance_one holding the snapshot: old_dirs / old_stps / ro in ring order from hist_head."""
    s = snap["state"]
    T = lambda a: torch.tensor(np.asarray(a, F64), dtype=dtype)
    st = LB.ReferenceState(s["lr"], s["max_iter"], s["max_eval"], s["tolerance_grad"], s["tolerance_change"], s["history_size"], s["n_steps"])
    for k in LB.COUNTERS:
        if k != "hist_len":
            setattr(st, k, s[k])
    if s["n_iter"] >= 1:
        slots = R.ring_slots(s["hist_head"], s["hist_len"], s["history_size"])
        st.old_dirs = [T(snap["Y"][k]) for k in slots]
        st.old_stps = [T(snap["S"][k]) for k in slots]
        st.ro = [T(snap["rho"][k]) for k in slots]
        st.d, st.prev_flat_grad = T(snap["d"]), T(snap["prev_grad"])
        st.t, st.H_diag, st.prev_loss = float(s["t"]), T(s["h_diag"]), float(s["prev_loss"])
    return st, float(snap["loss"]), T(snap["grad"]), T(snap["x"])


def torch_advance(snap, dtype):
    st, loss, g, x = to_torch(snap, dtype)
    LB._advance_one(st, loss, g, x)
    return st, x


def is_arith(snap, E):
    """A launch whose d comes out of the recursion and whose x moves: what the budgets are measured on."""
    return E.body and E.d_exact is None and E.moved


@functools.lru_cache(maxsize=None)
def budgets():
    """{hist_len: (d budget, x budget, torch's d error, torch's x error)} in ulps of the magnitudes: 4 x the largest error of torch's
    CPU fp32 _advance_one against the float64 reference on the same snapshot, at least 2, over the random cases of that length."""
    worst = {}
    for c in cases():
        for snap in c["snaps"]:
            e = torch_error(snap)
            if e is not None:
                w = worst.setdefault(e[0], [0.0, 0.0])
                w[0], w[1] = max(w[0], e[1]), max(w[1], e[2])
    return {k: (max(2.0, 4 * d), max(2.0, 4 * x), d, x) for k, (d, x) in sorted(worst.items())}


def torch_error(snap):
    """(hist_len in the recursion, d error, x error) of torch's CPU fp32 _advance_one against the float64 reference, or None."""
    E = R.advance(snap)
    if not is_arith(snap, E):
        return None
    st, x = torch_advance(snap, torch.float32)
    b = E.branches[0]
    return E.length, float(R.ulps(st.d.numpy(), b.d, b.M).max()), float(R.ulps(x.numpy(), b.x, b.xmag).max())


def budget_for(length, snap=None):
    """(d, x) budgets of a launch that runs the recursion over `length` pairs: the table's entry of that length (of the next longer one
    where the table has none); with `snap`, a launch of a real run, no less than 4 x torch's error on that very snapshot."""
    tab = budgets()
    keys = [k for k in tab if k >= length] or [max(tab)]
    d, x = tab[min(keys)][:2]
    if snap is not None:
        e = torch_error(snap)
        if e is not None:
            d, x = max(d, 4 * e[1]), max(x, 4 * e[2])
    return d, x


def simulate(snap, E, branch=0, dtype=F32):
    """The read-back of a launch that computes what the reference's branch says, d and x rounded to `dtype` once."""
    out = dict(snap)
    for k in ("x", "d", "prev_grad", "S", "Y", "rho"):
        out[k] = np.array(snap[k], dtype)
    st = dict(snap["state"])
    b = E.branches[branch]
    st.update(b.ints)
    if E.body:
        st["t"], st["h_diag"], st["prev_loss"] = b.t, b.h_diag, E.prev_loss
        out["prev_grad"] = np.array(snap["grad"], dtype)
        out["d"] = b.d.astype(dtype)
        if E.updated:
            out["S"][E.slot], out["Y"][E.slot], out["rho"][E.slot] = E.S_slot, E.Y_slot, b.rho_new
        if b.x is not None:     # from the d it stored, as a device does
            out["x"] = (np.asarray(snap["x"], F64) + b.t * out["d"].astype(F64)).astype(dtype)
    out["state"] = st
    return out

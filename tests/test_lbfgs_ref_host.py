"""The reference side of tests/test_hip_lbfgs_kernel.py, on the CPU: tests/lbfgs_ref.py (one launch of sg_lbfgs_advance_kernel in numpy)
against lbfgs._advance_one in torch float64 from the same snapshot (all integers equal, vectors to 1e-12), launch by launch along the ten
trajectories of tests/test_lbfgs_host.py against torch.optim.LBFGS (the chain torch -> _advance_one -> lbfgs_ref), the hand-derived
decisions of the planted cases, the coverage of the case table, the condition that no random case has an ambiguous decision under the
reference's own intervals (cap: 0 cases), the budgets (printed: torch's CPU kernels differ between hosts) and the comparison itself,
held to a simulated device that is right and to ones that are wrong.  DESIGN.md R39."""
import numpy as np
import pytest
import torch

import lbfgs_cases as K
import lbfgs_ref as R
import test_lbfgs_host as H
from supervised_gan_amd import lbfgs as LB

F64 = np.float64


def test_constants_are_the_header_s():
    assert (R.PHASE_START, R.PHASE_AFTER_MOVE) == (LB.PHASE_START, LB.PHASE_AFTER_MOVE)
    assert (R.EXIT_NONE, R.EXIT_OPT_START, R.EXIT_GTD, R.EXIT_MAX_ITER, R.EXIT_MAX_EVAL, R.EXIT_OPT_COND, R.EXIT_SMALL_STEP, R.EXIT_NO_PROGRESS) == (
        LB.EXIT_NONE, LB.EXIT_OPT_START, LB.EXIT_GTD, LB.EXIT_MAX_ITER, LB.EXIT_MAX_EVAL, LB.EXIT_OPT_COND, LB.EXIT_SMALL_STEP, LB.EXIT_NO_PROGRESS)
    fields = [f[0] for f in LB.LbfgsState._fields_]
    assert set(R.HYPER + R.INTS + ("reserved0", "reserved", "t", "h_diag", "prev_loss")) == set(fields)
    assert set(LB.COUNTERS) <= set(R.INTS)


def _close(a, b, what):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    assert a.shape == b.shape, what
    err = float(np.abs(a - b).max()) if a.size else 0.0
    assert err <= 1e-12 * max(1.0, float(np.abs(b).max()) if b.size else 0.0), (what, err)


def _held_to_torch(snap, cap, E, st, x, what):
    """E = advance(snap, exact=True) against the ReferenceState `st` and iterate `x` that _advance_one left from the same snapshot."""
    s = snap["state"]
    assert len(E.branches) == 1 and not E.ambiguous, what
    b = E.branches[0]
    for k in LB.COUNTERS:
        assert int(getattr(st, k)) == b.ints[k], (what, k, int(getattr(st, k)), b.ints[k])
    if E.frozen:
        assert np.array_equal(x.numpy(), np.asarray(snap["x"], F64))
        return
    after = K.simulate(snap, E, dtype=F64)
    _close(after["x"], x.numpy(), what + " x")
    if E.body:
        _close(after["d"], st.d.numpy(), what + " d")
        _close(after["prev_grad"], st.prev_flat_grad.numpy(), what + " prev_grad")
        _close(b.t, float(st.t), what + " t")
        _close(b.h_diag, float(st.H_diag), what + " h_diag")
        assert E.prev_loss == st.prev_loss, what
        slots = R.ring_slots(E.head, E.length, s["history_size"])
        assert len(slots) == len(st.old_dirs) == len(st.ro)
        for k, r in enumerate(slots):
            _close(after["S"][r], st.old_stps[k].numpy(), f"{what} S[{r}]")
            _close(after["Y"][r], st.old_dirs[k].numpy(), f"{what} Y[{r}]")
            rel = abs(float(after["rho"][r]) - float(st.ro[k])) / abs(float(st.ro[k]))
            assert rel <= 1e-12, (what, r, rel)


@pytest.mark.parametrize("c", K.cases(), ids=K.case_id)
def test_reference_matches_advance_one_in_float64(c):
    for j, snap in enumerate(c["snaps"]):
        what = f"{c['name']}[{j}]"
        E = R.advance(snap, exact=True)
        s = snap["state"]
        if not s["done"] and not 1 <= s["history_size"] <= c["cap"]:
            assert E.frozen, what       # the kernel's refusal; _advance_one has no history_cap
            continue
        st, x = K.torch_advance(snap, torch.float64)
        _held_to_torch(snap, c["cap"], E, st, x, what)


# ---- launch by launch along the trajectories of test_lbfgs_host.py -----------------------------------------------------------------
def _snapshot_of(st, loss, g, x):
    """The snapshot that holds a ReferenceState: the ring in torch's list order, so hist_head is 0."""
    n, hs = x.numel(), st.history_size
    fresh = st.d is None
    s = K.blank(n, hs, lr=st.lr, max_iter=st.max_iter, max_eval=st.max_eval, tolerance_grad=st.tolerance_grad, tolerance_change=st.tolerance_change,
                history_size=hs, n_steps=st.n_steps, hist_len=st.hist_len, hist_head=0, t=0.0 if fresh else float(st.t),
                h_diag=1.0 if fresh else float(st.H_diag), prev_loss=0.0 if fresh else st.prev_loss,
                **{k: int(getattr(st, k)) for k in LB.COUNTERS if k != "hist_len"})
    for k in ("d", "prev_grad", "S", "Y", "rho"):
        s[k] = s[k].astype(F64)
    s["x"], s["grad"], s["loss"] = x.numpy().copy(), g.numpy().copy(), float(loss)
    if not fresh:
        s["d"], s["prev_grad"] = st.d.numpy().copy(), st.prev_flat_grad.numpy().copy()
        for k in range(st.hist_len):
            s["S"][k], s["Y"][k], s["rho"][k] = st.old_stps[k].numpy(), st.old_dirs[k].numpy(), float(st.ro[k])
    return s


@pytest.mark.parametrize("name", sorted(H.CASES))
def test_reference_follows_torch_lbfgs_launch_by_launch(name):
    """torch.optim.LBFGS -> _advance_one at every step boundary (1e-12, as tests/test_lbfgs_host.py holds it) and _advance_one ->
    lbfgs_ref at EVERY launch, each from the snapshot of the state _advance_one is in: a free run of the reference would compound the
    1e-16 between math.fsum and torch's dot through Rosenbrock's own sensitivity (1.7e-7 after 80 launches of history_wrap)."""
    kind, n, n_steps, kw, must_exit = H.CASES[name]
    for seed in (0, 1):
        f = H._problem(kind, n, seed)
        x0 = torch.randn(n, generator=torch.Generator().manual_seed(10 + seed), dtype=torch.float64) * 0.5
        k_ = dict(kw)
        max_iter = k_.pop("max_iter", 20)
        st = LB.ReferenceState(k_.pop("lr", 1), max_iter, LB._default_max_eval(max_iter, k_.pop("max_eval", None)), k_.pop("tolerance_grad", 1e-7),
                               k_.pop("tolerance_change", 1e-9), k_.pop("history_size", 100), n_steps)
        assert not k_
        x = x0.clone()
        xs, exits, calls = [], set(), 0
        while not st.done:
            v, g = H.value_and_grad(f, x)
            snap = _snapshot_of(st, v, g, x)
            E = R.advance(snap, exact=True)
            before = st.steps
            LB._advance_one(st, v, g, x)
            _held_to_torch(snap, st.history_size, E, st, x, f"{name}[{seed}] launch {calls}")
            if st.steps > before:
                assert E.ints["last_exit"] == st.last_exit
                xs.append(x.clone())
                exits.add(st.last_exit)
            calls += 1
            assert calls < 100000
        xs_t, func_evals, n_iter = H.run_torch(f, x0, n_steps, **kw)
        assert len(xs) == n_steps
        for k, (a, b) in enumerate(zip(xs, xs_t)):
            err = float((a - b).abs().max())
            assert err <= 1e-12 * max(1.0, float(b.abs().max())), (name, seed, k, err)
        assert (st.func_evals, st.n_iter) == (func_evals, n_iter)
        assert must_exit <= exits, (name, seed, exits)
        if kw.get("history_size") == 3:
            assert st.hist_len == 3 and st.n_iter > 4


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
def _expectations():
    return [(c, j, s, R.advance(s)) for c in K.cases() for j, s in enumerate(c["snaps"])]


def test_planted_cases_decide_as_derived_by_hand():
    sides = {}
    for c in K.cases():
        if c["want"] is None:
            continue
        E = R.advance(c["snaps"][0])
        assert not E.ambiguous and len(E.branches) == 1, c["name"]
        assert (E.code, E.updated) == c["want"], (c["name"], E.code, E.updated, c["want"])
        if c["name"].startswith("frozen"):
            assert E.frozen
        if c["name"].startswith("ys_") and not E.updated:
            assert E.ints["n_skipped"] == c["snaps"][0]["state"]["n_skipped"] + 1 and E.branches[0].h_diag == c["snaps"][0]["state"]["h_diag"]
        if c["triple"]:
            sides.setdefault(c["triple"][0], {})[c["triple"][1]] = (E.code, E.updated)
        if c["formats"]:        # the fp32 form of tolerance_change decides the |d t| and g.d tests: all-double takes the other side
            assert (R.advance(c["snaps"][0], exact=True).code != E.code) == (c["name"] != "formats_loss"), c["name"]
    assert set(sides) == {"gmax_start", "gmax_after", "dt_value", "dt_product", "loss", "ys", "gtd"}
    for name, s in sides.items():
        assert set(s) == set(K.TRIPLE) and s["below"] != s["above"], (name, s)
        assert s["at"] in (s["below"], s["above"])
    last = [c for c in K.cases() if c["name"] in ("max_iter_at_move_last_step", "max_iter_at_move")]
    assert [R.advance(c["snaps"][0]).ints["done"] for c in last] == [1, 0]


def test_case_table_covers_what_the_issue_lists():
    ex = _expectations()
    cs = K.cases()
    assert {E.code for _, _, _, E in ex} | {0} == set(range(len(LB.EXIT_NAMES)))
    assert {s["state"]["phase"] for _, _, s, E in ex if not E.frozen} == {R.PHASE_START, R.PHASE_AFTER_MOVE}
    assert {c["n"] <= 4096 for c in cs} == {True, False}
    rnd = [c for c in cs if c["want"] is None]
    assert set(K.NS) <= {c["n"] for c in rnd} and set(K.JS) == {c["J"] for c in cs}
    assert {c["x_ld"] - c["n"] for c in rnd} == set(K.PADS) == {c["g_ld"] - c["n"] for c in rnd}
    assert {c["off"] for c in rnd} == {0, 1}
    assert {(c["x_ld"] - c["n"], c["g_ld"] - c["n"]) for c in rnd} >= {(0, 0), (1, 13), (13, 1), (0, 13), (13, 0)}
    geoms = {(s["state"]["history_size"], c["cap"], s["state"]["hist_len"], s["state"]["hist_head"]) for c, _, s, E in ex if K.is_arith(s, E)}
    assert set(K.GEOMS) | {K.BIG_RING} <= geoms
    for hs, cap, length, head in K.GEOMS:
        assert 0 <= head < hs <= cap and length <= hs
    full = {(hs, head) for hs, cap, length, head in geoms if length == hs and hs == 5}
    assert {(5, 0), (5, 2), (5, 4)} <= full                                              # the wrap: head first, middle, last
    assert {0, 1, 2, 4} <= {length for hs, _, length, _ in geoms if hs == 5}            # 0, 1, 2, history_size - 1
    assert {(3, 7), (100, 128)} <= {(hs, cap) for hs, cap, _, _ in geoms} and 1 in {hs for hs, _, _, _ in geoms}
    first = [E for _, _, s, E in ex if E.d_exact is not None and s["state"]["lr"] == K.f32(0.1)]
    arms = {E.branches[0].t == K.f32(0.1) for E in first}
    assert arms == {True, False}, "both arms of min(1, 1 / |g|_1)"
    multi = [c for c in cs if c["J"] > 1]
    for J in (5, 8):
        kinds = set()
        for c in multi:
            if c["J"] != J:
                continue
            for s in c["snaps"]:
                E = R.advance(s)
                kinds.add("done" if s["state"]["done"] else "start" if s["state"]["phase"] == R.PHASE_START else "skip" if E.body and not E.updated
                          else "wrap" if E.updated and s["state"]["hist_len"] == s["state"]["history_size"] else "other")
        assert {"done", "start", "skip", "wrap"} <= kinds, (J, kinds)
    assert any(c["n"] > 4096 and c["J"] > 1 for c in cs)
    assert any(E.updated is False and E.body and s["state"]["hist_len"] > 0 for _, _, s, E in ex), "a skip over a ring that holds pairs"


def test_no_random_case_has_an_ambiguous_decision():
    """Cap 0: every decision of every random case has one answer under the reference's own intervals (for a d budget of the table's
    largest).  Prints the share of launches whose fp32 scalars have two candidates: a fact about the inputs, no tolerance."""
    worst = max(b[0] for b in K.budgets().values())
    two = total = 0
    for c in K.cases():
        if c["want"] is not None:
            continue
        for j, s in enumerate(c["snaps"]):
            E = R.advance(s, d_ulps=worst)
            assert not E.ambiguous, (c["name"], j)
            if E.body:
                total += 1
                two += E.two_candidates
                assert all(np.isfinite(b.d).all() and (b.x is None or np.isfinite(b.x).all()) for b in E.branches), (c["name"], j)
                if E.updated:       # far from the thresholds: ys above 1e-10 and g.d below -tolerance_change by orders of magnitude
                    b = E.branches[0]
                    assert 1.0 / b.rho_new > 1e-7 and b.gtd + b.gtd_err < -1e-6, (c["name"], j, b.rho_new, b.gtd)
    print(f"fp32 scalars with two candidates: {two} of {total} launches that run the loop body ({two / total:.3f})")


def test_budgets_are_measured_on_torch():
    tab = K.budgets()
    assert {0, 1, 2, 3, 5, 18, 100, 1024} <= set(tab) | {0}
    for length, (d, x, td, tx) in tab.items():
        assert d >= 2.0 and x >= 2.0 and np.isfinite(d) and np.isfinite(x)
        print(f"hist_len {length:5d}: d budget {d:8.2f} ulp (torch {td:7.2f}), x budget {x:6.2f} ulp (torch {tx:5.2f})")


# ---- the comparison itself ---------------------------------------------------------------------------------------------------------------
def test_comparison_accepts_the_reference_and_refuses_wrong_launches():
    refused = 0
    for c, j, s, E in _expectations():
        what = f"{c['name']}[{j}]"
        d, x = K.budget_for(E.length)
        for k in range(len(E.branches)):
            good = K.simulate(s, E, k)
            assert R.compare(s, good, E, d, x, what)["branch"] == k
        if not K.is_arith(s, E):
            continue
        b = E.branches[0]
        i = int(np.argmax(b.M))
        wrongs = []
        w = K.simulate(s, E)
        w["d"][i] = np.float32(b.d[i] + (d + 2) * np.spacing(np.float32(b.M[i])))       # one element of d outside its budget
        wrongs.append(w)
        w = K.simulate(s, E)
        w["state"]["h_diag"] = float(np.nextafter(np.float32(b.h_diag), np.float32(0)))     # a scalar that is no candidate
        if all(np.float32(w["state"]["h_diag"]) != np.float32(o.h_diag) for o in E.branches):
            wrongs.append(w)
        w = K.simulate(s, E)
        other = (E.slot + 1) % c["cap"] if E.updated else 0
        w["S"][other][0] = 1.0      # a ring slot that is not the launch's
        wrongs.append(w)
        w = K.simulate(s, E)
        w["state"]["hist_head"] = (w["state"]["hist_head"] + 1) % s["state"]["history_size"] if s["state"]["history_size"] > 1 else 1
        wrongs.append(w)
        for w in wrongs:
            with pytest.raises(AssertionError):
                R.compare(s, w, E, d, x, what)
            refused += 1
    assert refused > 100

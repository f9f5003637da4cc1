"""sg_lbfgs_advance_kernel (csrc/sgan_lbfgs.hip) against tests/lbfgs_ref.py, ONE launch at a time.  tests/test_hip_lbfgs.py judges the
kernel through whole trajectories of a benign closure against fp32 torch on the same device (1e-5 of a row's largest element, at step
boundaries) and is unchanged; here every launch starts from a snapshot built on the host (tests/lbfgs_cases.py) or copied from the
device just before it, and everything the launch may and may not write is read back and held to the reference's expectation of that
snapshot: integers and decisions exactly, (rho[slot], h_diag, t) as one of the consistent candidate tuples to the bit, the new ring
slot, prev_grad and the first d to the bit, d and x within budgets in ulps of each element's magnitude (measured on torch's CPU fp32
_advance_one when the test runs, never on a kernel), exact zeros where the magnitude is 0.  The rules stand in lbfgs_ref's docstring;
tests/test_lbfgs_ref_host.py holds the reference side; DESIGN.md R39 has the budgets beside the kernel's own errors.

Storage: every operand lies in an allocation filled with NaN (the state's reserved words: a bit pattern) that ends in a guard band;
x and grad in rows of n, n + 1 and n + 13 with bases one float into their allocations; ring slots outside the live pairs, the slots
behind history_size, and d / prev_grad before the first iteration hold NaN.  After the launch: every ring slot and rho but the written
one, the row tails, grad, loss, the hyperparameters, the reserved words and the guards have their bits, a done problem and one with
history_size outside [1, history_cap] every bit of state and buffers.  Every case runs twice from the same snapshot with equal bits
everywhere (the kernel has no atomics).

Teacher-forced runs: DeviceLBFGS through 3 steps of max_iter 6 at history_size 3 and 100 on the quartic closure of
tests/test_hip_lbfgs.py, a non-separable SPD quadratic 0.5 (x - c)' A (x - c) of condition 100 and Rosenbrock (n = 64, lr 0.2); the
device's state and buffers are copied before every launch and the launch is held to lbfgs_ref.advance of that copy, so no trajectory
error accumulates and states nobody planted get checked (the wrap, a skip if one occurs).  A launch with an ambiguous decision is
counted and skipped: at most 2 % of a run.

That the file can fail: DESIGN.md R39 lists the one-line changes to a scratch copy of sgan_lbfgs.hip and the cases that fail for each.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import lbfgs_cases as K
import lbfgs_ref as R
from hip_utils import GUARD, _guard_intact, _guarded
from supervised_gan_amd import lbfgs as LB
from test_hip_lbfgs import closure_into, curvature, x0

pytestmark = pytest.mark.gpu

STATE_BYTES = C.sizeof(LB.LbfgsState)
FIGURES = {}        # hist_len -> [kernel's largest d error, x error] over the case table, printed by the last test


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import _lib, ops
    _lib.lib()
    return ops


def _state_raw(st):
    s = LB.LbfgsState()
    for k, v in st.items():
        if k == "reserved":
            for i, w in enumerate(v):
                s.reserved[i] = w
        else:
            setattr(s, k, v)
    return bytes(s)


def _state_dict(raw):
    s = LB.LbfgsState.from_buffer_copy(raw)
    out = {f[0]: getattr(s, f[0]) for f in LB.LbfgsState._fields_}
    out["reserved"] = list(s.reserved)
    return out


class Storage:
    """The device operands of one launch, each in a NaN-filled allocation that ends in a guard band."""

    def __init__(self, c):
        self.c = c
        J, n, cap, off = c["J"], c["n"], c["cap"], c["off"]
        snaps = c["snaps"]
        self.flat, self.guard, self.host = {}, {}, {}

        def put(name, host):
            self.host[name] = host.copy()
            self.flat[name], self.guard[name] = _guarded(torch.from_numpy(host))

        put("state", np.frombuffer(b"".join(_state_raw(s["state"]) for s in snaps), np.float32).copy())
        for name, key, ld in (("x", "x", c["x_ld"]), ("grad", "grad", c["g_ld"])):
            h = np.full(off + J * ld, np.nan, np.float32)
            h[off:].reshape(J, ld)[:, :n] = np.stack([s[key] for s in snaps])
            put(name, h)
        put("loss", np.array([s["loss"] for s in snaps], np.float32))
        for name, key in (("d", "d"), ("prev_grad", "prev_grad"), ("S", "S"), ("Y", "Y"), ("rho", "rho")):
            put(name, np.stack([s[key] for s in snaps]).astype(np.float32).reshape(-1))
        f = self.flat
        self.state = f["state"].view(torch.uint8).view(J, STATE_BYTES)
        self.x = f["x"][off:].view(J, c["x_ld"])[:, :n]
        self.grad = f["grad"][off:].view(J, c["g_ld"])[:, :n]
        self.args = (self.state, J, n, self.x, self.grad, f["loss"], f["d"].view(J, n), f["prev_grad"].view(J, n), f["S"].view(J, cap, n),
                     f["Y"].view(J, cap, n), f["rho"].view(J, cap))

    def read(self):
        torch.cuda.synchronize()
        for k, g in self.guard.items():
            assert _guard_intact(g), f"{self.c['name']}: the guard behind {k} was written"
        return {k: v.cpu().numpy().copy() for k, v in self.flat.items()}

    def afters(self, back):
        """The read-back as one snapshot-shaped dict per problem, after the checks on what lies between and behind the problems."""
        c = self.c
        J, n, cap, off = c["J"], c["n"], c["cap"], c["off"]
        bits = lambda a: a.view(np.int32)
        for k in ("grad", "loss"):
            assert np.array_equal(bits(back[k]), bits(self.host[k])), f"{c['name']}: {k} was written"
        xr, x0_ = back["x"][off:].reshape(J, c["x_ld"]), self.host["x"][off:].reshape(J, c["x_ld"])
        assert np.array_equal(bits(back["x"][:off]), bits(self.host["x"][:off])), f"{c['name']}: written in front of x"
        assert np.array_equal(bits(np.ascontiguousarray(xr[:, n:])), bits(np.ascontiguousarray(x0_[:, n:]))), f"{c['name']}: a row tail of x was written"
        out = []
        for j, s in enumerate(c["snaps"]):
            out.append(dict(state=_state_dict(back["state"].tobytes()[j * STATE_BYTES:(j + 1) * STATE_BYTES]), x=xr[j, :n].copy(),
                            d=back["d"].reshape(J, n)[j], prev_grad=back["prev_grad"].reshape(J, n)[j], S=back["S"].reshape(J, cap, n)[j],
                            Y=back["Y"].reshape(J, cap, n)[j], rho=back["rho"].reshape(J, cap)[j]))
        return out


def _same_everywhere(a, b, what):
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), f"{what}: the second run's {k} differs"


def _note(E, fig):
    f = FIGURES.setdefault(E.length, [0.0, 0.0])
    f[0], f[1] = max(f[0], fig["d"]), max(f[1], fig["x"])


def _hold(c, afters, label=""):
    for j, (s, a) in enumerate(zip(c["snaps"], afters)):
        what = f"{c['name']}[{j}]{label}"
        E = R.advance(s)
        db, xb = K.budget_for(E.length)
        fig = R.compare(s, a, E, db, xb, what)
        if K.is_arith(s, E):
            _note(E, fig)
            print(f"{what}: len {E.length}, d {fig['d']:.2f} of {db:.2f} ulp, x {fig['x']:.2f} of {xb:.2f} ulp, tuple {fig['branch']} of {len(E.branches)}")


@pytest.mark.parametrize("c", K.cases(), ids=K.case_id)
def test_one_launch(ops, c):
    runs = []
    for _ in range(2):
        st = Storage(c)
        ops.lbfgs_advance(*st.args)
        runs.append(st.read())
    _same_everywhere(runs[0], runs[1], c["name"])
    _hold(c, st.afters(runs[0]))


def _abi(ops, st, **over):
    from supervised_gan_amd import _lib
    c, f = st.c, st.flat
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    a = dict(state=st.state, J=c["J"], n=c["n"], x=st.x, x_ld=c["x_ld"], grad=st.grad, g_ld=c["g_ld"], loss=f["loss"], d=f["d"], prev_grad=f["prev_grad"],
             hist_s=f["S"], hist_y=f["Y"], hist_rho=f["rho"], history_cap=c["cap"])
    a.update(over)
    ptr = ("state", "x", "grad", "loss", "d", "prev_grad", "hist_s", "hist_y", "hist_rho")
    return _lib.lib().sgan_lbfgs_advance(*[P(a[k]) if k in ptr else a[k] for k in
                                           ("state", "J", "n", "x", "x_ld", "grad", "g_ld", "loss", "d", "prev_grad", "hist_s", "hist_y", "hist_rho", "history_cap")],
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))


def test_c_abi_refusals_launch_nothing(ops):
    """The C ABI driven directly: a good call has the wrapper's bits; a call with a null pointer, J of 0 or 9, a row stride below n or
    a history_cap of 0 or 1025 returns an error and leaves every bit of every operand."""
    c = next(k for k in K.cases() if k["name"] == "multi_J2_n65")
    st = Storage(c)
    ops.lbfgs_advance(*st.args)
    want = st.read()
    st = Storage(c)
    assert _abi(ops, st) == 0
    _same_everywhere(want, st.read(), "the direct call")
    bad = [{k: None} for k in ("state", "x", "grad", "loss", "d", "prev_grad", "hist_s", "hist_y", "hist_rho")]
    bad += [dict(J=0), dict(J=9), dict(J=-1), dict(x_ld=c["n"] - 1), dict(g_ld=c["n"] - 1), dict(n=0), dict(history_cap=0), dict(history_cap=1025)]
    for over in bad:
        st = Storage(c)
        assert _abi(ops, st, **over) != 0, over
        back = st.read()
        for k in back:
            assert np.array_equal(back[k].view(np.int32), st.host[k].view(np.int32)), (over, k, "a refused call wrote")


# ---- teacher-forced runs -------------------------------------------------------------------------------------------------------------
def _spd_quadratic(J, n, seed):
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (q * np.exp(rng.uniform(0.0, np.log(100.0), n))) @ q.T
    A = torch.tensor(0.5 * (A + A.T), dtype=torch.float32, device="cuda")
    c = torch.tensor(rng.standard_normal((J, n)), dtype=torch.float32, device="cuda")

    def closure(x, loss, grad):
        r = x - c
        grad.copy_(r @ A)
        loss.copy_(0.5 * (r * grad).sum(1))

    return closure


def _rosenbrock(x, loss, grad):
    a, b = x[:, :-1], x[:, 1:]
    u = b - a * a
    loss.copy_((100 * u * u + (1 - a) * (1 - a)).sum(1))
    grad.zero_()
    grad[:, :-1] += -400 * a * u - 2 * (1 - a)
    grad[:, 1:] += 200 * u


def _randn(J, n, seed, scale):
    return (torch.randn(J, n, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def _runs():
    out = {}
    for hs in (3, 100):
        out[f"quartic_h{hs}"] = (2, 200, dict(lr=0.1, history_size=hs), lambda J, n: (lambda x, l, g, dd=curvature(J, n): closure_into(x, l, g, dd)), lambda J, n: x0(J, n))
        out[f"quadratic_h{hs}"] = (2, 96, dict(lr=0.5, history_size=hs), lambda J, n: _spd_quadratic(J, n, 7), lambda J, n: _randn(J, n, 8, 1.0))
        out[f"rosenbrock_h{hs}"] = (2, 64, dict(lr=0.2, history_size=hs), lambda J, n: _rosenbrock, lambda J, n: _randn(J, n, 9, 0.5))
    return out


RUNS = _runs()


@pytest.mark.parametrize("name", sorted(RUNS))
def test_teacher_forced_run(ops, name):
    J, n, kw, make, start = RUNS[name]
    closure, x = make(J, n), start(J, n)
    dev = LB.DeviceLBFGS(n, J, device="cuda", max_iter=6, n_steps=3, **kw)
    hs = dev.hyper["history_size"]
    loss, grad = torch.zeros(J, device="cuda"), torch.zeros(J, n, device="cuda")
    launches = skipped = wraps = skips = 0
    used = 0.0
    exits = set()

    def copy():
        raw = dev.state.cpu().numpy().tobytes()
        h = lambda t: t.cpu().numpy().copy()
        xs, gs, ls, d, pg, S, Y, rho = (h(t) for t in (x, grad, loss, dev.d, dev.prev_grad, dev.hist_s, dev.hist_y, dev.hist_rho))
        return [dict(state=_state_dict(raw[j * STATE_BYTES:(j + 1) * STATE_BYTES]), n=n, x=xs[j], grad=gs[j], loss=ls[j], d=d[j], prev_grad=pg[j],
                     S=S[j], Y=Y[j], rho=rho[j]) for j in range(J)]

    calls = 0
    while not all(dev.done()):
        closure(x, loss, grad)
        before = copy()
        dev.advance(loss, grad, x)
        after = copy()
        for j in range(J):
            what = f"{name}[{j}] launch {calls}"
            s, a = before[j], after[j]
            assert np.array_equal(a["grad"].view(np.int32), s["grad"].view(np.int32)) and a["loss"].tobytes() == s["loss"].tobytes(), what
            if s["state"]["done"]:
                R.compare(s, a, R.advance(s), 0.0, 0.0, what)
                continue
            launches += 1
            db, xb = K.budget_for(R.advance(s).length, s)
            E = R.advance(s, d_ulps=db)
            if E.ambiguous:
                skipped += 1
                continue
            fig = R.compare(s, a, E, db, xb, what)
            wraps += E.updated and s["state"]["hist_len"] == hs
            skips += E.body and E.n_iter > 1 and not E.updated
            if E.code:
                exits.add(E.code)
            if K.is_arith(s, E):
                used = max(used, fig["d"] / db, fig["x"] / xb)
        calls += 1
        assert calls < 200
    print(f"{name}: {launches} launches, {skipped} skipped as ambiguous, {wraps} at the wrap, {skips} memory updates skipped, exits {sorted(exits)}, "
          f"at most {used:.2f} of a launch's budget used")
    assert launches >= 3 * J and skipped <= 0.02 * launches, (launches, skipped)
    if hs == 3:
        assert wraps > 0, "no launch of the run reached the wrap"


def test_print_kernel_errors_beside_budgets(ops):
    """Runs last: the kernel's largest errors of this module beside the budgets, per history length."""
    tab = K.budgets()
    for length in sorted(FIGURES):
        d, x = FIGURES[length]
        db, xb = K.budget_for(length)
        print(f"hist_len {length:5d}: d {db:8.2f} / {d:6.2f} ulp, x {xb:6.2f} / {x:5.2f} ulp (budget / kernel){'' if length in tab else ' (the next longer entry)'}")

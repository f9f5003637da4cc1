"""ONE launch of sg_lbfgs_advance_kernel (csrc/sgan_lbfgs.hip) for ONE problem, in numpy: no torch, no device.

`advance(snapshot)` takes the state struct as a dict plus the fp32 arrays the kernel reads (x[n], grad[n], loss, d[n], prev_grad[n],
S[cap][n], Y[cap][n], rho[cap]) and returns an Expectation of everything the launch may and may not write.  The control flow is
lbfgs._advance_one line by line in the kernel's number formats: tolerance_grad, lr, t, h_diag and rho are fp32; tolerance_change is a
double in the loss test and its fp32 rounding in the |d t| and g.d tests; 1e-10 is fp32; prev_loss is a double.  With exact=True every
rounding is the identity and every comparison is made in double: that form is held to torch's float64 _advance_one to 1e-12
(tests/test_lbfgs_ref_host.py), the fp32 form is what the device is held to (tests/test_hip_lbfgs_kernel.py).  DESIGN.md R39.

Error model.
  * Integers and decisions are exact: every counter of lbfgs.COUNTERS, hist_head, the exit code, phase and done.
  * max|g| and max|d t| are order-free and exact (fl(d t) is one fp32 product).
  * ys, yy, |g|_1 and g.d at n_iter == 1 are ONE fp32 rounding of an fp64 sum of fp32 terms numpy reproduces to the bit (y = g - pg,
    s = d t and their products are one fp32 operation each, and no contraction can cross the conversion to double).  The terms are
    summed exactly (math.fsum); an fp64 sum in any order lies within (m - 1) 2^-53 sum|term| of that (m non-zero terms), so the fp32
    value is one candidate or two adjacent ones (`sum_candidates`).  For every candidate rho_new = fl(1 / ys), h_diag = fl(ys /
    fl(yy)) and t follow to the bit: the device's (rho[slot], h_diag, t) must be one of these consistent tuples (`Expectation.tuples`).
  * Vectors that are one fp32 operation per element are compared bit for bit: the new ring slot S[slot] = fl(d t),
    Y[slot] = fl(g - pg), prev_grad = g, and d = -g at n_iter == 1.
  * d after the two-loop recursion is computed in float64 from the ring as the device holds it (fp32 pairs, the tuple's rho_new and
    h_diag) with the magnitude M_i = h |g_i| + h sum_k |al_k| |y_k,i| + sum_k |al_k - be_k| |s_k,i|: every contribution in absolute
    value.  Errors are counted in fp32 ulps of M_i (`ulps`); where M_i is 0 the device's d_i must be 0.  x = x + t d has the
    magnitude |x| + |t d|.  The budgets are measured on torch's CPU fp32 _advance_one, never on a kernel (tests/lbfgs_cases.py).
  * g.d after the recursion inherits d's error: it is an interval (`gtd_err`, for a d budget of `d_ulps`), and a launch whose
    g.d > -tolerance_change decision the interval straddles is `ambiguous`, as is one whose candidates disagree on a decision.
"""
import math

import numpy as np

F32, F64 = np.float32, np.float64
PHASE_START, PHASE_AFTER_MOVE = 0, 1
EXIT_NONE, EXIT_OPT_START, EXIT_GTD, EXIT_MAX_ITER, EXIT_MAX_EVAL, EXIT_OPT_COND, EXIT_SMALL_STEP, EXIT_NO_PROGRESS = range(8)
HYPER = ("lr", "tolerance_grad", "tolerance_change", "max_iter", "max_eval", "history_size", "n_steps")
INTS = ("func_evals", "n_iter", "steps", "phase", "done", "iter_in_step", "evals_in_step", "hist_len", "hist_head", "last_exit", "n_skipped")
MIN_NORMAL = float(np.finfo(F32).tiny)


class _Fmt:
    """The kernel's fp32 operations (exact=False) or their float64 idealisation (exact=True); arrays come back as float64."""

    def __init__(self, exact):
        self.exact = exact

    def rnd(self, v):
        return float(v) if self.exact else float(F32(v))

    def _op(self, f, a, b):
        if self.exact:
            r = f(np.asarray(a, F64), np.asarray(b, F64))
        else:
            with np.errstate(all="ignore"):
                r = f(np.asarray(a, F32), np.asarray(b, F32)).astype(F64)
        return r if r.ndim else float(r)

    def mul(self, a, b):
        return self._op(np.multiply, a, b)

    def sub(self, a, b):
        return self._op(np.subtract, a, b)

    def div(self, a, b):
        return self._op(np.divide, a, b)


def sum_candidates(terms, fmt):
    """Every value (float)(fp64 sum of `terms` in any order) can take: [one] or [two adjacent fp32 numbers]; (values, wide) with wide
    set when the order could move the sum across more than one fp32 boundary (cancellation: nothing is pinned then)."""
    terms = np.asarray(terms, F64).ravel()
    exact = math.fsum(terms.tolist())
    if fmt.exact:
        return [exact], False
    m = int(np.count_nonzero(terms))
    e = 1.01 * max(m - 1, 0) * 2.0 ** -53 * math.fsum(np.abs(terms).tolist()) + (2.0 ** -53 * abs(exact) if m > 1 else 0.0)
    lo, hi = F32(exact - e), F32(exact + e)
    out = [lo]
    while out[-1] < hi and len(out) < 2:
        out.append(np.nextafter(out[-1], F32(np.inf)))
    return [float(v) for v in out], bool(out[-1] < hi)


def ulps(got, ref, mag):
    """|got - ref| in fp32 ulps of `mag`, elementwise, after the absolute floor of one minimum normal."""
    got, ref, mag = (np.asarray(a, F64) for a in (got, ref, mag))
    ulp = np.spacing(np.maximum(mag, MIN_NORMAL).astype(F32)).astype(F64)
    return np.maximum(np.abs(got - ref) - MIN_NORMAL, 0.0) / ulp


def ring_slots(head, length, hs):
    """Ring slots oldest to newest."""
    return [(head + k) % hs for k in range(length)]


def two_loop(g, S, Y, rho, h):
    """torch's two-loop recursion in float64 over pairs listed oldest to newest.  Returns (d, M, al, be)."""
    m = len(rho)
    q = -np.asarray(g, F64)
    al, be = [0.0] * m, [0.0] * m
    for k in range(m - 1, -1, -1):
        al[k] = float(S[k] @ q) * rho[k]
        q = q - al[k] * Y[k]
    r = q * h
    for k in range(m):
        be[k] = float(Y[k] @ r) * rho[k]
        r = r + (al[k] - be[k]) * S[k]
    M = abs(h) * np.abs(g)
    for k in range(m):
        M = M + abs(h) * abs(al[k]) * np.abs(Y[k]) + abs(al[k] - be[k]) * np.abs(S[k])
    return r, M, al, be


class Branch:
    """What follows from ONE consistent tuple of the ambiguous scalars."""
    rho_new = None      # fp32 value written to rho[slot] (None: no update)
    h_diag = t = None
    d = M = None        # float64 direction and its magnitude
    gtd = gtd_err = None
    x = xmag = None     # float64 iterate after the move and its magnitude (None: no move)
    code = 0
    ints = None


class Expectation:
    frozen = False      # the launch must change nothing at all
    body = False        # one pass of torch's while body ran: prev_grad, prev_loss, t, d are written
    n_iter = 0          # after the launch
    updated = False     # a pair went into the ring
    slot = None         # the slot that took it
    S_slot = Y_slot = None      # its fp32 values, bit for bit
    d_exact = None      # d = -g at n_iter == 1, bit for bit
    length = head = 0   # the ring after the launch
    prev_loss = None
    branches = ()
    ambiguous = False   # a decision has more than one answer under the reference's own intervals
    two_candidates = False      # an fp32 scalar of this launch has two candidates (a fact about the inputs)

    @property
    def ints(self):
        return self.branches[0].ints

    @property
    def code(self):
        return self.branches[0].code

    @property
    def moved(self):
        return self.branches[0].x is not None

    def tuples(self):
        return [(b.rho_new, b.h_diag, b.t) for b in self.branches]

    def match(self, rho_slot, h_diag, t):
        """The branch whose (rho[slot], h_diag, t) has the given bits, or None."""
        key = lambda v: None if v is None else F32(v).tobytes()
        for b in self.branches:
            if (b.rho_new is None or key(b.rho_new) == key(rho_slot)) and key(b.h_diag) == key(h_diag) and key(b.t) == key(t):
                return b
        return None


def _end_step(st, code):
    st["last_exit"] = code
    st["steps"] += 1
    st["phase"] = PHASE_START
    if st["steps"] >= st["n_steps"]:
        st["done"] = 1


def advance(snap, exact=False, d_ulps=64.0):
    fmt = _Fmt(exact)
    st = dict(snap["state"])
    E = Expectation()
    cap = int(np.asarray(snap["rho"]).shape[0])
    hs = st["history_size"]
    if st["done"] or hs < 1 or hs > cap:
        E.frozen = True
        b = Branch()
        b.ints = {k: st[k] for k in INTS}
        b.code = 0
        E.branches = (b,)
        return E
    g = np.asarray(snap["grad"], F64)
    x = np.asarray(snap["x"], F64)
    loss = float(snap["loss"])
    lr, tg = fmt.rnd(st["lr"]), fmt.rnd(st["tolerance_grad"])
    tol = float(st["tolerance_change"])
    tol_f = fmt.rnd(tol)
    tiny = fmt.rnd(1e-10)
    t_old, h_old = fmt.rnd(st["t"]), fmt.rnd(st["h_diag"])
    opt_cond = float(np.abs(g).max()) <= tg
    st["func_evals"] += 1
    code = 0
    if st["phase"] == PHASE_START:
        st["evals_in_step"] = 1
        if opt_cond:
            code = EXIT_OPT_START
        else:
            st["iter_in_step"] = 0
    else:
        st["evals_in_step"] += 1
        if st["iter_in_step"] == st["max_iter"]:
            code = EXIT_MAX_ITER
        elif st["evals_in_step"] >= st["max_eval"]:
            code = EXIT_MAX_EVAL
        elif opt_cond:
            code = EXIT_OPT_COND
        else:
            dt = fmt.mul(np.asarray(snap["d"], F64), t_old)
            if float(np.abs(dt).max()) <= tol_f:
                code = EXIT_SMALL_STEP
            elif abs(loss - float(st["prev_loss"])) < tol:
                code = EXIT_NO_PROGRESS
    E.length, E.head, E.prev_loss = st["hist_len"], st["hist_head"], float(st["prev_loss"])
    if code:
        _end_step(st, code)
        b = Branch()
        b.ints, b.code, b.h_diag, b.t = {k: st[k] for k in INTS}, code, h_old, t_old
        E.n_iter, E.branches = st["n_iter"], (b,)
        return E
    E.body = True
    st["iter_in_step"] += 1
    st["n_iter"] += 1
    E.n_iter = st["n_iter"]
    E.prev_loss = loss
    scalars = []        # (rho_new, h_diag, t, gtd candidates or None)
    if st["n_iter"] == 1:
        st["hist_len"] = st["hist_head"] = 0
        E.d_exact = -g if exact else (-g).astype(F32)
        gl1, w1 = sum_candidates(np.abs(g), fmt)
        gtd, w2 = sum_candidates(fmt.mul(g, -g), fmt)
        E.ambiguous |= w1 or w2
        E.two_candidates = len(gl1) > 1 or len(gtd) > 1
        for c in gl1:
            inv = fmt.div(1.0, c)
            scalars.append((None, 1.0, fmt.mul(inv if inv < 1.0 else 1.0, lr), gtd))
        S = Y = np.zeros((0, g.size))
        rho = []
    else:
        pg, d_old = np.asarray(snap["prev_grad"], F64), np.asarray(snap["d"], F64)
        y, s = fmt.sub(g, pg), fmt.mul(d_old, t_old)
        ys_c, w1 = sum_candidates(fmt.mul(y, s), fmt)
        yy_c, w2 = sum_candidates(fmt.mul(y, y), fmt)
        upd = [c > tiny for c in ys_c]
        E.ambiguous |= w1 or (w2 and upd[0]) or len(set(upd)) > 1
        head, length = st["hist_head"], st["hist_len"]
        if upd[0]:
            E.updated = True
            E.two_candidates = len(ys_c) > 1 or len(yy_c) > 1
            if length == hs:
                E.slot = head
                head = (head + 1) % hs
            else:
                E.slot = (head + length) % hs
                length += 1
            E.S_slot, E.Y_slot = (s, y) if exact else (s.astype(F32), y.astype(F32))
            st["hist_len"], st["hist_head"] = length, head
            for ys in ys_c:
                for yy in yy_c:
                    scalars.append((fmt.div(1.0, ys), fmt.div(ys, yy), lr, None))
        else:
            st["n_skipped"] += 1
            scalars.append((None, h_old, lr, None))
        slots = ring_slots(head, length, hs)
        S, Y = np.asarray(snap["S"], F64)[slots], np.asarray(snap["Y"], F64)[slots]
        rho = [fmt.rnd(v) for v in np.asarray(snap["rho"], F64)[slots]]
        if E.updated:       # the newest pair is the one just formed, wherever the ring put it
            S[-1], Y[-1] = s, y
    E.length, E.head = st["hist_len"], st["hist_head"]
    branches = []
    for rho_new, h, t, gtd_c in scalars:
        b = Branch()
        b.rho_new, b.h_diag, b.t = rho_new, h, t
        if st["n_iter"] == 1:
            b.d, b.M = -g, np.abs(g)
            decisions = [c > -tol_f for c in gtd_c]
            b.gtd, b.gtd_err = gtd_c[0], 0.0
        else:
            b.d, b.M, _, _ = two_loop(g, S, Y, rho[:-1] + [rho_new] if rho_new is not None else rho, h)
            b.gtd = float(g @ b.d)
            gd = float(np.abs(g) @ np.abs(b.d))
            b.gtd_err = 0.0 if exact else (d_ulps * float(np.abs(g) @ np.spacing(np.maximum(b.M, MIN_NORMAL).astype(F32)).astype(F64))
                                           + 2.0 ** -23 * gd + 2.0 ** -23 * abs(b.gtd))
            decisions = [b.gtd + e > -tol_f for e in (-b.gtd_err, b.gtd_err)]
        E.ambiguous |= len(set(decisions)) > 1
        sb = dict(st)
        if decisions[0]:
            b.code = EXIT_GTD
        else:
            b.x, b.xmag = x + t * b.d, np.abs(x) + np.abs(t * b.d)
            if sb["iter_in_step"] != sb["max_iter"]:
                sb["phase"] = PHASE_AFTER_MOVE
            else:
                b.code = EXIT_MAX_ITER
        if b.code:
            _end_step(sb, b.code)
        b.ints = {k: sb[k] for k in INTS}
        branches.append(b)
    E.ambiguous |= len({(b.code, tuple(sorted(b.ints.items()))) for b in branches}) > 1
    E.branches = tuple(branches)
    return E


def compare(snap, after, E, d_budget, x_budget, what=""):
    """Hold one launch's read-back (`after`: the layout of a snapshot) to its expectation.  Asserts; returns the figures
    {"d": ulps, "x": ulps, "branch": index} of the launch.  Storage outside the problem (guards, tails) is the caller's."""
    s0, s1 = snap["state"], after["state"]
    bits = lambda a: np.ascontiguousarray(np.asarray(a, F32)).view(np.int32)
    same = lambda a, b: np.array_equal(bits(a), bits(b))
    f32b = lambda v: F32(v).tobytes()
    for k in HYPER + ("reserved0", "reserved"):
        assert s0[k] == s1[k], f"{what}: state.{k} changed: {s0[k]!r} -> {s1[k]!r}"
    fig = {"d": 0.0, "x": 0.0, "branch": 0}
    if E.frozen or not E.body:
        for k in INTS:
            assert s1[k] == E.ints[k], f"{what}: state.{k} = {s1[k]}, expected {E.ints[k]}"
        for k in ("t", "h_diag"):
            assert f32b(s0[k]) == f32b(s1[k]), f"{what}: state.{k} changed without a pass of the loop body"
        assert np.float64(s0["prev_loss"]).tobytes() == np.float64(s1["prev_loss"]).tobytes(), f"{what}: prev_loss changed"
        for k in ("x", "d", "prev_grad", "S", "Y", "rho"):
            assert same(snap[k], after[k]), f"{what}: {k} changed without a pass of the loop body"
        return fig
    assert not E.ambiguous, f"{what}: the case is ambiguous under the reference's own intervals"
    rho_slot = after["rho"][E.slot] if E.updated else None
    b = E.match(rho_slot, s1["h_diag"], s1["t"])
    assert b is not None, (f"{what}: (rho[slot], h_diag, t) = ({rho_slot!r}, {s1['h_diag']!r}, {s1['t']!r}) is none of the consistent "
                           f"tuples {E.tuples()!r}")
    fig["branch"] = E.branches.index(b)
    for k in INTS:
        assert s1[k] == b.ints[k], f"{what}: state.{k} = {s1[k]}, expected {b.ints[k]}"
    assert np.float64(s1["prev_loss"]).tobytes() == np.float64(E.prev_loss).tobytes(), f"{what}: prev_loss {s1['prev_loss']!r}, expected {E.prev_loss!r}"
    # the ring: the written slot to the bit, every other slot and rho untouched
    for k, want in (("S", E.S_slot), ("Y", E.Y_slot)):
        for r in range(np.asarray(snap[k]).shape[0]):
            if E.updated and r == E.slot:
                assert same(after[k][r], want), f"{what}: {k}[{r}] is not the new pair to the bit"
            else:
                assert same(after[k][r], snap[k][r]), f"{what}: ring slot {k}[{r}] was written"
    for r in range(np.asarray(snap["rho"]).shape[0]):
        if not (E.updated and r == E.slot):
            assert same(after["rho"][r], snap["rho"][r]), f"{what}: rho[{r}] was written"
    assert same(after["prev_grad"], snap["grad"]), f"{what}: prev_grad is not the gradient to the bit"
    d = np.asarray(after["d"], F64)
    assert np.isfinite(d).all(), f"{what}: d is not finite (a sentinel was read or an element not written)"
    if E.d_exact is not None:
        assert same(after["d"], E.d_exact), f"{what}: d is not -g to the bit"
    else:
        e = ulps(d, b.d, b.M)
        fig["d"] = float(e.max())
        assert fig["d"] <= d_budget, f"{what}: d off by {fig['d']:.2f} ulp of its magnitude at {int(e.argmax())}, budget {d_budget:.2f}"
        assert not (bits(after["d"])[b.M == 0.0] & 0x7FFFFFFF).any(), f"{what}: an element of d that is 0 by construction is not 0"
    xa = np.asarray(after["x"], F64)
    if b.x is None:
        assert same(after["x"], snap["x"]), f"{what}: x moved on an exit without a move"
    else:
        assert np.isfinite(xa).all(), f"{what}: x is not finite"
        e = ulps(xa, b.x, b.xmag)
        fig["x"] = float(e.max())
        assert fig["x"] <= x_budget, f"{what}: x off by {fig['x']:.2f} ulp of |x| + |t d| at {int(e.argmax())}, budget {x_budget:.2f}"
        # against the device's OWN d: fl(x + fl(t d)) or one fused rounding -- at most 1 ulp of |x| + |t d| either way
        own = np.asarray(snap["x"], F64) + b.t * d
        e = ulps(xa, own, (np.abs(np.asarray(snap["x"], F64)) + np.abs(b.t * d)) * (1 + 2.0 ** -22))
        assert float(e.max()) <= 1.0, f"{what}: x is not x + t d of the device's own d: {float(e.max()):.2f} ulp at {int(e.argmax())}"
    return fig

"""L-BFGS as a state machine that advances by one closure evaluation per call (latent reconstruction, fcgan_model.py:278-302).

`torch.optim.LBFGS(line_search_fn=None).step(closure)` called `n_steps` times is the same computation as this loop:

    while not opt.done():
        loss, grad = closure(x)         # at the current x
        opt.advance(loss, grad, x)      # torch's logic up to its next closure call; moves x in place

`advance` picks up where torch would be after a closure returned -- at the start of a step() (phase START) or after the move of an
iteration (phase AFTER_MOVE) -- and runs forward to the next point where torch calls the closure.  torch reads the loss and several
0-dim tensors back to the host on every iteration (about 2 m + 5 round trips with m history pairs); the kernel behind DeviceLBFGS
(sgan_lbfgs_advance) takes every one of those decisions on the device, so a closure plus an advance can be captured once and replayed.

`lbfgs_advance_reference` is the same state machine written with the torch operations of torch/optim/lbfgs.py, in the same order:
the specification, the CPU path of DeviceLBFGS and the oracle of the kernel's tests."""
import ctypes as C
import math

import torch

from ._lib import DEFINES, STRUCTS

PHASE_START, PHASE_AFTER_MOVE = DEFINES["SGAN_LBFGS_PHASE_START"], DEFINES["SGAN_LBFGS_PHASE_AFTER_MOVE"]
# why the last finished step() ended (state.last_exit)
EXIT_NONE, EXIT_OPT_START, EXIT_GTD, EXIT_MAX_ITER, EXIT_MAX_EVAL, EXIT_OPT_COND, EXIT_SMALL_STEP, EXIT_NO_PROGRESS = (
    DEFINES["SGAN_LBFGS_EXIT_" + n]
    for n in ("NONE", "OPT_START", "GTD", "MAX_ITER", "MAX_EVAL", "OPT_COND", "SMALL_STEP", "NO_PROGRESS"))
EXIT_NAMES = ["none", "opt_cond at step start", "gtd > -tolerance_change", "max_iter", "max_eval", "opt_cond", "|d t| small",
              "no progress"]
MAX_HISTORY = DEFINES["SGAN_LBFGS_MAX_HISTORY"]
LbfgsState = STRUCTS["sgan_lbfgs_state"]      # one problem's hyperparameters, counters and scalars, 128 bytes

COUNTERS = ("func_evals", "n_iter", "steps", "phase", "done", "iter_in_step", "evals_in_step", "hist_len", "last_exit", "n_skipped")


class ReferenceState:
    """One problem of lbfgs_advance_reference: torch's optimizer state plus the locals of the step() in flight."""

    def __init__(self, lr, max_iter, max_eval, tolerance_grad, tolerance_change, history_size, n_steps):
        self.lr, self.max_iter, self.max_eval = lr, max_iter, max_eval
        self.tolerance_grad, self.tolerance_change, self.history_size, self.n_steps = tolerance_grad, tolerance_change, history_size, n_steps
        self.func_evals = self.n_iter = self.steps = 0
        self.phase, self.done = PHASE_START, int(n_steps <= 0)
        self.iter_in_step = self.evals_in_step = 0
        self.last_exit, self.n_skipped = EXIT_NONE, 0
        self.d = self.t = self.H_diag = self.prev_flat_grad = self.prev_loss = None
        self.old_dirs, self.old_stps, self.ro = [], [], []

    @property
    def hist_len(self):
        return len(self.old_dirs)

    def counters(self):
        return {k: int(getattr(self, k)) for k in COUNTERS}


def _end_step(st, code):
    st.last_exit = code
    st.steps += 1
    st.phase = PHASE_START
    if st.steps >= st.n_steps:
        st.done = 1


def _advance_one(st, loss, flat_grad, x):
    """torch/optim/lbfgs.py step(), from the closure evaluation that just returned (loss, flat_grad) at x to the next one."""
    if st.done:
        return
    loss = float(loss)
    st.func_evals += 1
    if st.phase == PHASE_START:                      # orig_loss = closure()
        st.evals_in_step = 1
        if flat_grad.abs().max() <= st.tolerance_grad:
            return _end_step(st, EXIT_OPT_START)
        st.iter_in_step = 0
    else:                                            # loss = closure() after the move; the checks that end the while body
        st.evals_in_step += 1
        opt_cond = flat_grad.abs().max() <= st.tolerance_grad
        if st.iter_in_step == st.max_iter:
            return _end_step(st, EXIT_MAX_ITER)
        if st.evals_in_step >= st.max_eval:
            return _end_step(st, EXIT_MAX_EVAL)
        if opt_cond:
            return _end_step(st, EXIT_OPT_COND)
        if st.d.mul(st.t).abs().max() <= st.tolerance_change:
            return _end_step(st, EXIT_SMALL_STEP)
        if abs(loss - st.prev_loss) < st.tolerance_change:
            return _end_step(st, EXIT_NO_PROGRESS)
    # one pass of the while body
    st.iter_in_step += 1
    st.n_iter += 1
    if st.n_iter == 1:
        st.d = flat_grad.neg()
        st.old_dirs, st.old_stps, st.ro = [], [], []
        st.H_diag = 1
    else:
        y = flat_grad.sub(st.prev_flat_grad)
        s = st.d.mul(st.t)
        ys = y.dot(s)
        if ys > 1e-10:
            if len(st.old_dirs) == st.history_size:
                st.old_dirs.pop(0)
                st.old_stps.pop(0)
                st.ro.pop(0)
            st.old_dirs.append(y)
            st.old_stps.append(s)
            st.ro.append(1.0 / ys)
            st.H_diag = ys / y.dot(y)
        else:
            st.n_skipped += 1
        num_old = len(st.old_dirs)
        al = [None] * num_old
        q = flat_grad.neg()
        for i in range(num_old - 1, -1, -1):
            al[i] = st.old_stps[i].dot(q) * st.ro[i]
            q.add_(st.old_dirs[i], alpha=-al[i])
        st.d = r = torch.mul(q, st.H_diag)
        for i in range(num_old):
            be_i = st.old_dirs[i].dot(r) * st.ro[i]
            r.add_(st.old_stps[i], alpha=al[i] - be_i)
    if st.prev_flat_grad is None:
        st.prev_flat_grad = flat_grad.clone(memory_format=torch.contiguous_format)
    else:
        st.prev_flat_grad.copy_(flat_grad)
    st.prev_loss = loss
    if st.n_iter == 1:
        st.t = min(1.0, 1.0 / flat_grad.abs().sum()) * st.lr
    else:
        st.t = st.lr
    gtd = flat_grad.dot(st.d)
    if gtd > -st.tolerance_change:
        return _end_step(st, EXIT_GTD)
    x.add_(st.d, alpha=st.t)                        # _add_grad(t, d)
    if st.iter_in_step != st.max_iter:
        st.phase = PHASE_AFTER_MOVE                  # torch calls the closure next
        return
    return _end_step(st, EXIT_MAX_ITER)             # no re-evaluation after the max_iter-th move


def lbfgs_advance_reference(states, loss, grad, x):
    """states: [ReferenceState] * J; loss [J]; grad, x: [J, n].  Advances every problem that is not done; x is updated in place."""
    for j, st in enumerate(states):
        _advance_one(st, loss[j], grad[j], x[j])


def _default_max_eval(max_iter, max_eval):
    return max_iter * 5 // 4 if max_eval is None else max_eval


class DeviceLBFGS:
    """J independent L-BFGS problems of n unknowns each (the reconstruction trials), advanced by one closure evaluation per call.

    On a GPU device every call is ONE launch of sgan_lbfgs_advance that reads nothing back (capturable); the history is a ring of
    `history_size` (s, y, rho) triples per problem in device memory.  On the CPU the same state machine runs as
    lbfgs_advance_reference.  n_steps: how many torch step() calls each problem runs before it freezes (None: never)."""

    def __init__(self, n, J, lr=1, max_iter=20, max_eval=None, tolerance_grad=1e-7, tolerance_change=1e-9, history_size=100,
                 line_search_fn=None, n_steps=None, device="cuda"):
        if line_search_fn is not None:
            raise NotImplementedError("DeviceLBFGS: only line_search_fn=None (a fixed step of lr) is implemented")
        if not 1 <= J <= 8:
            raise ValueError(f"DeviceLBFGS: 1 <= J <= 8 problems per launch, got {J}")
        if not 1 <= history_size <= MAX_HISTORY:
            raise ValueError(f"DeviceLBFGS: history_size must be in [1, {MAX_HISTORY}], got {history_size}")
        if max_iter < 1:
            raise ValueError("DeviceLBFGS: max_iter >= 1")
        self.n, self.J, self.device = int(n), int(J), torch.device(device)
        self.hyper = dict(lr=float(lr), max_iter=int(max_iter), max_eval=int(_default_max_eval(max_iter, max_eval)),
                          tolerance_grad=float(tolerance_grad), tolerance_change=float(tolerance_change), history_size=int(history_size),
                          n_steps=int(n_steps) if n_steps is not None else 2 ** 31 - 1)
        if self.device.type == "cpu":
            self._ref = None
            self.reset()
            return
        self._ref = False
        m = self.hyper["history_size"]
        f32 = dict(dtype=torch.float32, device=self.device)
        self.state = torch.zeros((J, C.sizeof(LbfgsState)), dtype=torch.uint8, device=self.device)
        self.d = torch.zeros((J, self.n), **f32)
        self.prev_grad = torch.zeros((J, self.n), **f32)
        self.hist_s = torch.zeros((J, m, self.n), **f32)
        self.hist_y = torch.zeros((J, m, self.n), **f32)
        self.hist_rho = torch.zeros((J, m), **f32)
        self.reset()

    def _initial_state(self):
        h = self.hyper
        st = LbfgsState()
        st.lr, st.tolerance_grad, st.tolerance_change = h["lr"], h["tolerance_grad"], h["tolerance_change"]
        st.max_iter, st.max_eval, st.history_size, st.n_steps = h["max_iter"], h["max_eval"], h["history_size"], h["n_steps"]
        st.done = int(h["n_steps"] <= 0)
        st.h_diag = 1.0
        return st

    def reset(self):
        """Fresh optimizers (torch: a new LBFGS object); the history buffers are not cleared, the ring is simply empty."""
        if self.device.type == "cpu":
            h = self.hyper
            self.states = [ReferenceState(h["lr"], h["max_iter"], h["max_eval"], h["tolerance_grad"], h["tolerance_change"],
                                          h["history_size"], h["n_steps"]) for _ in range(self.J)]
            return
        raw = bytes(self._initial_state()) * self.J
        self.state.copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(self.J, -1), non_blocking=False)

    def advance(self, loss, grad, x):
        """loss [J] fp32, grad [J, n] (row stride >= n), x [J, n] updated in place."""
        if self.device.type == "cpu":
            lbfgs_advance_reference(self.states, loss, grad, x)
            return
        from . import ops
        ops.lbfgs_advance(self.state, self.J, self.n, x, grad, loss, self.d, self.prev_grad, self.hist_s, self.hist_y, self.hist_rho)

    def read_states(self):
        """[LbfgsState] * J (host copies; synchronises)."""
        if self.device.type == "cpu":
            out = []
            for st in self.states:
                s = self._initial_state()
                for k in COUNTERS:
                    setattr(s, k, int(getattr(st, k)))
                out.append(s)
            return out
        raw = self.state.cpu().numpy().tobytes()
        size = C.sizeof(LbfgsState)
        return [LbfgsState.from_buffer_copy(raw[j * size:(j + 1) * size]) for j in range(self.J)]

    def counters(self):
        return [{k: int(getattr(s, k)) for k in COUNTERS} for s in self.read_states()]

    def done(self):
        """[J] bools (a host read: call it every K replays, not after every advance)."""
        if self.device.type == "cpu":
            return [bool(st.done) for st in self.states]
        o = LbfgsState.done.offset
        return [bool(v) for v in self.state[:, o:o + 4].clone().view(torch.int32)[:, 0].cpu().tolist()]


def neg_log_likelihood(z):
    """-log N(z; 0, I) over all elements of z: (n log(2 pi) + |z|^2) / 2 (the reference's -multivariate_normal.logpdf)."""
    z = z.detach().double().reshape(-1)
    return 0.5 * (z.numel() * math.log(2 * math.pi) + float(z.dot(z)))

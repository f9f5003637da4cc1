"""lbfgs_advance_reference (one closure evaluation per call) against torch.optim.LBFGS.step x n_steps, in float64 on the CPU: the
same iterates at every step boundary and the same func_evals / n_iter counters, over cases that take every exit of torch's loop."""
import pytest
import torch

from supervised_gan_amd import lbfgs as LB


def quadratic(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    M = torch.randn(n, n, generator=g, dtype=torch.float64)
    A = M @ M.T / n + 0.5 * torch.eye(n, dtype=torch.float64)
    b = torch.randn(n, generator=g, dtype=torch.float64)
    return lambda x: 0.5 * x @ (A @ x) - b @ x


def rosenbrock(x):
    return (100 * (x[1:] - x[:-1] ** 2) ** 2 + (1 - x[:-1]) ** 2).sum()


def linear(n):
    c = torch.linspace(-1, 1, n, dtype=torch.float64)
    return lambda x: c @ x          # constant gradient: y = 0, every memory update is skipped


def value_and_grad(f, x):
    x = x.detach().clone().requires_grad_(True)
    v = f(x)
    (g,) = torch.autograd.grad(v, x)
    return v.detach(), g


def run_torch(f, x0, n_steps, **kw):
    p = x0.clone().requires_grad_(True)
    opt = torch.optim.LBFGS([p], **kw)

    def closure():
        opt.zero_grad()
        v = f(p)
        v.backward()
        return v

    xs = []
    for _ in range(n_steps):
        opt.step(closure)
        xs.append(p.detach().clone())
    st = opt.state[p]
    return xs, st["func_evals"], st["n_iter"]


def run_reference(fs, x0s, n_steps, **kw):
    """J problems at once: one closure evaluation each, then one advance, until every problem is done."""
    lr = kw.pop("lr", 1)
    max_iter = kw.pop("max_iter", 20)
    hyper = (lr, max_iter, LB._default_max_eval(max_iter, kw.pop("max_eval", None)), kw.pop("tolerance_grad", 1e-7),
             kw.pop("tolerance_change", 1e-9), kw.pop("history_size", 100), n_steps)
    assert not kw
    states = [LB.ReferenceState(*hyper) for _ in fs]
    x = torch.stack(x0s)
    xs = [[] for _ in fs]
    exits = [set() for _ in fs]
    calls = 0
    while not all(st.done for st in states):
        vg = [value_and_grad(f, x[j]) for j, f in enumerate(fs)]
        loss = torch.stack([v for v, _ in vg])
        grad = torch.stack([g for _, g in vg])
        before = [st.steps for st in states]
        LB.lbfgs_advance_reference(states, loss, grad, x)
        calls += 1
        for j, st in enumerate(states):
            if st.steps > before[j]:
                xs[j].append(x[j].clone())
                exits[j].add(st.last_exit)
        assert calls < 100000
    return xs, states, exits


CASES = {
    # name: (problem, n, n_steps, optimizer kwargs, exits that must occur)
    "quadratic_default": ("quad", 12, 4, dict(lr=1), {LB.EXIT_GTD, LB.EXIT_NO_PROGRESS}),
    "quadratic_lr01": ("quad", 30, 5, dict(lr=0.1), {LB.EXIT_MAX_ITER}),
    "rosenbrock": ("rosen", 6, 6, dict(lr=0.5), set()),
    "opt_cond_at_start": ("quad", 8, 3, dict(lr=0.1, tolerance_grad=1e3), {LB.EXIT_OPT_START}),
    "opt_cond_after_eval": ("quad", 8, 3, dict(lr=1, tolerance_grad=1e-3), {LB.EXIT_OPT_COND, LB.EXIT_OPT_START}),
    "gtd_break": ("quad", 8, 3, dict(lr=0.1, tolerance_change=1e2), {LB.EXIT_GTD}),
    "small_step": ("quad", 8, 3, dict(lr=1e-4, tolerance_change=1e-4), {LB.EXIT_SMALL_STEP, LB.EXIT_MAX_ITER}),
    "max_eval_below_max_iter": ("quad", 8, 3, dict(lr=0.1, max_iter=10, max_eval=4), {LB.EXIT_MAX_EVAL}),
    "history_wrap": ("rosen", 10, 4, dict(lr=0.2, history_size=3), {LB.EXIT_MAX_ITER}),
    "skipped_updates": ("linear", 6, 2, dict(lr=0.1, max_iter=5), {LB.EXIT_MAX_ITER}),
}


def test_cases_cover_every_exit():
    assert set().union(*(c[4] for c in CASES.values())) == set(range(1, len(LB.EXIT_NAMES)))


def _problem(kind, n, seed):
    if kind == "quad":
        return quadratic(n, seed)
    if kind == "rosen":
        return rosenbrock
    return linear(n)


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_matches_torch_lbfgs(name):
    kind, n, n_steps, kw, must_exit = CASES[name]
    fs = [_problem(kind, n, seed) for seed in (0, 1)]
    x0s = [torch.randn(n, generator=torch.Generator().manual_seed(10 + s), dtype=torch.float64) * 0.5 for s in (0, 1)]
    xs_ref, states, exits = run_reference(fs, x0s, n_steps, **dict(kw))
    for j, f in enumerate(fs):
        xs_t, func_evals, n_iter = run_torch(f, x0s[j], n_steps, **kw)
        assert len(xs_ref[j]) == n_steps
        for k, (a, b) in enumerate(zip(xs_ref[j], xs_t)):
            err = float((a - b).abs().max())
            assert err <= 1e-12 * max(1.0, float(b.abs().max())), (name, j, k, err)
        assert states[j].func_evals == func_evals, (name, j, states[j].func_evals, func_evals)
        assert states[j].n_iter == n_iter, (name, j, states[j].n_iter, n_iter)
        assert must_exit <= exits[j], (name, j, [LB.EXIT_NAMES[e] for e in exits[j]])
    if kind == "linear":
        assert all(st.n_skipped > 0 and st.hist_len == 0 for st in states)
    if kw.get("history_size") == 3:
        assert all(st.hist_len == 3 and st.n_iter > 4 for st in states)


def test_done_problem_is_frozen():
    f = quadratic(6)
    st = LB.ReferenceState(1, 20, 25, 1e-7, 1e-9, 100, 1)
    x = torch.randn(1, 6, dtype=torch.float64)
    while not st.done:
        v, g = value_and_grad(f, x[0])
        LB.lbfgs_advance_reference([st], v.view(1), g.view(1, -1), x)
    frozen, counters = x.clone(), st.counters()
    v, g = value_and_grad(f, x[0])
    LB.lbfgs_advance_reference([st], v.view(1), g.view(1, -1), x)
    assert torch.equal(x, frozen) and st.counters() == counters


def test_device_lbfgs_cpu_path_and_guards():
    opt = LB.DeviceLBFGS(6, 2, lr=1, n_steps=2, device="cpu")
    f = quadratic(6)
    x = torch.zeros(2, 6, dtype=torch.float64)
    while not all(opt.done()):
        vg = [value_and_grad(f, x[j]) for j in range(2)]
        opt.advance(torch.stack([v for v, _ in vg]), torch.stack([g for _, g in vg]), x)
    assert [c["steps"] for c in opt.counters()] == [2, 2]
    with pytest.raises(NotImplementedError):
        LB.DeviceLBFGS(6, 1, line_search_fn="strong_wolfe", device="cpu")
    with pytest.raises(ValueError):
        LB.DeviceLBFGS(6, 9, device="cpu")


def test_neg_log_likelihood_closed_form():
    import math
    z = torch.randn(2, 8, 4, 4, generator=torch.Generator().manual_seed(3))
    want = -torch.distributions.Normal(0.0, 1.0).log_prob(z.double()).sum().item()
    assert abs(LB.neg_log_likelihood(z) - want) <= 1e-9 * abs(want)
    assert abs(LB.neg_log_likelihood(torch.zeros(5)) - 2.5 * math.log(2 * math.pi)) < 1e-12


def test_state_struct_layout():
    assert LB.LbfgsState.done.offset == 48 and LB.LbfgsState.prev_loss.offset == 88

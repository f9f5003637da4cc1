"""sgan_lbfgs_advance against lbfgs_advance_reference (the same state machine in torch ops, fp32 on the same device), both fed the
same device closure (a separable quadratic + quartic per problem): iterates at every step boundary, exit decisions and counters after
every call, frozen problems, and a captured closure + advance replaying to the eager result."""
import pytest
import torch

from supervised_gan_amd import lbfgs as LB

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")


def closure_into(x, loss, grad, dd):
    """loss[j] = sum_i dd[j, i] x_i^2 / 2 + x_i^4 / 4 over the row x[j]; grad[j] its gradient.  Written into the given buffers
    (capturable).  The minimum is at 0, so no fp32 cancellation blurs the gradients the two implementations see."""
    x2 = x * x
    loss.copy_((0.5 * dd * x2 + 0.25 * x2 * x2).sum(1))
    grad.copy_(dd * x + x2 * x)


def x0(J, n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(J, n, generator=g) * 2 - 1) * (4.0 / n)).cuda()


def curvature(J, n, seed=1):
    g = torch.Generator().manual_seed(seed)
    return (1 + torch.rand(J, n, generator=g)).cuda()


def rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def linear_into(x, loss, grad, c):
    """loss[j] = c[j] . x[j]: a constant gradient, so y = 0 and every memory update is skipped."""
    loss.copy_((c * x).sum(1))
    grad.copy_(c.expand_as(x))


def _run_both(J, n, kw, closure, x_init):
    """Kernel and reference side by side, one closure evaluation each per call, until the reference is done.  Counters (phase,
    last_exit, n_skipped ... included) must agree after every call, x at every step boundary.  Returns (dev, x, last_exits seen)."""
    dev = LB.DeviceLBFGS(n, J, device="cuda", **kw)
    h = dev.hyper
    ref = [LB.ReferenceState(h["lr"], h["max_iter"], h["max_eval"], h["tolerance_grad"], h["tolerance_change"], h["history_size"],
                             h["n_steps"]) for _ in range(J)]
    xk, xr = x_init.clone(), x_init.clone()
    lk, gk = torch.zeros(J, device="cuda"), torch.zeros(J, n, device="cuda")
    lr_, gr = torch.zeros(J, device="cuda"), torch.zeros(J, n, device="cuda")
    calls, boundaries, exits = 0, 0, set()
    while not all(st.done for st in ref):
        closure(xk, lk, gk)
        closure(xr, lr_, gr)
        before = [st.steps for st in ref]
        dev.advance(lk, gk, xk)
        LB.lbfgs_advance_reference(ref, lr_, gr, xr)
        got = dev.counters()
        for j in range(J):
            want = ref[j].counters()
            assert got[j] == want, (calls, j, got[j], want)
            if ref[j].steps > before[j]:
                boundaries += 1
                exits.add(got[j]["last_exit"])
                assert rel(xk[j], xr[j]) <= 1e-5, (calls, j, rel(xk[j], xr[j]))
        calls += 1
        assert calls < 200
    assert boundaries == h["n_steps"] * J and all(dev.done())
    return dev, xk, exits


@pytest.mark.parametrize("J", [1, 3])
@pytest.mark.parametrize("n", [8, 512, 4100])
@pytest.mark.parametrize("history", [3, 100])
def test_kernel_matches_reference(J, n, history):
    _need_gpu()
    dd = curvature(J, n)
    closure = lambda x, loss, grad: closure_into(x, loss, grad, dd)
    dev, xk, _ = _run_both(J, n, dict(lr=0.1, max_iter=6, history_size=history, n_steps=3), closure, x0(J, n))
    if history == 3:
        assert all(c["hist_len"] == 3 for c in dev.counters())
    # a done problem is frozen: further calls change neither x nor the state
    lk, gk = torch.zeros(J, device="cuda"), torch.zeros(J, n, device="cuda")
    xs, ss = xk.clone(), dev.state.clone()
    for _ in range(2):
        closure(xk, lk, gk)
        dev.advance(lk, gk, xk)
    torch.cuda.synchronize()
    assert torch.equal(xk, xs) and torch.equal(dev.state, ss)


# settings that force each exit of torch's loop (with margins far above fp32 noise on both sides of every threshold)
EXIT_CASES = {
    "opt_cond_at_start": ("quartic", 64, dict(lr=0.1, tolerance_grad=1e3), {LB.EXIT_OPT_START}),
    "opt_cond_after_eval": ("quartic", 64, dict(lr=1, tolerance_grad=1e-3), {LB.EXIT_OPT_COND, LB.EXIT_OPT_START}),
    "gtd_break": ("quartic", 64, dict(lr=0.1, tolerance_change=1e2), {LB.EXIT_GTD}),
    "max_eval_below_max_iter": ("quartic", 64, dict(lr=0.1, max_iter=10, max_eval=4), {LB.EXIT_MAX_EVAL}),
    "small_step": ("quartic", 64, dict(lr=1e-4, tolerance_change=1e-4), {LB.EXIT_SMALL_STEP}),
    "no_progress": ("linear", 8, dict(lr=0.01, tolerance_change=6e-4), {LB.EXIT_NO_PROGRESS}),
    "skipped_updates": ("linear", 8, dict(lr=0.1, max_iter=5), {LB.EXIT_MAX_ITER}),
}


def test_exit_cases_cover_every_exit():
    assert set().union(*(c[3] for c in EXIT_CASES.values())) == set(range(1, len(LB.EXIT_NAMES)))


@pytest.mark.parametrize("name", sorted(EXIT_CASES))
def test_kernel_takes_every_exit_like_reference(name):
    _need_gpu()
    kind, n, kw, must = EXIT_CASES[name]
    J = 3
    if kind == "quartic":
        dd = curvature(J, n)
        closure = lambda x, loss, grad: closure_into(x, loss, grad, dd)
    else:
        c = (torch.linspace(-1, 1, n).repeat(J, 1) * 0.1 * torch.tensor([1.0, 0.9, 1.1]).view(J, 1)).cuda()
        closure = lambda x, loss, grad: linear_into(x, loss, grad, c)
    dev, _, exits = _run_both(J, n, dict(kw, n_steps=3), closure, x0(J, n))
    assert must <= exits, (name, [LB.EXIT_NAMES[e] for e in exits])
    if kind == "linear":
        assert all(c_["n_skipped"] > 0 and c_["hist_len"] == 0 for c_ in dev.counters())


def test_captured_advance_replays_eager_result():
    _need_gpu()
    J, n = 3, 512
    kw = dict(lr=0.1, max_iter=6, history_size=5, n_steps=3)

    dd = curvature(J, n)

    def program(opt, x, loss, grad):
        closure_into(x, loss, grad, dd)
        opt.advance(loss, grad, x)

    eager = LB.DeviceLBFGS(n, J, device="cuda", **kw)
    xe, le, ge = x0(J, n, 5), torch.zeros(J, device="cuda"), torch.zeros(J, n, device="cuda")
    for _ in range(40):
        program(eager, xe, le, ge)
    graphed = LB.DeviceLBFGS(n, J, device="cuda", **kw)
    xg, lg, gg = x0(J, n, 5), torch.zeros(J, device="cuda"), torch.zeros(J, n, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        program(graphed, xg, lg, gg)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(40):
        g.replay()
    torch.cuda.synchronize()
    assert all(eager.done()) and all(graphed.done())
    assert eager.counters() == graphed.counters()
    assert torch.equal(xe, xg)


def test_bad_arguments_are_refused():
    _need_gpu()
    from supervised_gan_amd._lib import SganError
    from supervised_gan_amd import ops
    with pytest.raises(ValueError):
        LB.DeviceLBFGS(8, 1, history_size=LB.MAX_HISTORY + 1, device="cuda")
    dev = LB.DeviceLBFGS(8, 2, device="cuda")
    with pytest.raises(SganError):
        ops.lbfgs_advance(dev.state, 2, 8, torch.zeros(2, 4, device="cuda"), torch.zeros(2, 8, device="cuda"),
                          torch.zeros(2, device="cuda"), dev.d, dev.prev_grad, dev.hist_s, dev.hist_y, dev.hist_rho)

"""The launch sequence of the conv chains is part of their behaviour: which `ops` launch wrappers a forward + backward calls, in which
order, with how many jobs each, and which statistics arenas it asks the pool for.  A recorder wraps the public wrappers as
pass-throughs and the lists are compared with tests/golden/chain_launches.json, recorded with this very file at commit 9b0ca27
("Add fcgan latent reconstruction with an on-device L-BFGS kernel"), the last one that had a single-chain walk next to the grouped
one.  `python tests/test_hip_chain_launches.py OUT.json` records."""
import contextlib
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "chain_launches.json")

# name -> number of jobs of a call
_JOBS = {"conv_fwd_grouped": lambda a: len(a[0]), "conv_dgrad_grouped": lambda a: len(a[0]), "conv_wgrad_grouped": lambda a: len(a[0]),
         "conv_bwd_grouped": lambda a: f"{len(a[0])}+{len(a[1])}", "norm_bwd_apply": lambda a: 1, "norm_bwd_apply_multi": lambda a: len(a[0]),
         "norm_apply_fwd": lambda a: 1, "norm_apply_bwd_sums": lambda a: 1, "tanh_bwd": lambda a: 1, "bn_running_update": lambda a: len(a[0]),
         "dropout_mask": lambda a: 1, "rng_advance": lambda a: 1, "stat_arena": lambda a: f"n={a[0]}"}


@contextlib.contextmanager
def recording(log):
    """Every wrapper in _JOBS appends "name jobs" to `log` and runs; ops' own calls between wrappers (conv_fwd -> conv_fwd_grouped,
    norm_bwd_apply -> norm_bwd_apply_multi -> stat_arena) go through the module's globals and are seen too."""
    from supervised_gan_amd import ops
    saved = {name: getattr(ops, name) for name in _JOBS}

    def wrap(name, fn):
        def call(*a, **k):
            log.append(f"{name} {_JOBS[name](a)}")
            return fn(*a, **k)
        return call
    for name, fn in saved.items():
        setattr(ops, name, wrap(name, fn))
    try:
        yield log
    finally:
        for name, fn in saved.items():
            setattr(ops, name, fn)


def _G(N, dropout=False):
    return N.define_G(2, 0, 8, "fcgan", "instance", dropout, n_layers_G=5, use_fcn=True, noise_nc=8, gpu_ids=[0])


def _Ds(N):
    return [N.define_D(2, 8, "n_layers", n_layers_D=3, norm="instance", use_sigmoid=True, scale_factor=s, gpu_ids=[0]) for s in (1, 2, 4)]


def _latent(seed, grad=True):
    g = torch.Generator().manual_seed(seed)
    buf = torch.zeros(2, 2, 8, device="cuda")
    from supervised_gan_amd import ops
    v = ops.logical_view(buf, 8)
    v.copy_(torch.randn(1, 8, 2, 2, generator=g).cuda())
    return v.requires_grad_(grad)


def _image(seed, hw=128, grad=False):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(1, 2, hw, hw, generator=g) * 2 - 1).cuda().requires_grad_(grad)


def case_fcgan_g(N, dropout=False):
    G = _G(N, dropout)
    log = []
    with recording(log):
        y = G.forward(_latent(1))
        (y * _image(2)).sum().backward()
    return log


def case_fcgan_g_dropout(N):
    return case_fcgan_g(N, dropout=True)


def case_fcgan_g_keep_pair(N):
    from supervised_gan_amd import chain
    G = _G(N)
    zb = _latent(1, grad=False)
    log = []
    with recording(log):
        G._keep_next = True
        G.forward(zb)
        zb.copy_(_latent(3, grad=False))
        ya, yb = chain.forward_pair(G, _latent(2, grad=False), zb)
        (yb * _image(2)).sum().backward()
    return log


def _d_single(N, need_dx):
    D = _Ds(N)[0]
    crit = N.GANLoss(use_lsgan=False)
    log = []
    with recording(log):
        crit(D.forward(_image(4, grad=need_dx)), True).backward()
    return log


def case_d_single_dx(N):
    return _d_single(N, True)


def case_d_single_nodx(N):
    return _d_single(N, False)


def _d_multi(N, grad_a, grad_b, wgrad=True):
    Ds = _Ds(N)
    for d in Ds:
        d.fuse_sigmoid_into_loss = True
        d.compute_param_grads = wgrad
    crit = N.GANLoss(use_lsgan=False)
    xa, xb = _image(5, 160, grad_a), _image(6, 160, grad_b)
    log = []
    with recording(log):
        preds = N.multi_forward([(d, xa) for d in Ds] + [(d, xb) for d in Ds])
        sum(crit(p, i % 2 == 0) for i, p in enumerate(preds)).backward()
    return log


def case_d_multi_dx_both(N):
    return _d_multi(N, True, True)


def case_d_multi_dx_one(N):
    return _d_multi(N, True, False)


def case_d_multi_no_dx(N):
    return _d_multi(N, False, False)


def case_d_multi_dx_only(N):
    return _d_multi(N, True, False, wgrad=False)


def case_recon_closure(N):
    """The reconstruction closure: grouped forward without running-statistics update, backward without weight gradients into given
    latent-gradient buffers."""
    from supervised_gan_amd import ops
    from supervised_gan_amd.reconstruct import LatentReconstructor
    G = _G(N)
    Z = torch.stack([ops.as_nhwc(_latent(10 + j, grad=False)).clone() for j in range(3)])
    rec = LatentReconstructor(G, _image(7), Z, 8, n_steps=1, lr=0.1, graph=False)
    log = []
    with recording(log):
        rec._closure_grouped()
    return log


CASES = {f.__name__[5:]: f for f in (case_fcgan_g, case_fcgan_g_dropout, case_fcgan_g_keep_pair, case_d_single_dx, case_d_single_nodx,
                                     case_d_multi_dx_both, case_d_multi_dx_one, case_d_multi_no_dx, case_d_multi_dx_only,
                                     case_recon_closure)}
MATHS = ("bf16x3", "f32")


def run_case(name, math):
    from supervised_gan_amd import _lib, networks, ops
    _lib.lib()
    prev = ops.get_math()
    ops.set_math(math)
    try:
        torch.manual_seed(0)
        log = CASES[name](networks)
        torch.cuda.synchronize()
    finally:
        ops.set_math(prev)
    return log


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("name", list(CASES))
def test_chain_launch_sequence(name, math):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    with open(GOLDEN) as f:
        want = json.load(f)[math][name]
    got = run_case(name, math)
    assert len(want) > 0
    assert got == want, "\n".join(f"{i}: {a!r} != {b!r}" for i, (a, b) in enumerate(zip(got, want)) if a != b)[:2000] + f"\n{len(got)} vs {len(want)} calls"


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    out = {math: {name: run_case(name, math) for name in CASES} for math in MATHS}
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=0)
    print({m: {n: len(v) for n, v in d.items()} for m, d in out.items()})

"""FCGANModel.reconstruction (models/fcgan_model.py:238-302) on the MI355X path against a CPU restatement of the reference's
reconstruct_cells -- the oracle's FCGANGenerator forward (BatchNorm in train mode) in float64 driven by torch.optim.LBFGS -- with the
same generator weights and the same trial latents: the first closure's loss and latent gradient, the latents after the first step(),
the closed-form log-likelihoods, the best-trial choice, graphed against eager, and the generator handed back unchanged."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sgan_oracle as O  # noqa: E402
from test_hip_step import build_model, real3  # noqa: E402

SMALL = dict(ngf=8, ndf=8, n_layers_G=3, noise_nc=8, noiseSize=4, n_update_G=1)      # z 8x4x4 -> 2x64x64


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def _model(cfg):
    m = build_model(cfg, 0)
    real = real3(cfg, 0).cuda()
    m.set_input({'A': real, 'A_paths': ['x.png']})
    return m, real[:, :2].double().cpu()


def _oracle_cells(sd, real2, z0, cfg, n_steps, lr=0.1):
    """reconstruct_cells of the reference in float64 on the CPU: (first loss, first latent gradient, latent after each step)."""
    sd = {k: v.double() for k, v in sd.items()}
    label = (real2 + 1) / 2.0
    noise = z0.double().contiguous().clone().requires_grad_(True)
    opt = torch.optim.LBFGS([noise], lr=lr)
    first = {}

    def closure():
        opt.zero_grad()
        gen = O.fcgan_g_forward(sd, noise, cfg.n_layers_G, update_running=False)
        loss = torch.nn.BCELoss()((gen + 1) / 2.0, label)
        loss.backward()
        if not first:
            first.update(loss=float(loss.detach()), grad=noise.grad.detach().clone())
        return loss

    zs = []
    for _ in range(n_steps):
        opt.step(closure)
        zs.append(noise.detach().clone())
    return first["loss"], first["grad"], zs


def _gen_state(m):
    return {k: v.detach().clone() for k, v in m.netG.state_dict().items()}


def test_first_closure_and_first_step_match_reference():
    cfg = O.FCGANConfig(**SMALL)
    m, real2 = _model(cfg)
    sd = {k: v.detach().cpu() for k, v in m.netG.state_dict().items()}
    zshape = (1, cfg.noise_nc, cfg.noiseSize, cfg.noiseSize)
    from supervised_gan_amd.reconstruct import LatentReconstructor
    from supervised_gan_amd import ops
    z0 = [O.np_normal(5000 + j, zshape) for j in range(3)]
    Z = torch.stack([ops.as_nhwc(z.cuda()).clone() for z in z0])
    rec = LatentReconstructor(m.netG, m.input, Z, cfg.noise_nc, n_steps=1, lr=0.1, graph=False)
    rec._closure_grouped()
    torch.cuda.synchronize()
    oracle = [_oracle_cells(sd, real2, z0[j], cfg, 1) for j in range(3)]
    for j in range(3):
        loss0, g0, _ = oracle[j]
        assert abs(float(rec.loss[j]) - loss0) <= 1e-4 * abs(loss0), (j, float(rec.loss[j]), loss0)
        g = ops.logical_view(rec.G[j], cfg.noise_nc)
        assert _rel(g, g0) <= 1e-4, (j, _rel(g, g0))
    before = _gen_state(m)
    e, ll, ll0 = m.reconstruction(num_trials=3, n_steps=1, lr=0.1)      # the model draws the same three latents (noise_source)
    for j in range(3):
        assert _rel(m.recon_trials["latents_init"][j], z0[j]) == 0.0
        assert _rel(m.recon_trials["latents"][j], oracle[j][2][0]) <= 1e-3, (j, _rel(m.recon_trials["latents"][j], oracle[j][2][0]))
    after = _gen_state(m)
    assert all(torch.equal(before[k], after[k]) for k in before), [k for k in before if not torch.equal(before[k], after[k])]


def test_reconstruction_improves_and_reports_reference_quantities():
    from scipy.stats import multivariate_normal
    cfg = O.FCGANConfig(**SMALL)
    m, real2 = _model(cfg)
    sd = {k: v.detach().cpu() for k, v in m.netG.state_dict().items()}
    e, ll, ll0 = m.reconstruction(num_trials=3, n_steps=4, lr=0.1)
    tr = m.recon_trials
    n = cfg.noise_nc * cfg.noiseSize ** 2
    mvn = multivariate_normal(np.zeros(n), np.identity(n))
    for j in range(3):
        z = tr["latents"][j].detach().cpu().double().reshape(-1).numpy()
        z0 = tr["latents_init"][j].detach().cpu().double().reshape(-1).numpy()
        assert abs(tr["ll"][j] + mvn.logpdf(z)) <= 1e-6 * abs(mvn.logpdf(z))
        assert abs(tr["ll_init"][j] + mvn.logpdf(z0)) <= 1e-6 * abs(mvn.logpdf(z0))
        # initial error of the trial (the reference's recon_init) is above the final one
        with torch.no_grad():
            y0 = O.fcgan_g_forward({k: v.double() for k, v in sd.items()}, torch.as_tensor(z0).view(1, cfg.noise_nc, cfg.noiseSize,
                                   cfg.noiseSize), cfg.n_layers_G, update_running=False)
            e0 = float(torch.nn.BCELoss()((y0 + 1) / 2, (real2 + 1) / 2))
        assert tr["errors"][j] < e0, (j, tr["errors"][j], e0)
        assert all(c["done"] == 1 and c["steps"] == 4 for c in tr["counters"])
    best = min(range(3), key=lambda j: (tr["errors"][j], j))
    assert tr["best"] == best and e == tr["errors"][best] and ll == tr["ll"][best] and ll0 == tr["ll_init"][best]
    assert m.noise.shape == (1, cfg.noise_nc, cfg.noiseSize, cfg.noiseSize)
    assert m.fake.shape == m.fake_init.shape == (1, 2, cfg.fineSize, cfg.fineSize)
    # every trial's final reconstruction error against the f64 reference after the same steps, and the reference's choice of the
    # best trial wherever its trial errors are apart by more than 5 %
    e_ref = []
    for j in range(3):
        zs = _oracle_cells(sd, real2, tr["latents_init"][j].detach().cpu(), cfg, 4)[2]
        with torch.no_grad():
            y = O.fcgan_g_forward({k: v.double() for k, v in sd.items()}, zs[-1], cfg.n_layers_G, update_running=False)
            e_ref.append(float(torch.nn.BCELoss()((y + 1) / 2, (real2 + 1) / 2)))
        assert abs(tr["errors"][j] - e_ref[j]) <= 0.02 * e_ref[j], (j, tr["errors"][j], e_ref[j])
    ref_best = min(range(3), key=lambda j: (e_ref[j], j))
    if all(abs(e_ref[ref_best] - e_ref[j]) > 0.05 * e_ref[ref_best] for j in range(3) if j != ref_best):
        assert tr["best"] == ref_best, (tr["errors"], e_ref)


def test_graphed_equals_eager_at_readme_shape():
    cfg = O.FCGANConfig()        # ngf 32, n_layers_G 5, z 8x8x8 -> 2x512x512
    m, _ = _model(cfg)
    before = _gen_state(m)
    out = {}
    for graph in (False, True):
        m.noise_source = (lambda it: (lambda: next(it)))(iter([O.np_normal(9000 + j, (1, 8, 8, 8)) for j in range(3)]))
        m.reconstruction(num_trials=3, n_steps=2, lr=0.1, graph=graph)
        out[graph] = ([z.detach().clone() for z in m.recon_trials["latents"]], m.recon_trials["counters"])
    for j in range(3):
        assert _rel(out[True][0][j], out[False][0][j]) <= 1e-5
    assert out[True][1] == out[False][1]
    after = _gen_state(m)
    assert all(torch.equal(before[k], after[k]) for k in before)


def test_training_step_between_reconstructions():
    cfg = O.FCGANConfig(**SMALL)
    m, real2 = _model(cfg)
    fresh, _ = _model(cfg)
    sd0 = {k: v.detach().cpu() for k, v in m.netG.state_dict().items()}
    m.reconstruction(num_trials=2, n_steps=1)
    first = [z.detach().clone() for z in m.recon_trials["latents"]]
    for j in range(2):      # the first reconstruction is right
        zs = _oracle_cells(sd0, real2, O.np_normal(5000 + j, (1, 8, 4, 4)), cfg, 1)[2]
        assert _rel(first[j], zs[0]) <= 1e-3, (j, _rel(first[j], zs[0]))
    step_src = lambda: (lambda it: (lambda: next(it)))(iter([O.np_normal(7700 + i, (1, 8, 4, 4)) for i in range(8)]))
    for mm in (m, fresh):
        mm.noise_source = step_src()
        mm.optimize_parameters()
    torch.cuda.synchronize()
    # the same step as on a model that never reconstructed.  Bit equality is not to be had -- the step's own floating-point atomics
    # sum in any order, and Adam's first step moves an element by ~lr however small its gradient -- so: the losses agree, and all but
    # a few elements whose gradient sums to ~0 agree to 1e-3 of a step
    a, b = _gen_state(m), _gen_state(fresh)
    lr = m.opt.lr
    # the bias of a conv feeding a BatchNorm has a gradient that is zero up to rounding: its Adam step is the sign of that rounding
    noise_only = {f"model.{L.key}.bias" for L in m.netG.layers if L.bias and L.norm == "bn"}
    for k in a:
        if k in noise_only:
            assert float((a[k].double() - b[k].double()).abs().max()) <= 2 * lr, k
            continue
        if not a[k].is_floating_point():
            assert torch.equal(a[k], b[k]), k
            continue
        d = (a[k].double() - b[k].double()).abs()
        assert float(d.max()) <= 2 * lr, k
        assert int((d > 1e-3 * lr).sum()) <= max(2, d.numel() // 1000), (k, int((d > 1e-3 * lr).sum()), d.numel())
    assert abs(float(m.loss_G.detach()) - float(fresh.loss_G.detach())) <= 1e-5 * abs(float(fresh.loss_G.detach()))
    assert abs(float(m.loss_D.detach()) - float(fresh.loss_D.detach())) <= 1e-5 * abs(float(fresh.loss_D.detach()))
    # a reconstruction after the step sees the updated weights
    sd = {k: v.detach().cpu() for k, v in m.netG.state_dict().items()}
    z0 = O.np_normal(8800, (1, 8, 4, 4))
    m.noise_source = lambda: z0
    m.reconstruction(num_trials=1, n_steps=1)
    zs = _oracle_cells(sd, real2, z0, cfg, 1)[2]
    assert _rel(m.recon_trials["latents"][0], zs[0]) <= 1e-3


def test_interpolate_and_fixed_noise():
    cfg = O.FCGANConfig(**SMALL)
    m, _ = _model(cfg)
    m.reconstruction(num_trials=1, n_steps=1)
    m.set_fixed_noise('A')
    assert m.fixed_noiseA is m.noise
    m.interpolate(0.0)
    assert m.fake.shape == (1, 2, cfg.fineSize, cfg.fineSize)
    assert math.isfinite(float(m.fake.abs().max()))


def test_eager_fallback_matches_grouped_and_reference():
    """The per-trial autograd path (what fcgan_star and dropout generators take) on the plain generator: the same latents, errors and
    counters as the grouped program (which test_first_closure_and_first_step_match_reference pins to the f64 reference), running
    statistics restored, no weight gradients."""
    cfg = O.FCGANConfig(**SMALL)
    m, real2 = _model(cfg)
    from supervised_gan_amd import ops
    from supervised_gan_amd.reconstruct import LatentReconstructor
    z0 = [O.np_normal(5100 + j, (1, 8, 4, 4)) for j in range(2)]
    Z = torch.stack([ops.as_nhwc(z.cuda()).clone() for z in z0])
    before, gflat = _gen_state(m), m.netG._gflat.clone()
    out = {}
    for grouped in (True, False):
        rec = LatentReconstructor(m.netG, m.input, Z, cfg.noise_nc, n_steps=1, lr=0.1, graph=False)
        rec.grouped = grouped
        rec.run()
        imgs = rec.images(rec.Z)
        out[grouped] = ([ops.logical_view(rec.Z[j], 8).clone() for j in range(2)], rec.errors(imgs), rec.opt.counters())
    for j in range(2):
        assert _rel(out[False][0][j], out[True][0][j]) <= 1e-5
        assert abs(out[False][1][j] - out[True][1][j]) <= 1e-5 * out[True][1][j]
    assert out[False][2] == out[True][2]
    assert torch.equal(m.netG._gflat, gflat)          # no weight gradients computed on either path
    after = _gen_state(m)
    assert all(torch.equal(before[k], after[k]) for k in before), [k for k in before if not torch.equal(before[k], after[k])]


def test_fcgan_star_reconstruction_matches_reference():
    """fcgan_star takes the per-trial autograd path: its first closure against the f64 reference, then the whole step() against
    torch.optim.LBFGS driving the same HIP closure (same fp32 losses, so the same decisions), generator state unchanged."""
    from supervised_gan_amd import networks as N
    from supervised_gan_amd import ops
    from supervised_gan_amd.losses import bce_on_rescaled
    from supervised_gan_amd.reconstruct import LatentReconstructor, grouped_supported
    nz, ngf = 8, 4
    G = N.define_G(2, 0, ngf, "fcgan_star", "batch", False, n_layers_G=5, use_fcn=True, noise_nc=nz, gpu_ids=[0])
    sd = O.init_fcgan_star(81, nz, ngf)
    G.load_state_dict(sd)
    assert not grouped_supported(G)
    real = O.np_uniform(7100, (1, 2, 128, 128)).cuda()
    z0 = O.np_normal(801, (1, nz, 2, 2))
    rec = LatentReconstructor(G, real, ops.as_nhwc(z0.cuda()).clone().unsqueeze(0), nz, n_steps=2, lr=0.1)
    with torch.no_grad():
        saved = [b.clone() for b in G.buffers()]
    rec._closure_eager()        # alone, outside run(): restore the running statistics it advanced
    with torch.no_grad():
        for b, v in zip(G.buffers(), saved):
            b.copy_(v)
    before = {k: v.detach().clone() for k, v in G.state_dict().items()}
    sd64 = {k: v.double().clone() for k, v in sd.items()}
    z64 = z0.double().clone().requires_grad_(True)
    loss64 = torch.nn.BCELoss()((O.fcgan_star_forward(sd64, z64, nz) + 1) / 2, (real.double().cpu() + 1) / 2)
    loss64.backward()
    assert abs(float(rec.loss[0]) - float(loss64.detach())) <= 1e-4 * float(loss64.detach())
    assert _rel(ops.logical_view(rec.G[0], nz), z64.grad) <= 1e-4
    rec.run()
    after = {k: v.detach().clone() for k, v in G.state_dict().items()}
    assert all(torch.equal(before[k], after[k]) for k in before), [k for k in before if not torch.equal(before[k], after[k])]
    # torch.optim.LBFGS over the same HIP closure
    z = z0.cuda().clone().requires_grad_(True)
    opt = torch.optim.LBFGS([z], lr=0.1)

    def closure():
        opt.zero_grad()
        loss = bce_on_rescaled(G.forward(z), real)
        loss.backward()
        return loss
    for _ in range(2):
        opt.step(closure)
    c = rec.opt.counters()[0]
    assert (c["func_evals"], c["n_iter"]) == (opt.state[z]["func_evals"], opt.state[z]["n_iter"]), (c, opt.state[z]["func_evals"])
    got = ops.logical_view(rec.Z[0], nz)
    assert _rel(got - z0.cuda(), z.detach() - z0.cuda()) <= 1e-4, _rel(got - z0.cuda(), z.detach() - z0.cuda())


def test_next_image_reuses_the_captured_program():
    cfg = O.FCGANConfig(**SMALL)
    m, _ = _model(cfg)
    res = []
    for _ in range(2):
        m.noise_source = (lambda it: (lambda: next(it)))(iter([O.np_normal(9100 + j, (1, 8, 4, 4)) for j in range(2)]))
        m.reconstruction(num_trials=2, n_steps=2)
        res.append(([z.detach().clone() for z in m.recon_trials["latents"]], m.recon_trials["counters"]))
    assert len(m._recon_cache) == 1
    rec = next(iter(m._recon_cache.values()))
    assert rec._graph is not None
    assert res[0][1] == res[1][1]
    assert all(_rel(a, b) <= 1e-6 for a, b in zip(res[0][0], res[1][0]))

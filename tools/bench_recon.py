#!/usr/bin/env python3
"""Latent reconstruction throughput at README shape (ngf 32, n_layers_G 5, z 8x8x8 -> 2x512x512, 3 trials): closures/s and seconds per
image (3 trials x `--steps` LBFGS step() calls) for the captured program, the eager program, and torch.optim.LBFGS driving the same
HIP closure (one trial at a time, the reference's loop).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--baseline_steps", type=int, default=2, help="torch.optim.LBFGS step() calls per trial timed (then scaled)")
    a = ap.parse_args()
    import sgan_oracle as O
    from supervised_gan_amd.fcgan_model import FCGANModel
    from supervised_gan_amd.losses import bce_on_rescaled
    from supervised_gan_amd.options import TrainOptions
    cfg = O.FCGANConfig()
    argv = ["--name", "bench_recon", "--model", "fcgan", "--which_direction", "A", "--fineSize", str(cfg.fineSize), "--input_nc", "2",
            "--which_model_netG", "deconv", "--n_layers_G", str(cfg.n_layers_G), "--ngf", str(cfg.ngf), "--which_model_netD", "n_layers",
            "--n_layers_D", "3", "--ndf", "8", "--scale_factor", "1", "--lambda_D", "1", "--noise_nc", str(cfg.noise_nc),
            "--noiseSize", str(cfg.noiseSize), "--norm", "instance", "--no_dropout", "--which_channel", "rg", "--gpu_ids", "0",
            "--checkpoints_dir", "/tmp/sgan_bench_recon"]
    m = FCGANModel()
    m.initialize(TrainOptions().parse(argv, save=False, verbose=False))
    m.netG.load_state_dict(O.init_fcgan_g(1, cfg.noise_nc, 2, cfg.ngf, cfg.n_layers_G))
    m.set_input({'A': O.np_uniform(7000, (1, 3, cfg.fineSize, cfg.fineSize)).cuda(), 'A_paths': ['x.png']})
    out = {"shape": "ngf32 nG5 z8x8x8 2x512x512", "trials": 3, "steps": a.steps}
    for graph in (True, False):
        m.reconstruction(num_trials=3, n_steps=a.steps, graph=graph)      # warm-up: the capture (graphed) happens here, once per shape
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.reconstruction(num_trials=3, n_steps=a.steps, graph=graph)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        k = "graphed" if graph else "eager"
        out[k + "_s_per_image"] = round(dt, 4)
        out[k + "_closures_per_s"] = round(m.recon_trials["closures"] / dt, 1)      # grouped closures (3 trials each)
        out[k + "_closures_issued"] = m.recon_trials["closures"]      # replays (rounded up to the done-flag check interval)
        out[k + "_func_evals"] = sum(c["func_evals"] for c in m.recon_trials["counters"])     # what torch's LBFGS would evaluate
    # baseline: torch.optim.LBFGS over the same HIP generator and BCE kernel, one trial, n step() calls
    z = m._draw_noise().detach().clone(memory_format=torch.contiguous_format).requires_grad_(True)
    opt = torch.optim.LBFGS([z], lr=0.1)
    evals = [0]
    saved = [b.detach().clone() for b in m.netG.buffers()]

    def closure():
        opt.zero_grad()
        loss = bce_on_rescaled(m.netG.forward(z), m.input)
        loss.backward()
        evals[0] += 1
        return loss
    opt.step(closure)
    torch.cuda.synchronize()
    evals[0] = 0
    t0 = time.perf_counter()
    for _ in range(a.baseline_steps):
        opt.step(closure)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    with torch.no_grad():
        for b, v in zip(m.netG.buffers(), saved):
            b.copy_(v)
    per_eval = dt / max(evals[0], 1)
    out["torch_lbfgs_closures_per_s"] = round(evals[0] / dt, 1)
    # seconds per image at the closure evaluations torch's LBFGS makes for the same three trials (the sum of their func_evals)
    out["torch_lbfgs_s_per_image_est"] = round(per_eval * out["graphed_func_evals"], 3)
    out["speedup_vs_torch_lbfgs"] = round(out["torch_lbfgs_s_per_image_est"] / out["graphed_s_per_image"], 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

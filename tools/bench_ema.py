"""Cost of the weight average (sgan_ema_multi) on the generator arenas of the three bench workloads -- the fcgan
generator (deconv, ngf 32), unet_256 (ngf 64, the cgan bench) and the segmentation U-Net (unet_256, ngf 32) -- in two comparisons:
  (a) launch: `--batch` sgan_ema_multi calls between two events against `--batch` sgan_adam_multi calls on the SAME segments from the
      same build, alternating, `--steps` samples each after `--warmup`; per call: median, min, p90.  The average moves 12 bytes per
      parameter, Adam 28: it should not take longer.  The bytes over the median give the achieved rate; per kernel the JSON says
      whether the call's arrays (2 for the average, 4 for Adam) fit the 256 MiB last-level cache -- then it is a cache rate -- or not.
  (b) step: the graphed 512 x 512 step of `--model segmentation --which_model_netD None` and of the fcgan bench recipe, without the
      option (the step as it was before the option existed) and with `--ema_decay 0.999`, both captured in this process and timed in
      alternating rounds of `--round` replays ending in a synchronise; per step: median, min, p90 and the difference of the medians.
The clocks `rocm-smi --showclocks` reports are recorded before and after (a query; nothing is set)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_region_stats import clocks, stats  # noqa: E402
from supervised_gan_amd import networks, ops  # noqa: E402
from supervised_gan_amd.optim import WeightEMA  # noqa: E402

LAST_LEVEL_CACHE = 256 << 20      # bytes; a call whose arrays fit is served from it between back-to-back calls

GENERATORS = {      # name -> define_G arguments of the bench workloads
    "fcgan_G_deconv_ngf32": dict(input_nc=2, output_nc=0, ngf=32, which_model_netG="deconv", norm="instance", use_dropout=False,
                                 n_layers_G=5, use_fcn=True, noise_nc=8),
    "cgan_G_unet_256_ngf64": dict(input_nc=2, output_nc=1, ngf=64, which_model_netG="unet_256", norm="instance", use_dropout=True,
                                  add_gaussian_noise=True),
    "segmentation_G_unet_256_ngf32": dict(input_nc=1, output_nc=2, ngf=32, which_model_netG="unet_256", norm="instance", use_dropout=False),
}
STEPS = {
    "segmentation_noD": (["--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "512",
                          "--which_model_netG", "unet_256", "--ngf", "32", "--which_model_netD", "None", "--norm", "instance", "--no_dropout",
                          "--which_channel", "b_rg", "--weights", "1", "2"]),
    "fcgan": (["--model", "fcgan", "--which_direction", "A", "--dataset_mode", "single", "--loadSize", "512", "--fineSize", "512",
               "--input_nc", "2", "--which_model_netG", "deconv", "--n_layers_G", "5", "--ngf", "32", "--which_model_netD", "n_layers",
               "--n_layers_D", "3", "3", "3", "--ndf", "32", "--scale_factor", "1", "2", "4", "--lambda_D", "0.5", "0.4", "0.1",
               "--noise_nc", "8", "--noiseSize", "8", "--norm", "instance", "--no_dropout", "--n_update_G", "2", "--no_lsgan",
               "--which_channel", "rg"]),
}


def launch_comparison(name, kw, a, dev):
    mk = lambda: networks.define_G(gpu_ids=[0], **kw)      # noqa: E731
    live, shadow = mk(), mk()
    ema = WeightEMA(live, shadow, 0.999, True)
    esegs = ema.segments()
    n = sum(s.numel() for s, _ in esegs)
    grads = [torch.randn_like(p) * 1e-3 for _, p in esegs]
    asegs = [(p, g, torch.zeros_like(p), torch.zeros_like(p), p.numel()) for (_, p), g in zip(esegs, grads)]
    lr = torch.full((1,), 2e-4, dtype=torch.float32, device=dev)
    astate = torch.zeros(4, dtype=torch.int32, device=dev)
    calls = {"ema_multi": lambda: ops.ema_multi(esegs, 0.999, True, ema._state),
             "adam_multi": lambda: ops.adam_multi(asegs, lr, 0.5, 0.999, 1e-8, astate)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in calls}
    for i in range(a.warmup + a.steps):
        for k, f in calls.items():      # alternating: both see the same clocks and the same neighbours
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.batch):
                f()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms[k].append(e0.elapsed_time(e1) / a.batch)
    res = {"parameters": n, "segments": len(esegs), "calls_per_sample": a.batch,
           "note": "per call = one prep launch + one streaming launch, back to back on one stream"}
    for k, nbytes, arrays in (("ema_multi", 12, 2), ("adam_multi", 28, 4)):      # shadow, p  /  p, g, m, v
        st = stats(ms[k])
        st["bytes_per_call"] = nbytes * n
        st["GB_per_s_at_median"] = nbytes * n / (st["median_ms"] * 1e-3) / 1e9
        st["footprint_MB"] = 4e-6 * arrays * n
        st["fits_256MiB_last_level_cache"] = 4 * arrays * n <= LAST_LEVEL_CACHE
        st["rate_is"] = ("a cache rate: the call's arrays stay in the last-level cache between calls" if st["fits_256MiB_last_level_cache"]
                         else "essentially an HBM rate: the call's arrays exceed the last-level cache")
        res[k] = st
    res["ema_over_adam_median"] = res["ema_multi"]["median_ms"] / res["adam_multi"]["median_ms"]
    print(name, json.dumps(res))
    return res


def step_comparison(name, argv, a, dev):
    from supervised_gan_amd.graph_step import GraphedStep
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    g = torch.Generator().manual_seed(1)
    ring = [{"A": (torch.rand(1, 3, 512, 512, generator=g) * 2 - 1).to(dev), "B": (torch.rand(1, 3, 512, 512, generator=g) * 2 - 1).to(dev),
             "A_paths": ["s"], "B_paths": ["s"]} for _ in range(4)]
    runs = {}
    for label, extra in (("without", []), ("with_ema_decay", ["--ema_decay", "0.999", "--ema_warmup"])):
        torch.manual_seed(0)
        opt = TrainOptions().parse(["--name", "bench_ema", "--gpu_ids", "0", "--manualSeed", "1", "--checkpoints_dir", "/tmp/sgan_bench_ckpt",
                                    *argv, *extra], save=False, verbose=False)
        m = create_model(opt)
        gs = GraphedStep(m)
        gs.capture(ring[0])
        runs[label] = gs
    ms = {k: [] for k in runs}
    for i in range(a.warmup_rounds + a.rounds):
        for k, gs in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for j in range(a.round):
                gs.step(ring[j % len(ring)])
            torch.cuda.synchronize()
            if i >= a.warmup_rounds:
                ms[k].append((time.perf_counter() - t0) * 1e3 / a.round)
    res = {k: stats(v) for k, v in ms.items()}
    res["steps_per_sample"] = a.round
    res["ema_updates"] = runs["with_ema_decay"].m.ema.count
    res["delta_median_ms"] = res["with_ema_decay"]["median_ms"] - res["without"]["median_ms"]
    res["delta_median_percent"] = 100.0 * res["delta_median_ms"] / res["without"]["median_ms"]
    print(name, json.dumps(res))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="(a): samples per kernel")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=20, help="(a): calls per sample")
    ap.add_argument("--rounds", type=int, default=30, help="(b): samples per variant")
    ap.add_argument("--warmup_rounds", type=int, default=3)
    ap.add_argument("--round", type=int, default=50, help="(b): replayed steps per sample")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_ema.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    out = {"clocks_before": clocks(), "device": torch.cuda.get_device_name(0), "unit": "ms", "steps": a.steps, "warmup": a.warmup,
           "launch": {}, "graphed_step_512": {}}
    for name, kw in GENERATORS.items():
        out["launch"][name] = launch_comparison(name, kw, a, dev)
    for name, argv_ in STEPS.items():
        out["graphed_step_512"][name] = step_comparison(name, argv_, a, dev)
    out["clocks_after"] = clocks()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":
    main()

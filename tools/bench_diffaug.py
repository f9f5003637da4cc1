"""Cost of the augmentation of discriminator inputs (sgan_diffaug_multi_fwd / _bwd) in two comparisons:
  (a) launch: forward and backward of one 512 x 512 image with 4 stored channels (3 logical, colour channel 2) under a record with a
      shift and a cutout, in the one-launch form (no contrast) and in the two-launch form (contrast 1.25), against a plain device
      `copy_` of the same tensor -- the memory-speed yardstick: 4 MiB read, 4 MiB written.  By bytes the one-launch form is 1 x the copy
      and the two-launch form 1.5 x (one more read).  `--batch` calls between two events, alternating, `--steps` samples each after
      `--warmup`; per call: median, min, p90.  4 MiB tensors stay in the last-level cache between back-to-back calls: these are cache
      rates and launch floors, not HBM rates.
  (b) step: the graphed 512 x 512 step of the cgan bench recipe (unet_256, ngf 64) and of the fcgan bench recipe, without the option
      and with `--diffaug translation,cutout,color`, both captured in this process and timed in alternating rounds of `--round`
      replays ending in a synchronise; per step: median, min, p90 and the difference of the medians.
The clocks `rocm-smi --showclocks` reports are recorded before and after (a query; nothing is set)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_region_stats import clocks, stats  # noqa: E402
from supervised_gan_amd import ops  # noqa: E402

STEPS = {
    "cgan_unet_256": (["--model", "cgan", "--which_direction", "AtoB", "--dataset_mode", "single", "--loadSize", "1024", "--fineSize", "512",
                       "--input_nc", "2", "--output_nc", "1", "--which_model_netG", "unet_256", "--ngf", "64", "--which_model_netD", "n_layers",
                       "--n_layers_D", "3", "4", "--ndf", "64", "--scale_factor", "1", "1", "--lambda_D", "0.5", "0.5", "--lambda_A", "10",
                       "--noise_nc", "8", "--noiseSize", "4", "--norm", "instance", "--weights", "2", "4", "--no_lsgan", "--add_gaussian_noise",
                       "--which_channel", "rg_b"], []),
    "fcgan": (["--model", "fcgan", "--which_direction", "A", "--dataset_mode", "single", "--loadSize", "512", "--fineSize", "512",
               "--input_nc", "2", "--which_model_netG", "deconv", "--n_layers_G", "5", "--ngf", "32", "--which_model_netD", "n_layers",
               "--n_layers_D", "3", "3", "3", "--ndf", "32", "--scale_factor", "1", "2", "4", "--lambda_D", "0.5", "0.4", "0.1",
               "--noise_nc", "8", "--noiseSize", "8", "--norm", "instance", "--no_dropout", "--n_update_G", "2", "--no_lsgan",
               "--which_channel", "rg"], ["--diffaug_color_channels", "g"]),
}


def _records(recs, dev):
    arr = np.zeros((len(recs), 8), dtype=np.int32)
    arr[:, :2] = np.array([r[:2] for r in recs], dtype=np.float32).view(np.int32)
    arr[:, 2:] = np.array([r[2:] for r in recs], dtype=np.int64)
    return torch.from_numpy(arr).to(dev)


def launch_comparison(a, dev):
    H = W = 512
    x = torch.randn((H, W, 4), dtype=torch.float32, device=dev)
    y = torch.empty_like(x)
    ws = ops.diffaug_workspace(1, dev)
    geo = (40, -25, 100, 356, 200, 456)
    plain, contrast = _records([(0.25, 1.0) + geo], dev), _records([(0.25, 1.25) + geo], dev)
    calls = {"copy_": lambda: y.copy_(x),
             "fwd": lambda: ops.diffaug_multi_fwd([x], [y], [3], 0b100, plain, None),
             "bwd": lambda: ops.diffaug_multi_bwd([x], [y], [3], 0b100, plain, None),
             "fwd_contrast": lambda: ops.diffaug_multi_fwd([x], [y], [3], 0b100, contrast, ws),
             "bwd_contrast": lambda: ops.diffaug_multi_bwd([x], [y], [3], 0b100, contrast, ws)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in calls}
    for i in range(a.warmup + a.steps):
        for k, f in calls.items():      # alternating: all see the same clocks and the same neighbours
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.batch):
                f()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms[k].append(e0.elapsed_time(e1) / a.batch)
    nbytes = x.numel() * 4
    res = {"shape": [H, W, 4], "calls_per_sample": a.batch, "record": {"ty": 40, "tx": -25, "cutout": list(geo[2:])},
           "note": "a 4 MiB tensor stays in the last-level cache between back-to-back calls: cache rates and launch floors"}
    for k, moved, launches in (("copy_", 2, 1), ("fwd", 2, 1), ("bwd", 2, 1), ("fwd_contrast", 3, 2), ("bwd_contrast", 3, 2)):
        st = stats(ms[k])
        st["bytes_per_call_at_most"] = moved * nbytes      # pixels with K = 0 are not read
        st["launches"] = launches
        st["byte_ratio_to_copy"] = moved / 2
        res[k] = st
    for k in ("fwd", "bwd", "fwd_contrast", "bwd_contrast"):
        res[k]["time_ratio_to_copy"] = res[k]["median_ms"] / res["copy_"]["median_ms"]
    print("launch", json.dumps(res))
    return res


def step_comparison(name, argv, aug_extra, a, dev):
    from supervised_gan_amd.graph_step import GraphedStep
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    g = torch.Generator().manual_seed(1)
    ring = [{"A": (torch.rand(1, 3, 512, 512, generator=g) * 2 - 1).to(dev), "B": (torch.rand(1, 3, 512, 512, generator=g) * 2 - 1).to(dev),
             "A_paths": ["s"], "B_paths": ["s"]} for _ in range(4)]
    runs = {}
    for label, extra in (("without", []), ("with_diffaug", ["--diffaug", "translation,cutout,color"] + aug_extra)):
        torch.manual_seed(0)
        opt = TrainOptions().parse(["--name", "bench_diffaug", "--gpu_ids", "0", "--manualSeed", "1", "--checkpoints_dir", "/tmp/sgan_bench_ckpt",
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
    res["philox_blocks_drawn"] = int(runs["with_diffaug"].m.diffaug.offset.item())
    res["delta_median_ms"] = res["with_diffaug"]["median_ms"] - res["without"]["median_ms"]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_diffaug.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    out = {"clocks_before": clocks(), "device": torch.cuda.get_device_name(0), "unit": "ms", "steps": a.steps, "warmup": a.warmup,
           "launch_512": launch_comparison(a, dev), "graphed_step_512": {}}
    for name, (argv_, aug_extra) in STEPS.items():
        out["graphed_step_512"][name] = step_comparison(name, argv_, aug_extra, a, dev)
    out["clocks_after"] = clocks()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":
    main()

"""Timing of the sliced Wasserstein score (sgan_swd.hip) on synthetic 64 x 64 images whose statistics differ between
the two sets.  Shapes: N = 3840 (30 images x 128 patches) and N = 16384 (128 x 128) descriptors per set, K = 49 and 147, J = 512
directions.  On data that is already on the device, `--steps` samples after `--warmup`, each sample `--batch` calls between two
events after a synchronise, the paths alternating so that a drift of the clocks meets all alike:
  (a) the three entries: lap_pyramid + swd_gather of one image (all levels), and swd_distances of the finest level in its split form
      (what `auto` runs) and its fused form
  (b) the same distances composed from torch on the same normalised descriptors: matmul, sort, (a - b).abs().mean(0); and torch's
      matmul and sort alone
in microseconds per call, and
  (c) util.swd_ref on the host, wall time, a few repetitions
each as median, min and p90.  The device distances are checked against the yardstick's bound (tests/test_hip_swd.py) before
anything is timed.  The clocks `rocm-smi --showclocks` reports are recorded before and after (a query; nothing is set).  Prints one
JSON line and writes it to --out."""
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
from bench_clean import clocks, stats  # noqa: E402
from supervised_gan_amd import ops  # noqa: E402
from supervised_gan_amd import util as U  # noqa: E402

SHAPES = ((30, 128), (128, 128))      # (images, patches per image)
J, SIDE = 512, 64


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=5, help="calls between the two events of one sample")
    ap.add_argument("--host_reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_swd.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    out = {"clocks_before": clocks(), "steps": a.steps, "warmup": a.warmup, "batch": a.batch, "device": torch.cuda.get_device_name(0),
           "unit": "microseconds per call", "J": J, "image": [SIDE, SIDE]}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def sample(fn):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.batch):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.batch

    for images, P in SHAPES:
        for C in (1, 3):
            N, K = images * P, C * 49
            rng = np.random.RandomState(N + C)
            sets = [rng.uniform(-1, 1, (images, C, SIDE, SIDE)).astype(np.float32),
                    (rng.uniform(-1, 1, (images, C, SIDE, SIDE)) ** 3).astype(np.float32)]
            desc, acc, pos = [], [], []
            dirs = None
            for s in (0, 1):
                p, dirs = U.swd_draw(0, 0, images, P, SIDE, SIDE, K, J, set_index=s)
                pos.append(torch.from_numpy(p).to(dev))
                desc.append(torch.zeros((N, K), dtype=torch.float32, device=dev))
                acc.append(torch.zeros(2 * C, dtype=torch.float64, device=dev))
                for i in range(images):
                    level = ops.lap_pyramid(torch.from_numpy(sets[s][i]).to(dev))[0]
                    ops.swd_gather(level, pos[s][i * P:(i + 1) * P], desc[s], i * P, acc[s])
            ops.check_metric_err(dev)
            d = torch.from_numpy(dirs).to(dev)
            # the device against the yardstick, before anything is timed
            norm = [U.swd_normalise_ref(desc[s].cpu().numpy(), *U.swd_stats_from_sums(acc[s].cpu().numpy(), N * 49)) for s in (0, 1)]
            t0 = time.perf_counter()
            ref = U.swd_ref(norm[0], norm[1], dirs)
            host_us = [(time.perf_counter() - t0) * 1e6]
            for _ in range(a.host_reps - 1):
                t0 = time.perf_counter()
                U.swd_ref(norm[0], norm[1], dirs)
                host_us.append((time.perf_counter() - t0) * 1e6)
            g = K * 2.0 ** -24 / (1 - K * 2.0 ** -24)
            ad = np.abs(dirs.astype(np.float64))
            bound = g * sum((np.abs(v.astype(np.float64)) @ ad.T).max(axis=0) for v in norm) + (N + 2) * 2.0 ** -53 * ref
            res = torch.empty(J, dtype=torch.float64, device=dev)
            for variant in (ops.SWD_SPLIT, ops.SWD_FUSED):
                got = ops.swd_distances(desc[0], desc[1], acc[0], acc[1], d, out=res, variant=variant).cpu().numpy()
                assert np.all(np.abs(got - ref) <= bound), (N, K, variant, np.abs(got - ref).max())
            nA, nB = (torch.from_numpy(v).to(dev) for v in norm)
            dT = d.t().contiguous()
            pA = nA @ dT

            def composed():
                return ((nA @ dT).sort(dim=0).values - (nB @ dT).sort(dim=0).values).abs().mean(dim=0)

            torch_err = float(np.abs(composed().double().cpu().numpy() - ref).max())
            img = torch.from_numpy(sets[0][0]).to(dev)

            def per_image():
                for l, level in enumerate(ops.lap_pyramid(img)):
                    if l == 0:
                        ops.swd_gather(level, pos[0][:P], desc[0], 0, acc[0])

            calls = {"pyramid_and_gather_one_image": per_image,
                     "distances_split": lambda: ops.swd_distances(desc[0], desc[1], acc[0], acc[1], d, out=res, variant=ops.SWD_SPLIT),
                     "distances_fused": lambda: ops.swd_distances(desc[0], desc[1], acc[0], acc[1], d, out=res, variant=ops.SWD_FUSED),
                     "torch_composed": composed,
                     "torch_matmul_alone": lambda: nA @ dT,
                     "torch_sort_alone": lambda: pA.sort(dim=0)}
            us = {k: [] for k in calls}
            for i in range(a.warmup + a.steps):
                for k, fn in calls.items():
                    v = sample(fn)
                    if i >= a.warmup:
                        us[k].append(v)
            r = out["N%d_K%d" % (N, K)] = {"N": N, "K": K, "score_x1e3": float(ref.mean() * 1e3), "max_err_split_fused": float(np.abs(got - ref).max()),
                                           "max_err_torch_composed_fp32": torch_err, "bound_min": float(bound.min()),
                                           "yardstick_swd_ref_host": stats(host_us)}
            r.update({k: stats(v) for k, v in us.items()})
            r["split_over_torch_composed"] = r["distances_split"]["median_us"] / r["torch_composed"]["median_us"]
            r["fused_over_split"] = r["distances_fused"]["median_us"] / r["distances_split"]["median_us"]
    out["clocks_after"] = clocks()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()

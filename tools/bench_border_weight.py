"""Timing of the border weight map (sgan_border_weight) at 512 x 512 and R = 20 (--border_weight 10 5) on the two
inputs of R13's table: the cell-like map (32-pixel cells, 2-pixel walls) and per-pixel noise at wall density 0.5.  Per input,
`--steps` calls after `--warmup`:
  (a) device: ccl_label + border_weight + pixel_weight_sum between two events, after a synchronise
  (b) enqueue: host wall time of the same three calls, nothing waited for
  (c) yardstick: the labelled map's `.cpu()` and util.border_weight_map on the host, wall time
each as median, min and p90.  The device planes are checked against the yardstick's first (d1sq, d2sq exact, bmap to 1e-4 relative).
The clocks `rocm-smi --showclocks` reports are recorded before and after (a query; nothing is set).  `--loop N` only enqueues N calls
on the cell map and exits: run that under a kernel trace for the per-kernel split."""
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
from bench_region_stats import clocks, inputs, stats  # noqa: E402
from supervised_gan_amd import ops  # noqa: E402
from supervised_gan_amd.util import border_weight_map  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--radius", type=int, default=20)
    ap.add_argument("--w0", type=float, default=10.0)
    ap.add_argument("--sigma", type=float, default=5.0)
    ap.add_argument("--loop", type=int, default=0, help="enqueue this many calls on the cell map and exit (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_border_weight.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, n = torch.device("cuda", 0), a.size
    cells = torch.empty((n, n), dtype=torch.int32, device=dev)
    bmap = torch.empty((n, n), dtype=torch.float32, device=dev)
    d1 = torch.empty((n, n), dtype=torch.int32, device=dev)
    d2 = torch.empty((n, n), dtype=torch.int32, device=dev)
    norm = torch.zeros((), dtype=torch.float32, device=dev)
    cw = torch.tensor([1.0, 2.0], dtype=torch.float32, device=dev)

    def call(plane, label, planes=False):
        ops.ccl_label(plane, cells)
        ops.border_weight(cells, a.radius, a.w0, a.sigma, bmap=bmap, d1sq=d1 if planes else None, d2sq=d2 if planes else None)
        ops.pixel_weight_sum(label, 2, cw, bmap.reshape(-1), norm)

    named = dict(inputs(n))
    order = ("cell_map", "per_pixel_noise")
    if a.loop:
        plane = torch.from_numpy(named["cell_map"]).to(dev)
        label = (plane <= 0.5).to(torch.int64).reshape(-1)
        for _ in range(a.loop):
            call(plane, label)
        torch.cuda.synchronize()
        ops.check_metric_err(dev)
        print("loop: %d calls, norm %r" % (a.loop, float(norm)))
        return None

    out = {"clocks_before": clocks(), "size": n, "radius": a.radius, "w0": a.w0, "sigma": a.sigma, "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "unit": "ms per call"}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name in order:
        wall = named[name]
        plane = torch.from_numpy(wall).to(dev)
        label = (plane <= 0.5).to(torch.int64).reshape(-1)      # class 0 = wall, 1 = cell
        call(plane, label, planes=True)
        w1, w2, wb = border_weight_map(cells.cpu().numpy(), a.radius, a.w0, a.sigma)
        assert np.array_equal(d1.cpu().numpy(), w1) and np.array_equal(d2.cpu().numpy(), w2), name
        got = bmap.cpu().numpy().astype(np.float64)
        assert (np.abs(got - wb) <= 1e-4 * wb + 1e-30).all(), name
        want_norm = float(np.where(wall > 0.5, 1.0, 2.0).sum() + wb.sum())
        assert abs(float(norm) - want_norm) <= 2e-4 * want_norm, (name, float(norm), want_norm)
        device_ms, enqueue_ms, host_ms = [], [], []
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            call(plane, label)
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if i >= a.warmup:
                device_ms.append(e0.elapsed_time(e1))
                enqueue_ms.append((t1 - t0) * 1e3)
        for i in range(1 + 3):               # the host path takes seconds: three calls after one
            t0 = time.perf_counter()
            border_weight_map(cells.cpu().numpy(), a.radius, a.w0, a.sigma)
            if i >= 1:
                host_ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = {"wall_pixels": int((wall > 0.5).sum()), "pixels_with_two_cells": int((w2 >= 0).sum()), "bmap_sum": float(wb.sum()),
                     "device_ccl_label_plus_border_weight_plus_pixel_weight_sum_events": stats(device_ms), "host_enqueue": stats(enqueue_ms),
                     "yardstick_cpu_copy_plus_border_weight_map": stats(host_ms)}
        print(name, json.dumps(out[name]))
    ops.check_metric_err(dev)
    out["clocks_after"] = clocks()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":
    main()

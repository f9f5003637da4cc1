"""Timing of the region statistics (sgan_region_stats) at 512 x 512 on the two inputs of R7's table: per-pixel noise
at wall density 0.5 and the cell-like map (32-pixel cells, 2-pixel walls).  Per input, `--steps` calls after `--warmup`:
  (a) device: ccl_label + region_stats between two events, after a synchronise
  (b) enqueue: host wall time of the same two calls, nothing waited for
  (c) yardstick: the labelled plane's `.cpu()` and util.region_table on the host, wall time
each as median, min and p90.  The device table is checked against the yardstick's first.  The clocks `rocm-smi --showclocks`
reports are recorded before and after (a query; nothing is set).  `--loop N` only enqueues N calls on the noise map and exits: run
that under a kernel trace for the per-kernel split."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from supervised_gan_amd import ops  # noqa: E402
from supervised_gan_amd.util import region_table  # noqa: E402


def clocks():
    """sclk / mclk lines of card 0 as rocm-smi prints them (read only), or the reason they could not be read."""
    try:
        txt = subprocess.run(["rocm-smi", "-d", "0", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [" ".join(l.split()) for l in txt.splitlines() if "sclk" in l or "mclk" in l] or ["no sclk/mclk line in rocm-smi's output"]
    except Exception as e:          # noqa: BLE001
        return ["rocm-smi not usable: %r" % (e,)]


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": statistics.median(ms), "min_ms": ms[0], "p90_ms": ms[int(0.9 * (len(ms) - 1))], "n": len(ms)}


def inputs(n):
    """name -> wall plane (1.0 = wall) as float32 numpy"""
    noise = (torch.rand(n, n, generator=torch.Generator().manual_seed(1)) < 0.5).numpy()
    y, x = np.mgrid[0:n, 0:n]
    cells = ((y % 32) < 2) | ((x % 32) < 2)
    return (("per_pixel_noise", noise.astype(np.float32)), ("cell_map", cells.astype(np.float32)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--loop", type=int, default=0, help="enqueue this many calls on the noise map and exit (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_region_stats.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, n = torch.device("cuda", 0), a.size
    labels = torch.empty((n, n), dtype=torch.int32, device=dev)
    capacity = ((n + 1) // 2) ** 2
    table = torch.zeros((capacity, ops.REGION_COLS), dtype=torch.int64, device=dev)
    cursor = torch.zeros(2, dtype=torch.int32, device=dev)

    def call(plane):
        cursor.zero_()
        ops.region_stats(ops.ccl_label(plane, labels), table, cursor)

    if a.loop:
        plane = torch.from_numpy(inputs(n)[0][1]).to(dev)
        for _ in range(a.loop):
            call(plane)
        torch.cuda.synchronize()
        ops.check_metric_err(dev)
        print("loop: %d calls, %d regions" % (a.loop, int(cursor[0])))
        return None

    out = {"clocks_before": clocks(), "size": n, "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "unit": "ms per call"}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, wall in inputs(n):
        plane = torch.from_numpy(wall).to(dev)
        call(plane)
        want = region_table(wall <= 0.5)
        assert int(cursor[0]) == len(want) and np.array_equal(table[:len(want)].cpu().numpy(), want), name
        device_ms, enqueue_ms, host_ms = [], [], []
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            call(plane)
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            if i >= a.warmup:
                device_ms.append(e0.elapsed_time(e1))
                enqueue_ms.append((t1 - t0) * 1e3)
        for i in range(3 + max(5, a.steps // 10)):               # the host path is ~100 x slower: a tenth of the calls
            t0 = time.perf_counter()
            region_table(plane.cpu().numpy() <= 0.5)
            if i >= 3:
                host_ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = {"regions": len(want), "largest_region": int(want[:, 0].max()),
                     "device_ccl_label_plus_region_stats_events": stats(device_ms), "host_enqueue": stats(enqueue_ms),
                     "yardstick_cpu_copy_plus_region_table": stats(host_ms)}
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

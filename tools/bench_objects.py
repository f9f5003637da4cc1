"""Timing of the object-level match counts (sgan_object_match_accumulate) at 512 x 512 on the two inputs of R7's
table: the cell-like map (32-pixel cells, 2-pixel walls) against a copy shifted by 3 pixels, and per-pixel noise at wall density 0.5
against other noise.  Per input, on label maps that are already on the device, `--steps` samples after `--warmup`, each sample
`--batch` calls between two events after a synchronise:
  (a) object_match_accumulate
  (b) rand_f_accumulate on the same maps in the same run, alternating with (a)
  (c) the two ccl_label calls that feed either
in microseconds per call, and
  (d) yardstick: util.object_match_counts on the host (scipy labelling included), wall time
each as median, min and p90.  The device counts are checked against the yardstick's before anything is timed.  The clocks
`rocm-smi --showclocks` reports are recorded before and after (a query; nothing is set).  `--loop N` only enqueues N times the two calls, alternating, on
the `--loop_input` pair and exits: run that under a kernel trace for the per-kernel split."""
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
from supervised_gan_amd.util import object_match_counts, object_scores  # noqa: E402


def clocks():
    """sclk / mclk lines of card 0 as rocm-smi prints them (read only), or the reason they could not be read."""
    try:
        txt = subprocess.run(["rocm-smi", "-d", "0", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [" ".join(l.split()) for l in txt.splitlines() if "sclk" in l or "mclk" in l] or ["no sclk/mclk line in rocm-smi's output"]
    except Exception as e:          # noqa: BLE001
        return ["rocm-smi not usable: %r" % (e,)]


def stats(us):
    us = sorted(us)
    return {"median_us": statistics.median(us), "min_us": us[0], "p90_us": us[int(0.9 * (len(us) - 1))], "n": len(us)}


def inputs(n):
    """name -> (prediction, truth) wall planes (1.0 = wall) as float32 numpy"""
    g = torch.Generator().manual_seed(1)
    noise_s, noise_t = ((torch.rand(n, n, generator=g) < 0.5).numpy().astype(np.float32) for _ in range(2))
    y, x = np.mgrid[0:n, 0:n]
    cells = lambda d: ((((y + d) % 32) < 2) | (((x + d) % 32) < 2)).astype(np.float32)      # noqa: E731
    return (("cell_map", (cells(3), cells(0))), ("per_pixel_noise", (noise_s, noise_t)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20, help="calls between the two events of one sample")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--min_area", type=int, default=1)
    ap.add_argument("--loop", type=int, default=0, help="enqueue this many times object_match_accumulate and rand_f_accumulate and exit (for a kernel trace)")
    ap.add_argument("--loop_input", default="per_pixel_noise", choices=("cell_map", "per_pixel_noise"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_objects.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, n = torch.device("cuda", 0), a.size
    acc_i, acc_f = torch.zeros(16, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.float64, device=dev)
    acc_r = torch.zeros(2, dtype=torch.float64, device=dev)
    counts, sums = torch.zeros(16, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.float64, device=dev)
    labels = torch.empty((2, n, n), dtype=torch.int32, device=dev)

    if a.loop:
        s, t = dict(inputs(n))[a.loop_input]
        t_lab, s_lab = ops.ccl_label(torch.from_numpy(t).to(dev), labels[0]), ops.ccl_label(torch.from_numpy(s).to(dev), labels[1])
        for _ in range(a.loop):                                     # the two calls alternating, so that one trace holds both
            ops.object_match_accumulate(t_lab, s_lab, acc_i, acc_f, min_area=a.min_area)
            ops.rand_f_accumulate(t_lab, s_lab, acc_r)
        torch.cuda.synchronize()
        ops.check_metric_err(dev)
        print("loop: %d calls, pooled %s" % (a.loop, acc_i.cpu().tolist()))
        return None

    out = {"clocks_before": clocks(), "size": n, "steps": a.steps, "warmup": a.warmup, "batch": a.batch, "min_area": a.min_area,
           "device": torch.cuda.get_device_name(0), "unit": "microseconds per call"}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def sample(fn):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.batch):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.batch

    for name, (s, t) in inputs(n):
        s_plane, t_plane = torch.from_numpy(s).to(dev), torch.from_numpy(t).to(dev)
        t_lab, s_lab = ops.ccl_label(t_plane, labels[0]), ops.ccl_label(s_plane, labels[1])
        ops.object_match_accumulate(t_lab, s_lab, acc_i, acc_f, min_area=a.min_area, counts_out=counts, sums_out=sums)
        want_c, want_s = object_match_counts(s, t, a.min_area)
        got_c, got_s = counts.cpu().numpy(), sums.cpu().numpy()
        assert np.array_equal(got_c, want_c), (name, got_c.tolist(), want_c.tolist())
        assert np.all(np.abs(got_s - want_s) <= max(1, int(want_c[10])) * 2.0 ** -52 * np.abs(want_s)), (name, got_s.tolist(), want_s.tolist())
        calls = {"object_match_accumulate": lambda: ops.object_match_accumulate(t_lab, s_lab, acc_i, acc_f, min_area=a.min_area),
                 "rand_f_accumulate": lambda: ops.rand_f_accumulate(t_lab, s_lab, acc_r),
                 "two_ccl_label": lambda: (ops.ccl_label(t_plane, labels[0]), ops.ccl_label(s_plane, labels[1]))}
        us = {k: [] for k in calls}
        for i in range(a.warmup + a.steps):
            for k, fn in calls.items():                             # alternating, so that a drift of the clocks meets all three alike
                v = sample(fn)
                if i >= a.warmup:
                    us[k].append(v)
        host_us = []
        for i in range(2 + max(5, a.steps // 10)):
            t0 = time.perf_counter()
            object_match_counts(s, t, a.min_area)
            if i >= 2:
                host_us.append((time.perf_counter() - t0) * 1e6)
        out[name] = {"counts": dict(zip(ops.OBJECT_COUNTS[:14], want_c[:14].tolist())), "sums": dict(zip(ops.OBJECT_SUMS, want_s.tolist())),
                     "scores": dict(object_scores(want_c, want_s)), "yardstick_object_match_counts_host": stats(host_us)}
        out[name].update({k: stats(v) for k, v in us.items()})
        out[name]["object_over_rand"] = out[name]["object_match_accumulate"]["median_us"] / out[name]["rand_f_accumulate"]["median_us"]
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

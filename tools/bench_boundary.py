"""Timing of the boundary scores (sgan_edt_sq twice + sgan_boundary_accumulate) at 512 x 512 on four inputs: R7's
cell-like map (32-pixel cells, 2-pixel walls) against a copy shifted by 3 pixels; per-pixel noise at wall density 0.5 against other
noise; an empty prediction against the cell map; and a prediction of ONE wall pixel in a corner against the cell map, the input on
which the row scan of the distance transform runs at full length.  Per input, on planes that are already on the device, `--steps`
samples after `--warmup`, each sample `--batch` calls between two events after a synchronise:
  (a) boundary_pair: edt_sq of the truth, edt_sq of the prediction, boundary_accumulate
  (b) the two edt_sq calls alone, and (c) boundary_accumulate alone
  (d) rand_f_accumulate on the label maps of the same planes, in the same run, alternating with the others
in microseconds per call, and
  (e) yardstick: util.boundary_counts on the host (its two util.edt_sq included, O(H W^2)), wall time, a few repetitions
each as median, min and p90.  The device counts are checked against the yardstick's before anything is timed.  The clocks
`rocm-smi --showclocks` reports are recorded before and after (a query; nothing is set).  Prints one JSON line and writes it to --out."""
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
from supervised_gan_amd.util import boundary_counts, boundary_scores  # noqa: E402


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
    one = np.zeros((n, n), dtype=np.float32)
    one[0, 0] = 1.0
    return (("cell_map", (cells(3), cells(0))), ("per_pixel_noise", (noise_s, noise_t)),
            ("empty_prediction", (np.zeros((n, n), dtype=np.float32), cells(0))), ("one_wall_pixel", (one, cells(0))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20, help="calls between the two events of one sample")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--host_reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_boundary.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, n = torch.device("cuda", 0), a.size
    acc_i, acc_f = torch.zeros(80, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.float64, device=dev)
    acc_r = torch.zeros(2, dtype=torch.float64, device=dev)
    counts, sums = torch.zeros(80, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.float64, device=dev)
    labels = torch.empty((2, n, n), dtype=torch.int32, device=dev)
    dsq = torch.empty((2, n, n), dtype=torch.int32, device=dev)
    out = {"clocks_before": clocks(), "size": n, "steps": a.steps, "warmup": a.warmup, "batch": a.batch,
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
        two_edt = lambda: (ops.edt_sq(t_plane, out=dsq[0]), ops.edt_sq(s_plane, out=dsq[1]))      # noqa: E731
        two_edt()
        ops.boundary_accumulate(dsq[0], dsq[1], acc_i, acc_f, counts_out=counts, sums_out=sums)
        host_us = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            want_c, want_s = boundary_counts(s, t)
            host_us.append((time.perf_counter() - t0) * 1e6)
        got_c, got_s = counts.cpu().numpy(), sums.cpu().numpy()
        assert np.array_equal(got_c, want_c), (name, got_c.tolist(), want_c.tolist())
        terms = np.array([max(2, int(want_c[68])), max(2, int(want_c[69])), 2, 2])
        assert np.all(np.abs(got_s - want_s) <= terms * 2.0 ** -52 * np.abs(want_s)), (name, got_s.tolist(), want_s.tolist())
        calls = {"boundary_pair": lambda: (two_edt(), ops.boundary_accumulate(dsq[0], dsq[1], acc_i, acc_f)),
                 "two_edt_sq": two_edt,
                 "boundary_accumulate": lambda: ops.boundary_accumulate(dsq[0], dsq[1], acc_i, acc_f),
                 "rand_f_accumulate": lambda: ops.rand_f_accumulate(t_lab, s_lab, acc_r)}
        us = {k: [] for k in calls}
        for i in range(a.warmup + a.steps):
            for k, fn in calls.items():                             # alternating, so that a drift of the clocks meets all alike
                v = sample(fn)
                if i >= a.warmup:
                    us[k].append(v)
        out[name] = {"counts": {k: int(want_c[ops.BOUNDARY_COUNTS.index(k)]) for k in ops.BOUNDARY_COUNTS[64:72]},
                     "sums": dict(zip(ops.BOUNDARY_SUMS[:3], want_s[:3].tolist())), "scores_at_tolerance_2": dict(boundary_scores(want_c, want_s, 2)),
                     "yardstick_boundary_counts_host": stats(host_us)}
        out[name].update({k: stats(v) for k, v in us.items()})
        out[name]["boundary_over_rand"] = out[name]["boundary_pair"]["median_us"] / out[name]["rand_f_accumulate"]["median_us"]
    ops.check_metric_err(dev)
    out["clocks_after"] = clocks()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()

"""Timing of the topology scores (sgan_topo_accumulate) at 512 x 512 with window 64, at stride 64 (64 windows) and at
stride 32 (225 windows), on three inputs: a cell-like map (32-pixel cells, 2-pixel walls) whose walls are punched with random gaps,
against the intact map; per-pixel noise at wall density 0.5 against other noise; and an empty prediction against the cell map.  Per
input, on planes that are already on the device, `--steps` samples after `--warmup`, each sample `--batch` calls between two events
after a synchronise:
  (a) topo_s64 / topo_s32: topo_accumulate without thinned planes -- the Betti launch and the summing launch
  (b) topo_s64_cldice: the same with both thinned planes given (made beforehand) -- plus the skeleton launch
  (c) ccl_label of the prediction, thin of the prediction, rand_f_accumulate on the label maps of the same planes, in the same run,
      alternating with the others
in microseconds per call, and
  (d) yardstick: util.topo_counts on the host at stride 64 (scipy.ndimage.label per window), wall time, a few repetitions
each as median, min and p90.  The device counts are checked against the yardstick's, at both strides, before anything is timed.  The
clocks `rocm-smi --showclocks` reports are recorded before and after (a query; nothing is set).  Prints one JSON line and writes it
to --out."""
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
from supervised_gan_amd.util import topo_counts, topo_scores  # noqa: E402


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
    cells = (((y % 32) < 2) | ((x % 32) < 2)).astype(np.float32)
    punched = cells.copy()
    punched[(torch.rand(n, n, generator=g) < 0.03).numpy()] = 0.0
    return (("cell_map_punched", (punched, cells)), ("per_pixel_noise", (noise_s, noise_t)),
            ("empty_prediction", (np.zeros((n, n), dtype=np.float32), cells)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20, help="calls between the two events of one sample")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--window", type=int, default=64)
    ap.add_argument("--host_reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_topo.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, n, win = torch.device("cuda", 0), a.size, a.window
    acc = torch.zeros(12, dtype=torch.int64, device=dev)
    counts = torch.zeros(12, dtype=torch.int64, device=dev)
    acc_r = torch.zeros(2, dtype=torch.float64, device=dev)
    labels = torch.empty((3, n, n), dtype=torch.int32, device=dev)
    thinned = torch.empty((3, n, n), dtype=torch.float32, device=dev)
    out = {"clocks_before": clocks(), "size": n, "window": win, "steps": a.steps, "warmup": a.warmup, "batch": a.batch,
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
        s_thin, t_thin = ops.thin(s_plane, out=thinned[0]), ops.thin(t_plane, out=thinned[1])
        s_thin_h, t_thin_h = s_thin.cpu().numpy(), t_thin.cpu().numpy()
        host_us, want = [], {}
        for stride in (win, win // 2):
            ops.topo_accumulate(t_plane, s_plane, acc, t_thin=t_thin, s_thin=s_thin, window=win, stride=stride, counts_out=counts)
            for _ in range(a.host_reps if stride == win else 1):
                t0 = time.perf_counter()
                want[stride] = topo_counts(s, t, win, stride, s_thin=s_thin_h, t_thin=t_thin_h)
                if stride == win:
                    host_us.append((time.perf_counter() - t0) * 1e6)
            got = counts.cpu().numpy()
            assert np.array_equal(got, want[stride]), (name, stride, got.tolist(), want[stride].tolist())
        calls = {"topo_s%d" % win: lambda: ops.topo_accumulate(t_plane, s_plane, acc, window=win, stride=win),
                 "topo_s%d" % (win // 2): lambda: ops.topo_accumulate(t_plane, s_plane, acc, window=win, stride=win // 2),
                 "topo_s%d_cldice" % win: lambda: ops.topo_accumulate(t_plane, s_plane, acc, t_thin=t_thin, s_thin=s_thin, window=win, stride=win),
                 "ccl_label": lambda: ops.ccl_label(s_plane, labels[2]),
                 "thin": lambda: ops.thin(s_plane, out=thinned[2]),
                 "rand_f_accumulate": lambda: ops.rand_f_accumulate(t_lab, s_lab, acc_r)}
        us = {k: [] for k in calls}
        for i in range(a.warmup + a.steps):
            for k, fn in calls.items():                             # alternating, so that a drift of the clocks meets all alike
                v = sample(fn)
                if i >= a.warmup:
                    us[k].append(v)
        out[name] = {"counts_s%d" % stride: dict(zip(ops.TOPO_COUNTS, (int(v) for v in want[stride]))) for stride in want}
        out[name]["scores_s%d" % win] = dict(topo_scores(want[win]))
        out[name]["yardstick_topo_counts_host_s%d" % win] = stats(host_us)
        out[name].update({k: stats(v) for k, v in us.items()})
        out[name]["topo_s%d_over_two_ccl_label" % win] = out[name]["topo_s%d" % win]["median_us"] / (2 * out[name]["ccl_label"]["median_us"])
        out[name]["topo_s%d_over_two_ccl_label" % (win // 2)] = out[name]["topo_s%d" % (win // 2)]["median_us"] / (2 * out[name]["ccl_label"]["median_us"])
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

"""Timing of the cleaning stage (sgan_clean_wall) at 512 x 512 on three predictions: a cell map (32-pixel cells,
2-pixel walls) with 1- to 3-pixel gaps punched into its walls and specks added; per-pixel noise at wall density 0.3; an empty
prediction.  Per input, on planes that are already on the device, `--steps` samples after `--warmup`, each sample `--batch` calls
between two events after a synchronise, alternating so that a drift of the clocks meets all alike:
  (a) clean_wall with each stage alone (close_rsq 2; min_wall 4; min_cell 10) and with all three
  (b) ccl_label and edt_sq of the same plane, rand_f_accumulate of its labels against the cell map's
in microseconds per call, and
  (c) yardstick: util.clean_wall with all three stages on the host, wall time, a few repetitions
each as median, min and p90.  new_passes_us = all three - 2 edt_sq - 2 ccl_label (medians): what the streaming passes of
sgan_clean.hip cost.  The device planes and counts are checked against the yardstick's before anything is timed.  The clocks
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
from supervised_gan_amd.util import clean_wall  # noqa: E402

PARAMS = {"close": (2, 0, 0), "min_wall": (0, 4, 0), "min_cell": (0, 0, 10), "all_three": (2, 4, 10)}


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
    """(the clean cell map, name -> predicted wall plane (1.0 = wall) as float32 numpy)"""
    rng = np.random.RandomState(1)
    y, x = np.mgrid[0:n, 0:n]
    cells = (((y % 32) < 2) | ((x % 32) < 2))
    punched = cells.copy()
    on = np.argwhere(cells)
    for k in range(n):                                  # gaps of 1 .. 3 pixels in the walls
        gy, gx = on[rng.randint(len(on))]
        punched[gy:gy + 1 + k % 3, gx:gx + 1 + k % 3] = False
    off = np.argwhere(~cells)
    for k in range(n):                                  # specks of 1 .. 3 pixels inside the cells
        sy, sx = off[rng.randint(len(off))]
        punched[sy, sx:sx + 1 + k % 3] = True
    noise = rng.rand(n, n) < 0.3
    f = lambda m: m.astype(np.float32)      # noqa: E731
    return f(cells), (("cell_map_with_gaps", f(punched)), ("per_pixel_noise", f(noise)), ("empty_prediction", np.zeros((n, n), dtype=np.float32)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20, help="calls between the two events of one sample")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--host_reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_clean.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, n = torch.device("cuda", 0), a.size
    acc = torch.zeros(len(ops.CLEAN_COUNTS), dtype=torch.int64, device=dev)
    acc_r = torch.zeros(2, dtype=torch.float64, device=dev)
    labels = torch.empty((2, n, n), dtype=torch.int32, device=dev)
    dsq = torch.empty((n, n), dtype=torch.int32, device=dev)
    cleaned = torch.empty((n, n), dtype=torch.float32, device=dev)
    out = {"clocks_before": clocks(), "size": n, "steps": a.steps, "warmup": a.warmup, "batch": a.batch,
           "device": torch.cuda.get_device_name(0), "unit": "microseconds per call", "params": {k: list(v) for k, v in PARAMS.items()}}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def sample(fn):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.batch):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.batch

    truth, planes = inputs(n)
    t_lab = ops.ccl_label(torch.from_numpy(truth).to(dev), labels[0])
    for name, s in planes:
        plane = torch.from_numpy(s).to(dev)
        s_lab = ops.ccl_label(plane, labels[1])
        counts = {}
        for key, p in PARAMS.items():                               # the device against the yardstick, before anything is timed
            acc.zero_()
            ops.clean_wall(plane, *p, out=cleaned, acc=acc)
            want, want_c = clean_wall(s, *p)
            assert torch.equal(cleaned.cpu(), torch.from_numpy(want.astype(np.float32))), (name, key)
            assert acc.cpu().tolist() == want_c.tolist(), (name, key, acc.cpu().tolist(), want_c.tolist())
            counts[key] = dict(zip(ops.CLEAN_COUNTS, want_c.tolist()))
        host_us = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            clean_wall(s, *PARAMS["all_three"])
            host_us.append((time.perf_counter() - t0) * 1e6)
        calls = {"clean_" + key: (lambda p=p: ops.clean_wall(plane, *p, out=cleaned, acc=acc)) for key, p in PARAMS.items()}
        calls.update({"ccl_label": lambda: ops.ccl_label(plane, labels[1]), "edt_sq": lambda: ops.edt_sq(plane, out=dsq),
                      "rand_f_accumulate": lambda: ops.rand_f_accumulate(t_lab, s_lab, acc_r)})
        us = {k: [] for k in calls}
        for i in range(a.warmup + a.steps):
            for k, fn in calls.items():
                v = sample(fn)
                if i >= a.warmup:
                    us[k].append(v)
        out[name] = {"counts": counts, "yardstick_clean_wall_host": stats(host_us)}
        out[name].update({k: stats(v) for k, v in us.items()})
        med = {k: out[name][k]["median_us"] for k in calls}
        out[name]["new_passes_us"] = med["clean_all_three"] - 2 * med["edt_sq"] - 2 * med["ccl_label"]
        out[name]["new_passes_over_edt_sq"] = out[name]["new_passes_us"] / med["edt_sq"]
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

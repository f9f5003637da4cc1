"""Timing of the cell-splitting stage (sgan_split_cells) at 512 x 512 on tools/bench_clean.py's three predictions: the
cell map with gaps punched into its walls and specks added, per-pixel noise at wall density 0.3, an empty prediction.  Per input, on
planes that are already on the device, `--steps` samples after `--warmup`, each sample `--batch` calls between two events after a
synchronise, alternating so that a drift of the clocks meets all alike:
  (a) split_cells at split_rsq 25 and 100 with the default budget of 64 rounds, and at split_rsq 25 with budgets of 8, 128 and 256
  (b) the yardsticks of the same run: clean_wall with all three stages, edt_sq and ccl_label of the same plane
  (c) seg_metrics.accumulate (RandScore ObjF1 BoundF) without an option and with --clean_split 5
in microseconds per call, and
  (d) util.split_cells on the host, wall time, a few repetitions
each as median, min and p90.  Derived from the medians at split_rsq 25: early_exit_us_per_launch = (budget 256 - budget 128) / 16,
valid where the flood needs fewer than 128 rounds (rounds_needed is recorded, and launches_working_of_8, the flood launches of the
default budget that did not return at once).  Events around whole calls do not separate the threshold pass, the working flood
launches and the cut pass; ccl_label is timed on the plane itself, while the call labels the core plane, which has fewer and
smaller components.  The device planes and counts are checked against
the yardstick's before anything is timed.  The clocks `rocm-smi --showclocks` reports are recorded before and after (a query; nothing
is set).  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_clean import clocks, inputs, stats  # noqa: E402
from supervised_gan_amd import ops  # noqa: E402
from supervised_gan_amd.seg_metrics import SegMetrics  # noqa: E402
from supervised_gan_amd.util import split_cells  # noqa: E402

CASES = {"rsq25": (25, 64), "rsq100": (100, 64), "rsq25_budget8": (25, 8), "rsq25_budget128": (25, 128), "rsq25_budget256": (25, 256)}
CLEAN = (2, 4, 10)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=20, help="calls between the two events of one sample")
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--host_reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_split.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, n = torch.device("cuda", 0), a.size
    acc = torch.zeros(len(ops.SPLIT_COUNTS), dtype=torch.int64, device=dev)
    acc_c = torch.zeros(len(ops.CLEAN_COUNTS), dtype=torch.int64, device=dev)
    labels = torch.empty((n, n), dtype=torch.int32, device=dev)
    dsq = torch.empty((n, n), dtype=torch.int32, device=dev)
    cleaned = torch.empty((n, n), dtype=torch.float32, device=dev)
    out = {"clocks_before": clocks(), "size": n, "steps": a.steps, "warmup": a.warmup, "batch": a.batch,
           "device": torch.cuda.get_device_name(0), "unit": "microseconds per call",
           "cases": {k: {"split_rsq": v[0], "max_rounds": v[1]} for k, v in CASES.items()}, "clean_wall_params": list(CLEAN)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def sample(fn):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.batch):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.batch

    def opt(**kw):
        return types.SimpleNamespace(which_metric=["RandScore", "ObjF1", "BoundF"], min_object_area=1, boundary_thin=False,
                                     boundary_tolerance=2, add_background_onehot_acc=False, isTrain=True, **kw)

    truth, planes = inputs(n)
    real = torch.from_numpy(np.stack([truth, 1 - truth])[None]).to(dev)
    for name, s in planes:
        plane = torch.from_numpy(s).to(dev)
        fake = torch.from_numpy(np.stack([s, 1 - s])[None]).to(dev)
        counts = {}
        for key, (rsq, rounds) in CASES.items():                    # the device against the yardstick, before anything is timed
            acc.zero_()
            ops.split_cells(plane, rsq, rounds, out=cleaned, acc=acc)
            want, want_c = split_cells(s, rsq, rounds)
            assert torch.equal(cleaned.cpu(), torch.from_numpy(want.astype(np.float32))), (name, key)
            assert acc.cpu().tolist() == want_c.tolist(), (name, key, acc.cpu().tolist(), want_c.tolist())
            counts[key] = dict(zip(ops.SPLIT_COUNTS, want_c.tolist()))
        ops.metric_err(dev).zero_()                                 # a budget of 8 may be hit: counted above, not an error
        host_us = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            split_cells(s, 25, 64)
            host_us.append((time.perf_counter() - t0) * 1e6)
        metrics = {"accumulate_plain": SegMetrics(opt(), dev, 2), "accumulate_clean_split_5": SegMetrics(opt(clean_split=5.0), dev, 2)}
        calls = {"split_" + key: (lambda p=p: ops.split_cells(plane, *p, out=cleaned, acc=acc)) for key, p in CASES.items()}
        calls.update({"clean_all_three": lambda: ops.clean_wall(plane, *CLEAN, out=cleaned, acc=acc_c),
                      "ccl_label": lambda: ops.ccl_label(plane, labels), "edt_sq": lambda: ops.edt_sq(plane, out=dsq)})
        calls.update({k: (lambda m=m: m.accumulate(fake, real, None, None)) for k, m in metrics.items()})
        us = {k: [] for k in calls}
        for i in range(a.warmup + a.steps):
            for k, fn in calls.items():
                v = sample(fn)
                if i >= a.warmup:
                    us[k].append(v)
        ops.metric_err(dev).zero_()
        r = out[name] = {"counts": counts, "yardstick_split_cells_host": stats(host_us)}
        r.update({k: stats(v) for k, v in us.items()})
        med = {k: r[k]["median_us"] for k in calls}
        needed = counts["rsq25_budget256"]["rounds"]
        working = min(8, needed // 8 + 1)                           # launch j >= 1 works iff round 8 j labelled something
        r["rounds_needed_rsq25"] = needed
        r["launches_working_of_8"] = working
        r["early_exit_us_per_launch"] = (med["split_rsq25_budget256"] - med["split_rsq25_budget128"]) / 16
        r["split_over_clean_all_three"] = med["split_rsq25"] / med["clean_all_three"]
    out["clocks_after"] = clocks()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()

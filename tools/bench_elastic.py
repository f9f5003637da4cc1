"""Timing of the elastic input pipeline tail (sgan_image_prep_elastic) beside the plain one (sgan_image_prep) for a
512 x 512 crop of a 572 x 572 image, `--elastic 8 10`-like control points (G = 8, SIGMA = 10).

A launch of either kernel lasts a few microseconds, less than two events resolve, so a timed window is `--reps` launches back to back
on one stream between two events, after a synchronise; the figure is the window over `--reps`: the time per launch of a busy queue,
which is the kernel plus the dispatch gap behind it.  The variants -- plain; elastic with nearest_mask 3 (the default: two label
channels, one image channel), 0 (all bilinear) and 7 (all nearest); elastic mask 3 with field_out -- take turns window by window,
`--steps` windows each after `--warmup`, so drift of the clocks or of the host falls on all of them alike.  Median, min and p90 over
the windows; bytes are what the algorithm needs (n^2 x 16 stored, the touched part of the image read once).  Also: the host wall time
of one enqueue, and of util.elastic_prep (the yardstick, NumPy) on the same input.  Before timing, the device output is checked
against the yardstick on the device's field and, with zero control points, against the plain kernel.  The clocks `rocm-smi
--showclocks` reports are recorded before and after (a query; nothing is set).  `--loop N` only enqueues N launches of each kernel,
alternating, and exits: run that under a kernel trace for the kernels' own durations."""
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
from supervised_gan_amd.util import elastic_prep  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40, help="timed windows per variant")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=500, help="launches per window")
    ap.add_argument("--image", type=int, default=572)
    ap.add_argument("--crop", type=int, default=512)
    ap.add_argument("--G", type=int, default=8)
    ap.add_argument("--sigma", type=float, default=10.0)
    ap.add_argument("--loop", type=int, default=0, help="enqueue this many launches of the plain kernel and of the elastic kernel (mask 3), "
                                                        "alternating, and exit (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_elastic.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, n, S = torch.device("cuda", 0), a.crop, a.image
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, size=(S, S, 3), dtype=np.uint8)
    ctrl = (rng.randn(a.G + 3, a.G + 3, 2) * a.sigma).astype(np.float32)
    x0 = y0 = (S - n) // 2
    flip, rot = True, 1
    img_d, ctrl_d = torch.from_numpy(img).to(dev), torch.from_numpy(ctrl).to(dev)
    out = torch.empty((n, n, 4), dtype=torch.float32, device=dev)
    field = torch.empty((n, n, 2), dtype=torch.float32, device=dev)

    # the timed launches compute what the yardstick computes
    for mask in (3, 0, 7):
        ops.image_prep_elastic(img_d, x0, y0, n, flip, rot, ctrl_d, mask, out=out, field_out=field)
        want = elastic_prep(img, x0, y0, n, flip, rot, None, a.G, mask, field=field.cpu().numpy())
        assert np.array_equal(out.cpu().numpy()[..., :3].transpose(2, 0, 1), want) and not out[..., 3].any(), mask
    plain = ops.image_prep(img_d, x0, y0, n, flip, rot)
    ops.image_prep_elastic(img_d, x0, y0, n, flip, rot, torch.zeros_like(ctrl_d), 3, out=out)
    assert torch.equal(out, plain)
    if a.loop:
        for _ in range(a.loop):
            ops.image_prep(img_d, x0, y0, n, flip, rot, out=out)
            ops.image_prep_elastic(img_d, x0, y0, n, flip, rot, ctrl_d, 3, out=out)
        torch.cuda.synchronize()
        print("loop: %d launches of each kernel" % a.loop)
        return None

    variants = {
        "plain_sgan_image_prep": lambda: ops.image_prep(img_d, x0, y0, n, flip, rot, out=out),
        "elastic_mask3": lambda: ops.image_prep_elastic(img_d, x0, y0, n, flip, rot, ctrl_d, 3, out=out),
        "elastic_mask0_all_bilinear": lambda: ops.image_prep_elastic(img_d, x0, y0, n, flip, rot, ctrl_d, 0, out=out),
        "elastic_mask7_all_nearest": lambda: ops.image_prep_elastic(img_d, x0, y0, n, flip, rot, ctrl_d, 7, out=out),
        "elastic_mask3_with_field_out": lambda: ops.image_prep_elastic(img_d, x0, y0, n, flip, rot, ctrl_d, 3, out=out, field_out=field),
    }
    per_launch = {k: [] for k in variants}
    enqueue = {k: [] for k in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    c_before = clocks()
    for i in range(a.warmup + a.steps):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                per_launch[name].append(e0.elapsed_time(e1) / a.reps)
                enqueue[name].append((t1 - t0) * 1e3)
    host_ms = []
    for i in range(1 + 3):
        t0 = time.perf_counter()
        elastic_prep(img, x0, y0, n, flip, rot, ctrl, a.G, 3)
        if i >= 1:
            host_ms.append((time.perf_counter() - t0) * 1e3)

    stored = n * n * 16
    read = min(S, n + 2 * 127) ** 2 * 3      # at most the window and the clamp's reach around it
    res = {"clocks_before": c_before, "clocks_after": clocks(), "device": torch.cuda.get_device_name(0), "image": S, "crop": n, "G": a.G,
           "sigma": a.sigma, "flip": flip, "rot": rot, "reps_per_window": a.reps, "windows": a.steps, "warmup_windows": a.warmup,
           "unit": "ms per launch, back-to-back launches on one stream between two events", "bytes_stored": stored, "bytes_read_at_most": read,
           "per_launch": {k: stats(v) for k, v in per_launch.items()}, "host_enqueue_one_call": {k: stats(v) for k, v in enqueue.items()},
           "yardstick_util_elastic_prep_host": stats(host_ms)}
    base = res["per_launch"]["plain_sgan_image_prep"]["median_ms"]
    res["ratio_to_plain_median"] = {k: v["median_ms"] / base for k, v in res["per_launch"].items()}
    res["stored_GB_per_s_median"] = {k: stored / (v["median_ms"] * 1e-3) / 1e9 for k, v in res["per_launch"].items()}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


if __name__ == "__main__":
    main()

"""Timing of the photometric augmentation kernel (sgan_image_photo) on a 512 x 512 crop with 4 stored channels and one
masked channel, for blur radii 0, 6 and 12, each without and with the point stages (gamma, contrast / brightness, noise, two boxes),
beside what it is to be read against, in the same run and on the same buffers: the plain input pipeline tail (sgan_image_prep), the
elastic one (sgan_image_prep_elastic, G = 8), the runtime's copy_ of the crop's bytes, and the sgan_normal_fill that the noise stage
adds in front.

A launch lasts a few microseconds, less than two events resolve, so a timed window is `--reps` launches back to back on one stream
between two events, after a synchronise; the figure is the window over `--reps`: the time per launch of a busy queue.  The variants
take turns window by window, `--steps` windows each after `--warmup`, so drift falls on all of them alike; median, min and p90 over
the windows.  Before timing, every photometric variant is checked against util.photo_bounds.

Also the graphed 512 x 512 `--which_model_netD None` segmentation step (tools/bench_segterms.build_step), alone and with one noise
fill and one photometric launch enqueued in front of every replay: the feeder runs outside the captured step, so the step itself is
the parent's.  Two figures, no assertion.  Writes profiles/<tag>_photo.json.
    python tools/bench_photo.py --tag r38 [--steps 30] [--warmup 5] [--reps 300] [--step_reps 100]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_region_stats import clocks, stats  # noqa: E402
from supervised_gan_amd import ops, util  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="r38")
    ap.add_argument("--steps", type=int, default=30, help="timed windows per variant")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=300, help="launches per window")
    ap.add_argument("--step_reps", type=int, default=100, help="replays of the graphed step per window (0: skip the step)")
    ap.add_argument("--step_rounds", type=int, default=5)
    ap.add_argument("--crop", type=int, default=512)
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, n, S = torch.device("cuda", 0), a.crop, a.crop + 60
    rng = np.random.RandomState(0)
    img_d = torch.from_numpy(rng.randint(0, 256, size=(S, S, 3), dtype=np.uint8)).to(dev)
    ctrl_d = torch.from_numpy((rng.randn(11, 11, 2) * 10.0).astype(np.float32)).to(dev)
    src = ops.image_prep(img_d, 30, 30, n, True, 1)
    out, other = torch.empty_like(src), torch.empty_like(src)
    noise = torch.empty((1, n, n), dtype=torch.float32, device=dev)
    ops.normal_fill(noise, 1234, None, advance=False)
    mask = 0b100
    point = dict(gamma=0.7, contrast=1.2, brightness=0.05, sigma_n=0.04, boxes=[(40, 120, 300, 420, 0.3), (400, 470, 10, 90, -0.6)])
    recs = {}
    for R in (0, 6, 12):
        taps = util.photo_taps(R / 3.0) if R else (1.0,)
        assert len(taps) - 1 == R
        recs["photo_R%d" % R] = (util.PhotoRec(taps=taps), None)
        recs["photo_R%d_point_stages" % R] = (util.PhotoRec(taps=taps, **point), noise)

    x, nz = src.cpu().numpy(), noise.cpu().numpy()
    for name, (rec, z) in recs.items():      # the timed launches compute what the yardstick allows
        ops.image_photo(src, rec, mask, noise=z, out=out)
        lo, hi = util.photo_bounds(x, rec, mask, None if z is None else nz)
        g = out.cpu().numpy().astype(np.float64)
        assert ((lo <= g) & (g <= hi)).all(), name

    variants = {
        "plain_sgan_image_prep": lambda: ops.image_prep(img_d, 30, 30, n, True, 1, out=other),
        "elastic_sgan_image_prep_elastic_G8": lambda: ops.image_prep_elastic(img_d, 30, 30, n, True, 1, ctrl_d, 3, out=other),
        "runtime_copy_": lambda: out.copy_(src),
        "sgan_normal_fill_one_plane": lambda: ops.normal_fill(noise, 1234, None, advance=False),
    }
    for name, (rec, z) in recs.items():
        variants[name] = (lambda rec=rec, z=z: ops.image_photo(src, rec, mask, noise=z, out=out))
    per_launch = {k: [] for k in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    c_before = clocks()
    for i in range(a.warmup + a.steps):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                per_launch[name].append(e0.elapsed_time(e1) / a.reps)

    res = {"device": torch.cuda.get_device_name(0), "clocks_before": c_before, "clocks_after": clocks(), "crop": n, "Cstore": 4,
           "channel_mask": mask, "reps_per_window": a.reps, "windows": a.steps, "warmup_windows": a.warmup,
           "unit": "ms per launch, back-to-back launches on one stream between two events", "bytes_read_plus_written": 2 * n * n * 16,
           "per_launch": {k: stats(v) for k, v in per_launch.items()}}
    base = res["per_launch"]["runtime_copy_"]["median_ms"]
    res["ratio_to_copy_median"] = {k: v["median_ms"] / base for k, v in res["per_launch"].items()}

    if a.step_reps:
        from bench_segterms import build_step, time_ms
        step = build_step((), size=n)
        rec, z = recs["photo_R6_point_stages"]

        def fed():
            ops.normal_fill(noise, 1234, None, advance=False)
            ops.image_photo(src, rec, mask, noise=z, out=out)
            step()
        runs = {"graphed_step": step, "noise_fill_photo_R6_then_graphed_step": fed}
        times = {k: [] for k in runs}
        for _ in range(a.step_rounds):
            for k, fn in runs.items():
                times[k].append(time_ms(fn, a.step_reps))
        res["graphed_step_512_netD_None_ms"] = {"rounds": times, "median": {k: float(np.median(v)) for k, v in times.items()}}

    print(json.dumps(res))
    path = os.path.join(ROOT, "profiles", "%s_photo.json" % a.tag)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


if __name__ == "__main__":
    main()

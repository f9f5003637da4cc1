"""The three arithmetic modes of the conv kernels on the flagship workload: one JSON line per mode.

    python tools/bench_math.py [--steps 200] [--warmup 20] [--modes f32,bf16x3,bf16x1] [--out FILE]

For each mode a FRESH child process (SGAN_MATH=<mode> in its environment; the mode is read when the library is first imported) builds
the fcgan 512^2 bs 1 trainer with bench.build_model (the bench.py headline workload, n_update_G 2, same seeds), takes the step-1
generator output `fake` on the first batch of bench.synthetic_ring, captures the training step into hipGraphs and times >= --steps
replays after --warmup (one HIP event per step).  The parent never touches the GPU: it starts the children one after the other, stops
at the first one that fails, and prints per mode ms/step median / min / max, images/s (wall clock over the timed steps) and
`fake_maxrel_vs_f32` = max|fake - fake_f32| / max|fake_f32| of the step-1 output against the f32 child (same seed, same latents).
bench.py itself only knows the default mode (its `dtype` label); this is where the others are measured."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("f32", "bf16x3", "bf16x1")


def child(mode, steps, warmup, fake_out):
    sys.path.insert(0, ROOT)
    import random
    import time

    import numpy as np
    import torch

    import bench
    from supervised_gan_amd import ops
    from supervised_gan_amd.graph_step import GraphedStep
    assert ops.get_math() == mode, (ops.get_math(), mode)
    torch.cuda.set_device(0)
    random.seed(0)
    bargs = argparse.Namespace(n_update_G=2, skip_wasted_D_wgrad=False, no_d_streams=False, no_group=False)
    model = bench.build_model(bargs, 0)
    ring = bench.synthetic_ring(64, 0, torch.device("cuda", 0))
    model.set_input(ring[0])
    model.forward()
    torch.cuda.synchronize()
    np.save(fake_out, model.fake.detach().float().cpu().numpy())
    gs = GraphedStep(model)
    gs.capture(ring[0])
    for i in range(warmup):
        gs.step(ring[i % len(ring)])
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(steps):
        gs.step(ring[(warmup + i) % len(ring)])
        marks[i + 1].record()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    per = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    med = per[steps // 2] if steps % 2 else 0.5 * (per[steps // 2 - 1] + per[steps // 2])
    errs = {k: float(v) for k, v in model.get_current_errors().items()}
    assert all(np.isfinite(v) for v in errs.values()), errs
    print(json.dumps({"mode": mode, "steps": steps, "warmup": warmup, "ms_per_step_median": round(med, 4),
                      "ms_per_step_min": round(per[0], 4), "ms_per_step_max": round(per[-1], 4),
                      "images_per_s": round(steps / dt, 2), "losses_last": errs}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--timeout", type=float, default=600.0, help="seconds per child")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--fake-out", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps, a.warmup, a.fake_out)
    if a.steps < 200:
        ap.error("--steps must be at least 200")
    import numpy as np
    modes = [m for m in a.modes.split(",") if m]
    assert all(m in MODES for m in modes), modes
    if "f32" in modes:      # the reference of the deviation column runs first
        modes = ["f32"] + [m for m in modes if m != "f32"]
    tmp = tempfile.mkdtemp(prefix="bench_math_")
    lines, fake = [], {}
    for mode in modes:
        env = dict(os.environ, SGAN_MATH=mode)
        fo = os.path.join(tmp, f"fake_{mode}.npy")
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--steps", str(a.steps), "--warmup", str(a.warmup), "--fake-out", fo]
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=a.timeout)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            raise SystemExit(f"bench_math: the {mode} child failed (exit {r.returncode}); no further modes started")
        rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        fake[mode] = np.load(fo).astype(np.float64)
        if "f32" in fake:
            ref = fake["f32"]
            rec["fake_maxrel_vs_f32"] = float(np.abs(fake[mode] - ref).max() / np.abs(ref).max())
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

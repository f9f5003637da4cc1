#!/usr/bin/env python3
"""Cost of the segmentation accuracies per training step at 512 x 512: the device path (SegmentationModel.accum_accs: kernels of
sgan_metrics.hip queued behind the step) against the host path it replaced (the parent commit's accum_accs: .cpu() +
util.compute_Rand_F_scores on channel 0 + a bincount confusion matrix read back), on the same tensors; and a graphed `segmentation`
step loop without accuracies, with the device path and with the host path after every step.

    python tools/bench_metrics.py [--steps 300] [--warmup 10] [--repeats 3] [--out profiles/r07_metrics.json]
    python tools/bench_metrics.py --metrics RandScore VInfo meanIU --compare RandScore meanIU --out profiles/r08_metrics.json
        (`--metrics`: what accum_accs is asked for; `--compare`: a second metric set timed on the same tensors in the same run --
        the cost of adding VInfo to RandScore is the difference of the two)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_metrics.py --metric_only 50 [--metrics ...]
        (only the metric launches, on per-pixel noise maps: the per-kernel split of one accum_accs)
    python tools/bench_metrics.py --thin [--steps 100] --out profiles/r11_thin.json
        (the thinned path on maps alone, no trainer: sgan_thin, the thinned score pair and the un-thinned pair on per-pixel noise,
        the cell map, the cell map with its walls dilated by 3 pixels, and an already thin map -- every tile launch but the first
        returns at once there, which is the cost of the early-exit launches)

Kernel time is taken with events around the queued kernels after a synchronise (warm-up excluded); the loops are wall time between
two synchronises, divided by the step count.  Every figure is reported per repeat so the spread is in the file, and the clocks
`rocm-smi --showclocks` reports are recorded before and after the measurement (a query; nothing is set)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from supervised_gan_amd import ops  # noqa: E402
from supervised_gan_amd.graph_step import GraphedStep  # noqa: E402
from supervised_gan_amd.models import create_model  # noqa: E402
from supervised_gan_amd.options import TrainOptions  # noqa: E402
from supervised_gan_amd.synthetic_data import SyntheticDataset  # noqa: E402
from supervised_gan_amd.util import compute_Rand_F_scores, compute_VInfo_scores  # noqa: E402


def host_accum(model, state):
    """The parent commit's accum_accs for --which_metric RandScore meanIU, with the Rand score on channel 0."""
    s, t = model.fake_B.detach()[:, :1].cpu().numpy(), model.real_B.detach()[:, :1].cpu().numpy()
    state["rand"].append(compute_Rand_F_scores(s, t)[0])
    k = model.num_classes
    labels, pred = model.label, model.logit.detach().argmax(dim=1)
    state["conf"] += torch.bincount((labels.reshape(-1) * k + pred.reshape(-1)), minlength=k * k).reshape(k, k).double().cpu().numpy()


def clocks():
    """sclk / mclk lines of card 0 as rocm-smi prints them (read only), or the reason they could not be read."""
    try:
        txt = subprocess.run(["rocm-smi", "-d", "0", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [" ".join(l.split()) for l in txt.splitlines() if "sclk" in l or "mclk" in l] or ["no sclk/mclk line in rocm-smi's output"]
    except Exception as e:          # noqa: BLE001
        return ["rocm-smi not usable: %r" % (e,)]


def metric_only(n_iter, n, dev, metrics=("RandScore", "meanIU")):
    """n_iter x (two labellings, the Rand sums -- with VInfo among `metrics` the one call that feeds both scores --, the confusion
    matrix) on per-pixel noise at wall density 0.5, nothing else: run under a kernel trace for the per-launch split."""
    g = torch.Generator().manual_seed(1)
    fb, rb = torch.rand(n, n, 4, generator=g).to(dev), torch.rand(n, n, 4, generator=g).to(dev)
    label = (rb[:, :, 0] < rb[:, :, 1]).long().reshape(-1).contiguous()
    labels = torch.empty((2, n, n), dtype=torch.int32, device=dev)
    acc, conf = torch.zeros(2, dtype=torch.float64, device=dev), torch.zeros((2, 2), dtype=torch.int64, device=dev)
    acc_v = torch.zeros(2, dtype=torch.float64, device=dev)
    for _ in range(n_iter):
        if "RandScore" in metrics or "VInfo" in metrics:
            ops.ccl_label(rb[:, :, 0], labels[0])
            ops.ccl_label(fb[:, :, 0], labels[1])
        if "VInfo" in metrics:
            ops.vinfo_accumulate(labels[0], labels[1], acc_v, acc_rand=acc if "RandScore" in metrics else None)
        elif "RandScore" in metrics:
            ops.rand_f_accumulate(labels[0], labels[1], acc)
        if "meanIU" in metrics:
            ops.confusion_accumulate(fb, 2, conf, label=label)
    torch.cuda.synchronize()
    ops.check_metric_err(dev)
    print("metric_only: %d iterations, mean F %.6f, mean VInfo %.6f" % (n_iter, float(acc[0] / acc[1]), float(acc_v[0] / acc_v[1])))


def thin_bench(a, dev):
    """sgan_thin alone, the thinned score pair (thin, two labellings, one counting pass for both scores) and the un-thinned pair on
    the same maps.  Each is timed twice: with events around one eager call after a synchronise (what a training loop that is not
    graphed pays, host enqueue gaps included) and as the mean of 10 calls captured in one hipGraph (device time alone)."""
    from scipy import ndimage
    from supervised_gan_amd.util import thin as host_thin
    n = a.size
    g = torch.Generator().manual_seed(1)
    noise = torch.rand(2, n, n, generator=g)
    cs, ct = (m[0, 0].cpu() for m in cell_maps(n, dev))
    thick = torch.from_numpy(ndimage.binary_dilation(cs.numpy() > 0.5, structure=np.ones((3, 3), bool), iterations=3).astype(np.float32))
    thin_map = torch.from_numpy(host_thin(cs.numpy() > 0.5)[0].astype(np.float32))
    inputs = (("per_pixel_noise", noise[0], noise[1]), ("cell_map", cs, ct), ("cell_map_walls_dilated_3", thick, ct),
              ("already_thin_early_exit_launches", thin_map, ct))
    out = {"clocks_before": clocks(), "size": n, "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "budget_iterations": n // 2 + 2, "unit": "ms per call"}
    labels = torch.empty((3, n, n), dtype=torch.int32, device=dev)
    plane = torch.empty((n, n), dtype=torch.float32, device=dev)
    acc = torch.zeros((2, 2), dtype=torch.float64, device=dev)
    it = torch.zeros(1, dtype=torch.int32, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def eager(fn):
        ms = []
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return stats(ms)

    def graphed(fn, calls=10):
        gr = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(gr):
            for _ in range(calls):
                fn()
        ms = []
        for i in range(3 + max(5, a.steps // calls)):
            torch.cuda.synchronize()
            e0.record()
            gr.replay()
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                ms.append(e0.elapsed_time(e1) / calls)
        return stats(ms)

    for name, s_host, t_host in inputs:
        s, t = s_host.to(dev).contiguous(), t_host.to(dev).contiguous()

        def only_thin():
            ops.thin(s, out=plane, iters_out=it)

        def thinned_pair():
            ops.ccl_label(t, labels[0])
            ops.thin(s, out=plane)
            ops.ccl_label(plane, labels[2])
            ops.vinfo_accumulate(labels[0], labels[2], acc[1], acc_rand=acc[0])

        def plain_pair():
            ops.ccl_label(t, labels[0])
            ops.ccl_label(s, labels[1])
            ops.vinfo_accumulate(labels[0], labels[1], acc[1], acc_rand=acc[0])

        only_thin()
        want, n_host = host_thin(s_host.numpy() > 0.5)
        assert np.array_equal(plane.cpu().numpy() == 1.0, want) and int(it.item()) == n_host, name
        out[name] = {"wall_pixels": int((s_host > 0.5).sum()), "wall_pixels_thinned": int(want.sum()), "changing_iterations": n_host}
        for key, fn in (("sgan_thin", only_thin), ("thinned_score_pair", thinned_pair), ("unthinned_score_pair", plain_pair)):
            out[name][key] = {"eager_events": eager(fn), "graphed": graphed(fn)}
        print(name, json.dumps(out[name]))
    ops.check_metric_err(dev)
    out["clocks_after"] = clocks()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": statistics.median(ms), "min_ms": ms[0], "p90_ms": ms[int(0.9 * (len(ms) - 1))], "max_ms": ms[-1], "n": len(ms)}


def cell_maps(n, dev):
    """A boundary map that looks like the task's: ~32-pixel cells with 2-pixel walls (truth) and the same map with every fourth
    wall broken and a shifted extra wall (prediction); channel 1 is the complement."""
    y, x = np.mgrid[0:n, 0:n]
    t = ((y % 32) < 2) | ((x % 32) < 2)
    s = t.copy()
    s[(y % 128 < 2) & (x % 64 > 20) & (x % 64 < 40)] = False
    s[(x % 96) == 50] = True
    mk = lambda m: torch.from_numpy(np.stack([m, ~m]).astype(np.float32)[None]).to(dev)      # noqa: E731
    return mk(s), mk(t)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--metric_only", type=int, default=0, help="run only this many metric iterations on noise maps and exit")
    ap.add_argument("--thin", action="store_true", help="time the thinned path on maps alone (no trainer) and exit")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_metrics.json"))
    ap.add_argument("--metrics", nargs="+", default=["RandScore", "meanIU"], help="--which_metric of the trainer")
    ap.add_argument("--compare", nargs="+", default=None, help="a second metric set, timed on the same tensors (device kernels only)")
    a = ap.parse_args(argv)
    n = a.size
    if a.metric_only:
        return metric_only(a.metric_only, n, torch.device("cuda", 0), a.metrics)
    if a.thin:
        return thin_bench(a, torch.device("cuda", 0))
    with tempfile.TemporaryDirectory() as tmp:
        argv_m = ("--name bench_metrics --model segmentation --which_direction AtoB --dataset_mode aligned --fineSize %d "
                  "--which_model_netG unet_256 --ngf 32 --norm instance --which_channel b_rg --gpu_ids 0 --no_dropout --dataroot synthetic "
                  "--manualSeed 4 --which_metric %s --which_model_netD n_layers --n_layers_D 3 --ndf 32 --scale_factor 1 "
                  "--lambda_D 1.0 --weights 1 2 --no_lsgan --checkpoints_dir %s" % (n, " ".join(a.metrics), tmp)).split()
        opt = TrainOptions().parse(argv_m, save=False, verbose=False)
        model = create_model(opt)
        data = list(SyntheticDataset(opt, 4))
        graphed = GraphedStep(model)
        graphed.capture(data[0])
        for i in range(a.warmup):
            graphed.step(data[i % 4])
            model.accum_accs()
        torch.cuda.synchronize()
        dev = model.device
        out = {"clocks_before": clocks(), "size": n, "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
               "metrics": a.metrics,
               "baseline": "parent commit's accum_accs (host): .cpu() + util.compute_Rand_F_scores on channel 0 + bincount confusion"}

        # ---- the metric alone, on the trainer's tensors and on a cell-like boundary map ------------------------------------------
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        trainer_maps = (model.fake_B, model.real_B)

        def device_times():
            dev_ms, enq_ms = [], []
            for i in range(a.warmup + a.steps):
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                e0.record()
                model.accum_accs()
                e1.record()
                w1 = time.perf_counter()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    dev_ms.append(e0.elapsed_time(e1))
                    enq_ms.append((w1 - w0) * 1e3)
            return dev_ms, enq_ms

        for name, (fb, rb) in (("trainer_tensors_synthetic_noise", trainer_maps), ("cell_map", cell_maps(n, dev))):
            model.fake_B, model.real_B = fb, rb
            host_ms = []
            dev_ms, enq_ms = device_times()
            compare = None
            if a.compare:          # the same trainer asked for the other metric set, on the same tensors, back to back
                model.opt.which_metric = a.compare
                compare = {"metrics": a.compare, "device_kernels": stats(device_times()[0])}
                model.opt.which_metric = a.metrics
            state = {"rand": [], "conf": np.zeros((2, 2))}
            for i in range(a.warmup + a.steps):
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                host_accum(model, state)
                if i >= a.warmup:
                    host_ms.append((time.perf_counter() - w0) * 1e3)
            model.reset_accs()
            model.accum_accs()
            got = model.get_current_accs()
            if "RandScore" in got:
                assert abs(got["RandScore"] - state["rand"][-1]) < 1e-9, (got, state["rand"][-1])
            out[name] = {"device_kernels": stats(dev_ms), "device_enqueue_host_side": stats(enq_ms), "host_path": stats(host_ms),
                         "regions_truth": int(torch.unique(model.seg_metrics.truth_labels).numel())}
            out[name].update({k: float(v) for k, v in got.items()})
            if "VInfo" in got:
                want = float(compute_VInfo_scores(model.fake_B.detach()[0, 0].cpu().numpy(), model.real_B.detach()[0, 0].cpu().numpy())[0])
                assert abs(got["VInfo"] - want) < 1e-9, (got, want)
            if compare is not None:
                out[name]["compare"] = compare
            print(name, json.dumps(out[name]))
        model.fake_B, model.real_B = trainer_maps

        # ---- the graphed step loop ---------------------------------------------------------------------------------------------
        def loop(after):
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            for i in range(a.steps):
                graphed.step(data[i % 4])
                after()
            torch.cuda.synchronize()
            return (time.perf_counter() - w0) * 1e3 / a.steps

        state = {"rand": [], "conf": np.zeros((2, 2))}
        variants = (("no_metric", lambda: None), ("device_accum_accs", model.accum_accs), ("host_accum_accs", lambda: host_accum(model, state)))
        out["graphed_step_loop_ms_per_step"] = {k: [] for k, _ in variants}
        for _ in range(a.repeats):
            for k, fn in variants:
                model.reset_accs()
                out["graphed_step_loop_ms_per_step"][k].append(loop(fn))
        ops.check_metric_err(dev)
        out["clocks_after"] = clocks()
        print("clocks", out["clocks_before"], out["clocks_after"])
        print("graphed_step_loop_ms_per_step", json.dumps(out["graphed_step_loop_ms_per_step"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":
    main()

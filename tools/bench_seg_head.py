#!/usr/bin/env python3
"""The loss section of a discriminator-less segmentation step (`--which_model_netD None`) at 512 x 512: the composition of the existing
kernels (softmax: sgan_softmax_fwd + sgan_ce_fwd + sgan_ce_bwd; sigmoid: sgan_sigmoid_nhwc_fwd + sgan_bce_weighted_fwd +
sgan_bce_weighted_bwd + sgan_sigmoid_nhwc_bwd) against the one launch of sgan_seg_head, in the same process on the same operands.

    python tools/bench_seg_head.py [--size 512] [--reps 50] [--rounds 21] [--out profiles/r10_seg_head.jsonl]

Two figures per variant, both between device events: `graph_us`, one section inside a hipGraph of --reps sections replayed back to
back (kernels and the gaps between them, no host in the way), and `eager_us`, the same launches issued from Python (what an eager
step pays: mostly the host).  The variants alternate round by round; medians and the 10th / 90th percentile of the rounds go out,
one JSON line per case.  Before anything is timed the two variants' p, loss and dlogits are compared on the timed operands."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def operands(size, C_, dev):
    from supervised_gan_amd.ops import pad4
    g = torch.Generator().manual_seed(size + C_)
    Cs = pad4(C_)
    z = torch.zeros(size, size, Cs)
    z[..., :C_] = torch.randn(size, size, C_, generator=g) * 1.5
    lab = torch.randint(0, C_, (size * size,), generator=g)
    t = torch.zeros(size, size, Cs)
    t[..., :C_] = F.one_hot(lab, C_).float().view(size, size, C_)
    cw = torch.tensor([2.0, 5.0, 0.5, 3.0][:C_])
    return z.to(dev), lab.to(dev), t.to(dev), cw.to(dev)


def sections(mode, size, C_, dev, reps):
    """(composed, fused, outputs): two callables that each launch ONE loss section, and the tensors they leave their results in."""
    from supervised_gan_amd import ops
    z, lab, t, cw = operands(size, C_, dev)
    one = torch.ones((), device=dev)
    new = lambda: torch.empty_like(z)      # noqa: E731
    pc, dc, pf, df, dp = new(), new(), new(), new(), new()
    lc, lf = torch.zeros((), device=dev), torch.zeros((), device=dev)
    if mode == "softmax":
        norm = torch.zeros((), device=dev)
        ops.label_weight_sum(lab, C_, cw, norm)
        accs = torch.zeros(reps + 1, 4, dtype=torch.float64, device=dev)      # sgan_ce_fwd wants zeroed sums: one set per section of a replay
        state = {"i": 0}

        def composed():
            acc = accs[state["i"] % (reps + 1)][:3]
            state["i"] += 1
            ops.softmax_fwd(z, C_, pc)
            ops.ce_fwd(z, C_, lab, 0, cw, acc, lc)
            ops.ce_bwd(z, C_, lab, 0, cw, acc, one, dc)

        def fused():
            assert ops.seg_head(z, C_, ops.SEGHEAD_SOFTMAX, lab, cw, C_, norm, pf, df, lf)

        def reset():
            state["i"] = 0
            accs.zero_()
    else:
        def composed():
            ops.sigmoid_nhwc_fwd(z, C_, pc)
            ops.bce_weighted_fwd(pc, t, C_, cw, C_, lc)
            ops.bce_weighted_bwd(pc, t, C_, cw, C_, one, dp)
            ops.sigmoid_nhwc_bwd(dp, pc, C_, dc)

        def fused():
            assert ops.seg_head(z, C_, ops.SEGHEAD_SIGMOID, t, cw, C_, None, pf, df, lf)

        def reset():
            pass
    return composed, fused, reset, (pc, lc, dc), (pf, lf, df)


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


def time_us(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def stats(us):
    s = sorted(us)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]      # noqa: E731
    return {"median_us": round(q(0.5), 3), "p10_us": round(q(0.1), 3), "p90_us": round(q(0.9), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=50, help="loss sections per timed window")
    ap.add_argument("--rounds", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_seg_head.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seg_head.py measures on an MI355X; no CUDA/HIP device is visible")
    dev = torch.device("cuda", 0)
    lines = []
    for mode in ("softmax", "sigmoid"):
        for C_ in (2, 3):
            composed, fused, reset, out_c, out_f = sections(mode, a.size, C_, dev, a.reps)
            reset()
            composed()
            fused()
            torch.cuda.synchronize()
            diff = {k: rel(f, c) for k, f, c in zip(("p", "loss", "dlogits"), out_f, out_c)}
            graphs = {}
            side = torch.cuda.Stream()
            for name, fn in (("composed", composed), ("fused", fused)):
                reset()
                g = torch.cuda.CUDAGraph()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    for _ in range(3):
                        fn()
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                reset()
                with torch.cuda.graph(g):
                    for _ in range(a.reps):
                        fn()
                graphs[name] = g

            def eager(fn):
                for _ in range(a.reps):
                    fn()
            res = {"composed": {"graph": [], "eager": []}, "fused": {"graph": [], "eager": []}}
            for r in range(a.rounds + 2):
                for name, fn in (("composed", composed), ("fused", fused)):
                    reset()
                    torch.cuda.synchronize()
                    tg = time_us(graphs[name].replay, a.reps)
                    reset()
                    torch.cuda.synchronize()
                    te = time_us(lambda: eager(fn), a.reps)
                    if r >= 2:      # two warm-up rounds
                        res[name]["graph"].append(tg)
                        res[name]["eager"].append(te)
            line = {"tool": "bench_seg_head", "device": torch.cuda.get_device_name(0), "mode": mode, "size": a.size, "C": C_,
                    "launches_composed": 3 if mode == "softmax" else 4, "launches_fused": 1, "reps": a.reps, "rounds": a.rounds,
                    "fused_vs_composed_rel_diff": diff}
            for name in ("composed", "fused"):
                line[name + "_graph"] = stats(res[name]["graph"])
                line[name + "_eager"] = stats(res[name]["eager"])
            line["graph_speedup"] = round(line["composed_graph"]["median_us"] / line["fused_graph"]["median_us"], 3)
            line["eager_speedup"] = round(line["composed_eager"]["median_us"] / line["fused_eager"]["median_us"], 3)
            print(json.dumps(line))
            lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

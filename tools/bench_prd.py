"""Timing of the k-nearest-neighbour passes of the precision / recall / density / coverage scores (sgan_prd.hip) on
synthetic descriptors (rank-6 structure plus noise, as tests/test_hip_prd.py draws them).  Shapes: N = 3840 and N = 16384 rows per set,
K = 49 and 147, k = 3, group = 128.  On data that is already on the device, `--steps` samples after `--warmup`, each sample `--batch`
calls between two events after a synchronise, the paths alternating so that a drift of the clocks meets all alike:
  (a) knn_radii and prd_rows, each in its direct and its gram form
  (b) the same results composed from torch on the same normalised descriptors: cdist (its matmul form) squared, a mask of the groups and
      topk for the radii; comparisons, a sum, a min for the rows
in microseconds per call, each as median, min and p90.  Before anything is timed, the two forms are held against each other (the
radii within the sum of their two bounds, the counts within the rows that differ).  The clocks `rocm-smi --showclocks` reports are
recorded before and after (a query; nothing is set).  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_clean import clocks, stats  # noqa: E402
from supervised_gan_amd import ops  # noqa: E402
from supervised_gan_amd import util as U  # noqa: E402

SHAPES = ((3840, 49), (3840, 147), (16384, 49), (16384, 147))
KNN, GROUP = 3, 128


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=3, help="calls between the two events of one sample")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_prd.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    out = {"clocks_before": clocks(), "steps": a.steps, "warmup": a.warmup, "batch": a.batch, "device": torch.cuda.get_device_name(0),
           "unit": "microseconds per call", "k": KNN, "group": GROUP}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def sample(fn):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.batch):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.batch

    for N, K in SHAPES:
        C = K // 49
        rng = np.random.RandomState(N + K)
        W = rng.randn(6, K)
        A = (rng.randn(N, 6) @ W + 0.1 * rng.randn(N, K)).astype(np.float32)
        B = (rng.randn(N, 6) @ W + 0.1 * rng.randn(N, K)).astype(np.float32)
        per = A.reshape(N, C, 49).astype(np.float64)
        stats_np = np.concatenate([per.sum(axis=(0, 2)), (per * per).sum(axis=(0, 2))])
        mean, std = U.swd_stats_from_sums(stats_np, N * 49)
        dA, dB, st = torch.from_numpy(A).to(dev), torch.from_numpy(B).to(dev), torch.from_numpy(stats_np).to(dev)
        nA, nB = (torch.from_numpy(U.swd_normalise_ref(x, mean, std)).to(dev) for x in (A, B))
        ws = ops.prd_workspace(N, N, K, dev)
        rad, nn1 = torch.empty(N, device=dev), torch.empty(N, device=dev)
        cnt, nn_d2, nn_idx = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
        # the two forms against each other, before anything is timed
        rd = ops.knn_radii(dA, st, KNN, GROUP, variant=ops.PRD_DIRECT)[0].double()
        rg = ops.knn_radii(dA, st, KNN, GROUP, variant=ops.PRD_GRAM)[0].double()
        u = 2.0 ** -24
        n2 = float((nA.double() ** 2).sum(dim=1).max())
        bound = (K + 2) * u / (1 - (K + 2) * u) * float(rd.max()) * 1.01 + (K + 3) * u / (1 - (K + 3) * u) * 4 * n2
        assert float((rd - rg).abs().max()) <= bound, (N, K, float((rd - rg).abs().max()), bound)
        cd = ops.prd_rows(dB, dA, st, rd.float(), variant=ops.PRD_DIRECT)[0]
        cg = ops.prd_rows(dB, dA, st, rd.float(), variant=ops.PRD_GRAM)[0]
        differ = int((cd != cg).sum())
        assert differ <= 0.02 * N, (N, K, differ)
        gid = torch.arange(N, device=dev) // GROUP
        same = gid[:, None] == gid[None, :]
        rad_t = rd.float()

        def torch_knn():
            d2 = torch.cdist(nA, nA, compute_mode="use_mm_for_euclid_dist").square_()
            d2.masked_fill_(same, float("inf"))
            v = d2.topk(KNN, dim=1, largest=False).values
            return v[:, KNN - 1], v[:, 0]

        def torch_rows():
            d2 = torch.cdist(nB, nA, compute_mode="use_mm_for_euclid_dist").square_()
            m = d2.min(dim=1)
            return (d2 <= rad_t[None, :]).sum(dim=1), m.values, m.indices

        torch_rad_err = float((torch_knn()[0].double() - rd).abs().max())
        calls = {"knn_radii_direct": lambda: ops.knn_radii(dA, st, KNN, GROUP, rad=rad, nn1=nn1, workspace=ws, variant=ops.PRD_DIRECT),
                 "knn_radii_gram": lambda: ops.knn_radii(dA, st, KNN, GROUP, rad=rad, nn1=nn1, workspace=ws, variant=ops.PRD_GRAM),
                 "prd_rows_direct": lambda: ops.prd_rows(dB, dA, st, rad_t, cnt=cnt, nn_d2=nn_d2, nn_idx=nn_idx, workspace=ws, variant=ops.PRD_DIRECT),
                 "prd_rows_gram": lambda: ops.prd_rows(dB, dA, st, rad_t, cnt=cnt, nn_d2=nn_d2, nn_idx=nn_idx, workspace=ws, variant=ops.PRD_GRAM),
                 "torch_knn_radii": torch_knn,
                 "torch_prd_rows": torch_rows}
        us = {k: [] for k in calls}
        for i in range(a.warmup + a.steps):
            for k, fn in calls.items():
                v = sample(fn)
                if i >= a.warmup:
                    us[k].append(v)
        r = out["N%d_K%d" % (N, K)] = {"N": N, "K": K, "max_diff_rad_direct_gram": float((rd - rg).abs().max()), "bound_of_that": bound,
                                       "rows_whose_cnt_differs_direct_gram": differ, "max_err_rad_torch_fp32_vs_direct": torch_rad_err}
        r.update({k: stats(v) for k, v in us.items()})
        for e in ("knn_radii", "prd_rows"):
            for f in ("direct", "gram"):
                r["%s_%s_over_torch" % (e, f)] = r["%s_%s" % (e, f)]["median_us"] / r["torch_" + e]["median_us"]
        del same, nA, nB, dA, dB
        torch.cuda.empty_cache()
    out["clocks_after"] = clocks()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()

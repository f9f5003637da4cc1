"""Timing of the three launches of whole-image inference (csrc/sgan_tile.hip) at T = 512 on a 1024 x 1024 image, and of a
whole 1024 x 1024 unet_256 prediction with and without --tta d4.  An instrument, not a gate: no threshold is read from it.

A launch lasts microseconds, less than two events resolve, so a timed window is `--reps` launches back to back on one stream between
two events after a synchronise, and the figure is the window over `--reps`: the time per launch of a busy queue.  Beside every kernel
stands a torch device copy of the bytes that kernel moves (read + written), timed the same way in the same run, window by window in
turn with it.  image_prep_tile and tile_blend are timed at rot 0 and rot 1 (under a rotation the gather side strides).  The whole
prediction is SegmentationModel.test() on a freshly initialised unet_256 (ngf 64), host wall time around a synchronise."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_region_stats import clocks, stats  # noqa: E402
from supervised_gan_amd import ops, util  # noqa: E402


def _whole_prediction(img, T, M, R, steps, warmup, ngf):
    """Wall ms of model.test() on `img` with and without --tta d4: {'none': stats, 'd4': stats, 'passes': {...}}."""
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TestOptions, TrainOptions
    H, W = img.shape[:2]
    res = {"passes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        net = ["--name", "bench_tile", "--model", "segmentation", "--dataset_mode", "single", "--fineSize", str(T), "--which_model_netG", "unet_256",
               "--ngf", str(ngf), "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout", "--checkpoints_dir", tmp]
        create_model(TrainOptions().parse(net + ["--dataroot", "synthetic", "--which_model_netD", "None"], save=False, verbose=False)).save("latest")
        u8 = torch.from_numpy(img).cuda()
        data = {"A": ops.logical_view(ops.image_prep_tile(u8, 0, 0, H, W, False, 0), 3), "A_u8": u8, "A_paths": ["bench"]}
        for tta in ("none", "d4"):
            flags = ["--dataroot", tmp, "--whole_image", "--tile", str(T), "--tile_margin", str(M), "--tile_ramp", str(R), "--tta", tta]
            model = create_model(TestOptions().parse(net + flags, save=False, verbose=False))
            model.set_input(data)
            ms = []
            for i in range(warmup + steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                model.test()
                torch.cuda.synchronize()
                if i >= warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            res[tta] = stats(ms)
            res["passes"][tta] = len(model._tile_st["passes"])
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30, help="timed windows per variant")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200, help="launches per window")
    ap.add_argument("--image", type=int, default=1024)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--margin", type=int, default=16)
    ap.add_argument("--ramp", type=int, default=16)
    ap.add_argument("--ngf", type=int, default=64)
    ap.add_argument("--predict_steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_tile.json"))
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "needs an MI355X"
    dev, S, T, M, R, C = torch.device("cuda", 0), a.image, a.tile, a.margin, a.ramp, 2
    img = np.random.RandomState(0).randint(0, 256, size=(S, S, 3), dtype=np.uint8)
    u8 = torch.from_numpy(img).to(dev)
    stride = max(1, T - 2 * M - R)
    oy, ox, Wy, Wx = util.tile_plan(S, S, T, M, R, stride)
    wy, wx = torch.tensor(Wy, dtype=torch.int32, device=dev), torch.tensor(Wx, dtype=torch.int32, device=dev)
    tile = torch.empty((T, T, 4), dtype=torch.float32, device=dev)
    logits = torch.randn((T, T, 4), device=dev)
    canvas = torch.zeros((S, S, 4), dtype=torch.float32, device=dev)
    prob, logp = torch.empty_like(canvas), torch.empty_like(canvas)
    y0 = x0 = oy[1] if len(oy) > 2 else oy[0]      # an inner tile: all of its non-margin part lies inside the image

    # the timed launches compute what the yardsticks compute
    for rot in (0, 1):
        got = ops.image_prep_tile(u8, -M, -M, T, T, True, rot, out=tile)[..., :3].permute(2, 0, 1).cpu().numpy()
        assert np.array_equal(got, util.prep_tile_ref(img, -M, -M, T, T, True, rot)), rot
    inner = (T - 2 * M) ** 2
    moved = {"image_prep_tile": T * T * (3 + 16), "tile_blend": inner * (16 + 16 + 16), "tile_finish": S * S * (16 + 16 + 16) + 8 * S}

    def copy_of(nbytes):
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)      # a copy of n/2 bytes reads n/2 and writes n/2
        dst = torch.empty_like(src)
        return lambda: dst.copy_(src)

    variants = {}
    for rot in (0, 1):
        variants["image_prep_tile_rot%d" % rot] = (lambda rot=rot: ops.image_prep_tile(u8, x0, y0, T, T, False, rot, out=tile), "image_prep_tile")
        variants["tile_blend_rot%d" % rot] = (lambda rot=rot: ops.tile_blend(logits, C, ops.SEGHEAD_SOFTMAX, x0, y0, M, R, False, rot, canvas), "tile_blend")
    variants["tile_finish"] = (lambda: ops.tile_finish(canvas, C, wy, wx, 8, prob, logp), "tile_finish")
    for k in list(moved):
        variants["copy_of_%s_bytes" % k] = (copy_of(moved[k]), k)
    us = {k: [] for k in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    c_before = clocks()
    for i in range(a.warmup + a.steps):
        for name, (fn, _) in variants.items():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                us[name].append(e0.elapsed_time(e1) / a.reps)      # ms
    per = {k: {kk.replace("_ms", "_us"): (vv * 1e3 if kk.endswith("_ms") else vv) for kk, vv in stats(v).items()} for k, v in us.items()}
    ratio = {k: per[k]["median_us"] / per["copy_of_%s_bytes" % kind]["median_us"] for k, (_, kind) in variants.items() if not k.startswith("copy_of")}
    res = {"device": torch.cuda.get_device_name(0), "clocks_before": c_before, "image": S, "tile": T, "margin": M, "ramp": R, "stride": stride,
           "classes": C, "reps_per_window": a.reps, "windows": a.steps, "warmup_windows": a.warmup,
           "unit": "us per launch, back-to-back launches on one stream between two events; one run on one card",
           "bytes_moved": moved, "per_launch": per, "ratio_to_copy_of_same_bytes_median": ratio,
           "whole_prediction_unet_256_wall_ms": _whole_prediction(img, T, M, R, a.predict_steps, 2, a.ngf), "clocks_after": clocks()}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


if __name__ == "__main__":
    main()

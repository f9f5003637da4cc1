"""Times the Lovasz-softmax term alone at 512 x 512 for n = 1 and 2 listed classes (forward, and forward + backward; hip events over
`--reps` calls) on a cell map with soft walls, on per-pixel noise and on a saturated (binary) prediction, beside the same
computation composed from torch.sort on the keys, cumsum, gathers and index_put on the same device, and the graphed
no-discriminator segmentation step without and with --lovasz_weight; writes profiles/<tag>_lovasz.json.
    python tools/bench_lovasz.py --tag r30 [--reps 200] [--steps 200]"""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def time_ms(fn, reps):
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def inputs(kind, size, dev):
    """(p [1, 3, size, size], label [size, size]): class 0 is the wall."""
    g = torch.Generator(device="cpu").manual_seed(7)
    if kind == "cell_map":      # 32-pixel cells behind 3-pixel walls; the prediction is the truth blurred, so the walls are soft
        y, x = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
        wall = ((y % 32) < 3) | ((x % 32) < 3)
        label = torch.where(wall, 0, 1 + ((y // 32 + x // 32) % 2)).long()
        onehot = torch.nn.functional.one_hot(label, 3).permute(2, 0, 1)[None].float()
        p = torch.nn.functional.avg_pool2d(onehot, 5, 1, 2, count_include_pad=False)
        p = (p + 0.02 * torch.rand(p.shape, generator=g)) / 1.02
    else:
        label = torch.randint(0, 3, (size, size), generator=g)
        p = torch.softmax(2.0 * torch.randn((1, 3, size, size), generator=g), 1)
        if kind == "saturated":
            p = torch.nn.functional.one_hot(p.argmax(1), 3).permute(0, 3, 1, 2).float()
    return p.contiguous().to(dev), label.to(dev)


def composed(p, label, classes):
    """The same loss and gradient from ATen calls: the unique 64-bit key, sort, gathers, cumsum, and index_put for the gradient."""
    N = label.numel()
    idx = torch.arange(N, device=p.device)
    dp = torch.zeros_like(p).view(p.shape[1], N)
    losses = []
    for c in classes:
        fg = label.view(N) == c
        pc = p[0, c].reshape(N)
        e = (fg.float() - pc).abs()
        key = ((0xFFFFFFFF - e.view(torch.int32).long()) << 32) | idx
        _, pi = torch.sort(key)
        f = fg[pi]
        G = f.sum()
        ck = torch.cumsum(f, 0)
        k1 = idx + 1
        inter, union = G - ck, G + (k1 - ck)
        g = torch.where(f, 1.0 / union.double(), inter.double() / (union * (union - 1)).clamp(min=1).double())
        losses.append((e[pi].double() * g).sum())
        dp[c].index_put_((pi,), (torch.sign(pc - fg.float())[pi].double() * g).float())
    return torch.stack(losses).mean().float(), dp / len(classes)      # every listed class of the bench inputs is present


def term_times(reps, size=512):
    from supervised_gan_amd import ops
    dev = torch.device("cuda", 0)
    out = {}
    for kind in ("cell_map", "noise", "saturated"):
        p, label = inputs(kind, size, dev)
        for classes in ((0,), (0, 1)):
            work = ops.new_lovasz_workspace(size, size, len(classes), dev)
            loss, dp = torch.empty((), device=dev), torch.empty_like(p)

            def fwd():
                ops.lovasz_forward(p, label, classes, work, loss_out=loss)

            def both():
                fwd()
                ops.lovasz_backward(p, classes, work, dp=dp)
            ref = composed(p, label, classes)
            both()
            torch.cuda.synchronize()
            out["%s_n%d" % (kind, len(classes))] = {
                "forward_ms": time_ms(fwd, reps), "forward_backward_ms": time_ms(both, reps),
                "composed_forward_backward_ms": time_ms(lambda: composed(p, label, classes), max(reps // 4, 10)),
                "loss": float(loss), "composed_loss": float(ref[0]), "max_abs_dp_diff": float((dp[0].view(3, -1) - ref[1]).abs().max())}
    return out


def step_time(extra, steps, size=512):
    from supervised_gan_amd.graph_step import GraphedStep
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    argv = ["--name", "b", "--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", str(size),
            "--which_model_netG", "unet_256", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout", "--dataroot",
            "synthetic", "--which_model_netD", "None", "--weights", "1", "2"]
    with tempfile.TemporaryDirectory() as ckpt:      # the options want a checkpoint directory; nothing is saved
        opt = TrainOptions().parse(argv + ["--checkpoints_dir", ckpt] + list(extra), save=False, verbose=False)
        m = create_model(opt)
        data = SyntheticDataset(opt, 1).ring[0]
        g = GraphedStep(m)
        g.capture(data)
        return time_ms(lambda: g.step(data), steps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="r30")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    res = {"term_512": term_times(a.reps),
           "graphed_step_ms": {"without": step_time((), a.steps), "lovasz_0.5": step_time(("--lovasz_weight", "0.5"), a.steps),
                               "lovasz_0.5_classes_0_1": step_time(("--lovasz_weight", "0.5", "--lovasz_classes", "0", "1"), a.steps)},
           "device": torch.cuda.get_device_name(0)}
    path = os.path.join(ROOT, "profiles", "%s_lovasz.json" % a.tag)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

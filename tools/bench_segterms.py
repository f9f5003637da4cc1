"""Times the Tversky / focal loss terms on the logits at 512 x 512 with 3 classes (hip events over `--reps` calls, `--rounds` rounds that
alternate what is compared): the forward launch, the backward launch and both, beside sgan_seg_head on the same buffers and beside the
same terms composed from torch ops (forward and autograd backward) on the same device; then the graphed unet_256 segmentation step
without a discriminator, without and with `--dice_weight 0.5 --focal_weight 0.5`.  Also the bytes each launch has to move, from the
shapes, over its time.  Writes profiles/<tag>_segterms.json.
    python tools/bench_segterms.py --tag r31 [--reps 300] [--steps 200] [--rounds 3]"""
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


def composed(z, label, classes, a, b, s, E, gamma, w):
    """Both terms from ATen calls on the [npix, C] logits, softmax head, and their gradient through autograd."""
    z = z.detach().requires_grad_(True)
    C = z.shape[1]
    p = torch.softmax(z, 1)
    t = torch.nn.functional.one_hot(label, C).float()
    LT = 0
    for c in classes:
        TP = (p[:, c] * t[:, c]).sum()
        FP = (p[:, c] * (1 - t[:, c])).sum()
        FN = ((1 - p[:, c]) * t[:, c]).sum()
        LT = LT + (1 - (TP + s) / (TP + a * FP + b * FN + s)) ** E
    LT = LT / len(classes)
    lp = torch.log_softmax(z, 1).gather(1, label[:, None])[:, 0]
    wy = w[label]
    LF = (wy * (1 - lp.exp()) ** gamma * -lp).sum() / wy.sum()
    (0.5 * LT + 0.5 * LF).backward()
    return LT.detach(), LF.detach(), z.grad


def term_times(reps, rounds, size=512, C=3):
    from supervised_gan_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(7)
    npix = size * size
    zb = torch.zeros((size, size, 4))
    zb[:, :, :C] = 2.0 * torch.randn((size, size, C), generator=g)
    zb = zb.to(dev)
    label = torch.randint(0, C, (npix,), generator=g).to(dev)
    cw = torch.tensor([1.0, 2.0, 1.5], device=dev)
    classes, par, gamma = [0, 1], (0.5, 0.5, 1.0, 1.0), 2.0
    state, work = ops.new_seg_terms_state(dev), ops.new_seg_terms_workspace(dev)
    lT, lF = torch.zeros((), device=dev), torch.zeros((), device=dev)
    half = torch.full((), 0.5, device=dev)
    dz, p, dh = torch.empty_like(zb), torch.empty_like(zb), torch.empty_like(zb)
    norm, loss = torch.zeros((), device=dev), torch.zeros((), device=dev)
    ops.label_weight_sum(label, C, cw, norm)
    zl = zb[:, :, :C].reshape(npix, C).contiguous()

    def fwd():
        ops.seg_terms_forward(zb, C, ops.SEGHEAD_SOFTMAX, label, classes, *par, gamma, cw, state, lT, lF, work)

    def bwd():
        ops.seg_terms_backward(zb, C, ops.SEGHEAD_SOFTMAX, label, classes, gamma, cw, state, half, half, dz)

    def both():
        fwd()
        bwd()

    def head():
        ops.seg_head(zb, C, ops.SEGHEAD_SOFTMAX, label, cw, C, norm, p, dh, loss)

    def torch_ops():
        return composed(zl, label, classes, *par, gamma, cw)

    both()
    ref = torch_ops()
    torch.cuda.synchronize()
    names = {"forward_ms": fwd, "backward_ms": bwd, "forward_backward_ms": both, "seg_head_ms": head, "composed_forward_backward_ms": torch_ops}
    times = {k: [] for k in names}
    for _ in range(rounds):      # alternating: every round times each of them once
        for k, fn in names.items():
            times[k].append(time_ms(fn, reps if k != "composed_forward_backward_ms" else max(reps // 4, 10)))
    # what each launch has to move at this shape: logits rows of 16 bytes, int64 labels, gradient / prediction rows of 16 bytes
    moved = {"forward": npix * (16 + 8), "backward": npix * (16 + 8 + 16), "seg_head": npix * (16 + 8 + 16 + 16)}
    best = {k: min(v) for k, v in times.items()}
    return {"rounds": times, "best": best, "bytes": moved,
            "gbytes_per_s": {"forward": moved["forward"] / best["forward_ms"] / 1e6, "backward": moved["backward"] / best["backward_ms"] / 1e6,
                             "seg_head": moved["seg_head"] / best["seg_head_ms"] / 1e6},
            "L_T": float(lT), "L_F": float(lF), "composed_L_T": float(ref[0]), "composed_L_F": float(ref[1]),
            "max_abs_dz_diff": float((dz[:, :, :C].reshape(npix, C) - ref[2]).abs().max()), "max_abs_dz": float(ref[2].abs().max())}


def build_step(extra, size=512):
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
        return lambda: g.step(data)


def step_times(steps, rounds):
    runs = {"without": build_step(()), "dice_0.5_focal_0.5": build_step(("--dice_weight", "0.5", "--focal_weight", "0.5"))}
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            times[k].append(time_ms(fn, steps))
    return {"rounds": times, "best": {k: min(v) for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="r31")
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_segterms.py measures on the device; none is visible"
    res = {"term_512_c3": term_times(a.reps, a.rounds), "graphed_step_ms": step_times(a.steps, a.rounds),
           "device": torch.cuda.get_device_name(0)}
    path = os.path.join(ROOT, "profiles", "%s_segterms.json" % a.tag)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

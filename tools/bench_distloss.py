"""Times the distance-map loss terms at 512 x 512 with 3 classes (hip events over `--reps` calls, `--rounds` rounds that alternate what
is compared): sgan_signed_edt_sq beside two sgan_edt_sq calls on the same plane; the forward launch, the backward launch and both of
the boundary / Hausdorff node beside sgan_seg_terms_forward / _backward on the same buffers and beside the same two terms composed
from torch ops (forward and autograd backward) on the same device; then the graphed unet_256 segmentation step without a
discriminator, without and with `--boundary_loss_weight 0.01 --hausdorff_weight 0.001`.  Also the bytes each launch has to move, from
the shapes, over its time.  No training outcome is measured.  Writes profiles/<tag>_distloss.json.
    python tools/bench_distloss.py --tag r32 [--reps 300] [--steps 200] [--rounds 3] [--out FILE]"""
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


def composed(z, label, cls, t_s, p_s, alpha):
    """Both terms from ATen calls on the [npix, C] logits, softmax head, the fields float constants, and their gradient through
    autograd."""
    z = z.detach().requires_grad_(True)
    p = torch.softmax(z, 1)[:, cls]
    g = (label == cls).float()
    d = t_s.abs().sqrt()
    phi = torch.where(t_s > 0, d, torch.where(t_s < 0, 1 - d, torch.zeros_like(d)))
    LB = (phi * p).mean()
    F = t_s.abs() ** (alpha / 2) + p_s.abs() ** (alpha / 2)
    LH = ((p - g) ** 2 * F).mean()
    (0.5 * LB + 0.5 * LH).backward()
    return LB.detach(), LH.detach(), z.grad


def term_times(reps, rounds, size=512, C=3):
    from supervised_gan_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator(device="cpu").manual_seed(7)
    npix = size * size
    zb = torch.zeros((size, size, 4))
    zb[:, :, :C] = 2.0 * torch.randn((size, size, C), generator=g)
    zb = zb.to(dev)
    # a cell map: walls every 32 pixels, 2 wide; the prediction's walls shifted by 3 pixels
    yy, xx = torch.meshgrid(torch.arange(size), torch.arange(size), indexing="ij")
    truth = ((yy % 32 < 2) | (xx % 32 < 2)).float().to(dev)
    pred = (((yy + 3) % 32 < 2) | ((xx + 3) % 32 < 2)).float().to(dev)
    label = torch.where(truth.reshape(-1) > 0.5, torch.zeros(npix, dtype=torch.int64, device=dev),
                        torch.randint(1, C, (npix,), generator=g).to(dev))
    cls, alpha = 0, 2.0
    t_s, p_s = ops.signed_edt_sq(truth), ops.signed_edt_sq(pred)
    d1, d2 = torch.empty_like(t_s), torch.empty_like(t_s)
    state, work = ops.new_dist_loss_state(dev), ops.new_dist_loss_workspace(dev)
    lB, lH = torch.zeros((), device=dev), torch.zeros((), device=dev)
    half = torch.full((), 0.5, device=dev)
    dz = torch.empty_like(zb)
    st_state, st_work = ops.new_seg_terms_state(dev), ops.new_seg_terms_workspace(dev)
    cw = torch.tensor([1.0, 2.0, 1.5], device=dev)
    zl = zb[:, :, :C].reshape(npix, C).contiguous()
    tf, pf = t_s.reshape(-1).float(), p_s.reshape(-1).float()

    def signed():
        ops.signed_edt_sq(pred, out=d1)

    def two_edt():
        ops.edt_sq(pred, out=d1)
        ops.edt_sq(truth, out=d2)

    def fwd():
        ops.dist_loss_forward(zb, C, ops.SEGHEAD_SOFTMAX, label, cls, t_s, p_s, True, alpha, state, lB, lH, work)

    def bwd():
        ops.dist_loss_backward(zb, C, ops.SEGHEAD_SOFTMAX, label, cls, t_s, p_s, True, alpha, half, half, dz)

    def both():
        fwd()
        bwd()

    def st_fwd():
        ops.seg_terms_forward(zb, C, ops.SEGHEAD_SOFTMAX, label, [0, 1], 0.5, 0.5, 1.0, 1.0, 2.0, cw, st_state, lB, lH, st_work)

    def st_bwd():
        ops.seg_terms_backward(zb, C, ops.SEGHEAD_SOFTMAX, label, [0, 1], 2.0, cw, st_state, half, half, dz)

    def torch_ops():
        return composed(zl, label, cls, tf, pf, alpha)

    st_fwd()
    both()
    torch.cuda.synchronize()
    LB, LH = float(lB), float(lH)
    mine = dz[:, :, :C].reshape(npix, C).clone()
    ref = torch_ops()
    torch.cuda.synchronize()
    names = {"signed_edt_ms": signed, "two_edt_ms": two_edt, "forward_ms": fwd, "backward_ms": bwd, "forward_backward_ms": both,
             "seg_terms_forward_ms": st_fwd, "seg_terms_backward_ms": st_bwd, "composed_forward_backward_ms": torch_ops}
    times = {k: [] for k in names}
    for _ in range(rounds):      # alternating: every round times each of them once
        for k, fn in names.items():
            times[k].append(time_ms(fn, reps if k != "composed_forward_backward_ms" else max(reps // 4, 10)))
    # what each launch has to move at this shape: logits rows of 16 bytes, int64 labels, two int32 maps, gradient rows of 16 bytes
    moved = {"forward": npix * (16 + 8 + 4 + 4), "backward": npix * (16 + 8 + 4 + 4 + 16)}
    best = {k: min(v) for k, v in times.items()}
    return {"rounds": times, "best": best, "bytes": moved,
            "gbytes_per_s": {"forward": moved["forward"] / best["forward_ms"] / 1e6, "backward": moved["backward"] / best["backward_ms"] / 1e6},
            "L_B": LB, "L_H": LH, "composed_L_B": float(ref[0]), "composed_L_H": float(ref[1]),
            "max_abs_dz_diff": float((mine - ref[2]).abs().max()), "max_abs_dz": float(ref[2].abs().max())}


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
    """g.step(data) includes set_input, which with the options refreshes the truth's map: what a training step pays."""
    runs = {"without": build_step(()), "boundary_0.01": build_step(("--boundary_loss_weight", "0.01")),
            "boundary_0.01_hausdorff_0.001": build_step(("--boundary_loss_weight", "0.01", "--hausdorff_weight", "0.001"))}
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            times[k].append(time_ms(fn, steps))
    return {"rounds": times, "best": {k: min(v) for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="r32")
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="the file to write instead of profiles/<tag>_distloss.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_distloss.py measures on the device; none is visible"
    res = {"term_512_c3": term_times(a.reps, a.rounds), "graphed_step_ms": step_times(a.steps, a.rounds),
           "device": torch.cuda.get_device_name(0), "not_measured": "any training outcome (BoundF / HausD / ASSD of a trained model)"}
    path = a.out or os.path.join(ROOT, "profiles", "%s_distloss.json" % a.tag)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

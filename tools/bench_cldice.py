"""Times the soft-clDice term alone at 512 x 512 for K = 3, 5, 10 (forward + finish + backward, hip events over `--reps` calls) and
the graphed no-discriminator segmentation step without and with --cldice_weight, and writes profiles/<tag>_cldice.json.
    python tools/bench_cldice.py --tag r29 [--reps 200] [--steps 200]"""
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


def term_times(reps, size=512):
    from supervised_gan_amd import ops
    dev = torch.device("cuda", 0)
    p = torch.rand(size, size, device=dev)
    t = (torch.rand(size, size, device=dev) < 0.3).float()
    out = {}
    for K in (3, 5, 10):
        work, state = ops.new_cldice_workspace(size, size, K, dev, backward=True), ops.new_cldice_state(dev)
        st = ops.soft_skeleton(t, K)
        sp, dp, loss = torch.empty_like(p), torch.empty_like(p), torch.empty((), device=dev)

        def fwd():
            ops.soft_skeleton(p, K, out=sp, work=work)
            ops.cldice_finish(sp, t, st, p, state, loss)

        def both():
            fwd()
            ops.cldice_backward(t, st, state, K, work, dp=dp)
        out["K%d" % K] = {"forward_ms": time_ms(fwd, reps), "forward_backward_ms": time_ms(both, reps)}
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
    ap.add_argument("--tag", default="r29")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    res = {"term_512": term_times(a.reps),
           "graphed_step_ms": {"without": step_time((), a.steps), "cldice_0.5_K5": step_time(("--cldice_weight", "0.5"), a.steps)},
           "device": torch.cuda.get_device_name(0)}
    path = os.path.join(ROOT, "profiles", "%s_cldice.json" % a.tag)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

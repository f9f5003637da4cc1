"""Step time of the supervised segmentation baseline (`--which_model_netD None --weights 1 2`: 512 x 512, unet_256, ngf 32, instance
norm, synthetic data -- whose labels are per-pixel noise, the costly input of the border kernel) with and without `--border_weight 10 5`
(DESIGN.md R14): host wall time per step (set_input + step, ending in a synchronise) over 7 blocks of 50 steps per version, the two
versions alternating block by block, graphed and eager.  Writes profiles/r14_step_time.json."""
import json, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from supervised_gan_amd.models import create_model
from supervised_gan_amd.options import TrainOptions
from supervised_gan_amd.synthetic_data import SyntheticDataset
from supervised_gan_amd.graph_step import GraphedStep

def build(border, graph):
    argv = ["--name", "t", "--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "512",
            "--which_model_netG", "unet_256", "--ngf", "32", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout",
            "--checkpoints_dir", os.path.join(ROOT, "checkpoints"), "--dataroot", "synthetic", "--manualSeed", "4", "--which_model_netD", "None",
            "--weights", "1", "2"] + (["--border_weight", "10", "5"] if border else [])
    opt = TrainOptions().parse(argv, save=False, verbose=False)
    torch.manual_seed(4)
    m = create_model(opt)
    data = SyntheticDataset(opt, 16).ring
    g = None
    if graph:
        g = GraphedStep(m)
        g.capture(data[0])
    def step(i):
        d = data[i % 16]
        if g is None:
            m.set_input(d); m.optimize_parameters()
        else:
            g.step(d)
    for i in range(10):
        step(i)
    torch.cuda.synchronize()
    return m, step

def block(step, per):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(per):
        step(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / per

out = {}
blocks, per = 7, 50
for graph in (True, False):
    models = {"plain": build(False, graph), "border": build(True, graph)}
    ms = {"plain": [], "border": []}
    for b in range(blocks):      # the two versions alternate
        for k in ("plain", "border"):
            ms[k].append(block(models[k][1], per))
    for k in ("plain", "border"):
        key = ("graphed_" if graph else "eager_") + k
        out[key] = {"median_ms": statistics.median(ms[k]), "min_ms": min(ms[k]), "max_ms": max(ms[k]), "blocks": blocks, "steps_per_block": per,
                    "G_CE": models[k][0].get_current_errors()["G_CE"]}
        print(key, json.dumps(out[key]), flush=True)
    del models
with open(os.path.join(ROOT, "profiles", "r14_step_time.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")

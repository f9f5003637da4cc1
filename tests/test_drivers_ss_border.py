"""train_ss.py on the supervised baseline with the U-Net border term, `--which_model_netD None --weights 1 2 --border_weight 10 5`, at
64 x 64: the graphed run against the eager run, and the parser's refusal of the option beside a discriminator.

The graphed run's first iteration is the capture: its two warm-up steps are real optimizer steps, and the loss it logs names the
captured step's tensor, which holds no step's result yet (train_ss.py).  Its later iterations are replays, and replay k runs on the
weights after k + 1 updates.  The runs are therefore fed ONE image (`--epoch_size 1`: every epoch is one step on it, followed by a
validation pass that overwrites the trainer's label, border map and norm buffers): the two replays of a three-iteration graphed run
are steps 3 and 4 of a four-step eager run.  Tolerance: the graphed-against-eager rule of this project (tests/test_hip_segm_nod.py),
|a - b| < 5e-3 max(1, |b|), on the logged losses (three decimals) and on the last loss as the trainer holds it.

One image cannot tell a graph that reads the trainer's live label, border map and norm buffers from one that reads orphaned copies
holding the capture's contents.  test_replays_read_the_buffers_set_input_writes feeds a captured step DISTINCT images against an eager
twin that takes the same sequence of updates, and checks that the three buffers are the objects they were at the capture and hold
the current image's values."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NET = ["--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "64", "--which_model_netG",
       "resnet_6blocks", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout", "--dataroot",
       "synthetic", "--manualSeed", "4", "--which_model_netD", "None", "--weights", "1", "2", "--border_weight", "10", "5",
       "--print_freq", "1", "--valSize", "64", "--save_epoch_freq", "100"]
DRIVER = ["--epoch_size", "1", "--val_epoch_size", "1"]      # train_ss.py's own arguments


def logged_losses(ckpt, name):
    lines = [l for l in (ckpt / name / "loss_log.txt").read_text().splitlines() if l.startswith("(epoch:")]
    assert all("G_CE:" in l and "G_GAN" not in l for l in lines), lines
    return [float(l.split("G_CE:")[1].split()[0]) for l in lines]


@pytest.mark.gpu
def test_graphed_run_follows_the_eager_run(tmp_path):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    import train_ss
    from supervised_gan_amd import ops
    ckpt = tmp_path / "ckpt"
    common = NET + DRIVER + ["--checkpoints_dir", str(ckpt)]
    eager, _ = train_ss.main(common + ["--name", "eager", "--niter", "3", "--niter_decay", "1"])
    torch.cuda.synchronize()
    want_last = eager.get_current_errors()["G_CE"]
    assert eager.opt.border_radius == 20 and eager.bmap is not None and float(eager.bmap.max()) > 0.0
    graphed, _ = train_ss.main(common + ["--name", "graphed", "--niter", "2", "--niter_decay", "1", "--graph"])
    torch.cuda.synchronize()
    got_last = graphed.get_current_errors()["G_CE"]
    want, got = logged_losses(ckpt, "eager"), logged_losses(ckpt, "graphed")
    print(f"eager {want} (last {want_last!r}), graphed {got} (last {got_last!r})")
    assert len(want) == 4 and len(got) == 3 and np.isfinite(want + got).all()
    assert want[3] < want[0]      # the run trains
    for a, b in zip(got[1:], want[2:]):
        assert abs(a - b) < 5e-3 * max(1.0, abs(b)), (got, want)
    assert abs(got_last - want_last) < 5e-3 * max(1.0, abs(want_last))
    ops.check_metric_err(eager.device)


@pytest.mark.gpu
def test_replays_read_the_buffers_set_input_writes(tmp_path):
    """capture on image 0 (its two warm-up steps are updates on image 0), then replays on images 1, 2 and 0, against an eager twin
    stepping on images 0, 0, 1, 2, 0 from the same weights: the loss after every replay by the rule above, the border map and the
    norm bit for bit (integers and one fixed-order sum: no tolerance), and label / bmap / norm at the addresses the graph captured."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd.graph_step import GraphedStep
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    from supervised_gan_amd.util import border_weight_map

    def build():
        opt = TrainOptions().parse(NET + ["--name", "t", "--checkpoints_dir", str(tmp_path)], save=False, verbose=False)
        torch.manual_seed(4)
        return opt, create_model(opt)

    opt, twin = build()
    data = SyntheticDataset(opt, 3).ring
    assert len(data) == 3 and not torch.equal(data[0]["B"], data[1]["B"])
    want = []
    for i in (0, 0, 1, 2, 0):
        twin.set_input(data[i])
        twin.optimize_parameters()
        want.append((twin.get_current_errors()["G_CE"], twin.bmap.clone(), twin.norm.clone()))
    _, m = build()
    g = GraphedStep(m)
    g.capture(data[0])
    where = [t.data_ptr() for t in (m.label, m.bmap, m.norm)]
    for i, (loss, bmap, norm) in zip((1, 2, 0), want[2:]):
        g.step(data[i])
        torch.cuda.synchronize()
        got = m.get_current_errors()["G_CE"]
        print(f"image {i}: graphed G_CE {got!r}, eager twin {loss!r}, norm {float(m.norm)!r}")
        assert abs(got - loss) < 5e-3 * max(1.0, abs(loss))
        assert torch.equal(m.bmap, bmap) and torch.equal(m.norm, norm)
        assert [t.data_ptr() for t in (m.label, m.bmap, m.norm)] == where
    # the map the last replay read is the map of ITS image: the yardstick on the trainer's own cell labelling
    cells = m._border_cells.cpu().numpy()
    assert np.array_equal(cells == 0, (m.label[0] == 0).cpu().numpy())
    wb = border_weight_map(cells, 20, 10.0, 5.0)[2]
    assert (np.abs(m.bmap.cpu().numpy().astype(np.float64) - wb) <= 1e-4 * wb + 1e-30).all() and wb.max() > 0


def test_the_parser_refuses_border_weight_beside_a_discriminator():
    from supervised_gan_amd.options import TrainOptions
    argv = ["--name", "t", "--model", "segmentation", "--dataroot", "synthetic", "--gpu_ids", "-1", "--which_model_netD", "n_layers",
            "--border_weight", "10", "5"]
    with pytest.raises(AssertionError, match="--which_model_netD None"):
        TrainOptions().parse(argv, save=False, verbose=False)

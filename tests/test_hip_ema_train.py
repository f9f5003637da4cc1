"""--ema_decay through the trainers on the device: the shadow generator against the fp64 reference (ema_ref.py) over snapshots of the
live weights, eagerly and under a graphed step; what an unset option leaves alone; evaluation on the average after replays (the
stale-derived-copies hazard); checkpoints, --use_ema and --continue_train; the trainers that refuse the option."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ema_ref import T_MAX, ema_bound, ema_ref  # noqa: E402

pytestmark = pytest.mark.gpu

HW = 128
# the smallest option sets of test_graph_step.py / test_hip_segm_nod.py
ARCH = {
    "segmentation": ["--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", str(HW),
                     "--which_model_netG", "unet_128", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--no_dropout"],
    "fcgan": ["--model", "fcgan", "--which_direction", "A", "--dataset_mode", "single", "--fineSize", str(HW), "--input_nc", "2",
              "--which_model_netG", "deconv", "--n_layers_G", "5", "--ngf", "8", "--noise_nc", "8", "--noiseSize", "2", "--no_dropout",
              "--which_channel", "rg", "--norm", "instance"],
    "cgan": ["--model", "cgan", "--which_direction", "AtoB", "--dataset_mode", "single", "--fineSize", str(HW), "--which_model_netG",
             "unet_128", "--ngf", "8", "--which_channel", "rg_b", "--norm", "batch", "--no_dropout"],
}
TRAIN = {
    "segmentation": ["--which_model_netD", "None", "--weights", "1", "2"],
    "fcgan": ["--which_model_netD", "n_layers", "--n_layers_D", "3", "3", "3", "--ndf", "8", "--scale_factor", "1", "2", "4",
              "--lambda_D", "0.5", "0.4", "0.1", "--no_lsgan"],
    "cgan": ["--which_model_netD", "n_layers", "--n_layers_D", "3", "--ndf", "8", "--scale_factor", "1", "--lambda_D", "1.0",
             "--weights", "2", "4", "--no_lsgan"],
}
EMA = ["--ema_decay", "0.5", "--ema_warmup"]
KINDS = ["segmentation", "fcgan", "cgan"]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")


def build(kind, ckpt, extra=(), train=True):
    _need_gpu()
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TestOptions, TrainOptions
    argv = ["--name", "t", "--gpu_ids", "0", "--manualSeed", "5", "--checkpoints_dir", str(ckpt)] + ARCH[kind]
    torch.manual_seed(0)
    if train:      # a step large enough that three updates move the output well clear of rounding
        return create_model(TrainOptions().parse(argv + TRAIN[kind] + ["--lr", "0.002"] + list(extra), save=False, verbose=False))
    return create_model(TestOptions().parse(argv + list(extra), save=False, verbose=False))


def data(i):
    g = torch.Generator().manual_seed(100 + i)
    return {"A": (torch.rand(1, 3, HW, HW, generator=g) * 2 - 1).cuda(), "B": (torch.rand(1, 3, HW, HW, generator=g) * 2 - 1).cuda(),
            "A_paths": ["s"], "B_paths": ["s"]}


def flat(net):
    return net._flat.detach().cpu().numpy().copy()


def check_shadow(m, s0, snaps, t0, what):
    ref, t = ema_ref(s0, snaps, 0.5, True, t0=t0)
    bound = ema_bound(s0, snaps)
    dev = np.abs(flat(m.netG_ema).astype(np.float64) - ref)
    print(f"{what}: shadow against the reference over {len(snaps)} updates: largest deviation {dev.max():.3e}, bound {bound:.3e}")
    assert (dev <= bound).all()
    assert m.ema.count == t
    assert not np.array_equal(flat(m.netG_ema), snaps[-1])      # it is an average, not a copy of the last iterate


@pytest.mark.parametrize("kind", KINDS)
def test_eager_steps_follow_the_reference(tmp_path, kind):
    m = build(kind, tmp_path, EMA)
    assert m.netG_ema is not m.netG and type(m.netG_ema) is type(m.netG)
    assert all(not p.requires_grad for p in m.netG_ema.parameters())
    assert getattr(m.netG_ema, "_rng_seed", None) == getattr(m.netG, "_rng_seed", None)
    own = {id(p) for g in m.optimizer_G.param_groups for p in g["params"]}
    assert not any(id(p) in own for p in m.netG_ema.parameters())
    s0 = flat(m.netG_ema)
    assert np.array_equal(s0, flat(m.netG))      # loaded from netG
    snaps = []
    for i in range(3):
        m.set_input(data(i))
        m.optimize_parameters()
        snaps.append(flat(m.netG))
    check_shadow(m, s0, snaps, 0, kind + " eager")
    assert m.ema.count == m.optimizer_G.step_count == 3


@pytest.mark.parametrize("kind", KINDS)
def test_unset_option_changes_nothing(tmp_path, kind):
    m = build(kind, tmp_path)
    assert m.ema is None and not hasattr(m, "netG_ema")
    labels = [label for label, _ in m.checkpoint_nets()]
    assert labels == ["G"] + ["D_%d" % i for i in range(len(labels) - 1)]
    # the program as BaseModel.step_program built it before the option existed
    want = []
    for optimizer, backward, n in m.step_stages():
        for _ in range(n):
            want += [[optimizer.zero_grad, backward], ("sync", optimizer), [optimizer.step] + ([m.sample_noise] if n > 1 else [])]
    assert m.step_program() == want
    e = build(kind, tmp_path, EMA)
    prog = e.step_program()
    assert len(prog) == len(want) and sum(len(x) for x in prog if isinstance(x, list)) == sum(len(x) for x in want if isinstance(x, list)) + 1
    assert prog[-1] == [e.optimizer_G.step, e.ema.update]
    assert [label for label, _ in e.checkpoint_nets()] == ["G", "G_ema"] + labels[1:]


def _fresh_output(m, kind, inp, noise):
    """The output of a newly built generator loaded with the shadow's state_dict, on test()'s input."""
    from supervised_gan_amd import networks
    o = m.opt
    fresh = networks.define_G(o.input_nc, 0 if kind == "fcgan" else o.output_nc, o.ngf, o.which_model_netG, o.norm, not o.no_dropout,
                              n_layers_G=o.n_layers_G, use_fcn=o.noiseSize != 1, noise_nc=o.noise_nc, gpu_ids=o.gpu_ids)
    fresh.load_state_dict(m.netG_ema.state_dict())
    with torch.no_grad():
        if kind == "fcgan":
            return fresh.forward(noise), m.netG.forward(noise)
        if kind == "segmentation":
            ident = lambda x: x      # noqa: E731
            return fresh.forward(inp, noise, activation=ident), m.netG.forward(inp, noise, activation=ident)
        return fresh.forward(inp, noise), m.netG.forward(inp, noise)


def _snapshot_inside_the_program(m, n_update_G):
    """With several generator updates per step the live weights between them exist only inside the replayed graph: put one device copy
    of the live arena behind every ema.update of the step program (in front of the re-draw, which stays the program's last call, the
    slot GraphedStep's prefetch replaces), so that it is captured and replayed with the step.  Returns the buffers, in update order."""
    bufs = [torch.empty_like(m.netG._flat) for _ in range(n_update_G)]
    built = m.step_program

    def copy_into(buf):
        def snapshot():
            with torch.no_grad():
                torch.mul(m.netG._flat, 1.0, out=buf)      # a kernel, not a memcpy node; x * 1 keeps every bit
        return snapshot

    def program():
        prog, k = built(), 0
        for item in prog:
            if isinstance(item, list) and m.ema.update in item:
                item.insert(item.index(m.ema.update) + 1, copy_into(bufs[k]))
                k += 1
        assert k == n_update_G
        return prog
    m.step_program = program
    return bufs


def _graphed(tmp_path, kind, n_update_G, invalidate=True):
    """capture, an evaluation on the average (its derived weight copies now exist and are keyed), three replays with the live weights
    recorded after every generator update, the shadow against the reference over them, another evaluation.
    Returns the relative L2 distances of test()'s output to a fresh generator holding the shadow's weights and to netG's output."""
    from supervised_gan_amd.graph_step import GraphedStep
    m = build(kind, tmp_path, EMA + ["--ema_eval", "--n_update_G", str(n_update_G)])
    if not invalidate:      # the mutation the stale-copies check must catch: prepare_eval() without its invalidation
        m.ema._chains = lambda: []
    bufs = _snapshot_inside_the_program(m, n_update_G) if n_update_G > 1 else None
    gs = GraphedStep(m)
    gs.capture(data(0))
    torch.cuda.synchronize()
    if n_update_G > 1 and kind == "fcgan":
        assert gs._prefetch and m.step_program()[-1][-1] == m.sample_noise
    m.set_input(data(5))
    m.test()
    gs.reinstall()
    s0, t0 = flat(m.netG_ema), m.ema.count
    assert t0 == 2 * n_update_G      # the two warm-up steps of the capture
    snaps = []
    for i in range(1, 4):
        gs.step(data(i))
        torch.cuda.synchronize()
        if bufs is None:
            snaps.append(flat(m.netG))
        else:
            snaps += [b.cpu().numpy().copy() for b in bufs]
            assert np.array_equal(snaps[-1], flat(m.netG))      # the last recorded update is what the step left behind
            assert not np.array_equal(snaps[-1], snaps[-2])
    assert m.ema.count == m.optimizer_G.step_count == t0 + 3 * n_update_G      # every generator update made, the warm-up's included
    check_shadow(m, s0, snaps, t0, "%s graphed, n_update_G %d" % (kind, n_update_G))
    m.set_input(data(5))
    m.test()
    out = {"segmentation": "logit", "fcgan": "fake", "cgan": "fake_B"}[kind]
    y = getattr(m, out).detach().double().clone()
    y_fresh, y_live = (t.double() for t in _fresh_output(m, kind, getattr(m, "real_A", None), m.noise))
    return float((y - y_fresh).norm() / y_fresh.norm()), float((y - y_live).norm() / y_live.norm())


# two forwards of equal weights: test_checkpoint_round_trip of test_hip_segm_nod.py finds them equal; the figure is printed and the
# bound leaves room for nothing but the last bits of fp32 sums taken in another order
SAME_WEIGHTS = 1e-5


@pytest.mark.parametrize("kind,n_update_G", [("segmentation", 1), ("cgan", 1), ("fcgan", 1), ("fcgan", 2)])
def test_graphed_steps_and_evaluation_on_the_average(tmp_path, kind, n_update_G):
    d_fresh, d_live = _graphed(tmp_path, kind, n_update_G)
    print(f"{kind}: test() under --ema_eval against a fresh generator with the shadow's weights {d_fresh:.3e}, against netG {d_live:.3e}")
    assert d_fresh <= SAME_WEIGHTS
    assert d_live > 1000 * SAME_WEIGHTS


def test_evaluation_without_invalidation_reads_stale_copies(tmp_path):
    """The same run with prepare_eval()'s invalidation taken out: the replays moved the shadow's weights under derived copies the
    host believes current, and test() no longer gives the shadow's output -- what the unconditional invalidation is there for."""
    d_fresh, _ = _graphed(tmp_path, "segmentation", 1, invalidate=False)
    print(f"without invalidation: test() against a fresh generator with the shadow's weights {d_fresh:.3e}")
    assert d_fresh > 1000 * SAME_WEIGHTS


def test_validation_pass_prepares_the_average_once(tmp_path):
    """train_ss.validate under --ema_eval: every forward of the pass runs netG_ema, prepared once for the whole pass; without the flag
    the pass runs netG and prepares nothing."""
    import train_ss
    for flags, net in ((["--ema_eval"], "netG_ema"), ([], "netG")):
        m = build("segmentation", tmp_path, EMA + flags + ["--which_metric", "meanIU"])
        for i in range(2):
            m.set_input(data(i))
            m.optimize_parameters()
        calls, prepare = [], m.ema.prepare_eval
        m.ema.prepare_eval = lambda: (calls.append(1), prepare())[1]
        train_ss.validate(m, [data(5), data(6)])
        assert len(calls) == (1 if flags else 0)
        logit = m.logit.clone()
        with torch.no_grad():      # the last image of the pass through the network the pass should have run
            want = getattr(m, net).forward(m.real_A, None, activation=lambda x: x)
            other = getattr(m, "netG" if flags else "netG_ema").forward(m.real_A, None, activation=lambda x: x)
        assert torch.equal(logit, want) and not torch.equal(logit, other)


def _bits_equal(sd_a, sd_b):
    return list(sd_a) == list(sd_b) and all(torch.equal(sd_a[k].cpu(), sd_b[k].cpu()) for k in sd_a)


def test_checkpoints_use_ema_and_continue_train(tmp_path):
    m = build("cgan", tmp_path, EMA)
    for i in range(2):
        m.set_input(data(i))
        m.optimize_parameters()
    m.save("latest")
    d = tmp_path / "t"
    assert sorted(os.listdir(d)) == ["latest_net_D_0.pth", "latest_net_G.pth", "latest_net_G_ema.pth"]
    g, e = torch.load(d / "latest_net_G.pth"), torch.load(d / "latest_net_G_ema.pth")
    assert list(g) == list(e) and all(g[k].shape == e[k].shape and g[k].dtype == e[k].dtype for k in g)
    stats = [k for k in g if "running_" in k or "num_batches_tracked" in k]
    assert stats and all(torch.equal(g[k], e[k]) for k in stats)                  # --norm batch: the live statistics ride along
    assert any(float(g[k].float().abs().sum()) > 0 and "running_mean" in k for k in stats)
    assert any(not torch.equal(g[k], e[k]) for k in g if k.endswith("weight"))      # and the weights are the average
    assert _bits_equal(e, m.netG_ema.state_dict())
    # test side: --use_ema puts the average into netG
    t = build("cgan", tmp_path, ["--use_ema"], train=False)
    assert t.ema is None and not hasattr(t, "netG_ema") and _bits_equal(t.netG.state_dict(), e)
    plain = build("cgan", tmp_path, train=False)
    assert _bits_equal(plain.netG.state_dict(), g)
    # --continue_train with the file: loaded, and the warm-up is over
    c = build("cgan", tmp_path, EMA + ["--continue_train"])
    assert _bits_equal(c.netG_ema.state_dict(), e) and _bits_equal(c.netG.state_dict(), g) and c.ema.count == T_MAX
    c.set_input(data(3))
    c.optimize_parameters()
    assert c.ema.count == T_MAX
    # without the file: --use_ema names the path it misses, --continue_train starts the average from the loaded generator
    os.remove(d / "latest_net_G_ema.pth")
    with pytest.raises(FileNotFoundError, match="latest_net_G_ema.pth"):
        build("cgan", tmp_path, ["--use_ema"], train=False)
    r = build("cgan", tmp_path, EMA + ["--continue_train"])
    assert _bits_equal(r.netG_ema.state_dict(), g) and r.ema.count == 0
    # a run without the option loads as it always did
    n = build("cgan", tmp_path, ["--continue_train"])
    assert n.ema is None and _bits_equal(n.netG.state_dict(), g)


def test_test_model_loads_the_average_with_use_ema(tmp_path):
    """`--model test`: one generator, read from <which_epoch>_net_G_ema.pth under --use_ema and from <which_epoch>_net_G.pth without;
    a missing file is an error that names the path."""
    _need_gpu()
    from supervised_gan_amd import networks
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TestOptions
    torch.manual_seed(1)
    sds = {}
    os.makedirs(tmp_path / "t")
    for label in ("G", "G_ema"):      # two different generators of TestModel's shape (3 -> 3 channels)
        net = networks.define_G(3, 3, 8, "unet_128", "instance", False, gpu_ids=[0])
        sds[label] = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
        torch.save(sds[label], tmp_path / "t" / ("latest_net_%s.pth" % label))
    argv = ["--name", "t", "--gpu_ids", "0", "--checkpoints_dir", str(tmp_path), "--model", "test", "--dataset_mode", "single",
            "--which_model_netG", "unet_128", "--ngf", "8", "--norm", "instance", "--no_dropout"]
    plain = create_model(TestOptions().parse(argv, save=False, verbose=False))
    avg = create_model(TestOptions().parse(argv + ["--use_ema"], save=False, verbose=False))
    assert _bits_equal(plain.netG.state_dict(), sds["G"]) and _bits_equal(avg.netG.state_dict(), sds["G_ema"])
    assert not _bits_equal(sds["G"], sds["G_ema"])
    os.remove(tmp_path / "t" / "latest_net_G_ema.pth")
    with pytest.raises(FileNotFoundError, match="latest_net_G_ema.pth"):
        create_model(TestOptions().parse(argv + ["--use_ema"], save=False, verbose=False))


def test_multi_generator_trainers_refuse(tmp_path):
    _need_gpu()
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    argv = ["--name", "t", "--gpu_ids", "0", "--checkpoints_dir", str(tmp_path), "--model", "cgan_cycle", "--which_direction", "AtoB",
            "--dataset_mode", "single", "--fineSize", "256", "--which_channel", "rg_b", "--which_model_netG1", "unet_128", "--ngf1", "8",
            "--which_model_netG2", "unet_128", "--ngf2", "8", "--n_layers_D1", "3", "--ndf1", "8", "--scale_factor1", "1",
            "--lambda_D1", "1.0", "--no_dropout1", "--no_dropout2", "--no_lsgan1", "--ema_decay", "0.9"]
    with pytest.raises(NotImplementedError, match="ema_decay"):
        create_model(TrainOptions().parse(argv, save=False, verbose=False))

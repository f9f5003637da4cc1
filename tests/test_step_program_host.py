"""The training step of every trainer as a sequence of host calls, on CPU-built trainers whose forward / backward / optimizer
methods are recorders: what optimize_parameters() calls in which order (against traces written out from the reference's loops),
what ops.begin_step receives, that the program graph_step.GraphedStep captures is that same sequence, that the pool overrides
replace the ImagePool queries of the discriminator step, and the file names / learning rates save() and update_learning_rate()
leave behind."""
import os

import pytest
import torch

from test_graph_step import CGAN, CGAN_CYCLE, FACTD, FCGAN, TWOSTAGE


def graphed(m):
    """(program, pools, override setter) of the step as GraphedStep captures it; building the GraphedStep runs the capture checks."""
    from supervised_gan_amd.graph_step import GraphedStep
    GraphedStep(m)
    return m.step_program(), [pool for pool, _ in m.step_pools()], lambda views: setattr(m, "_pool_overrides", views)


SEGM = ["--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "128", "--which_model_netG", "unet_128",
        "--ngf", "8", "--which_channel", "b_rg", "--no_dropout", "--weights", "1", "3"]
SEGM_D = SEGM + ["--which_model_netD", "n_layers", "--ndf", "8", "--n_layers_D", "3", "--scale_factor", "1", "--lambda_D", "1.0"]
SEGM_CYCLE = ["--model", "segmentation_cycle", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "128",
              "--which_model_netG1", "unet_128", "--ngf1", "8", "--which_model_netG2", "unet_128", "--ngf2", "8", "--which_channel", "b_rg",
              "--no_dropout1", "--no_dropout2", "--which_model_netD2", "n_layers", "--n_layers_D2", "3", "--ndf2", "8", "--scale_factor2", "1",
              "--lambda_D2", "1.0", "--no_lsgan2"]
TWOSTAGE_PLAIN = [a for a in FACTD if a != "--no_lsgan2"]
TWOSTAGE_PLAIN[TWOSTAGE_PLAIN.index("twostage_factd")] = "twostage"
TWOSTAGE_ONE_PAIR = list(TWOSTAGE)
del TWOSTAGE_ONE_PAIR[TWOSTAGE_ONE_PAIR.index("--GAN_losses_D2") + 1]      # D2 sees the (fake_A, fake_B) pair only


def _set(argv, **kw):
    """argv with `--key value` replaced (or appended)."""
    argv = list(argv)
    for k, v in kw.items():
        if "--" + k in argv:
            argv[argv.index("--" + k) + 1] = str(v)
        else:
            argv += ["--" + k, str(v)]
    return argv


D, G = "D.zero_grad backward_D sync:D D.step", "G.zero_grad backward_G sync:G G.step"
D1, D2 = "D1.zero_grad backward_D1 sync:D1 D1.step", "D2.zero_grad backward_D2 sync:D2 D2.step"
# name -> (argv, the calls of one optimize_parameters() in order, "optimizer_D's zeroing goes to begin_step", GraphedStep takes it)
CASES = {
    "fcgan_d1_g2": (FCGAN, f"begin_step forward {D} {G} sample_noise {G} sample_noise", True, True),
    "fcgan_d2_g1": (_set(FCGAN, n_update_D=2, n_update_G=1), f"begin_step forward {D} sample_noise {D} sample_noise {G}", True, False),
    "cgan_g2": (CGAN, f"begin_step forward {D} {G} sample_noise {G} sample_noise", True, True),
    "segmentation_d": (SEGM_D, f"begin_step forward {D} {G}", True, True),
    "segmentation_nod_g2": (SEGM + ["--which_model_netD", "None", "--n_update_G", "2"], f"begin_step forward {G} sample_noise {G} sample_noise",
                            False, True),
    "cgan_cycle": (CGAN_CYCLE, f"begin_step forward {D1} {G}", False, True),
    "cgan_cycle_d2": (_set(CGAN_CYCLE, n_update_D1=2), f"begin_step forward {D1} sample_noise {D1} sample_noise {G}", False, False),
    "segmentation_cycle": (SEGM_CYCLE, f"begin_step forward {D2} {G}", False, True),
    "twostage_cycle": (TWOSTAGE, f"begin_step forward {D1} {D2} {G}", False, True),
    "twostage_cycle_212": (_set(TWOSTAGE, n_update_D1=2, n_update_G=2),
                           f"begin_step forward {D1} sample_noise {D1} sample_noise {D2} {G} sample_noise {G} sample_noise", False, False),
    "twostage_ignores_n_update": (_set(TWOSTAGE_PLAIN, n_update_D1=2, n_update_D2=2, n_update_G=2), f"begin_step forward {D1} {D2} {G}", False, True),
    "twostage_factd": (FACTD, f"begin_step forward {D1} {D2} {G}", False, True),
}


def _build(argv, tmp, extra=()):
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    return create_model(TrainOptions().parse(["--name", "t", "--norm", "instance", "--gpu_ids", "-1", "--checkpoints_dir", str(tmp), *argv, *extra],
                                             save=False, verbose=False))


def _optimizers(m):
    return {k[len("optimizer_"):]: v for k, v in vars(m).items() if k.startswith("optimizer_")}


def _record(m, monkeypatch, sync):
    """Every call of the step appends its label to the returned log and does nothing else."""
    from supervised_gan_amd import ops
    log, begun = [], []
    rec = lambda label: lambda *a, **k: log.append(label)      # noqa: E731
    for name in ["forward", "sample_noise"] + [n for n in dir(m) if n.startswith("backward_")]:
        setattr(m, name, rec(name))
    for tag, o in _optimizers(m).items():
        o.zero_grad, o.step, o.zeroing = rec(tag + ".zero_grad"), rec(tag + ".step"), ["zeroing of " + tag]
        o.take_zeroing = lambda o=o: o.zeroing
        o.tag = tag
    monkeypatch.setattr(ops, "begin_step", lambda also_zero=(): (log.append("begin_step"), begun.append(also_zero)))
    m.grad_sync = (lambda o: log.append("sync:" + o.tag)) if sync else None
    return log, begun


def _flatten(m, program, log):
    """Runs a captured program's calls in order; a sync item counts where the eager step would call grad_sync."""
    for item in program:
        if isinstance(item, list):
            for f in item:
                f()
        elif m.grad_sync is not None:
            assert item[0] == "sync"
            log.append("sync:" + item[1].tag)


@pytest.mark.parametrize("sync", [False, True], ids=["alone", "grad_sync"])
@pytest.mark.parametrize("case", list(CASES))
def test_eager_step_and_captured_program(case, sync, tmp_path, monkeypatch):
    argv, calls, folds_d, graphable = CASES[case]
    m = _build(argv, tmp_path)
    log, begun = _record(m, monkeypatch, sync)
    m.optimize_parameters()
    want = [c for c in calls.split() if sync or not c.startswith("sync:")]
    assert log == want
    assert len(begun) == 1
    if folds_d:
        assert begun[0] is m.optimizer_D.zeroing
    else:
        assert len(begun[0]) == 0
    if not graphable:
        with pytest.raises(AssertionError):
            graphed(m)
        return
    from supervised_gan_amd.graph_step import GraphedStep
    program, pools, _ = graphed(m)
    del log[:]
    _flatten(m, program, log)
    assert log == want[2:]
    GraphedStep(m)._begin()
    assert len(begun) == 2 and (begun[1] is begun[0] if folds_d else len(begun[1]) == 0)


def test_fixed_noise_is_not_graphable(tmp_path):
    with pytest.raises(AssertionError):
        graphed(_build(TWOSTAGE, tmp_path, ["--use_fixed_noise1", "--noise_pool_size", "2"]))


# ---- pools -------------------------------------------------------------------------------------------------------------------------
# name -> (argv, the pools in query order, the discriminator backward passes, the method of the trainer every loss goes through)
POOLS = {
    "fcgan": (FCGAN, ["fake_pool"], ["backward_D"], "_d_losses"),
    "cgan": (CGAN, ["fake_pool"], ["backward_D"], "_d_losses"),
    "segmentation_d": (SEGM_D, ["fake_pool"], ["backward_D"], "_d_losses"),
    "segmentation_nod": (SEGM + ["--which_model_netD", "None"], [], [], None),
    "cgan_cycle": (CGAN_CYCLE, ["fake_pool1"], ["backward_D1"], "_gan"),
    "segmentation_cycle": (SEGM_CYCLE, ["fake_pool2"], ["backward_D2"], "_gan"),
    "twostage_cycle": (TWOSTAGE, ["fake_pool1", "fake_pool2", "fake_pool2"], ["backward_D1", "backward_D2"], "_gan"),
    "twostage_cycle_one_pair": (TWOSTAGE_ONE_PAIR, ["fake_pool1", "fake_pool2"], ["backward_D1", "backward_D2"], "_gan"),
    "twostage_multi_class": (TWOSTAGE + ["--use_multi_class_GAN", "--no_lsgan2"], ["fake_pool1", "fake_pool2_1", "fake_pool2_2"], ["backward_D1"], "_gan"),
    "twostage_factd": (FACTD, ["fake_pool1", "fake_pool2", "fake_pool2"], ["backward_D1", "backward_D2"], "_gan _factd_loss"),
}


@pytest.mark.parametrize("case", list(POOLS))
def test_pools_and_overrides(case, tmp_path, monkeypatch):
    """The pools are the trainer's, in the reference's query order; once overrides are set the discriminator step reads them -- in
    that order -- and asks no pool."""
    argv, pool_names, backwards, loss_methods = POOLS[case]
    m = _build(argv, tmp_path)
    program, pools, set_overrides = graphed(m)
    assert len(pools) == len(pool_names) and all(p is getattr(m, n) for p, n in zip(pools, pool_names))
    if not pools:
        return
    img = lambda v: torch.full((1, 2, 8, 8), float(v))      # noqa: E731
    for i, name in enumerate(("real", "real_A", "real_B", "fake", "fake_A", "fake_B", "fake_B_from_real_A", "fake_B_from_fake_A")):
        setattr(m, name, img(i))
    m.transform = m.transform_inverse = lambda x: x
    queried, seen = [], []
    for p in set(pools):
        monkeypatch.setattr(p, "query", lambda x, p=p: (queried.append(p), x)[1])

    def loss(*a):      # (jobs, weights) or (criterion, jobs, weights): [(net or index, [label,] input, target)]
        jobs = a[-2]
        seen.extend(float(j[-2].flatten()[0]) for j in jobs)
        return torch.zeros(()), torch.zeros(len(jobs))
    for name in loss_methods.split():
        monkeypatch.setattr(m, name, loss)
    monkeypatch.setattr(m, "_backward", lambda l: None)
    monkeypatch.setattr(m, "_join_streams", lambda: None, raising=False)      # fcgan: waits on its side streams
    for b in backwards:
        getattr(m, b)()
    assert queried == pools[:len(queried)] and len(queried) == (1 if "multi_class" in case else len(pools))
    del queried[:], seen[:]
    set_overrides([img(100 + i) for i in range(len(pools))])
    for b in backwards:
        getattr(m, b)()
    assert queried == []
    fed = [v for v in dict.fromkeys(seen) if v >= 100]
    assert fed == [100.0 + i for i in range(len(fed))] and len(fed) == (1 if "multi_class" in case else len(pools))


# ---- save / update_learning_rate ------------------------------------------------------------------------------------------------------
FILES = {
    "fcgan_d1_g2": ["D_0", "D_1", "D_2", "G"], "cgan_g2": ["D_0", "D_1", "G"], "segmentation_d": ["D_0", "G"], "segmentation_nod_g2": ["G"],
    "cgan_cycle": ["D1_0", "D1_1", "G1", "G2"], "segmentation_cycle": ["D2_0", "G1", "G2"],
    "twostage_cycle": ["D1_0", "D1_1", "D2_0", "D2_1", "F2", "G1", "G2"], "twostage_ignores_n_update": ["D1_0", "D1_1", "D2_0", "D2_1", "G1", "G2"],
    "twostage_factd": ["D1_0", "D1_1", "D2_0", "D2_1", "G1", "G2"],
}


@pytest.mark.parametrize("case", list(FILES))
def test_save_writes_the_reference_file_names(case, tmp_path):
    m = _build(CASES[case][0], tmp_path)
    m.save("t")
    assert sorted(os.listdir(tmp_path / "t")) == ["t_net_%s.pth" % label for label in FILES[case]]
    # what was written is what --continue_train reads
    m2 = _build(CASES[case][0], tmp_path, ["--continue_train", "--which_epoch", "t"])
    for name in ("netG", "netG1", "netG2", "netF2"):
        if getattr(m, name, None) is not None:
            for (k, a), (_, b) in zip(getattr(m, name).state_dict().items(), getattr(m2, name).state_dict().items()):
                assert torch.equal(a, b), (name, k)
    for name in ("netD", "netD1", "netD2"):
        for da, db in zip(getattr(m, name, []), getattr(m2, name, [])):
            for (k, a), (_, b) in zip(da.state_dict().items(), db.state_dict().items()):
                assert torch.equal(a, b), (name, k)


def _lr_step(m, capsys):
    """One update_learning_rate(): ({optimizer: [(group name, lr)]}, the old_lr* before it, the printed line)."""
    synced = []
    for tag, o in _optimizers(m).items():
        o.sync_lr = lambda tag=tag: synced.append(tag)
    before = {k: getattr(m, k) for k in ("old_lr", "old_lr1", "old_lr2") if hasattr(m, k)}
    capsys.readouterr()
    m.update_learning_rate()
    assert sorted(synced) == sorted(_optimizers(m))
    rates = {tag: [(g.get("name"), g["lr"]) for g in o.param_groups] for tag, o in _optimizers(m).items()}
    return rates, before, capsys.readouterr().out


@pytest.mark.parametrize("case", ["fcgan_d1_g2", "cgan_g2", "segmentation_d", "segmentation_nod_g2"])
def test_single_rate_schedule(case, tmp_path, capsys):
    """lr = old_lr - opt.lr / niter_decay on every group, NOT clamped: the second call below goes negative, as in the reference."""
    m = _build(CASES[case][0], tmp_path, ["--lr", "0.0003", "--niter_decay", "2"])
    for old, new in ((0.0003, 0.00015), (0.00015, 0.0), (0.0, -0.00015)):
        rates, before, out = _lr_step(m, capsys)
        assert out == "update learning rate: %f -> %f\n" % (before["old_lr"], m.old_lr)
        assert abs(before["old_lr"] - old) < 1e-12 and abs(m.old_lr - new) < 1e-12
        assert sorted(rates) == (["D", "G"] if "nod" not in case else ["G"])
        assert all(lr == m.old_lr for groups in rates.values() for _, lr in groups)
    assert m.old_lr < 0


@pytest.mark.parametrize("case", ["cgan_cycle", "segmentation_cycle", "twostage_cycle", "twostage_ignores_n_update", "twostage_factd"])
def test_three_rate_schedule(case, tmp_path, capsys):
    """lr / lr1 / lr2 each fall by their own base / niter_decay and stop at 0; G1 (and D1) follow lr1, G2, F2 (and D2) follow lr2."""
    m = _build(CASES[case][0], tmp_path, ["--lr", "0.0003", "--lr1", "0.0004", "--lr2", "0.0001", "--niter_decay", "2"])
    m.old_lr2 = 0.00002      # the clamp bites on the first call for lr2 and on the third for the others
    follows = {"G1": "old_lr1", "G2": "old_lr2", "F2": "old_lr2", "D1": "old_lr1", "D2": "old_lr2"}
    for lr, lr1, lr2 in ((0.00015, 0.0002, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)):
        rates, before, out = _lr_step(m, capsys)
        assert out == "update learning rate: %f -> %f, %f -> %f\n" % (before["old_lr1"], m.old_lr1, before["old_lr2"], m.old_lr2)
        for got, want in ((m.old_lr, lr), (m.old_lr1, lr1), (m.old_lr2, lr2)):
            assert abs(got - want) < 1e-12 and got >= 0
        assert [n for n, _ in rates["G"]] == ["G1", "G2"] + (["F2"] if case == "twostage_cycle" else [])
        for tag, groups in rates.items():
            for name, rate in groups:
                assert rate == getattr(m, follows[name or tag]), (tag, name)


# ---- GraphedStep.step(replay=False): the captured calls, launch by launch ------------------------------------------------------------
class _FakeGraph:
    """torch.cuda.CUDAGraph for a host without a GPU: what ran while it was 'captured' is its content, replay() logs its number."""
    made = []

    def __init__(self):
        self.captured, self.no = None, len(_FakeGraph.made)
        _FakeGraph.made.append(self)

    def pool(self):
        return None

    def replay(self):
        self.log.append("replay:%d" % self.no)


class _FakeStream:
    def __init__(self, *a, **k):
        pass

    def wait_stream(self, other):
        pass


def _fake_cuda(monkeypatch, log):
    import contextlib

    @contextlib.contextmanager
    def graph(g, **kw):
        start = len(log)
        yield
        g.captured, g.log = log[start:], log
        del log[start:]

    _FakeGraph.made = []
    monkeypatch.setattr(torch.cuda, "CUDAGraph", _FakeGraph)
    monkeypatch.setattr(torch.cuda, "graph", graph)
    monkeypatch.setattr(torch.cuda, "Stream", _FakeStream)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: _FakeStream())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)


LAUNCHES = {"fcgan": (FCGAN, False), "fcgan_prefetch": (FCGAN, True), "twostage_cycle": (TWOSTAGE, False), "cgan_g2": (CGAN, False)}


@pytest.mark.parametrize("sync", [False, True], ids=["alone", "grad_sync"])
@pytest.mark.parametrize("case", list(LAUNCHES))
def test_launch_by_launch_step_calls_what_was_captured(case, sync, tmp_path, monkeypatch):
    """step(replay=False) makes, in order, exactly the calls each graph was captured from, with the pool copies and the gradient
    exchanges where step() has them; the step(replay=True) after it first re-installs the captured step's tensors."""
    from supervised_gan_amd import ops
    from supervised_gan_amd.graph_step import GraphedStep
    argv, prefetch = LAUNCHES[case]
    m = _build(argv, tmp_path)
    log, begun = _record(m, monkeypatch, sync)
    _fake_cuda(monkeypatch, log)
    rec = lambda label: lambda *a, **k: log.append(label)      # noqa: E731
    m.set_input = lambda data: None
    m.sample_noise_and_prefetch, m.adopt_prefetched = rec("sample_noise_and_prefetch"), rec("adopt_prefetched")
    img = torch.zeros(1, 2, 8, 8)
    for name in ("real_A", "real_B", "fake", "fake_A", "fake_B", "fake_B_from_real_A", "fake_B_from_fake_A"):
        setattr(m, name, img)
    m._fake_next = m._noise_alt = img
    m.transform = m.transform_inverse = lambda x: x
    monkeypatch.setattr(ops, "as_nhwc", lambda x: x.permute(0, 2, 3, 1)[0])
    monkeypatch.setattr(ops, "slice_nhwc", lambda q, c0, n, out=None: log.append("pool_copy"))
    gs = GraphedStep(m)
    gs._prefetch = prefetch
    gs.capture(None)
    graphs = list(_FakeGraph.made)
    updates = sum(n for _, _, n in m.step_stages())
    assert all(g.captured for g in graphs) and len(graphs) == (0 if prefetch else 1) + (updates + 1 if sync else 1)
    want = ["adopt_prefetched"] if prefetch else list(graphs[0].captured)
    want += ["pool_copy"] * len(gs.pools)
    assert [obj for kind, obj in gs.segs if kind == "graph"] == graphs[0 if prefetch else 1:]
    for kind, obj in gs.segs:      # the captured pieces with the gradient exchanges between them, as step() walks them
        want += obj.captured if kind == "graph" else ["sync:" + obj.tag]
    assert len([c for c in want if c.startswith("sync:")]) == (updates if sync else 0)
    assert want[:2] == (["adopt_prefetched", "pool_copy"] if prefetch else ["begin_step", "forward"])
    assert ("sample_noise_and_prefetch" in want) == prefetch and "begin_step" in want
    del log[:]
    m.marker = torch.zeros(1)      # an attribute the launches rebind: the next replay must see the captured step's again
    gs._step_tensors["marker"] = m.marker
    gs.step(None, replay=False)
    assert log == want
    m.marker = torch.ones(1)
    del log[:]
    gs.step(None)
    replays = ["replay:%d" % g.no for g in graphs]
    assert [c for c in log if c.startswith("replay:")] == replays and not [c for c in log if c in want and c not in ("adopt_prefetched", "pool_copy")
                                                                               and not c.startswith("sync:")]
    assert m.marker is gs._step_tensors["marker"]

"""One hipGraph replay of the training step against the launches it was captured from, both from ONE device state.

tests/test_graph_step.py compares trajectories that diverged during warm-up and has to accept 2e-2 / 15 %.  Here the state after
capture is snapshotted (tests/graph_state.py), one step is replayed, the snapshot is written back in place and the same step runs
launch by launch (GraphedStep.step(replay=False)): the two differ by the order of the floating-point atomics alone.

The program both sides run carries probes (copies inside the program, captured like any other call): the gradients every optimizer
step is about to consume, and the BatchNorm statistics as the step's opening forward left them.  What is compared, R_g (replay)
against R_e (launches):

  exact   counters, learning rates, Philox offsets, the latents, num_batches_tracked, pool and `random` state: bit for bit;
  first   what the step computes before its first optimizer update (the first gradient probe, that optimizer's moments,
          fake_for_D, the statistics probe): max-abs over max-abs of R_e;
  grads   later gradient probes, the gradient arenas at the end of the step, the other moments;
  later   every other float (running statistics, the kept forward, losses one by one, the output);
  update  || (R_g - S) - (R_e - S) || / || R_e - S || of every optimizer segment, over the elements whose gradient is at least
          MASK of the segment's largest in every probe of R_e.  An element below that (a bias ahead of a normalisation: its gradient
          is rounding noise alone) gets a full +-lr from Adam in a direction the atomics decide; the mask is made from R_e only.

Each bound is 8 x the largest value its class showed between two runs of the LAUNCHES from the snapshot (R_e, R_e2), over every
configuration and three runs of this file on an MI355X; a replay is never part of what sets them."""
import gc
import os
import random
import sys
from collections import OrderedDict

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from graph_state import DERIVED, compare, restore, snapshot, state_tensors, update_rel      # noqa: E402
from test_graph_step import CGAN, FCGAN, SEGM, TWOSTAGE, _build, _ring      # noqa: E402

# name -> (argv, image size, the trainer's output, SGAN_NO_G_PREFETCH)
CONFIGS = {
    "fcgan_prefetch": (FCGAN, 128, "fake", "0"),
    "fcgan_no_prefetch": (FCGAN, 128, "fake", "1"),
    "fcgan_ema": (FCGAN + ["--ema_decay", "0.999"], 128, "fake", "0"),
    "cgan": (CGAN, 256, "fake_B", "0"),
    "twostage_cycle": (TWOSTAGE, 256, "fake_B_from_fake_A", "0"),
    "segmentation": (SEGM, 128, "fake_B", "0"),
}

MASK = 1e-3      # update metric: elements whose gradient is >= MASK x the segment's largest, in every probe of the reference
# 8 x the largest launches-vs-launches value of the class (DESIGN.md R6.4 has the figures).  Only `first` has a bound: the launches
# against themselves showed 1.1e-2 (grads: fcgan second generator update, one run; 4e-6 otherwise), 1.1e-3 (later: fcgan output, that run;
# 4.4e-4 on its statistics always) and 9.7e-3 (update, that run; 7e-6 otherwise), and 8 x any of these is above the 1e-3 beyond which a bound no longer separates a
# fault from the reference's own spread.  Those classes are printed with every comparison and not asserted.
BOUNDS = {"first": 8 * 3.361e-6}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")


def _stage_label(m, opt):
    return next(k for k, v in vars(m).items() if v is opt)


def _stage_segs(opt):
    """(param arena, grad arena, offset, n) behind opt.segments(), in its order."""
    return [s for f in (getattr(opt, "optimizers", None) or [opt]) for s in f._segs]


def _install_probes(m):
    """Every program the trainer builds from now on copies, right after each backward, the gradients the optimizer is about to
    consume, and at its start the BatchNorm statistics the opening forward left.  m._probes: name -> buffer, filled by the step."""
    built, probes = m.step_program, OrderedDict()
    stats = [("probe.stats.%s.%s" % (label, k), b) for label, net in m.checkpoint_nets() for k, b in net.named_buffers()
             if k.endswith(("running_mean", "running_var"))]

    def copy_stats():
        for name, b in stats:
            if name not in probes:
                probes[name] = torch.empty_like(b)
            probes[name].copy_(b)

    def copy_grads(k, opt):
        label = _stage_label(m, opt)

        def run():
            for j, (_, g) in enumerate(opt.segments()):
                name = "probe.%d.%s.%d" % (k, label, j)
                if name not in probes:
                    probes[name] = torch.empty_like(g)
                probes[name].copy_(g)
        return run

    def program():
        prog, k = built(), 0
        for item in prog:
            if isinstance(item, list):
                for opt, backward, _ in m.step_stages():
                    if backward in item:
                        item.insert(item.index(backward) + 1, copy_grads(k, opt))
                        k += 1
        if stats:
            prog[0].insert(0, copy_stats)
        return prog
    m.step_program, m._probes = program, probes


def _record(gs, out):
    torch.cuda.synchronize()
    m = gs.m
    return {"snap": snapshot(gs), "errors": [float(v) for v in m.get_current_errors().values()], "out": getattr(m, out).detach().clone(),
            "probes": OrderedDict((k, t.clone()) for k, t in m._probes.items())}


def _captured(argv, hw, no_prefetch, prepare=None):
    """(GraphedStep after capture on ring[0], the ring)."""
    from supervised_gan_amd.graph_step import GraphedStep
    ring = _ring(hw)
    random.seed(11)
    m = _build(argv)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SGAN_NO_G_PREFETCH", no_prefetch)      # read in GraphedStep.__init__
        gs = GraphedStep(m)
    assert gs._prefetch == (argv[1] == "fcgan" and no_prefetch == "0")
    _install_probes(m)
    if prepare is not None:
        prepare(m)
    gs.capture(ring[0])
    torch.cuda.synchronize()
    return gs, ring


def _runs(name):
    """The steps of one configuration, each from the snapshot S taken after capture: replay (g), launches (e), launches again (e2:
    the reference against itself), replay after the launch-by-launch interlude (g2)."""
    argv, hw, out, no_prefetch = CONFIGS[name]
    gs, ring = _captured(argv, hw, no_prefetch)
    S = snapshot(gs)
    r = {"gs": gs, "ring": ring, "out": out, "S": S}
    for key, replay in (("g", True), ("e", False), ("e2", False), ("g2", True)):
        if key != "g":
            restore(gs, S)
        gs.step(ring[1], replay=replay)
        r[key] = _record(gs, out)
    return r


@pytest.fixture(autouse=True)
def _graphs_die_between_tests():
    """A GraphedStep is cyclic garbage once its test (or fixture) lets go of it, and the collector may then destroy its hipGraphs in
    the middle of a later capture, which the runtime answers with an abort: collect after every test, when nothing captures."""
    yield
    gc.collect()
    torch.cuda.synchronize()


@pytest.fixture(scope="module", params=list(CONFIGS))
def runs(request):
    _need_gpu()
    yield _runs(request.param)
    gc.collect()
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def fcgan():
    """One prefetching fcgan for the tests that disturb it; every one of them starts from restore(S), and the fixture hands it out
    restored, with the captured step's tensors installed and the learning rates as captured."""
    _need_gpu()
    r = _runs("fcgan_prefetch")
    r["lr"] = r["gs"].m.optimizer_D.param_groups[0]["lr"]
    yield r
    del r
    gc.collect()
    torch.cuda.synchronize()


@pytest.fixture
def fresh(fcgan):
    gs, m = fcgan["gs"], fcgan["gs"].m

    def reset():
        for o in (m.optimizer_D, m.optimizer_G):
            o.param_groups[0]["lr"] = fcgan["lr"]
            o.sync_lr()
        restore(gs, fcgan["S"])
    reset()
    yield fcgan
    reset()


def _first_names(gs, rec):
    """The float names of the class `first`: computed before the step's first optimizer update."""
    m = gs.m
    opt = m.step_stages()[0][0]
    label = _stage_label(m, opt)
    members = getattr(opt, "optimizers", None) or [opt]
    moments = [k for k in rec["snap"]["tensors"] if any(k.startswith(p) for p in (label + ".m.", label + ".v."))
               or any(k.startswith("%s.%d." % (label, i)) and (".m." in k or ".v." in k) for i in range(len(members)))]
    first = [k for k in rec["probes"] if k.startswith("probe.0.") or (k.startswith("probe.stats.") and not gs._prefetch)]
    return set(moments + first + [k for k in rec["snap"]["tensors"] if k.startswith("fake_for_D.")])


def _masked_updates(gs, rec, ref, S):
    """{stage.segment: update metric over the elements the mask keeps}, and the smallest number of elements a mask kept."""
    m, live = gs.m, state_tensors(gs)
    by_ptr = {t.data_ptr(): k for k, t in live.items() if k.endswith(".params")}
    out, kept = {}, float("inf")
    for opt, _, _ in m.step_stages():
        label = _stage_label(m, opt)
        for j, (ap, _, off, n) in enumerate(_stage_segs(opt)):
            name = by_ptr[ap.data_ptr()]
            keep = torch.ones(n, dtype=torch.bool, device=ap.device)
            probes = [t for k, t in ref["probes"].items() if k.startswith("probe.") and k.endswith(".%s.%d" % (label, j))]
            assert probes
            for g in probes:
                keep &= g.abs() >= MASK * g.abs().max()
            kept = min(kept, int(keep.sum()))
            a, b, s = (x["snap"]["tensors"][name][off: off + n] if "snap" in x else x["tensors"][name][off: off + n] for x in (rec, ref, S))
            out["%s.%d" % (label, j)] = update_rel(a, b, s, keep)
    return out, kept


def _classes(gs, rec, ref, S):
    """(exact mismatches, {class: (largest value, its name)}, raw update metrics of the whole arenas)."""
    bad, floats, raw = compare(rec, ref, S)
    first = _first_names(gs, ref)
    assert first <= set(floats), sorted(first - set(floats))
    upd, kept = _masked_updates(gs, rec, ref, S)
    assert kept >= 64, "every segment keeps enough elements to carry a norm"
    worst = {}
    grads = {k for k in floats if k not in first and (k.startswith("probe.") and not k.startswith("probe.stats.") or k.endswith(".grads")
                                                      or ".extra_grad." in k or ".m." in k or ".v." in k)}
    for cls, d in (("first", {k: v for k, v in floats.items() if k in first}), ("grads", {k: v for k, v in floats.items() if k in grads}),
                   ("later", {k: v for k, v in floats.items() if k not in first and k not in grads}), ("update", upd)):
        k = max(d, key=d.get)
        worst[cls] = (d[k], k)
    return bad, worst, raw


def _assert_same_step(gs, rec, ref, S, what):
    bad, worst, raw = _classes(gs, rec, ref, S)
    print(f"{what}: exact mismatches {bad}; " + "; ".join(f"{c} {v:.3e} ({k})" for c, (v, k) in worst.items())
          + f"; unmasked update {max(raw.values()):.3e}")
    assert not bad, (what, bad)
    for cls, bound in BOUNDS.items():
        assert worst[cls][0] <= bound, (what, cls, worst[cls])


def test_replay_equals_its_launches_from_one_snapshot(runs, request):
    r, name = runs, request.node.callspec.id
    gs = r["gs"]
    _, worst, raw = _classes(gs, r["e2"], r["e"], r["S"])
    print(f"SPREAD {name}: " + "; ".join(f"{c} {v:.3e} ({k})" for c, (v, k) in worst.items()) + f"; unmasked update {max(raw.values()):.3e}")
    moved = [k for k, v in r["e"]["snap"]["tensors"].items() if k.endswith(".params") and not torch.equal(v, r["S"]["tensors"][k])]
    assert len(moved) == len([k for k in r["S"]["tensors"] if k.endswith(".params")]), "a step updates every network"
    _assert_same_step(gs, r["g"], r["e"], r["S"], f"{name}: replay vs launches")
    _assert_same_step(gs, r["g2"], r["e"], r["S"], f"{name}: replay after the launches vs launches")


def test_derived_copies_are_the_repack_of_the_replayed_parameters(runs):
    """Bit for bit, as tests/test_hip_adam_pack.py holds for the kernel: the transposed copy and the three 16-bit packs a replay leaves
    are what sgan_pack_weights makes of the parameters it leaves.  (The EMA shadow's copies are stale by design,
    WeightEMA.prepare_eval.)"""
    from supervised_gan_amd import ops
    r = runs
    m, t = r["gs"].m, r["g"]["snap"]["tensors"]
    checked = 0
    for label, net in m.checkpoint_nets():
        if net is getattr(m, "netG_ema", None) or "net.%s.derived._flat_t" % label not in t:
            continue
        params = t["net.%s.params" % label]
        mates = getattr(net, "_arena_mates", None) or [net]
        segs = [s for n in mates for s in n._conv_segments(n._arena[2])]
        fresh = [torch.zeros_like(params) for _ in range(4)]
        ops.pack_weights(params, fresh[0], fresh[1], fresh[2], segs, fresh[3])
        torch.cuda.synchronize()
        for dname, f in zip(DERIVED, fresh):
            got = t["net.%s.derived.%s" % (label, dname)]
            for o, taps, co, ci in segs:
                n = taps * co * ci
                assert torch.equal(got[o: o + n].view(torch.int32), f[o: o + n].view(torch.int32)), (label, dname, o)
                checked += 1
    assert checked > 0


# ---- sensitivity: one fault on the captured side each, fcgan 128^2; the bounds must tell them apart ----------------------------------
def test_bounds_see_a_gradient_buffer_the_captured_program_never_zeroes(monkeypatch):
    """Captured with optimizer_D.zero_grad dropped from the program and take_zeroing() reporting the buffers as handed over without
    handing them over: in fcgan the step's first launch clears the discriminators' gradients (step_zeroing -> take_zeroing) and
    zero_grad is a no-op behind it, so the drop alone changes nothing (1.4e-6 measured), while a slip in that bookkeeping leaves the
    buffers accumulating.  The launch side runs the very calls that were captured, with the trainer's own take_zeroing."""
    _need_gpu()
    argv, hw, out, no_prefetch = CONFIGS["fcgan_prefetch"]

    def seed_fault(m):
        program, o = m.step_program, m.optimizer_D

        def without_zero_grad():
            prog = program()
            for item in prog:
                if isinstance(item, list) and o.zero_grad in item:
                    item.remove(o.zero_grad)
            return prog

        def take_nothing():
            o._grads_clean = True
            return []
        monkeypatch.setattr(m, "step_program", without_zero_grad)
        monkeypatch.setattr(o, "take_zeroing", take_nothing)
    gs, ring = _captured(argv, hw, no_prefetch, prepare=seed_fault)
    monkeypatch.undo()
    m = gs.m
    assert not any(m.optimizer_D.zero_grad in fns for fns in gs.seg_fns if fns)
    m.optimizer_D._grads_clean = False      # as every sound step leaves it
    S = snapshot(gs)
    gs.step(ring[1])
    faulty = _record(gs, out)
    restore(gs, S)
    gs.step(ring[1], replay=False)
    ref = _record(gs, out)
    _, floats, _ = compare(faulty, ref, S)
    print(f"un-zeroed D gradients: {floats['probe.0.optimizer_D.0']:.3e}")
    assert floats["probe.0.optimizer_D.0"] > max(BOUNDS["first"], 1e-2)


def test_bounds_see_a_learning_rate_that_did_not_reach_the_replay(fresh):
    r = fresh
    gs, m, S = r["gs"], r["gs"].m, r["S"]
    for o in (m.optimizer_D, m.optimizer_G):
        o.param_groups[0]["lr"] = r["lr"] / 2
        o.sync_lr()
    gs.step(r["ring"][1], replay=False)
    halved = _record(gs, r["out"])
    bad, _, _ = compare(r["g"], halved, S)
    upd, _ = _masked_updates(gs, r["g"], halved, S)
    print(f"half the learning rate: exact mismatches {bad}; update {upd}")
    assert "optimizer_D.lr_dev" in bad and "optimizer_G.lr_dev" in bad
    assert min(upd.values()) > 0.5      # the update halves: the metric is 1; launches against themselves stay under 1e-2


def test_bounds_see_a_perturbed_running_mean():
    """Without prefetch, where the step opens with a forward: the statistics probe shows what that forward made of the buffer."""
    _need_gpu()
    r = _runs("fcgan_no_prefetch")
    gs, S = r["gs"], r["S"]
    restore(gs, S)
    name = next(k for k in S["tensors"] if k.startswith("net.G.buffer.") and k.endswith("running_mean"))
    live = dict(gs.m.netG.named_buffers())[name[len("net.G.buffer."):]]
    assert float(live.abs().max()) > 0
    live.mul_(1.01)
    gs.step(r["ring"][1])
    off = _record(gs, r["out"])
    _, floats, _ = compare(off, r["e"], S)
    probe = "probe.stats.G." + name[len("net.G.buffer."):]
    print(f"running_mean off by 1 %: {floats[probe]:.3e} after the opening forward, {floats[name]:.3e} at the end of the step")
    assert floats[probe] > max(BOUNDS["first"], 5e-3)      # 0.9 x 1 % survives the momentum update


# ---- prefetch: one generator forward ahead, exactly ---------------------------------------------------------------------------------------
def _bn_counts(net):
    return {k: int(b) for k, b in net.named_buffers() if k.endswith("num_batches_tracked")}


def test_prefetching_step_is_one_generator_forward_ahead():
    """What a checkpoint saved from a prefetching GraphedStep holds: integer identities, no tolerance."""
    _need_gpu()
    K = 2
    gs, ring = _captured(FCGAN, 128, "0")
    for i in range(1, 1 + K):
        gs.step(ring[i])
    torch.cuda.synchronize()
    random.seed(11)
    e = _build(FCGAN)
    for i in [0, 0] + list(range(1, 1 + K)):      # capture() warms up with two steps on its example input
        e.set_input(ring[i])
        e.optimize_parameters()
    torch.cuda.synchronize()
    g_counts, g_off = _bn_counts(gs.m.netG), int(gs.m._rng_offset)
    e_counts, e_off = _bn_counts(e.netG), int(e._rng_offset)
    assert len(g_counts) >= 2 and g_counts == {k: v + 1 for k, v in e_counts.items()}
    e.set_input(ring[1 + K])
    e.forward()
    torch.cuda.synchronize()
    one_forward = int(e._rng_offset) - e_off
    assert one_forward > 0 and g_off == e_off + one_forward
    assert _bn_counts(e.netG) == g_counts and int(e._rng_offset) == g_off


# ---- what may and may not run between two prefetching replays -------------------------------------------------------------------------
def test_test_between_two_prefetching_replays_leaves_the_kept_latent(fresh):
    r = fresh
    gs, m, S = r["gs"], r["gs"].m, r["S"]
    kept = m.netG._kept["x"].clone()
    m.set_input(r["ring"][2])
    m.test()
    torch.cuda.synchronize()
    assert torch.equal(m.netG._kept["x"], kept), "test() overwrote the latent the next step's first-layer backward-weight reads"


def test_eager_step_on_a_prefetching_trainer_is_refused_and_harmless(fresh):
    from supervised_gan_amd._lib import SganError
    r = fresh
    gs, m, S = r["gs"], r["gs"].m, r["S"]
    kept, full = m.netG._kept, m.netG._kept_full
    m.set_input(r["ring"][1])
    with pytest.raises(SganError):
        m.forward()
    with pytest.raises(SganError):
        m.optimize_parameters()
    assert m.netG._kept is kept and m.netG._kept_full is full
    gs.step(r["ring"][1])
    _assert_same_step(gs, _record(gs, r["out"]), r["e"], S, "replay after the refused calls vs launches")

"""Everything a trainer under graph_step.GraphedStep carries from one step to the next, by name: state_tensors() lists the device
tensors, snapshot() clones them (with python's `random` state and the ImagePools' host counters), restore() writes a snapshot back
in place, so that a captured graph -- which holds raw addresses -- goes on from exactly the snapshot's state.  compare() holds the
metrics tests/test_graph_step_snapshot.py judges two steps from one snapshot by.  Imports no GPU code."""
import random
from collections import OrderedDict

import torch

DERIVED = ("_flat_t", "_pk_f", "_pk_b", "_pk_bh")


def _networks(m):
    """[(label, network)]: checkpoint_nets() (the EMA shadow is among them under --ema_decay)."""
    return list(m.checkpoint_nets())


def _optimizers(m):
    """[(label, FusedAdam)]: AdamGroups opened into their members."""
    out = []
    for k, o in sorted(vars(m).items()):
        if k.startswith("optimizer_"):
            members = getattr(o, "optimizers", None) or [o]
            out += [("%s.%d" % (k, i) if len(members) > 1 else k, f) for i, f in enumerate(members)]
    return out


def _pools(m):
    from supervised_gan_amd.image_pool import ImagePool
    return [(k, p) for k, p in sorted(vars(m).items()) if isinstance(p, ImagePool)]


def state_tensors(gs):
    """name -> tensor, in a fixed order; one entry per allocation (networks packed into one arena share its entry)."""
    m = gs.m
    out, seen = OrderedDict(), set()

    def add(name, t):
        if not torch.is_tensor(t):
            return
        key = (t.data_ptr(), t.numel(), t.dtype, tuple(t.stride()))
        if t.numel() and key in seen:
            return
        seen.add(key)
        assert name not in out, name
        out[name] = t

    for label, net in _networks(m):
        arena_p, arena_g, _ = net._arena
        add("net.%s.params" % label, arena_p)
        add("net.%s.grads" % label, arena_g)
        lo, hi = arena_p.data_ptr(), arena_p.data_ptr() + arena_p.numel() * arena_p.element_size()
        for k, p in net.named_parameters():      # a parameter kept outside the arena (the discriminators' fixed Gaussian pre-filter)
            if p.numel() and not lo <= p.data_ptr() < hi:
                add("net.%s.extra.%s" % (label, k), p.detach())
                add("net.%s.extra_grad.%s" % (label, k), p.grad)
        for k, b in net.named_buffers():
            add("net.%s.buffer.%s" % (label, k), b)
        der = getattr(arena_p, "_sgan_derived", None)
        for i, name in enumerate(DERIVED):
            add("net.%s.derived.%s" % (label, name), der[i] if der is not None else getattr(net, name, None))
        for k, mod in net.named_modules():
            add("net.%s.rng_offset.%s" % (label, k), getattr(mod, "_rng_offset", None))
        kept = getattr(net, "_kept", None)
        if kept is not None:
            add("net.%s.kept.x" % label, kept["x"])
            for i, t in enumerate(kept["outs"]):
                add("net.%s.kept.outs.%d" % (label, i), t)
            add("net.%s.kept.full" % label, getattr(net, "_kept_full", None))
    for label, o in _optimizers(m):
        for i, t in enumerate(getattr(o, "_m", None) or []):
            add("%s.m.%d" % (label, i), t)
        for i, t in enumerate(getattr(o, "_v", None) or []):
            add("%s.v.%d" % (label, i), t)
        add("%s.state" % label, getattr(o, "_state", None))
        add("%s.lr_dev" % label, getattr(o, "_lr_dev", None))
    if getattr(m, "ema", None) is not None:
        add("ema.state", m.ema._state)
    add("rng_offset", getattr(m, "_rng_offset", None))
    if getattr(m, "diffaug", None) is not None:
        add("diffaug.rng_offset", getattr(m.diffaug, "offset", None))
    for k in ("_noise_buf", "_noise_buf_alt"):
        add(k, getattr(m, k, None))
    for i, t in enumerate(getattr(gs, "fake_for_D", None) or []):
        add("fake_for_D.%d" % i, t)
    for k, p in _pools(m):
        add("pool.%s.slots" % k, p._slots)
    add("fake_next", getattr(m, "_fake_next", None))
    return out


def snapshot(gs):
    """{"tensors": clones of state_tensors(gs), "random": python's generator state, "pools": {name: num_imgs}}."""
    return {"tensors": OrderedDict((k, t.detach().clone()) for k, t in state_tensors(gs).items()),
            "random": random.getstate(), "pools": {k: p.num_imgs for k, p in _pools(gs.m)}}


def restore(gs, snap):
    """Writes `snap` back: copy_ into the live tensors (no address moves), python's generator, the pools' counters.  The names must
    be the ones the snapshot was taken with: state that appeared since (a pool's first allocation) cannot be rolled back.
    The copies go through `.data`, as the kernels' own writes go past torch: no version counter moves, so the autograd node a
    prefetched forward left on these buffers stays usable and no derived-copy key goes stale on the host."""
    live = state_tensors(gs)
    assert list(live) == list(snap["tensors"]), sorted(set(live) ^ set(snap["tensors"]))
    with torch.no_grad():
        for k, t in live.items():
            t.data.copy_(snap["tensors"][k])
    random.setstate(snap["random"])
    for k, p in _pools(gs.m):
        p.num_imgs = snap["pools"][k]


# ---- comparison of two records taken after one step from the same snapshot -----------------------------------------------------------
EXACT, UPDATE, PACKED, FLOAT = "exact", "update", "packed", "float"


def kind(name):
    """How a state tensor of two steps from one snapshot is compared: bit for bit (counters, learning rates, Philox offsets and the
    latents they determine), by its update (parameter arenas), not at all here (the derived weight copies: the 16-bit packs are bit
    patterns and the transposed copy a permutation; the repack test holds all four bit for bit), or as floats."""
    if name.endswith((".state", ".lr_dev", "num_batches_tracked")) or "rng_offset" in name or name.startswith("_noise_buf") \
            or name.endswith(".kept.x"):
        return EXACT
    if ".derived." in name:
        return PACKED
    if name.endswith(".params"):
        return UPDATE
    return FLOAT


def max_rel(a, b):
    """max |a - b| / max |b|  (0 when both are all zero)."""
    a, b = a.double(), b.double()
    if a.numel() == 0:
        return 0.0
    d, ref = float((a - b).abs().max()), float(b.abs().max())
    if d != d or ref != ref:
        return float("inf")
    return d / ref if ref > 0 else (0.0 if d == 0 else float("inf"))


def update_rel(a, b, s, keep=None):
    """|| (a - s) - (b - s) ||_2 / || b - s ||_2: the step's update of a parameter tensor, not its value; keep: a mask of the elements
    that count."""
    a, b, s = a.double(), b.double(), s.double()
    da, db = a - s, b - s
    if keep is not None:
        da, db = da[keep], db[keep]
    num, den = float((da - db).norm()), float(db.norm())
    if num != num or den != den:
        return float("inf")
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))


def compare(rec, ref, start):
    """rec, ref: records {"snap": snapshot, "errors": [floats], "out": tensor, "probes": {name: tensor}} of two steps from the
    snapshot `start`; `ref` is the reference.  Returns (names that must match exactly and do not, {name: max-abs over max-abs of
    the reference} for the float tensors, the probes, every loss scalar on its own and the output, {name: update metric})."""
    bad, floats, update = [], {}, {}
    a, b, s = rec["snap"]["tensors"], ref["snap"]["tensors"], start["tensors"]
    assert list(a) == list(b) == list(s)
    for k in a:
        how = kind(k)
        if k.startswith("pool."):      # the slots a pool has not filled yet are uninitialised memory
            n = ref["snap"]["pools"][k[len("pool."):-len(".slots")]]
            floats[k] = max_rel(a[k][:n], b[k][:n])
        elif how == EXACT:
            if not torch.equal(a[k], b[k]):
                bad.append(k)
        elif how == UPDATE:
            update[k] = update_rel(a[k], b[k], s[k])
        elif how == FLOAT:
            floats[k] = max_rel(a[k], b[k])
    if rec["snap"]["random"] != ref["snap"]["random"]:
        bad.append("random.getstate()")
    if rec["snap"]["pools"] != ref["snap"]["pools"]:
        bad.append("pool counters")
    assert len(rec["errors"]) == len(ref["errors"])
    for i, (x, y) in enumerate(zip(rec["errors"], ref["errors"])):
        floats["loss.%d" % i] = max_rel(torch.tensor([x]), torch.tensor([y]))
    floats["output"] = max_rel(rec["out"], ref["out"])
    assert list(rec.get("probes", {})) == list(ref.get("probes", {}))
    for k, t in rec.get("probes", {}).items():
        floats[k] = max_rel(t, ref["probes"][k])
    return bad, floats, update

"""tests/graph_state.py on CPU-built trainers (as tests/test_step_program_host.py builds them): state_tensors() names every parameter,
gradient, buffer and optimizer tensor exactly once, restore(snapshot()) is the identity, and restore() moves no address -- what a
captured graph, which holds raw addresses, needs of the snapshots tests/test_graph_step_snapshot.py takes."""
import random

import pytest
import torch

from graph_state import restore, snapshot, state_tensors
from test_graph_step import CGAN, FCGAN, TWOSTAGE
from test_step_program_host import SEGM_D, _build

CASES = {"fcgan": FCGAN, "fcgan_ema": FCGAN + ["--ema_decay", "0.999"], "cgan": CGAN, "twostage_cycle": TWOSTAGE, "segmentation_d": SEGM_D}


def _trainer(argv, tmp_path):
    """A GraphedStep over a CPU trainer whose lazy state exists: optimizer moments, one pooled image, the static pool buffer."""
    from supervised_gan_amd.graph_step import GraphedStep
    from supervised_gan_amd.image_pool import ImagePool
    m = _build(argv, tmp_path)
    gs = GraphedStep(m)
    for k, o in vars(m).items():
        if k.startswith("optimizer_"):
            o.sync_lr()
    g = torch.Generator().manual_seed(3)
    for p in (p for p in vars(m).values() if isinstance(p, ImagePool)):
        p.query(torch.rand(1, 2, 8, 8, generator=g))
    gs.fake_for_D = [torch.rand(8, 8, 4, generator=g)]
    return gs


def _same_bits(a, b):
    """Equality of the bytes: a pool's unfilled slots are uninitialised memory and may hold NaN patterns."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def _span(t):
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


def _holders(st, t):
    lo, hi = _span(t)
    return [k for k, s in st.items() if s.numel() and _span(s)[0] <= lo and hi <= _span(s)[1]]


@pytest.mark.parametrize("case", list(CASES))
def test_state_tensors_name_every_tensor_once(case, tmp_path):
    gs = _trainer(CASES[case], tmp_path)
    m, st = gs.m, state_tensors(gs)
    n_params = n_bufs = n_opt = 0
    for label, net in m.checkpoint_nets():
        for k, p in net.named_parameters():
            if p.numel():
                assert len(_holders(st, p)) == 1, (label, k, _holders(st, p))
                n_params += 1
                if p.grad is not None:
                    assert len(_holders(st, p.grad)) == 1, (label, k, "grad")
        for k, b in net.named_buffers():
            assert _holders(st, b) == ["net.%s.buffer.%s" % (label, k)]
            n_bufs += 1
    opts = [f for k, o in vars(m).items() if k.startswith("optimizer_") for f in (getattr(o, "optimizers", None) or [o])]
    for o in opts:
        for t in o._m + o._v + [o._state, o._lr_dev]:
            assert len(_holders(st, t)) == 1
            n_opt += 1
    assert n_params > 0 and n_opt >= 4 * len(opts) > 0
    assert n_bufs > 0 or case in ("cgan", "segmentation_d")      # instance norm keeps no buffers
    if case == "fcgan_ema":
        assert "ema.state" in st and "net.G_ema.params" in st
    assert "rng_offset" in st and "fake_for_D.0" in st and any(k.startswith("pool.") for k in st)
    spans = sorted(_span(t) for t in st.values() if t.numel())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "two state tensors overlap"


@pytest.mark.parametrize("case", list(CASES))
def test_restore_of_a_snapshot_is_the_identity_and_moves_nothing(case, tmp_path):
    gs = _trainer(CASES[case], tmp_path)
    random.seed(5)
    snap = snapshot(gs)
    ptrs = {k: t.data_ptr() for k, t in state_tensors(gs).items()}
    assert all(c.data_ptr() != ptrs[k] or c.numel() == 0 for k, c in snap["tensors"].items()), "a snapshot holds clones"
    with torch.no_grad():
        for t in state_tensors(gs).values():
            t.add_(1)
    random.random()
    from supervised_gan_amd.image_pool import ImagePool
    pools = [p for p in vars(gs.m).values() if isinstance(p, ImagePool)]
    for p in pools:
        p.num_imgs += 3
    changed = snapshot(gs)
    assert all(not _same_bits(changed["tensors"][k], v) for k, v in snap["tensors"].items() if v.numel())
    assert changed["random"] != snap["random"] and changed["pools"] != snap["pools"]
    restore(gs, snap)
    back = snapshot(gs)
    assert list(back["tensors"]) == list(snap["tensors"])
    for k, v in snap["tensors"].items():
        assert _same_bits(back["tensors"][k], v), k
    assert back["random"] == snap["random"] == random.getstate() and back["pools"] == snap["pools"]
    assert {k: t.data_ptr() for k, t in state_tensors(gs).items()} == ptrs

"""ops.graph_capture: the capture every product graph goes through (GraphedStep, LatentReconstructor).  Dead reference cycles are
collected before the capture begins and the cycle collector is off until it ends, so no dead trainer's graphs or memory pool can be
destroyed by a collection that an allocation inside the capture happens to start ("What the tests found")."""
import gc
import weakref

import pytest
import torch

pytestmark = pytest.mark.gpu


class _Node:
    pass


def test_capture_collects_first_and_keeps_the_collector_off():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import ops
    a = _Node()
    a.me, a.t = a, torch.ones(4, device="cuda")      # a dead cycle that holds device memory
    dead = weakref.ref(a)
    del a
    assert gc.isenabled()
    x = torch.zeros(8, device="cuda")
    g = torch.cuda.CUDAGraph()
    with ops.graph_capture(g):
        assert dead() is None and not gc.isenabled()
        y = x + 1
    assert gc.isenabled()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y.cpu(), torch.ones(8))
    gc.disable()        # a caller that had the collector off gets it back off
    try:
        with ops.graph_capture(torch.cuda.CUDAGraph()):
            x + 1
        assert not gc.isenabled()
    finally:
        gc.enable()

"""sgan_ema_multi through ops.ema_multi on the device against the fp64 reference (ema_ref.py): segments at every misalignment of
shadow and p, the exact cases, the segment limit, the refused calls, and a captured update replayed against eager updates."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ema_ref import ema_bound, ema_ref  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = (1, 3, 4, 255, 256, 257, 1025, 70001)
OFFSETS = (0, 1, 2, 3, 5)
GUARD = 8      # floats on both sides of every slice that nobody may touch
K = 20


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")


def _layout(rng):
    """Every length as a slice of one big buffer, shadow and p offsets drawn independently so that every (shadow offset, p offset)
    residue pair modulo 4 occurs: [(shadow start, p start, n)], the buffer lengths."""
    spans, s_pos, p_pos = [], 0, 0
    pairs = [(a, b) for a in OFFSETS for b in OFFSETS]
    rng.shuffle(pairs)
    i = 0
    for n in LENGTHS:
        for _ in range(4):      # 8 lengths x 4 = 32 segments >= the 25 offset pairs
            so, po = pairs[i % len(pairs)]
            i += 1
            s_start = (s_pos + GUARD + 3) // 4 * 4 + so      # a 16-byte aligned position plus the offset
            p_start = (p_pos + GUARD + 3) // 4 * 4 + po
            spans.append((s_start, p_start, n))
            s_pos, p_pos = s_start + n, p_start + n
    return spans, s_pos + GUARD + 8, p_pos + GUARD + 8


@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warmup"])
@pytest.mark.parametrize("decay", [0.5, 0.999])
def test_updates_match_the_reference(decay, warmup):
    _need_gpu()
    from supervised_gan_amd import ops
    rng = np.random.default_rng(17)
    spans, ns, npp = _layout(rng)
    assert len(spans) <= 64 and {(s % 4, p % 4) for s, p, _ in spans} >= {(a % 4, b % 4) for a in OFFSETS for b in OFFSETS}
    s0 = rng.standard_normal(ns).astype(np.float32)
    S = torch.from_numpy(s0.copy()).cuda()
    P = torch.zeros(npp, dtype=torch.float32, device="cuda")
    assert S.data_ptr() % 16 == 0 and P.data_ptr() % 16 == 0
    state = torch.zeros(4, dtype=torch.int32, device="cuda")
    segs = [(S[a: a + n], P[b: b + n]) for a, b, n in spans]
    p_seq = []
    for _ in range(K):
        p = rng.standard_normal(npp).astype(np.float32)
        p_seq.append(p)
        P.copy_(torch.from_numpy(p))
        ops.ema_multi(segs, decay, warmup, state)
        assert np.array_equal(P.cpu().numpy().view(np.uint32), p.view(np.uint32)), "p was written"
    got = S.cpu().numpy()
    touched = np.zeros(ns, dtype=bool)
    worst = 0.0
    for a, b, n in spans:
        ref, t = ema_ref(s0[a: a + n], [p[b: b + n] for p in p_seq], decay, warmup)
        bound = ema_bound(s0[a: a + n], [p[b: b + n] for p in p_seq])
        dev = np.abs(got[a: a + n].astype(np.float64) - ref)
        worst = max(worst, float((dev / bound).max()))
        assert (dev <= bound).all(), (a, b, n, float(dev.max()), bound)
        touched[a: a + n] = True
    print(f"decay {decay} warmup {warmup}: largest deviation / bound over {len(spans)} segments = {worst:.3f}")
    assert np.array_equal(got.view(np.uint32)[~touched], s0.view(np.uint32)[~touched]), "a guard element of shadow changed"
    assert (~touched).sum() >= 2 * GUARD
    assert int(state[0].item()) == K == t


def _one(n=1031, off=(1, 2), seed=5):
    rng = np.random.default_rng(seed)
    s = torch.from_numpy(rng.standard_normal(n + 16).astype(np.float32)).cuda()
    p = torch.from_numpy(rng.standard_normal(n + 16).astype(np.float32)).cuda()
    p[3] = 1e-8      # against a shadow of order 1: fl(fl(p - s) + s) != p
    s[7] = -0.0      # 0 * (p - s) + (-0) = +0
    return s, p, (s[off[0]: off[0] + n], p[off[1]: off[1] + n])


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32).copy()


def test_decay_one_leaves_shadow_and_decay_zero_copies_p():
    _need_gpu()
    from supervised_gan_amd import ops
    s, p, seg = _one()
    before, state = _bits(s), torch.zeros(4, dtype=torch.int32, device="cuda")
    ops.ema_multi([seg], 1.0, False, state)
    assert np.array_equal(_bits(s), before) and int(state[0].item()) == 1
    ops.ema_multi([seg], 0.0, False, state)
    assert np.array_equal(_bits(seg[0]), _bits(seg[1])) and int(state[0].item()) == 2
    after = _bits(s)
    assert np.array_equal(after[:1], before[:1]) and np.array_equal(after[1 + 1031:], before[1 + 1031:])


def test_64_segments_and_the_empty_calls():
    _need_gpu()
    from supervised_gan_amd import ops
    rng = np.random.default_rng(9)
    s0, p0 = rng.standard_normal(64 * 37 + 3).astype(np.float32), rng.standard_normal(64 * 37 + 3).astype(np.float32)
    S, P = torch.from_numpy(s0.copy()).cuda(), torch.from_numpy(p0.copy()).cuda()
    state = torch.zeros(4, dtype=torch.int32, device="cuda")
    segs = [(S[37 * i + 1: 37 * i + 34], P[37 * i + 2: 37 * i + 35]) for i in range(64)]
    ops.ema_multi(segs, 0.5, False, state)
    ops.ema_multi(segs, 0.5, False, state)
    got = S.cpu().numpy()
    for i in range(64):
        a, b = 37 * i + 1, 37 * i + 2
        ref, _ = ema_ref(s0[a: a + 33], [p0[b: b + 33]] * 2, 0.5, False)
        assert (np.abs(got[a: a + 33] - ref) <= ema_bound(s0[a: a + 33], [p0[b: b + 33]] * 2)).all()
        assert np.array_equal(got[a + 33: a + 37].view(np.uint32), s0[a + 33: a + 37].view(np.uint32))
    # no segment, and segments without elements: nothing is averaged, the update counts
    before = _bits(S)
    ops.ema_multi([], 0.5, False, state)
    ops.ema_multi([(S[5:5], P[9:9])], 0.5, False, state)
    assert np.array_equal(_bits(S), before) and int(state[0].item()) == 4


@pytest.mark.parametrize("case", ["nseg65", "negative", "above_one", "alias"])
def test_refused_calls_change_nothing(case):
    _need_gpu()
    from supervised_gan_amd import ops
    from supervised_gan_amd._lib import SganError
    s, p, seg = _one()
    state = torch.zeros(4, dtype=torch.int32, device="cuda")
    ops.ema_multi([seg], 0.5, False, state)      # a counter that is not 0
    before = _bits(s)
    segs, decay = [seg], 0.5
    if case == "nseg65":
        segs = [(s[8 * i: 8 * i + 8], p[8 * i: 8 * i + 8]) for i in range(65)]
    elif case == "negative":
        decay = -0.1
    elif case == "above_one":
        decay = 1.1
    else:
        segs = [(seg[0], seg[0])]
    with pytest.raises(SganError):
        ops.ema_multi(segs, decay, False, state)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(s), before) and int(state[0].item()) == 1


def test_captured_update_replays_with_the_right_count():
    """One update captured in a graph and replayed five times against five eager updates, p rewritten in place in between, warm-up
    on so that a count frozen at capture would show.  The kernel is elementwise and has no atomics: bit for bit."""
    _need_gpu()
    from supervised_gan_amd import ops
    rng = np.random.default_rng(23)
    n = 70001 + 257
    s0 = rng.standard_normal(n + 8).astype(np.float32)
    ps = [rng.standard_normal(n + 8).astype(np.float32) for _ in range(5)]
    cut = [(1, 2, 70001), (70001 + 4, 70001 + 3, 257)]

    def run(graphed):
        S, P = torch.from_numpy(s0.copy()).cuda(), torch.zeros(n + 8, dtype=torch.float32, device="cuda")
        state = torch.zeros(4, dtype=torch.int32, device="cuda")
        segs = [(S[a: a + m], P[b: b + m]) for a, b, m in cut]
        if graphed:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):      # library handles and the like exist before the capture
                ops.ema_multi(segs, 0.999, True, state)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            S.copy_(torch.from_numpy(s0))
            state.zero_()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                ops.ema_multi(segs, 0.999, True, state)
            S.copy_(torch.from_numpy(s0))      # the capture itself runs nothing, but start from a known state all the same
            state.zero_()
        for p in ps:
            P.copy_(torch.from_numpy(p))
            if graphed:
                g.replay()
            else:
                ops.ema_multi(segs, 0.999, True, state)
        torch.cuda.synchronize()
        return _bits(S), int(state[0].item())

    eager, te = run(False)
    replayed, tr = run(True)
    assert te == tr == 5
    assert np.array_equal(eager, replayed)
    ref, _ = ema_ref(s0[1: 70002], [p[2: 70003] for p in ps], 0.999, True)
    assert (np.abs(eager.view(np.float32)[1: 70002] - ref) <= ema_bound(s0[1: 70002], [p[2: 70003] for p in ps])).all()

"""The optimizer launches on their own, fed known gradients, against the fp64 reference of tests/adam_ref.py:
sgan_adam_pack (sg_adam_pack_kernel: Adam on LDS tiles of the conv-weight ranges + their three derived copies + plain Adam over the
gaps + gradient zeroing + the ticket that moves the step number on), sgan_adam_multi, sgan_sgd_multi and sgan_zero_multi.

Given the gradients the update is deterministic, so -- unlike two independent training runs -- parameters CAN be compared here.
Bound (adam_ref.assert_within_yardstick): the kernel's p (absolute), m and v (relative to their largest magnitude) stay within 4 x
the deviation of the float32 restatement of the same formula from float64, on the same inputs.  Everything else -- derived copies,
gradients, `state`, guards, the zero-gradient slice -- is exact.

fp32 yardstick after 5 steps, deviation from fp64 as (max |dp|, max |dm| / max |m|, max |dv| / max |v|); "body" = outside the three
fixed slices (over [0, n) the 1e12 slice owns max |m| and max |v|).  Every test prints the kernel's figures beside these (pytest -s):
    layout       [0, n)                          body
    gaps_only    3.00e-7  3.49e-8  4.85e-8       3.00e-7  4.46e-8  5.55e-8
    one_tiny     3.56e-7  1.63e-8  5.49e-8       (13 elements: no body bound)
    pack_pair    4.07e-7  3.86e-8  5.64e-8       4.07e-7  4.78e-8  8.43e-8
    ragged       4.18e-7  3.77e-8  7.33e-8       4.18e-7  4.05e-8  8.19e-8
    table_full   4.72e-7  2.49e-8  3.54e-8       4.72e-7  5.46e-8  8.61e-8
    walk         7.12e-7  3.25e-8  6.78e-8       7.12e-7  3.90e-8  7.32e-8
"""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_ref as A

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = A.as_f32(2e-4, 0.5, 0.999, 1e-8)      # what crosses the C ABI (floats), on both sides of every comparison
STEPS = 5
GUARD = 1024                                            # elements of sentinel behind (zero_multi: around) every buffer
MIN_BODY = 512                                          # elements outside the fixed slices for the body-only bound (Case.check)
PATTERN = 0x7E570000                                    # derived copies start as 0x7E57xxxx words: finite, non-zero, recognisable


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import _lib, ops
    _lib.lib()
    return ops


# ---- guarded buffers ----------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


class Guards:
    """Buffers whose storage ends in GUARD sentinel elements (NaN, or 0x5A5A5A5A for integers): an over-read that is used turns
    a result NaN, an over-write changes the sentinel's bits."""

    def __init__(self):
        self.guards = []

    def make(self, host):
        host = torch.from_numpy(np.array(host)) if isinstance(host, np.ndarray) else host
        fill = float("nan") if host.dtype == torch.float32 else 0x5A5A5A5A
        flat = torch.full((host.numel() + GUARD,), fill, dtype=host.dtype, device="cuda")
        flat[: host.numel()] = host.reshape(-1)
        self.guards.append((flat[host.numel():], _bits(flat[host.numel():]).clone()))
        return flat[: host.numel()]

    def intact(self):
        return all(torch.equal(_bits(g), snap) for g, snap in self.guards)


def _pattern(n):
    return torch.from_numpy((PATTERN | (np.arange(n, dtype=np.int64) & 0xFFFF)).astype(np.int32)).view(torch.float32)


def _dev(a):
    """A (read-only) host array as a fresh device tensor."""
    return torch.from_numpy(np.array(a)).cuda()


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---- layouts ------------------------------------------------------------------------------------------------------------------
def _layouts():
    """name -> (n, [(off, taps, cout, cin)]): the smallest that reach each branch of sg_adam_pack_kernel."""
    out = {"gaps_only": (1029, []),                                            # nseg = 0; two chunks, the second 5 long; n % 4 = 1
           "one_tiny": (16, [(0, 1, 4, 4)]),                                   # no gap; one partial tile; no 16-bit copy (4 % 8)
           "pack_pair": (15368 + 9 * 16 * 12 + 1024, [(0, 16, 40, 24), (15368, 9, 16, 12)])}      # 8-float gap; a chunk with no tail
    o2 = 4 + 9 * 36 * 100 + 1028
    out["ragged"] = (o2 + 49 * 8 * 64 + 3, [(4, 9, 36, 100), (o2, 49, 8, 64)])       # 4-wide / 4-tall tiles, skipped copies, 49 taps
    out["table_full"] = (4 + 68 * 63 + 64 + 4, [(4 + 68 * i, 1, 8, 8) for i in range(64)])      # 64 ranges, 65 gaps
    out["walk"] = (16 * 264 * 264 + 2052, [(0, 16, 264, 264)])                 # 1296 tiles + 3 chunks > 1024 workgroups
    return out


LAYOUTS = _layouts()
_CASES = {}


class Case:
    """Inputs of one layout and their references, computed once and never written again."""

    def __init__(self, name):
        self.name = name
        self.n, self.segs = LAYOUTS[name]
        n = self.n
        rng = np.random.default_rng(sum(name.encode()))
        self.p0 = rng.standard_normal(n).astype(np.float32)
        self.grads = [(rng.standard_normal(n) * 10.0 ** (s - 3)).astype(np.float32) for s in range(STEPS)]
        k = max(1, min(97, n // 16))       # 97 > 68: in table_full every slice covers a whole range and the gaps on both sides
        self.zero, self.tiny, self.huge = (slice(a, a + k) for a in (n // 4, n // 2, 3 * n // 4))
        self.body = np.ones(n, dtype=bool)
        for g in self.grads:
            g[self.zero] = 0.0
            g[self.tiny] = 1e-20
            g[self.huge] *= np.float32(1e12)
        for s in (self.zero, self.tiny, self.huge):
            self.body[s] = False
        assert all(np.isfinite(g.astype(np.float32) ** 2).all() for g in self.grads)
        self.ref = A.adam_run(A.adam_step, self.p0.astype(np.float64), self.grads, LR, B1, B2, EPS)
        self.f32 = A.adam_run(A.adam_step_f32, self.p0, self.grads, LR, B1, B2, EPS)
        for a in (self.p0, *self.grads, *self.ref, *self.f32):
            a.setflags(write=False)

    def check(self, got, what):
        """The bound over [0, n), and the same bound over the body alone: over [0, n) the 1e12 slice owns max |m| and max |v|,
        which would leave the moments of everything else unchecked.  The body check needs a body: a maximum over a dozen
        elements says little about how far fp32 rounding reaches (one_tiny's 13 body elements put the v yardstick at 0.3 ulp,
        which a single differently rounded product exceeds fourfold), so it runs where the body has at least MIN_BODY elements."""
        A.assert_within_yardstick(got, self.f32, self.ref, f"{self.name} {what} [0, n)")
        if int(self.body.sum()) >= MIN_BODY:
            A.assert_within_yardstick(got, self.f32, self.ref, f"{self.name} {what} body", self.body)


def _case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def _state_words(t, lr=LR):
    step_size, inv = A.bias_corrections(t, lr, B1, B2)
    return [t, int(np.float32(step_size).view(np.int32)), int(np.float32(inv).view(np.int32)), 0]


def test_layouts_reach_what_they_claim():
    """Host arithmetic only: the layouts are sorted, disjoint, 4-aligned, and hit the table limits / the walk they are named for."""
    for name, (n, segs) in LAYOUTS.items():
        cur, gaps, tiles, chunks = 0, [], 0, 0
        for off, taps, co, ci in segs:
            assert off % 4 == 0 and off >= cur, name
            if off > cur:
                gaps.append(off - cur)
            tiles += taps * -(-co // 32) * -(-ci // 32)
            cur = off + taps * co * ci
        assert cur <= n, name
        if cur < n:
            gaps.append(n - cur)
        chunks = sum(-(-g // 1024) for g in gaps)
        if name == "gaps_only":
            assert (tiles, chunks, gaps) == (0, 2, [1029])
        if name == "one_tiny":
            assert (tiles, gaps) == (1, [])
        if name == "pack_pair":
            assert gaps == [8, 1024]
        if name == "ragged":
            assert gaps == [4, 1028, 3] and 100 % 32 == 4 and 36 % 32 == 4 and 100 % 8 and 36 % 8
        if name == "table_full":
            assert len(segs) == 64 and len(gaps) == 65 and set(gaps) == {4}
        if name == "walk":
            assert tiles == 1296 and chunks == 3 and tiles + chunks > 1024


# ---- sgan_adam_pack -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero_grads", [0, 1], ids=["keep_grads", "zero_grads"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_adam_pack_five_steps(ops, layout, zero_grads):
    """Five ops.adam_pack steps over a layout: p / m / v against fp64, `state`, the gradient buffer, the four derived copies against
    a fresh ops.pack_weights of the final master, the fixed slices, every guard."""
    c = _case(layout)
    n, G = c.n, Guards()
    p, g = G.make(c.p0), G.make(np.zeros(n, dtype=np.float32))
    m, v = G.make(np.zeros(n, dtype=np.float32)), G.make(np.zeros(n, dtype=np.float32))
    der = [G.make(_pattern(n)) for _ in range(4)]
    state = G.make(torch.zeros(4, dtype=torch.int32))
    lr = G.make(np.full(1, LR, dtype=np.float32))
    for s in range(STEPS):
        gin = _dev(c.grads[s])
        g.copy_(gin)
        ops.adam_pack(p, g, m, v, lr, B1, B2, EPS, state, *der, c.segs, zero_grads)
        if zero_grads:
            assert _same_bits(g, torch.zeros_like(g)), f"step {s + 1}: a consumed gradient was not cleared to +0.0"
        else:
            assert _same_bits(g, gin), f"step {s + 1}: the gradient was written"
    torch.cuda.synchronize()
    assert state.cpu().tolist() == _state_words(STEPS)
    got = tuple(t.cpu().numpy() for t in (p, m, v))
    c.check(got, "adam_pack")
    # gradient exactly 0 on every step: p, m and v bit-identical to the start (no NaN from 0 / eps, no drift)
    assert np.array_equal(got[0][c.zero].view(np.int32), c.p0[c.zero].view(np.int32))
    assert not got[1][c.zero].view(np.int32).any() and not got[2][c.zero].view(np.int32).any()
    assert all(np.isfinite(a).all() for a in got)
    # the derived copies: exactly what a fresh pack of the final master writes, and nothing else
    fresh = [_pattern(n).cuda() for _ in range(4)]
    ops.pack_weights(p, fresh[0], fresh[1], fresh[2], c.segs, fresh[3])
    torch.cuda.synchronize()
    for name, a, b in zip(("flat_t", "pk_f", "pk_b", "pk_bh"), der, fresh):
        assert _same_bits(a, b), f"{name} differs from a fresh pack of the updated master"
    if c.segs:
        off, taps, co, ci = c.segs[-1]
        w = p[off: off + taps * co * ci].view(taps, co, ci)
        assert torch.equal(der[0][off: off + taps * co * ci].view(taps, ci, co), w.transpose(1, 2))      # flat_t is the NEW master, transposed
        assert not _same_bits(der[0][off: off + taps * co * ci], _pattern(n).cuda()[off: off + taps * co * ci])
    assert G.intact()


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_adam_multi_one_segment_meets_the_same_bound(ops, layout):
    """The same five steps through the other kernel (sgan_adam_multi, one segment): the same bound.  Not bit equality with
    sg_adam_pack_kernel -- the compiler may contract different products into FMAs."""
    c = _case(layout)
    n, G = c.n, Guards()
    p, g = G.make(c.p0), G.make(np.zeros(n, dtype=np.float32))
    m, v = G.make(np.zeros(n, dtype=np.float32)), G.make(np.zeros(n, dtype=np.float32))
    state = G.make(torch.zeros(4, dtype=torch.int32))
    lr = G.make(np.full(1, LR, dtype=np.float32))
    for s in range(STEPS):
        g.copy_(_dev(c.grads[s]))
        ops.adam_multi([(p, g, m, v, n)], lr, B1, B2, EPS, state)
    torch.cuda.synchronize()
    assert state.cpu().tolist() == _state_words(STEPS)
    assert _same_bits(g, _dev(c.grads[-1]))
    got = tuple(t.cpu().numpy() for t in (p, m, v))
    c.check(got, "adam_multi")
    assert np.array_equal(got[0][c.zero].view(np.int32), c.p0[c.zero].view(np.int32))
    assert not got[1][c.zero].view(np.int32).any() and not got[2][c.zero].view(np.int32).any()
    assert G.intact()


def test_adam_pack_graph_replay_advances_the_step(ops):
    """What the ticket protocol exists for: ONE captured ops.adam_pack launch, replayed three times with a new gradient copied
    into the captured buffer each time, applies steps t0 + 1 ... t0 + 3 with their own bias corrections (t0: the steps that ran
    before the first replay -- one eager launch, so that nothing is loaded during the capture, plus whatever the capture itself
    executed, counted from state[0])."""
    c = _case("pack_pair")
    n, G = c.n, Guards()
    p, g = G.make(c.p0), G.make(c.grads[0])
    m, v = G.make(np.zeros(n, dtype=np.float32)), G.make(np.zeros(n, dtype=np.float32))
    der = [G.make(_pattern(n)) for _ in range(4)]
    state = G.make(torch.zeros(4, dtype=torch.int32))
    lr = G.make(np.full(1, LR, dtype=np.float32))
    ops.adam_pack(p, g, m, v, lr, B1, B2, EPS, state, *der, c.segs, 0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.adam_pack(p, g, m, v, lr, B1, B2, EPS, state, *der, c.segs, 0)
    torch.cuda.synchronize()
    t0 = int(state[0].item())
    assert t0 in (1, 2)
    applied = [c.grads[0]] * t0
    for s in range(1, 4):
        g.copy_(_dev(c.grads[s]))
        graph.replay()
        applied.append(c.grads[s])
    torch.cuda.synchronize()
    assert state.cpu().tolist() == _state_words(t0 + 3)
    ref = A.adam_run(A.adam_step, c.p0.astype(np.float64), applied, LR, B1, B2, EPS)
    f32 = A.adam_run(A.adam_step_f32, c.p0, applied, LR, B1, B2, EPS)
    got = tuple(t.cpu().numpy() for t in (p, m, v))
    A.assert_within_yardstick(got, f32, ref, "replay [0, n)")
    A.assert_within_yardstick(got, f32, ref, "replay body", c.body)      # pack_pair: 17829 body elements
    fresh = [_pattern(n).cuda() for _ in range(4)]
    ops.pack_weights(p, fresh[0], fresh[1], fresh[2], c.segs, fresh[3])
    torch.cuda.synchronize()
    assert all(_same_bits(a, b) for a, b in zip(der, fresh))
    assert G.intact()


BAD_RANGES = {
    "65 ranges": [(64 * i, 1, 8, 8) for i in range(65)],
    "overlapping": [(0, 1, 8, 8), (32, 1, 8, 8)],
    "unsorted": [(128, 1, 8, 8), (0, 1, 8, 8)],
    "offset % 4": [(6, 1, 8, 8)],
    "past n": [(8192 - 32, 1, 8, 8)],
    "zero taps": [(0, 0, 8, 8)],
}


@pytest.mark.parametrize("what", list(BAD_RANGES))
def test_adam_pack_rejects_bad_ranges(ops, what):
    """Through the ctypes entry point: a non-zero status, a message, and every buffer left as it was."""
    from supervised_gan_amd import _lib
    L = _lib.lib()
    n, G = 8192, Guards()
    rng = np.random.default_rng(3)
    bufs = [G.make(rng.standard_normal(n).astype(np.float32)) for _ in range(4)] + [G.make(_pattern(n)) for _ in range(4)]
    state = G.make(torch.tensor([7, 11, 13, 0], dtype=torch.int32))
    lr = G.make(np.full(1, LR, dtype=np.float32))
    before = [_bits(t).clone() for t in bufs + [state]]
    segs = BAD_RANGES[what]
    arr = (_lib.WtSeg * len(segs))(*[_lib.WtSeg(*s) for s in segs])
    ptr = [C.c_void_p(t.data_ptr()) for t in bufs]
    rc = L.sgan_adam_pack(*ptr[:4], n, C.c_void_p(lr.data_ptr()), B1, B2, EPS, C.c_void_p(state.data_ptr()), *ptr[4:], arr, len(segs), 1,
                          ops._stream())
    torch.cuda.synchronize()
    assert rc != 0 and L.sgan_last_error()
    assert all(torch.equal(_bits(t), b) for t, b in zip(bufs + [state], before)) and G.intact()


# ---- sgan_adam_multi / sgan_sgd_multi over 64 segments -------------------------------------------------------------------------
SEG_LENGTHS = [1, 2, 3, 5, 1023, 1024, 1025, 2_100_001] + [7 + 2 * i for i in range(56)]      # 2.1 M: past the bx = 1024 cap, n % 4 = 1
_MULTI = {}


def _multi_inputs():
    """64 segments in one arena per operand, each 16-byte aligned with >= 4 sentinel floats behind it."""
    if not _MULTI:
        offs, cur = [], 0
        for n in SEG_LENGTHS:
            offs.append(cur)
            cur += (n + 3) // 4 * 4 + 4
        live = np.zeros(cur, dtype=bool)
        for o, n in zip(offs, SEG_LENGTHS):
            live[o: o + n] = True
        rng = np.random.default_rng(64)
        p0 = np.full(cur, np.nan, dtype=np.float32)
        p0[live] = rng.standard_normal(int(live.sum()))
        grads = []
        for s in range(STEPS):
            g = np.full(cur, np.nan, dtype=np.float32)
            g[live] = rng.standard_normal(int(live.sum())) * 10.0 ** (s - 3)
            grads.append(g)
        _MULTI.update(offs=offs, total=cur, live=live, p0=p0, grads=grads)
        for a in (live, p0, *grads):
            a.setflags(write=False)
    return _MULTI


def _moment0(M):
    z = np.full(M["total"], np.nan, dtype=np.float32)
    z[M["live"]] = 0.0
    return z


def _dead_bits_kept(t, host0, live):
    """The sentinel floats between the segments kept their bits."""
    return np.array_equal(t.cpu().numpy().view(np.int32)[~live], host0.view(np.int32)[~live])


def test_adam_multi_64_segments(ops):
    """One sgan_adam_multi call over 64 segments (AdamGroups' path): lengths around the vector width and the block size, one past
    the grid cap whose tail block 0 handles; every segment against fp64, the floats between the segments untouched."""
    M = _multi_inputs()
    live, offs = M["live"], M["offs"]
    p, g = _dev(M["p0"]), _dev(M["grads"][0])
    m0 = _moment0(M)
    m, v = _dev(m0), _dev(m0)
    G = Guards()
    state = G.make(torch.zeros(4, dtype=torch.int32))
    lr = G.make(np.full(1, LR, dtype=np.float32))
    segs = [(p[o: o + n], g[o: o + n], m[o: o + n], v[o: o + n], n) for o, n in zip(offs, SEG_LENGTHS)]
    assert len(segs) == 64 and all(t.data_ptr() % 16 == 0 for s in segs for t in s[:4])
    for s in range(STEPS):
        g.copy_(_dev(M["grads"][s]))
        ops.adam_multi(segs, lr, B1, B2, EPS, state)
    torch.cuda.synchronize()
    assert state.cpu().tolist() == _state_words(STEPS)
    grads = [x[live] for x in M["grads"]]
    ref = A.adam_run(A.adam_step, M["p0"][live].astype(np.float64), grads, LR, B1, B2, EPS)
    f32 = A.adam_run(A.adam_step_f32, M["p0"][live], grads, LR, B1, B2, EPS)
    got = tuple(t.cpu().numpy()[live] for t in (p, m, v))
    dev, yard = A.assert_within_yardstick(got, f32, ref, "adam_multi x64")
    pos = np.cumsum([0] + SEG_LENGTHS)
    for i, n in enumerate(SEG_LENGTHS):         # the same bound, segment by segment: names the one that went wrong
        sl = slice(pos[i], pos[i + 1])
        assert np.abs(got[0][sl] - ref[0][sl]).max() <= A.YARDSTICK_FACTOR * yard[0], (i, n)
        assert np.abs(got[1][sl] - ref[1][sl]).max() <= A.YARDSTICK_FACTOR * yard[1] * np.abs(ref[1]).max(), (i, n)
        assert np.abs(got[2][sl] - ref[2][sl]).max() <= A.YARDSTICK_FACTOR * yard[2] * np.abs(ref[2]).max(), (i, n)
    assert _dead_bits_kept(p, M["p0"], live) and _dead_bits_kept(m, m0, live) and _dead_bits_kept(v, m0, live)
    assert G.intact()


def test_adam_multi_rejects_65_segments_and_misaligned_pointers(ops):
    from supervised_gan_amd._lib import SganError
    G = Guards()
    rng = np.random.default_rng(9)
    p, g, m, v = (G.make(rng.standard_normal(4096).astype(np.float32)) for _ in range(4))
    state = G.make(torch.tensor([3, 0, 0, 0], dtype=torch.int32))
    lr = G.make(np.full(1, LR, dtype=np.float32))
    before = [_bits(t).clone() for t in (p, g, m, v, state)]
    with pytest.raises(SganError, match="sgan_adam_multi"):
        ops.adam_multi([(p[16 * i: 16 * i + 16], g[16 * i: 16 * i + 16], m[16 * i: 16 * i + 16], v[16 * i: 16 * i + 16], 16) for i in range(65)],
                       lr, B1, B2, EPS, state)
    for k in range(4):                          # each operand in turn one float (4 bytes) off
        t = [p[:64], g[:64], m[:64], v[:64]]
        t[k] = (p, g, m, v)[k][1:65]
        with pytest.raises(SganError, match="aligned"):
            ops.adam_multi([(p[128:192], g[128:192], m[128:192], v[128:192], 64), (*t, 64)], lr, B1, B2, EPS, state)
    with pytest.raises(SganError, match="sgan_sgd_multi"):
        ops.sgd_multi([(p[16 * i: 16 * i + 16], g[16 * i: 16 * i + 16], None, 16) for i in range(65)], lr, 0.9)
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(t), b) for t, b in zip((p, g, m, v, state), before)) and G.intact()


def test_sgd_multi_64_segments(ops):
    """sgan_sgd_multi over the same 64 segments, momentum 0.9; every third segment has no buffer (buf=None: plain p -= lr * g even
    though the call's momentum is not 0).  Bound: the same 4 x rule against sgd_step_f32, p absolute, buf relative to max |buf|."""
    M = _multi_inputs()
    live, offs = M["live"], M["offs"]
    lr_h, mu = A.as_f32(0.05, 0.9)
    p, g = _dev(M["p0"]), _dev(M["grads"][0])
    b0 = _moment0(M)
    buf = _dev(b0)
    G = Guards()
    lr = G.make(np.full(1, lr_h, dtype=np.float32))
    has_buf = [i % 3 != 0 for i in range(64)]
    segs = [(p[o: o + n], g[o: o + n], buf[o: o + n] if hb else None, n) for o, n, hb in zip(offs, SEG_LENGTHS, has_buf)]
    for s in range(STEPS):
        g.copy_(_dev(M["grads"][s]))
        ops.sgd_multi(segs, lr, mu)
    torch.cuda.synchronize()
    mom = np.zeros(M["total"], dtype=bool)      # elements that carry momentum
    for o, n, hb in zip(offs, SEG_LENGTHS, has_buf):
        mom[o: o + n] = hb
    got_p, got_b = p.cpu().numpy(), buf.cpu().numpy()
    for sel, mu_sel, what in ((mom, mu, "momentum 0.9"), (live & ~mom, 0.0, "buf=None")):
        grads = [x[sel] for x in M["grads"]]
        ref = A.sgd_run(A.sgd_step, M["p0"][sel].astype(np.float64), grads, lr_h, mu_sel)
        f32 = A.sgd_run(A.sgd_step_f32, M["p0"][sel], grads, lr_h, mu_sel)
        got = (got_p[sel], got_b[sel]) if mu_sel else (got_p[sel],)
        dev, yard = A.deviation(got, ref), A.deviation(f32[:len(got)], ref)
        print(f"sgd_multi x64 {what}: deviation from fp64 {dev} | fp32 yardstick {yard}")
        assert all(np.isfinite(d) and d <= A.YARDSTICK_FACTOR * y for d, y in zip(dev, yard)), (what, dev, yard)
        assert float(np.abs(ref[0] - M["p0"][sel]).max()) > 0.5        # the five steps moved the parameters far beyond the bound
    assert np.array_equal(got_b.view(np.int32)[live & ~mom], b0.view(np.int32)[live & ~mom])      # no buffer: none written
    assert _dead_bits_kept(p, M["p0"], live) and _dead_bits_kept(buf, b0, live)
    assert _same_bits(g, _dev(M["grads"][-1])) and G.intact()


# ---- sgan_zero_multi ----------------------------------------------------------------------------------------------------------
ZERO_N16 = sorted({1, 2, 3, 255, 256, 257, 64 * 256 - 1, 64 * 256, 64 * 256 + 1} | {1 + 257 * i for i in range(9, 64)})


def _fenced(n_floats, value):
    """[GUARD sentinel | n_floats of `value` | GUARD sentinel] -> (buffer view, whole allocation)."""
    flat = torch.full((n_floats + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    flat[GUARD: GUARD + n_floats] = value
    return flat[GUARD: GUARD + n_floats], flat


def test_zero_multi_64_buffers(ops):
    """64 buffers from 16 B up to one 16-byte unit past a single grid pass (64 workgroups x 256 lanes x 16 B), each pre-filled and
    fenced on both sides: afterwards exactly zero, the fences intact."""
    assert len(ZERO_N16) == 64 and ZERO_N16[0] == 1 and ZERO_N16[-1] == 64 * 256 + 1
    pairs = [_fenced(4 * n16, 7.0) for n16 in ZERO_N16]
    ops.zero_multi([b for b, _ in pairs])
    torch.cuda.synchronize()
    for n16, (b, flat) in zip(ZERO_N16, pairs):
        assert not _bits(b).any(), n16
        assert bool(torch.isnan(flat[:GUARD]).all()) and bool(torch.isnan(flat[GUARD + 4 * n16:]).all()), n16


def test_zero_multi_rejects_bad_buffers(ops):
    from supervised_gan_amd import _lib
    from supervised_gan_amd._lib import SganError
    L = _lib.lib()
    b, flat = _fenced(64, 7.0)
    before = _bits(flat).clone()
    with pytest.raises(SganError, match="aligned"):
        ops.zero_multi([b[:16], b[17:21]])          # pointer 4 bytes off
    with pytest.raises(SganError, match="aligned"):
        ops.zero_multi([b[:16], b[16:19]])          # 12 bytes
    ptrs = (C.c_void_p * 65)(*[b.data_ptr()] * 65)
    nb = (C.c_int64 * 65)(*[16] * 65)
    for count in (0, 65):
        assert L.sgan_zero_multi(ptrs, nb, count, ops._stream()) != 0 and L.sgan_last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(flat), before)

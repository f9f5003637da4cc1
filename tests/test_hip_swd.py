"""The device entries of the sliced Wasserstein score (sgan_swd.hip) against the float64 yardsticks of util.py.

Bounds, with u = 2^-24 and gamma_n = n u / (1 - n u); none is fitted.

Pyramid.  The weights g[dy][dx] and 4 g[dy][dx] are exact in fp32 and, per parity class, sum to 1.  `down` is a chain of 25 FMAs: its
result differs from the exact sum by at most gamma_25 sum |w x| <= gamma_25 M, M = max |input|.  `up` is a chain of at most 9 FMAs
(error <= gamma_9 Mc, Mc = max |coarse|) and the subtraction rounds once more (u (|fine| + |up|)): together <= gamma_10 (Mf + Mc).
A whole pyramid compounds them: the Gaussian level l carries e_l <= l gamma_25 M (a convex combination passes an input error on
undiminished at most, and adds gamma_25 M), and the Laplacian level l at most e_l + e_{l+1} + gamma_10 2 M.  The comparison value is
the float64 yardstick, whose own error is 2^-29 of these.

Distances.  A projection is a chain of K FMAs over float32 normalised descriptors that the yardstick holds bit for bit, so it differs
from the float64 projection by at most gamma_K sum_k |n_ik d_jk|.  Sorting does not expand the max-norm (|sort(a) - sort(a')|_inf <=
|a - a'|_inf), the differences of the sorted values are taken exactly in fp64, and the mean of N terms in fp64 adds at most
(N + 1) 2^-53 of itself.  Per direction j: |out_j - ref_j| <= gamma_K (max_i sum_k |nA_ik d_jk| + max_i sum_k |nB_ik d_jk|)
+ (N + 2) 2^-53 ref_j, computed from the data."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from supervised_gan_amd import util as U  # noqa: E402

U32 = 2.0 ** -24


def gamma(n):
    return n * U32 / (1 - n * U32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- pyramid ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", [(16, 16), (18, 34), (64, 96)])
def test_lap_steps(dev, C, H, W):
    from supervised_gan_amd import ops
    rng = np.random.RandomState(H * 7 + C)
    x = rng.uniform(-1, 1, (C, H, W)).astype(np.float32)
    coarse = rng.uniform(-1, 1, (C, H // 2, W // 2)).astype(np.float32)
    down = ops.lap_down(_t(x, dev)).cpu().numpy().astype(np.float64)
    err = np.abs(down - U.lap_down_ref(x)).max()
    print("down %dx%dx%d: max err %.3e, bound %.3e" % (C, H, W, err, gamma(25) * np.abs(x).max()))
    assert down.shape == (C, H // 2, W // 2) and err <= gamma(25) * np.abs(x).max()
    lap = ops.lap_up_sub(_t(x, dev), _t(coarse, dev)).cpu().numpy().astype(np.float64)
    err = np.abs(lap - (x.astype(np.float64) - U.lap_up_ref(coarse))).max()
    bound = gamma(10) * (np.abs(x).max() + np.abs(coarse).max())
    print("up-sub: max err %.3e, bound %.3e" % (err, bound))
    assert err <= bound
    # a row pitch wider than the row: the planes of a wider tensor, read where they lie
    wide = torch.full((C, H, W + 5), 9.0, dtype=torch.float32, device=dev)
    wide[:, :, :W] = _t(x, dev)
    assert np.array_equal(ops.lap_down(wide[:, :, :W]).cpu().numpy().astype(np.float64), down)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W", [(16, 16), (18, 34), (64, 96)])
def test_lap_pyramid(dev, C, H, W):
    from supervised_gan_amd import ops
    x = np.random.RandomState(H + C).uniform(-1, 1, (C, H, W)).astype(np.float32)
    got = [l.cpu().numpy().astype(np.float64) for l in ops.lap_pyramid(_t(x, dev))]
    want = U.lap_pyramid_ref(x)
    assert [g.shape for g in got] == [w.shape for w in want] and len(got) == (3 if H == 64 else 1)
    M = float(np.abs(x).max())
    for l, (g, w) in enumerate(zip(got, want)):
        last = l == len(got) - 1
        bound = l * gamma(25) * M if last else (2 * l + 1) * gamma(25) * M + gamma(10) * 2 * M
        err = np.abs(g - w).max()
        print("level %d: max err %.3e, bound %.3e" % (l, err, bound))
        assert err <= bound
    if len(got) == 1:
        assert np.array_equal(got[0], x.astype(np.float64))


def test_lap_refusals(dev):
    from supervised_gan_amd import ops
    from supervised_gan_amd._lib import SganError
    with pytest.raises(SganError, match="bad shape"):
        ops.lap_down(torch.zeros((1, 15, 16), device=dev))
    with pytest.raises(SganError, match="bad shape"):
        ops.lap_down(torch.zeros((1, 2, 16), device=dev))


# ---- gather ----------------------------------------------------------------------------------------------------------------------------
def _gather_case(dev, C, H, W, yx, row0, rows, pitch=0):
    from supervised_gan_amd import ops
    rng = np.random.RandomState(C * 100 + H)
    level = rng.uniform(-1, 1, (C, H, W)).astype(np.float32)
    pos = np.array([[5, y, x] for y, x in yx], np.int32)
    pos0 = pos.copy()
    pos0[:, 0] = 0
    lev = _t(level, dev)
    if pitch:
        wide = torch.full((C, H, W + pitch), 7.0, dtype=torch.float32, device=dev)
        wide[:, :, :W] = lev
        lev = wide[:, :, :W]
    desc = torch.full((rows, C * 49), -3.0, dtype=torch.float32, device=dev)
    acc = torch.zeros(2 * C, dtype=torch.float64, device=dev)
    ops.swd_gather(lev, _t(pos, dev), desc, row0, acc)
    return level, pos0, desc.cpu().numpy(), acc.cpu().numpy()


@pytest.mark.parametrize("C,H,W,pitch", [(1, 16, 24, 0), (3, 17, 9, 3), (2, 7, 7, 0)])
def test_gather(dev, C, H, W, pitch):
    yx = [(0, 0), (0, W - 7), (H - 7, 0), (H - 7, W - 7), (0, (W - 7) // 2), (H - 7, (W - 7) // 2), ((H - 7) // 2, 0), ((H - 7) // 2, W - 7),
          ((H - 7) // 2, (W - 7) // 2), ((H - 7) // 2, (W - 7) // 2)]      # every corner and border, and one position twice
    level, pos, desc, acc = _gather_case(dev, C, H, W, yx, 3, 16, pitch)
    want, mean, std = U.swd_descriptors_ref([level], pos)
    assert np.array_equal(desc[3:3 + len(yx)], want)                      # the copy is exact
    assert np.all(desc[:3] == -3.0) and np.all(desc[3 + len(yx):] == -3.0)
    # a sum of n = 49 P fp64 terms of magnitude <= m, in any order, is within n 2^-53 n m of the exact sum: the mean within n 2^-53 m
    # (twice that: the yardstick's own sum), sumsq / n within n 2^-53 m^2 and mean^2 within 2 m times the mean's error -- 3 n 2^-53 m^2
    # for the variance, and as much again for the yardstick's
    n, m = 49 * len(yx), float(np.abs(level).max())
    got_mean, got_std = U.swd_stats_from_sums(acc, n)
    print("mean err", np.abs(got_mean - mean).max(), "var err", np.abs(got_std ** 2 - std ** 2).max())
    assert np.abs(got_mean - mean).max() <= 2 * n * 2.0 ** -53 * m
    assert np.abs(got_std ** 2 - std ** 2).max() <= 6 * n * 2.0 ** -53 * m * m
    # P = 1, into a matrix of one row
    _, _, desc1, acc1 = _gather_case(dev, C, H, W, yx[:1], 0, 1)
    assert np.array_equal(desc1, want[:1])
    v = want[:1].astype(np.float64).reshape(C, 49)
    assert np.allclose(acc1, np.concatenate([v.sum(axis=1), (v * v).sum(axis=1)]), rtol=1e-14, atol=1e-15)


def test_gather_out_of_range(dev):
    from supervised_gan_amd import ops
    from supervised_gan_amd._lib import SganError
    ops.check_metric_err(dev)
    H, W = 12, 20
    yx = [(1, 2), (H - 6, 0), (3, W - 6), (-1, 4), (2, -1), (5, 13), (1 << 20, 0)]
    level, pos, desc, acc = _gather_case(dev, 2, H, W, yx, 1, 9)
    ok = [0, 5]
    want, _, _ = U.swd_descriptors_ref([level], pos[ok])
    assert np.array_equal(desc[[1, 6]], want)
    assert np.all(desc[[2, 3, 4, 5, 7]] == 0.0) and np.all(desc[[0, 8]] == -3.0)      # zero-filled rows, nothing else touched
    v = want.astype(np.float64).reshape(2, 2, 49)
    assert np.allclose(acc, np.concatenate([v.sum(axis=(0, 2)), (v * v).sum(axis=(0, 2))]), rtol=1e-14, atol=1e-15)
    assert int(ops.metric_err(dev).item()) == 128
    with pytest.raises(SganError, match="128"):
        ops.check_metric_err(dev)
    assert int(ops.metric_err(dev).item()) == 0


# ---- distances -------------------------------------------------------------------------------------------------------------------------
def _sums(desc, C):
    v = desc.reshape(len(desc), C, 49).astype(np.float64)
    return np.concatenate([v.sum(axis=(0, 2)), (v * v).sum(axis=(0, 2))])


def _make(kind, N, K, rng):
    C = K // 49
    if kind == "random":
        return (rng.randn(N, K) * 0.3 + 0.1).astype(np.float32), (rng.randn(N, K) * 0.5 - 0.2).astype(np.float32)
    if kind in ("sorted", "reversed"):
        # rows t_i v: every projection of A ascends (or descends) with i; B interleaves and runs the other way for `reversed`
        v = rng.uniform(0.5, 1.0, K)
        t = np.arange(N, dtype=np.float64) / max(N - 1, 1) - 0.5
        a = np.outer(t, v)
        b = np.outer((t + 0.25 / max(N, 1)) * 1.5, v)
        return (a if kind == "sorted" else a[::-1]).astype(np.float32), (b if kind == "sorted" else b).astype(np.float32)
    if kind == "equal":
        row = rng.uniform(-1, 1, K).astype(np.float32)
        return np.tile(row, (N, 1)), np.tile(row[::-1].copy(), (N, 1))
    if kind == "ties":
        return rng.randint(-1, 2, (N, K)).astype(np.float32), rng.randint(-1, 2, (N, K)).astype(np.float32)
    assert kind == "constant_channel"
    a, b = (rng.randn(N, K) * 0.3).astype(np.float32), (rng.randn(N, K) * 0.4).astype(np.float32)
    a[:, (C - 1) * 49:] = 0.625
    b[:, :49] = -0.125
    return a, b


_REF = {}


def _reference(kind, N, K, J):
    """(A, B, sums, dirs, ref, bound) of a case, computed once."""
    key = (kind, N, K, J)
    if key not in _REF:
        rng = np.random.RandomState(abs(hash((N, K, J))) % (1 << 31) + len(kind))
        A, B = _make(kind, N, K, rng)
        C = K // 49
        sA, sB = _sums(A, C), _sums(B, C)
        _, dirs = U.swd_draw(11, N % 7, 1, 1, 16, 16, K, J)
        nA = U.swd_normalise_ref(A, *U.swd_stats_from_sums(sA, N * 49))
        nB = U.swd_normalise_ref(B, *U.swd_stats_from_sums(sB, N * 49))
        ref = U.swd_ref(nA, nB, dirs)
        ad = np.abs(dirs.astype(np.float64))
        bound = gamma(K) * ((np.abs(nA.astype(np.float64)) @ ad.T).max(axis=0) + (np.abs(nB.astype(np.float64)) @ ad.T).max(axis=0)) \
            + (N + 2) * 2.0 ** -53 * ref
        _REF[key] = (A, B, sA, sB, dirs, ref, bound)
    return _REF[key]


def _run(dev, case, variant):
    from supervised_gan_amd import ops
    A, B, sA, sB, dirs, ref, bound = case
    out = ops.swd_distances(_t(A, dev), _t(B, dev), _t(sA, dev), _t(sB, dev), _t(dirs, dev), variant=variant)
    return out.cpu().numpy()


def _check(dev, kind, N, K, J):
    from supervised_gan_amd import ops
    case = _reference(kind, N, K, J)
    ref, bound = case[5], case[6]
    for variant in (ops.SWD_AUTO, ops.SWD_FUSED):
        got = _run(dev, case, variant)
        assert got.dtype == np.float64 and got.shape == (J,)
        err = np.abs(got - ref)
        print("%s N %d K %d J %d variant %d: max err %.3e, bound there %.3e, ref %.3e"
              % (kind, N, K, J, variant, err.max(), bound[err.argmax()], ref[err.argmax()]))
        assert np.all(err <= bound)
        assert np.array_equal(_run(dev, case, variant), got)                # the same bits on every run
    return got


@pytest.mark.parametrize("K", [49, 147])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1000, 1024, 1025, 16384])
def test_distances_sizes(dev, N, K):
    for J in (1, 3):
        _check(dev, "random", N, K, J)


@pytest.mark.parametrize("K", [49, 147])
@pytest.mark.parametrize("N", [1000, 16384])
def test_distances_512_directions(dev, N, K):
    _check(dev, "random", N, K, 512)


@pytest.mark.parametrize("K", [49, 147])
@pytest.mark.parametrize("kind", ["sorted", "reversed", "equal", "ties", "constant_channel"])
def test_distances_inputs(dev, kind, K):
    for N in (65, 1000):
        got = _check(dev, kind, N, K, 3)
        assert np.all(np.isfinite(got)) and np.all(got >= 0)
        if kind == "equal":                                                  # one value per projection: |pA - pB|, and no sort can move it
            assert np.all(np.abs(got - _reference(kind, N, K, 3)[5]) <= _reference(kind, N, K, 3)[6])


@pytest.mark.parametrize("N,K", [(2, 49), (65, 147), (1000, 49), (1025, 147), (16384, 49)])
def test_distances_permutation_is_zero(dev, N, K):
    from supervised_gan_amd import ops
    rng = np.random.RandomState(N)
    A = (rng.randn(N, K) * 0.3 + 0.1).astype(np.float32)
    B = A[rng.permutation(N)]
    s = _sums(A, K // 49)
    _, dirs = U.swd_draw(3, 0, 1, 1, 16, 16, K, 5)
    for variant in (ops.SWD_AUTO, ops.SWD_FUSED):
        got = _run(dev, (A, B, s, s, dirs, None, None), variant)
        assert np.array_equal(got, np.zeros(5)), got


def test_distances_more_than_one_chunk_of_directions(dev):
    """J = 513: the second chunk of 512 directions holds one; its result is that of the direction run alone."""
    case = _reference("random", 65, 49, 513)
    got = _run(dev, case, 0)
    assert np.all(np.abs(got - case[5]) <= case[6])
    alone = _run(dev, case[:4] + (case[4][512:],) + (None, None), 0)
    assert np.array_equal(alone, got[512:])


def test_distances_refusals(dev):
    """N = 16385, K = 50, J = 0 and a short workspace: an error status with its reason, and nothing launched."""
    import ctypes
    from supervised_gan_amd import _lib, ops
    lib = _lib.lib()
    a = torch.zeros((16385, 147), device=dev)
    s = torch.ones(6, dtype=torch.float64, device=dev)
    d = torch.zeros((8, 147), device=dev)
    out = torch.full((8,), -1.0, dtype=torch.float64, device=dev)
    ws = torch.empty(1 << 19, dtype=torch.int64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(N, K, J, ws_bytes=ws.numel() * 8):
        p = [ctypes.c_void_p(t.data_ptr()) for t in (a, a, s, s, d)]
        rc = lib.sgan_swd_distances(*p, N, K, J, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws_bytes, 0, st)
        return rc, lib.sgan_last_error().decode()

    for args, word in (((16385, 49, 8), "N 16385"), ((64, 50, 8), "K 50"), ((64, 49, 0), "J 0"), ((64, 49, 4097), "J 4097"), ((0, 49, 8), "N 0")):
        rc, msg = call(*args)
        assert rc < 0 and word in msg and "1 <= N <= 16384" in msg, (args, rc, msg)
    rc, msg = call(64, 49, 8, ws_bytes=2 * 8 * 64 * 4 - 16)
    assert rc < 0 and "workspace" in msg and "nothing was launched" in msg
    with pytest.raises(_lib.SganError, match="49, 98 or 147"):
        ops.swd_distances(a[:64, :50].contiguous(), a[:64, :50].contiguous(), s[:2], s[:2], d[:, :50].contiguous())
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.full(8, -1.0))               # nothing was launched
    assert call(64, 49, 8, ws_bytes=2 * 8 * 64 * 4)[0] == 0                   # exactly enough
    assert np.array_equal(out.cpu().numpy(), np.zeros(8))


def test_distances_graph_capture(dev):
    from supervised_gan_amd import ops
    A, B, sA, sB, dirs, ref, bound = _reference("random", 1000, 98, 3)
    a, b, ta, tb, d = (_t(v, dev) for v in (A, B, sA, sB, dirs))
    out = torch.zeros(3, dtype=torch.float64, device=dev)
    ws = ops.swd_workspace(1000, 98, 3, dev)
    eager = ops.swd_distances(a, b, ta, tb, d).cpu().numpy()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.swd_distances(a, b, ta, tb, d, out=out, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.swd_distances(a, b, ta, tb, d, out=out, workspace=ws)
    for _ in range(2):
        out.fill_(-1.0)
        g.replay()
        assert np.array_equal(out.cpu().numpy(), eager)
    assert np.all(np.abs(eager - ref) <= bound)
    # the graph reads its inputs where they lie: other data, the same launches
    b.copy_(a)
    tb.copy_(ta)
    g.replay()
    assert np.array_equal(out.cpu().numpy(), np.zeros(3))

"""The device entries of the precision / recall / density / coverage scores (sgan_prd.hip) against the float64 yardsticks of util.py
(knn_radii_ref, prd_rows_ref, prd_scores_ref).

Exact cases.  Descriptors are integers in [-8, 8] and the statistics are sum = 0, sumsq = count, so the normalisation is the identity
and every operation of both variants is exact in fp32 (K 16^2 = 37632 < 2^24): every output equals the yardstick bit for bit.  Integer
data is full of ties and exact duplicates; these cases carry the tile edges (63, 64, 65 rows; 130 = two blocks and a short third
column step; 2049 = a one-row last block behind 32 full ones and a one-column last step), the top-k merge, the group exclusion
(a group that does not divide N included) and the tie rule of nn_idx.  On integers the all-pairs matrix is taken in int64 by the Gram
form, which is exact there, and handed to the yardsticks (tests/test_prd_host.py holds them to a triple loop).

Real-valued cases.  Bounds per pair, with u = 2^-24 and gamma_n = n u / (1 - n u); none is fitted.  The yardstick works on the float32
normalised descriptors, which the device holds bit for bit (util.swd_normalise_ref).
  direct: diff = fl(q_k - r_k) (1 rounding, squared: 2), then K FMAs: |d2' - d2| <= gamma_{K+2} d2.
  gram:   the norms are K-FMA chains (gamma_K n), their sum rounds once, q.r is a K-FMA chain (gamma_K sum |q_k r_k|) and the last FMA
          rounds once: |d2' - d2| <= gamma_{K+3} (n_q + n_r + 2 sum_k |q_k r_k|); clamping at 0 only moves towards d2 >= 0.
The k-th order statistic and the minimum of a row are 1-Lipschitz in the max-norm, so rad, nn1 and nn_d2 are held to the largest
per-pair bound of their row.  nn_idx: the device takes the argmin of its own values, so d2[idx] - b <= d2'[idx] <= d2'[j*] <= min + b:
the named column's true d2 is within 2 b of the minimum, b the row's bound.  cnt: a pair is ambiguous where |d2 - rad_j| <= the pair's
bound + the bound of rad_j (the device counts against its OWN radii, which carry that error); cnt must lie between the unambiguous hits
and those plus the ambiguous pairs.  Rows with an ambiguous pair may be at most 2 % -- else the input is a bad one and the test fails.
On the CPU, over both passes, the two inputs below give: seed 0, 0 rows of 512 with the direct bound and 1 (1 pair of 524,288) with
the looser gram bound; seed 1, 7 rows of 520 (7 pairs of 540,800) and 10 rows (10 pairs): 1.3 % and 1.9 %."""
import ctypes
import functools
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
VARIANTS = ((1, "direct"), (2, "gram"))


def gamma(n):
    return n * U32 / (1 - n * U32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _identity_stats(N, C, dev):
    """sum = 0, sumsq = count = 49 N: mean 0, std 1."""
    return _t(np.concatenate([np.zeros(C), np.full(C, 49.0 * N)]), dev)


def _int_d2(X, Y):
    X, Y = X.astype(np.int64), Y.astype(np.int64)
    return ((X * X).sum(1)[:, None] + (Y * Y).sum(1)[None, :] - 2 * X @ Y.T).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _exact_case(N, Nq, K, k, group):
    """A [N, K], B [Nq, K] integer sets; B repeats rows of A (exact hits, ties of the minimum) and A repeats rows of its own -- inside a
    group and across groups.  Returns the sets and the yardstick's results, computed once per case."""
    rng = np.random.RandomState(N * 1000 + Nq + K + k + group)
    A = rng.randint(-8, 9, size=(N, K)).astype(np.float32)
    A[N // 2] = A[0]                       # across groups (N // 2 >= group in every case below)
    A[1] = A[0]                            # inside group 0 when group > 1; a neighbour at distance 0 when group == 1
    A[N - 1] = A[N // 3]
    B = rng.randint(-8, 9, size=(Nq, K)).astype(np.float32)
    take = rng.randint(0, N, size=Nq)
    copy = rng.rand(Nq) < 0.4
    B[copy] = A[take[copy]]
    B[0] = A[0]                            # its minimum 0 is attained at columns 0, 1 and N // 2: nn_idx must say 0
    knnA = U.knn_radii_ref(A, k, group, d2=_int_d2(A, A))
    rowsB = U.prd_rows_ref(B, A, knnA[0], d2=_int_d2(B, A))
    out = dict(A=A, B=B, knnA=knnA, rowsB=rowsB)
    if Nq == N:
        knnB = U.knn_radii_ref(B, k, group, d2=_int_d2(B, B))
        rowsA = U.prd_rows_ref(A, B, knnB[0], d2=_int_d2(A, B))
        out.update(knnB=knnB, rowsA=rowsA, scores=U.prd_scores_ref(rowsB, rowsA, knnA, knnB, k))
    return out


EXACT = [  # N, Nq, K, k, group
    (9, 9, 49, 1, 1), (9, 9, 98, 3, 2), (63, 63, 98, 3, 8), (64, 64, 147, 8, 1), (65, 65, 49, 8, 8), (65, 65, 147, 1, 1),
    (130, 130, 98, 1, 8), (130, 130, 147, 3, 7), (130, 65, 49, 3, 1), (65, 130, 98, 8, 8), (2049, 2049, 49, 3, 8), (2049, 2049, 147, 8, 1),
    (2049, 2049, 98, 1, 100),
]


@pytest.mark.parametrize("N,Nq,K,k,group", EXACT)
def test_exact(dev, N, Nq, K, k, group):
    from supervised_gan_amd import ops
    c = _exact_case(N, Nq, K, k, group)
    A, B = _t(c["A"], dev), _t(c["B"], dev)
    sA, sB = _identity_stats(N, K // 49, dev), _identity_stats(Nq, K // 49, dev)
    seen = []
    for variant, name in VARIANTS:
        rad, nn1 = ops.knn_radii(A, sA, k, group, variant=variant)
        cnt, nn_d2, nn_idx = ops.prd_rows(B, A, sA, rad, variant=variant)
        got = [rad.cpu().numpy(), nn1.cpu().numpy(), cnt.cpu().numpy(), nn_d2.cpu().numpy(), nn_idx.cpu().numpy()]
        want = [c["knnA"][0], c["knnA"][1], c["rowsB"][0], c["rowsB"][1], c["rowsB"][2]]
        for what, g, w in zip(("rad", "nn1", "cnt", "nn_d2", "nn_idx"), got, want):
            assert g.shape == w.shape and np.array_equal(g.astype(np.float64), w.astype(np.float64)), (name, what, np.flatnonzero(g != w)[:5])
        assert got[1][0] == 0.0 if group == 1 else True      # row 1 copies row 0
        assert got[4][0] == 0 and got[3][0] == 0.0              # the smallest of the columns 0, 1, N // 2 that tie at 0
        if Nq == N:
            radB, nn1B = ops.knn_radii(B, sB, k, group, variant=variant)
            assert np.array_equal(radB.cpu().numpy().astype(np.float64), c["knnB"][0]) and np.array_equal(nn1B.cpu().numpy().astype(np.float64), c["knnB"][1])
            cntA, nnA, idxA = ops.prd_rows(A, B, sB, radB, variant=variant)
            assert np.array_equal(cntA.cpu().numpy(), c["rowsA"][0]) and np.array_equal(idxA.cpu().numpy(), c["rowsA"][2])
            out4 = ops.prd_finish(cnt, cntA, nnA, rad).cpu().numpy()
            assert out4.dtype == np.int64 and np.array_equal(out4, c["scores"]["counts"]), (name, out4, c["scores"]["counts"])
            assert U.prd_from_counts(out4, N, k)["density"] == c["scores"]["density"]
            got.append(out4)
        seen.append(got)
    for a, b in zip(*seen):      # the variants agree with each other
        assert np.array_equal(a, b)


def test_one_row_is_refused(dev):
    from supervised_gan_amd import ops
    from supervised_gan_amd._lib import SganError
    with pytest.raises(SganError, match="N - group"):
        ops.knn_radii(torch.zeros((1, 49), device=dev), _identity_stats(1, 1, dev), 1, 1)


# ---- real-valued ------------------------------------------------------------------------------------------------------------------------
def real_case(seed, N, K):
    """Rank-6 structure plus 0.1 noise, both sets from one mixing matrix; normalised by A's statistics.  Returns (A, B raw float32,
    stats float64 [2 C], nA, nB normalised float32)."""
    rng = np.random.RandomState(seed)
    W = rng.randn(6, K)
    A = (rng.randn(N, 6) @ W + 0.1 * rng.randn(N, K)).astype(np.float32)
    B = (rng.randn(N, 6) @ W + 0.1 * rng.randn(N, K)).astype(np.float32)
    C = K // 49
    per = A.reshape(N, C, 49).astype(np.float64)
    stats = np.concatenate([per.sum(axis=(0, 2)), (per * per).sum(axis=(0, 2))])
    mean, std = U.swd_stats_from_sums(stats, N * 49)
    return A, B, stats, U.swd_normalise_ref(A, mean, std), U.swd_normalise_ref(B, mean, std)


def pair_bounds(nQ, nR, d2, K, variant):
    """[Nq, Nr] per-pair bounds of the variant, from the data."""
    if variant == 1:
        return gamma(K + 2) * d2
    q, r = np.abs(nQ.astype(np.float64)), np.abs(nR.astype(np.float64))
    return gamma(K + 3) * ((q * q).sum(1)[:, None] + (r * r).sum(1)[None, :] + 2 * q @ r.T)


def ambiguity(nA, nB, k, group, K, variant):
    """The yardstick's side of a real-valued case: results, per-row bounds, and per pass the ambiguous pairs."""
    N = len(nA)
    g = np.arange(N) // group
    admitted = g[:, None] != g[None, :]
    out = {}
    for s, X in (("A", nA), ("B", nB)):
        d2 = U._prd_d2(X, X)
        b = pair_bounds(X, X, d2, K, variant)
        out["knn" + s] = U.knn_radii_ref(X, k, group, d2=d2)
        out["bknn" + s] = np.where(admitted, b, 0.0).max(axis=1)
    for s, Q, R in (("B", nB, nA), ("A", nA, nB)):      # rows of B against the balls of A, then the reverse
        d2 = U._prd_d2(Q, R)
        b = pair_bounds(Q, R, d2, K, variant)
        radR, bradR = out["knn" + ("A" if s == "B" else "B")][0], out["bknn" + ("A" if s == "B" else "B")]
        amb = np.abs(d2 - radR[None, :]) <= b + bradR[None, :]
        out["rows" + s] = U.prd_rows_ref(Q, R, radR, d2=d2)
        out["d2" + s], out["brow" + s], out["amb" + s] = d2, b.max(axis=1), amb
        out["sure" + s] = ((d2 <= radR[None, :]) & ~amb).sum(axis=1)
    return out


REAL = [(0, 512, 49, 3, 1), (1, 520, 147, 5, 8)]


@pytest.mark.parametrize("seed,N,K,k,group", REAL)
def test_real_valued(dev, seed, N, K, k, group):
    from supervised_gan_amd import ops
    A, B, stats, nA, nB = real_case(seed, N, K)
    dA, dB, st = _t(A, dev), _t(B, dev), _t(stats, dev)
    for variant, name in VARIANTS:
        y = ambiguity(nA, nB, k, group, K, variant)
        rows_amb = int((y["ambB"].any(axis=1) | y["ambA"].any(axis=1)).sum())
        print("%s seed %d: ambiguous pairs %d + %d, rows with one %d of %d" % (name, seed, y["ambB"].sum(), y["ambA"].sum(), rows_amb, N))
        assert rows_amb <= 0.02 * N, "a bad input: too many pairs sit on a ball's surface"
        knn = {"A": ops.knn_radii(dA, st, k, group, variant=variant), "B": ops.knn_radii(dB, st, k, group, variant=variant)}
        again = ops.knn_radii(dA, st, k, group, variant=variant)
        assert all(torch.equal(a, b) for a, b in zip(knn["A"], again))                        # the same bytes on every run
        for s in "AB":
            for what, got, want in zip(("rad", "nn1"), knn[s], y["knn" + s]):
                err = np.abs(got.cpu().numpy().astype(np.float64) - want)
                i = int((err - y["bknn" + s]).argmax())
                print("  %s %s[%s]: max err %.3e; worst row: err %.3e, bound %.3e" % (name, what, s, err.max(), err[i], y["bknn" + s][i]))
                assert np.all(err <= y["bknn" + s]), (name, what, s)
        for s, Q, R, rad in (("B", dB, dA, knn["A"][0]), ("A", dA, dB, knn["B"][0])):
            cnt, nn_d2, nn_idx = ops.prd_rows(Q, R, st, rad, variant=variant)
            cnt2, nn2, idx2 = ops.prd_rows(Q, R, st, rad, variant=variant)
            assert torch.equal(cnt, cnt2) and torch.equal(nn_d2, nn2) and torch.equal(nn_idx, idx2)
            cnt, nn_d2, nn_idx = cnt.cpu().numpy(), nn_d2.cpu().numpy().astype(np.float64), nn_idx.cpu().numpy()
            err = np.abs(nn_d2 - y["rows" + s][1])
            i = int((err - y["brow" + s]).argmax())
            print("  %s nn_d2[%s]: max err %.3e; worst row: err %.3e, bound %.3e; cnt differs from the yardstick in %d rows"
                  % (name, s, err.max(), err[i], y["brow" + s][i], int((cnt != y["rows" + s][0]).sum())))
            assert np.all(err <= y["brow" + s])
            assert np.all(cnt >= y["sure" + s]) and np.all(cnt <= y["sure" + s] + y["amb" + s].sum(axis=1))
            assert nn_idx.min() >= 0 and nn_idx.max() < N
            assert np.all(y["d2" + s][np.arange(N), nn_idx] <= y["rows" + s][1] + 2 * y["brow" + s])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from supervised_gan_amd import _lib, ops
    l = _lib.lib()
    N, K = 64, 49
    desc = torch.zeros((N, 50), dtype=torch.float32, device=dev)
    st = _identity_stats(N, 1, dev)
    ws = ops.prd_workspace(N, N, K, dev)
    wsb = ws.numel() * 8
    f = [torch.full((N,), -7.0, dtype=torch.float32, device=dev) for _ in range(3)]
    i = [torch.full((N,), -7, dtype=torch.int32, device=dev) for _ in range(3)]
    o4 = torch.full((4,), -7, dtype=torch.int64, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    knn = lambda desc_, N_, K_, k_, g_, ws_, wsb_, v_=0: l.sgan_knn_radii(desc_, p(st), N_, K_, k_, g_, p(f[0]), p(f[1]), ws_, wsb_, v_, None)      # noqa: E731
    rows = lambda q_, Nq_, Nr_, K_, ws_, wsb_, v_=0: l.sgan_prd_rows(q_, p(desc), p(st), p(f[2]), Nq_, Nr_, K_, p(i[0]), p(f[0]), p(i[1]), ws_, wsb_, v_, None)      # noqa: E731
    cases = [("K = 50", lambda: knn(p(desc), N, 50, 3, 1, p(ws), wsb), b"K in"),
             ("k = 9", lambda: knn(p(desc), N, K, 9, 1, p(ws), wsb), b"k 9"),
             ("k = 0", lambda: knn(p(desc), N, K, 0, 1, p(ws), wsb), b"k 0"),
             ("k > N - group", lambda: knn(p(desc), N, K, 3, 62, p(ws), wsb), b"N - group"),
             ("N = 16385", lambda: knn(p(desc), 16385, K, 3, 1, p(ws), 1 << 30), b"16384"),
             ("null", lambda: knn(None, N, K, 3, 1, p(ws), wsb), b"null pointer"),
             ("short workspace", lambda: knn(p(desc), N, K, 3, 1, p(ws), 16), b"workspace"),
             ("variant", lambda: knn(p(desc), N, K, 3, 1, p(ws), wsb, 3), b"variant"),
             ("rows K = 50", lambda: rows(p(desc), N, N, 50, p(ws), wsb), b"K in"),
             ("rows Nr = 16385", lambda: rows(p(desc), N, 16385, K, p(ws), 1 << 30), b"16384"),
             ("rows Nq = 0", lambda: rows(p(desc), 0, N, K, p(ws), wsb), b"16384"),
             ("rows null", lambda: rows(None, N, N, K, p(ws), wsb), b"null pointer"),
             ("rows short workspace", lambda: rows(p(desc), N, N, K, p(ws), 8 * N - 16), b"workspace"),
             ("finish null", lambda: l.sgan_prd_finish(p(i[0]), None, p(f[0]), p(f[1]), N, p(o4), None), b"null pointer"),
             ("finish N", lambda: l.sgan_prd_finish(p(i[0]), p(i[1]), p(f[0]), p(f[1]), 16385, p(o4), None), b"16384")]
    for what, call, word in cases:
        rc = call()
        assert rc < 0 and word in l.sgan_last_error(), (what, rc, l.sgan_last_error())
    assert l.sgan_prd_workspace(64, 64, 50) < 0 and l.sgan_prd_workspace(0, 64, 49) < 0 and l.sgan_prd_workspace(64, 16385, 49) < 0
    assert l.sgan_prd_workspace(16384, 16384, 147) >= 2 * 16384 * 4 and l.sgan_prd_workspace(3, 6, 49) % 16 == 0
    torch.cuda.synchronize()
    for t in f + i + [o4]:      # nothing was launched: every output still holds the sentinel
        assert bool((t == -7).all())

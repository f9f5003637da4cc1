"""CPU tests of the host yardsticks of the precision / recall / density / coverage scores (util.knn_radii_ref, prd_rows_ref,
prd_scores_ref): against a brute-force triple loop, and on hand-built sets whose answers are known -- plus the C surface of the new
entries and the option checks of swd.py --prd_k."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from supervised_gan_amd import util as U  # noqa: E402

N, K = 12, 49


def _loop_d2(x, y):
    s = 0.0
    for a, b in zip(x, y):
        s += (float(a) - float(b)) ** 2
    return s


def _loop_knn(X, k, group):
    rad, nn1 = [], []
    for i in range(len(X)):
        d = sorted(_loop_d2(X[i], X[j]) for j in range(len(X)) if j // group != i // group)
        rad.append(d[k - 1])
        nn1.append(d[0])
    return np.array(rad), np.array(nn1)


def _loop_rows(Q, R, radR):
    cnt, nn, idx = [], [], []
    for i in range(len(Q)):
        d = [_loop_d2(Q[i], R[j]) for j in range(len(R))]
        cnt.append(sum(1 for j in range(len(R)) if d[j] <= radR[j]))
        best = 0
        for j in range(1, len(R)):
            if d[j] < d[best]:
                best = j
        nn.append(d[best])
        idx.append(best)
    return np.array(cnt), np.array(nn), np.array(idx)


def _sets():
    rng = np.random.RandomState(4)
    A = rng.randint(-3, 4, size=(N, K)).astype(np.float32)      # integers: the loop and the yardstick are both exact
    A[1] = A[0]          # a duplicate inside group 0 (group = 4): must NOT give row 0 a neighbour at distance 0
    A[9] = A[4]          # a duplicate across groups: must give rows 4 and 9 one
    B = rng.randint(-3, 4, size=(N, K)).astype(np.float32)
    B[0] = A[4]          # its nearest row of A is attained at columns 4 and 9: nn_idx says 4
    return A, B


def test_knn_radii_against_the_loop():
    A, _ = _sets()
    for k, group in ((1, 1), (3, 1), (2, 4), (8, 4), (3, 5)):      # 5 does not divide 12: the last group is short
        rad, nn1 = U.knn_radii_ref(A, k, group)
        want_rad, want_nn1 = _loop_knn(A, k, group)
        assert rad.dtype == np.float64 and np.array_equal(rad, want_rad) and np.array_equal(nn1, want_nn1), (k, group)
    _, nn1 = U.knn_radii_ref(A, 1, 4)
    assert nn1[0] > 0 and nn1[1] > 0 and nn1[4] == 0 and nn1[9] == 0
    _, nn1 = U.knn_radii_ref(A, 1, 1)
    assert nn1[0] == 0 and nn1[1] == 0                             # plain self-exclusion: the copy is a neighbour
    rad2, _ = U.knn_radii_ref(np.concatenate([A[:3], A[:3]]), 2, 1)
    assert np.array_equal(rad2 > 0, [False, False, True] * 2)      # rows 0 and 1 are equal: each has three neighbours at 0 among the six; row 2 has one
    with pytest.raises(AssertionError):
        U.knn_radii_ref(A, 9, 4)                                   # k > N - group


def test_prd_rows_against_the_loop_and_the_tie_rule():
    A, B = _sets()
    radA, _ = U.knn_radii_ref(A, 3, 4)
    cnt, nn, idx = U.prd_rows_ref(B, A, radA)
    want = _loop_rows(B, A, radA)
    assert cnt.dtype == np.int64 and np.array_equal(cnt, want[0]) and np.array_equal(nn, want[1]) and np.array_equal(idx, want[2])
    assert idx[0] == 4 and nn[0] == 0 and cnt[0] >= 2               # inside the balls of rows 4 and 9 at least
    # the boundary counts: a row exactly on a ball's surface is inside
    R = np.zeros((2, K), np.float32)
    R[1, 0] = 10
    Q = np.zeros((1, K), np.float32)
    Q[0, 0] = 3
    assert U.prd_rows_ref(Q, R, np.array([9.0, 48.0]))[0].tolist() == [1]
    assert U.prd_rows_ref(Q, R, np.array([8.99, 49.0]))[0].tolist() == [1]


def _scores(A, B, k, group):
    knnA, knnB = U.knn_radii_ref(A, k, group), U.knn_radii_ref(B, k, group)
    return U.prd_scores_ref(U.prd_rows_ref(B, A, knnA[0]), U.prd_rows_ref(A, B, knnB[0]), knnA, knnB, k)


def test_prd_scores_on_hand_built_sets():
    rng = np.random.RandomState(1)
    A = rng.randn(N, K).astype(np.float32)
    s = _scores(A, A.copy(), 2, 1)
    assert s["precision"] == s["recall"] == s["coverage"] == 1.0 and s["nn_fake_real"] == 0.0 and s["nn_ratio"] == 0.0
    assert s["density"] >= 1.0 and s["counts"].dtype == np.int64 and s["counts"].tolist()[:2] == [N, N]
    far = _scores(A, A + np.float32(1000.0), 2, 1)
    assert far["precision"] == far["recall"] == far["density"] == far["coverage"] == 0.0 and far["nn_ratio"] > 1e3
    # every row of B is A's row 5: it lies in row 5's ball (precision 1); B's own radii are 0, so only A's row 5 is recalled
    one = _scores(A, np.repeat(A[5:6], N, axis=0), 2, 1)
    assert one["precision"] == 1.0 and one["recall"] == 1.0 / N and one["coverage"] >= 1.0 / N and one["nn_fake_real"] == 0.0
    # the medians are numpy's: the mean of the two middle values of an even count
    knn = (np.arange(4.0), np.array([1.0, 2.0, 4.0, 8.0]))
    rows = (np.ones(4, np.int64), np.array([0.0, 1.0, 3.0, 9.0]), np.zeros(4, np.int64))
    s = U.prd_scores_ref(rows, rows, knn, knn, 1)
    assert s["nn_fake_real"] == 2.0 and s["nn_real_real"] == 3.0 and s["nn_ratio"] == 2.0 / 3.0
    assert s["counts"].tolist() == [4, 4, 4, 2] and s["density"] == 1.0 and s["coverage"] == 0.5
    assert U.prd_ratio(0.0, 0.0) == 1.0 and U.prd_ratio(1.0, 0.0) == float("inf")


NEW = ("sgan_prd_workspace", "sgan_knn_radii", "sgan_prd_rows", "sgan_prd_finish")


def test_entry_points_are_declared_and_bound(built_lib):
    from supervised_gan_amd import _lib
    header = open(os.path.join(ROOT, "include", "sgan_hip.h")).read()
    raw = ctypes.CDLL(built_lib)
    for name in NEW:
        m = re.search(r"\b(int|int64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert m, name + " is not declared in sgan_hip.h"
        assert hasattr(raw, name), name + " is not exported"
        assert len(m.group(2).split(",")) == len(_lib.SIGNATURES[name]), name
    assert _lib.RESTYPES["sgan_prd_workspace"] is ctypes.c_int64
    for name in ("SGAN_PRD_AUTO 0", "SGAN_PRD_DIRECT 1", "SGAN_PRD_GRAM 2"):
        assert "#define " + name in header
    l = _lib.lib()
    assert l.sgan_prd_workspace(1000, 10, 49) >= 1010 * 4 and l.sgan_prd_workspace(1000, 10, 49) % 16 == 0
    for bad in ((16385, 64, 49), (64, 0, 49), (64, 64, 50), (64, 64, 196)):
        assert l.sgan_prd_workspace(*bad) < 0, bad
        assert b"1 <= N <= 16384" in l.sgan_last_error()
    # malformed arguments are refused before anything touches a device
    p = ctypes.c_void_p(64)      # never dereferenced: the checks come before any launch
    assert l.sgan_knn_radii(None, None, 64, 49, 3, 1, None, None, None, 0, 0, None) < 0 and b"null pointer" in l.sgan_last_error()
    assert l.sgan_prd_rows(p, p, p, None, 64, 64, 49, p, p, p, p, 1 << 20, 0, None) < 0 and b"null pointer" in l.sgan_last_error()
    assert l.sgan_prd_finish(p, p, p, p, 64, None, None) < 0 and b"null pointer" in l.sgan_last_error()
    assert l.sgan_knn_radii(p, p, 64, 49, 9, 1, p, p, p, 1 << 20, 0, None) < 0 and b"k 9" in l.sgan_last_error()
    assert l.sgan_knn_radii(p, p, 64, 49, 3, 0, p, p, p, 1 << 20, 0, None) < 0 and b"group 0" in l.sgan_last_error()
    assert l.sgan_knn_radii(p, p, 64, 49, 3, 62, p, p, p, 1 << 20, 0, None) < 0 and b"N - group" in l.sgan_last_error()
    assert l.sgan_knn_radii(p, p, 1, 49, 1, 1, p, p, p, 1 << 20, 0, None) < 0 and b"N - group" in l.sgan_last_error()
    assert l.sgan_knn_radii(p, p, 64, 49, 3, 1, p, p, p, 16, 0, None) < 0 and b"workspace" in l.sgan_last_error()
    assert l.sgan_knn_radii(p, p, 64, 49, 3, 1, p, p, p, 1 << 20, 3, None) < 0 and b"variant" in l.sgan_last_error()
    assert l.sgan_prd_rows(p, p, p, p, 64, 16385, 49, p, p, p, p, 1 << 40, 0, None) < 0 and b"16384" in l.sgan_last_error()
    assert l.sgan_prd_rows(p, p, p, p, 64, 64, 49, p, p, p, ctypes.c_void_p(68), 1 << 20, 0, None) < 0 and b"aligned" in l.sgan_last_error()
    assert l.sgan_prd_finish(p, p, p, p, 0, p, None) < 0 and b"16384" in l.sgan_last_error()


def test_driver_refusals(tmp_path, capsys):
    import swd
    base = ["--name", "x", "--dataroot", "synthetic", "--gpu_ids", "-1", "--checkpoints_dir", str(tmp_path), "--which_channel", "rg", "--model", "fcgan"]
    for extra, word in ((["--prd_k", "9"], "--prd_k"),
                        (["--prd_k", "-1"], "--prd_k"),
                        (["--prd_k", "3", "--how_many", "1", "--swd_patches", "16"], "N - swd_patches"),       # one image: no other image's patches
                        (["--prd_k", "8", "--how_many", "2", "--swd_patches", "7"], "14 - 7"),                  # 7 admitted neighbours
                        (["--prd_k", "3", "--how_many", "4", "--swd_patches", "16"], "GPU")):                   # accepted; the run itself needs a device
        with pytest.raises(SystemExit) as e:
            swd.main(base + extra)
        assert e.value.code == 2
        assert word in capsys.readouterr().err
    assert "set A's statistics" in swd.__doc__ and "not image features" in swd.__doc__
    text = swd.prd_summary_text([(64, 64), (32, 32)], {key: [0.5, 0.25] for key in swd.PRD_KEYS})
    assert text.splitlines()[0] == "64x64: " + " ".join("%s 0.500000" % key for key in swd.PRD_KEYS)
    assert text.splitlines()[-1].startswith("average: precision 0.375000 ")

"""The numpy Philox / Box-Muller reference (tests/philox_ref.py) against published vectors and its own invariants -- no GPU.
The GPU tests (tests/test_hip_rng.py) hold the kernels to this reference, so it has to be right on its own."""
import math

import numpy as np
import pytest

import philox_ref as P

# Random123 known-answer vectors for philox4x32-10 (kat_vectors of the Random123 distribution): counter, key, output
KAT = [((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_known_answer_vectors(ctr, key, out):
    got = P.philox4x32_10(*ctr, *key)
    assert all(g.dtype == np.uint32 and g.shape == (1,) for g in got)
    assert tuple(int(g[0]) for g in got) == out


def test_known_answer_vectors_vectorised():
    """All three at once: the rounds must not mix lanes."""
    c = [np.array([k[0][i] for k in KAT], dtype=np.uint64) for i in range(4)]
    k = [np.array([k[1][i] for k in KAT], dtype=np.uint64) for i in range(2)]
    got = np.stack(P.philox4x32_10(*c, *k), axis=1)
    assert np.array_equal(got, np.array([k[2] for k in KAT], dtype=np.uint32))


@pytest.mark.parametrize("seed,c2", [(7, 0), (0x9E3779B97F4A7C15, 1)])
def test_counter_carries_into_c1(seed, c2):
    w = P.words(seed, 2 ** 32 - 2, 4, c2)
    assert w.shape == (4, 4) and w.dtype == np.uint32
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for row, (c0, c1) in zip(w, [(0xfffffffe, 0), (0xffffffff, 0), (0, 1), (1, 1)]):
        assert np.array_equal(row, np.concatenate(P.philox4x32_10(c0, c1, c2, 0, k0, k1)))
    assert len({tuple(r) for r in w.tolist()}) == 4


def test_words_depend_on_both_key_words_and_on_c2():
    base = P.words(7, 11, 3, 0)
    assert not np.array_equal(base, P.words(7 + 2 ** 32, 11, 3, 0))      # k1
    assert not np.array_equal(base, P.words(8, 11, 3, 0))                # k0
    assert not np.array_equal(base, P.words(7, 11, 3, 1))                # c2
    assert np.array_equal(base[1:], P.words(7, 12, 2, 0))                # consecutive counters


def test_dropout_ref_edges():
    for n in (1, 5, 43):
        ones = P.dropout_ref(n, 0.0, 7, 3)
        assert ones.dtype == np.float32 and ones.shape == (n,) and np.array_equal(ones, np.ones(n, np.float32))
    m = P.dropout_ref(4096, 0.5, 7, 0)
    assert set(np.unique(m).tolist()) == {0.0, 2.0}
    m = P.dropout_ref(4096, 0.2, 7, 0)
    assert set(np.unique(m).tolist()) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(0.2)))}
    assert np.array_equal(P.dropout_ref(43, 0.5, 7, 5)[4:], P.dropout_ref(39, 0.5, 7, 6))


def test_normal_ref_bound_and_layout():
    z, rad = P.normal_ref(1 << 16, 7, 0)
    assert z.dtype == np.float64 and z.shape == rad.shape == (1 << 16,)
    assert np.isfinite(z).all() and np.abs(z).max() <= P.ZMAX and rad.max() <= P.ZMAX
    assert math.isclose(P.ZMAX, math.sqrt(-2.0 * math.log(2.0 ** -24)), rel_tol=1e-15)
    assert np.allclose(z[0::2] ** 2 + z[1::2] ** 2, rad[0::2] ** 2, rtol=1e-12, atol=1e-300)      # (cos, sin) pairs share a radius
    assert np.array_equal(rad[0::2], rad[1::2])
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    zt, _ = P.normal_ref(105, 7, 0)
    assert np.array_equal(zt, z[:105])
    z2, _ = P.normal_ref(8, 7, P.blocks(105))
    assert np.array_equal(z2, z[108:116])          # the stream after 105 values continues at block 27


def test_to_nhwc():
    flat = np.arange(3 * 7 * 5, dtype=np.float64)
    b = P.to_nhwc(flat, 3, 7, 5, 4, 7.0)
    assert b.shape == (7, 5, 4) and (b[:, :, 3] == 7.0).all()
    for c, h, w in [(0, 0, 0), (2, 6, 4), (1, 3, 2)]:
        assert b.reshape(-1)[(h * 5 + w) * 4 + c] == flat[(c * 7 + h) * 5 + w]

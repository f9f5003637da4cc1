"""Plain numpy reference of the library's random streams (csrc/sgan_ew.hip): Philox4x32-10 keyed by the 64-bit seed, counter
(c0, c1) = the 64-bit block counter, c2 = 0 for the normal fills / 1 for the dropout masks, c3 = 0; Box-Muller on top for the
normal fills.  No torch, no GPU: the tests compare the kernels with this, never the other way round."""
import math

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
C2_NORMAL, C2_DROPOUT = 0, 1
TWO_PI_F32 = np.float32(6.28318530717958647692)      # the kernel's float literal: 6.2831855f
ZMAX = math.sqrt(48.0 * math.log(2.0))               # largest Box-Muller radius: u1 = 2^-24


def _u64(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64)) & M32


def philox4x32_10(c0, c1, c2, c3, k0, k1, rounds=10):
    """Philox4x32 of Salmon et al. (Random123), vectorised: every argument a uint64 array (or scalar) holding 32-bit words.
    Returns the four output words as uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(_u64(c0), _u64(c1), _u64(c2), _u64(c3), _u64(k0), _u64(k1))
    for _ in range(rounds):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2          # 32 x 32 -> 64 bit products: exact in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def blocks(n):
    """Philox blocks (counters) that n values consume."""
    return (int(n) + 3) // 4


def words(seed, offset, nq, c2):
    """[nq, 4] uint32: the words of counters offset .. offset + nq - 1 (mod 2^64) of the stream (seed, c2)."""
    seed, offset = int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    ctr = np.uint64(offset) + np.arange(int(nq), dtype=np.uint64)        # uint64 addition wraps like the kernel's
    w = philox4x32_10(ctr & M32, ctr >> np.uint64(32), c2, 0, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(w, axis=1)


def dropout_ref(n, p, seed, offset):
    """float32[n] keep mask: 0 where the 24-bit uniform falls under p, else 1 / (1 - p) -- every step exact in float32."""
    w = words(seed, offset, blocks(n), C2_DROPOUT).reshape(-1)[:n]
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return np.where(u < np.float32(p), np.float32(0.0), keep).astype(np.float32)


def normal_ref(n, seed, offset):
    """(z, rad): float64[n] N(0, 1) values and the Box-Muller radius behind each.  The uniforms are exact; the angle is rounded to
    float32 where the kernel rounds it (one IEEE multiply); log, sqrt, cos and sin are float64."""
    w = words(seed, offset, blocks(n), C2_NORMAL)
    w1, w2 = w[:, 0::2], w[:, 1::2]                       # [nq, 2]: words (0, 1) make outputs (0, 1), words (2, 3) outputs (2, 3)
    u1 = ((w1 >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24          # (0, 1]
    u2 = (w2 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)      # [0, 1), exact in float32
    ang = (TWO_PI_F32 * u2).astype(np.float64)
    rad = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=2).reshape(-1)[:n]
    return z, np.repeat(rad, 2, axis=1).reshape(-1)[:n]


def to_nhwc(flat, C, H, W, Cs, fill):
    """The [H, W, Cs] buffer a logical [C, H, W] tensor lands in: element (c, h, w) at [(h * W + w) * Cs + c], `fill` elsewhere."""
    flat = np.asarray(flat)
    out = np.full((H, W, Cs), fill, dtype=flat.dtype)
    out[:, :, :C] = flat.reshape(C, H, W).transpose(1, 2, 0)
    return out

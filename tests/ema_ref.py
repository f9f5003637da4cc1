"""fp64 restatement of sgan_ema_multi / optim.WeightEMA in numpy, and the deviation bound the GPU tests hold the kernel to.

The update at count t = t0 + 1, t0 + 2, ... (the counter saturates at T_MAX = 2^30):

    shadow <- shadow + (1 - d_t) * (p_t - shadow),     d_t = decay                              (no warm-up)
                                                        d_t = min(decay, (1 + t) / (10 + t))     (warm-up)

Bound.  The kernel computes fl(omd * fl(p - s) + s) in fp32, omd = fl(1 - d_t) derived in fp64 and rounded once; u = 2^-24, M the
largest magnitude among the initial shadow and every p (every shadow value is a convex combination of those, so |s| <= M too):
  * fl(p - s) is off by at most u |p - s| <= 2 u M, and enters scaled by omd;
  * omd is off by at most u omd, which moves the result by at most u omd |p - s| <= 2 u omd M;
  * the fma rounds once: at most u |result| <= u M.
One update therefore commits at most (4 omd_t + 1) u M -- about 3 u max(|p|, |s|) at omd = 1/2 -- and, the recurrence
s' = d s + (1 - d) p being a contraction, scales the deviation e it inherits by d_t:  e_t <= d_t e_(t-1) + (4 omd_t + 1) u M.  Unrolled,
with omd_k prod_(j>k) d_j = prod_(j>k) d_j - prod_(j>=k) d_j telescoping to at most 1:

    e_K <= u M (K + 4 sum_k omd_k prod_(j>k) d_j) <= (K + 4) u M <= 3 K u M      for K >= 2,

which is the bound the tests use (K = 20 for the kernel, K = 3 for the trainers): |shadow_gpu - shadow_ref| <= 3 K u M per element.
decay == 1 and decay == 0 (no warm-up) are exact: the kernel leaves shadow alone, or copies p."""
import numpy as np

T_MAX = 1 << 30
U = 2.0 ** -24


def ema_decay_at(t, decay, warmup):
    """d_t of update number t (1-based)."""
    return min(float(decay), (1.0 + t) / (10.0 + t)) if warmup else float(decay)


def ema_ref(shadow, p_seq, decay, warmup, t0=0):
    """(shadow after len(p_seq) updates, counter) in fp64; `shadow` and every p are array-likes of one shape.  The C ABI takes
    `decay` as a float, so the decay that is averaged with IS the nearest float: the reference rounds it the same way."""
    decay = float(np.float32(decay))
    s = np.asarray(shadow, dtype=np.float64).copy()
    t = int(t0)
    for p in p_seq:
        t = min(t + 1, T_MAX)
        d, p = ema_decay_at(t, decay, warmup), np.asarray(p, dtype=np.float64)
        if d == 0.0:      # s + 1 * (p - s) rounds, in any precision: d = 0 is the copy it means (the kernel does the same)
            s = p.copy()
        else:
            s += (1.0 - d) * (p - s)
    return s, t


def ema_bound(shadow0, p_seq):
    """3 K u M (K = len(p_seq) >= 2): see the module docstring."""
    assert len(p_seq) >= 2
    m = max([float(np.abs(np.asarray(shadow0, dtype=np.float64)).max(initial=0.0))] +
            [float(np.abs(np.asarray(p, dtype=np.float64)).max(initial=0.0)) for p in p_seq])
    return 3.0 * len(p_seq) * U * m

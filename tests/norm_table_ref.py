"""Host reference of the finalised normalisation statistics (sgan_norm_desc.mean_rstd): float64 (mean, rstd) of every channel from
the SAME fp64 (sum, sum of squares) arrays the device reads, replicas added in the device's order.

Bound.  The device evaluates  m = s / n,  var = max(q / n - m^2, 0),  rstd = 1 / sqrt(var + eps)  in fp64 from the same sums and
rounds each result to float once.  Its fp64 value differs from this file's by a few fp64 roundings (2^-53 each: the reciprocal of
the count against the division here, the square root); rounding a value to float moves it by at most half a float ulp, and a
relative 2^-51 in front of that rounding can move the result across one rounding boundary at most.  So |device - float64| <= 1 ulp
of float at the reference value, for `mean` and `rstd` alike; no term of it comes from a measurement."""
import numpy as np

REPLICAS = 8      # SGAN_STAT_REPLICAS


def make_stats(x, sq_stride=0, rep_stride=0, split=None, pad=0.0):
    """x: float64 [count, C] samples.  Returns (buffer float64, C): sums at [c], sums of squares at [(sq_stride or C) + c]; with
    rep_stride > 0 the samples are dealt to REPLICAS copies rep_stride apart by `split` (a list of REPLICAS row-index arrays, some
    possibly empty), whose sum is the statistic.  Everything else in the buffer holds `pad` (a wider concat buffer's other values)."""
    count, C = x.shape
    sq = sq_stride or C
    width = sq + C
    if not rep_stride:
        buf = np.full(width, pad, dtype=np.float64)
        buf[:C] = x.sum(0)
        buf[sq: sq + C] = (x * x).sum(0)
        return buf
    assert rep_stride >= width
    buf = np.full(REPLICAS * rep_stride, pad, dtype=np.float64)
    for r in range(REPLICAS):
        rows = x[split[r]]
        buf[r * rep_stride: r * rep_stride + C] = rows.sum(0)
        buf[r * rep_stride + sq: r * rep_stride + sq + C] = (rows * rows).sum(0)
    return buf


def mean_rstd_f64(buf, C, count, eps, sq_stride=0, rep_stride=0):
    """float64 [C, 2] from the sums in `buf` (the copies added first to last, as the device adds them)."""
    sq = sq_stride or C
    s, q = buf[:C].copy(), buf[sq: sq + C].copy()
    if rep_stride:
        for r in range(1, REPLICAS):
            s += buf[r * rep_stride: r * rep_stride + C]
            q += buf[r * rep_stride + sq: r * rep_stride + sq + C]
    m = s / count
    var = np.maximum(q / count - m * m, 0.0)
    return np.stack([m, 1.0 / np.sqrt(var + np.float64(np.float32(eps)))], 1)


def ulps(got_f32, ref_f64):
    """|got - ref| in float ulps at the reference value."""
    ref32 = ref_f64.astype(np.float32)
    return np.abs(got_f32.astype(np.float64) - ref_f64) / np.spacing(np.abs(ref32)).astype(np.float64)

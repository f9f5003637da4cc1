"""Plain numpy reference of the reflection-pad and norm-backward kernels of csrc/sgan_ew.hip (sg_pad_reflect_fwd_kernel,
sg_pad_reflect_bwd_kernel, sg_norm_bwd_apply_kernel, sg_norm_apply_fwd_kernel, sg_norm_apply_bwd_sums_kernel, sg_add_act_kernel,
sg_tanh_bwd_kernel).  No torch, no autograd, no GPU: the tests compare the kernels with this, never the other way round
(tests/test_pad_norm_ref_host.py holds it to torch.nn.functional and torch.autograd on its own).

Every function takes `dtype`.  np.float64 is the reference: the operation itself.  np.float32 is the YARDSTICK: the same formula in
the order the kernel's source writes it, every intermediate rounded to float32 (no FMA).  It is no second implementation to test;
its distance from the float64 result on the very inputs of a GPU run says how far a correct fp32 kernel may be from float64
(`within_yardstick`: YARDSTICK_FACTOR x that distance, as tests/adam_ref.py does for the optimizer).

Arrays are NHWC, [H, W, C] with C the stored channel count; statistics are (sum, sum of squares) in one float64 array, the squares
`sq_stride` doubles behind the sums (0: C), optionally kept in `replicas` copies `rep` doubles apart that add up (sg_stat_sum).
mean / rstd are formed in float64 by both (sg_mean_rstd); the yardstick rounds them to float32 as the kernels do, the reference
keeps them -- so the kernels' rounding of the coefficients is inside the yardstick, and the reference is the exact operation."""
import numpy as np

YARDSTICK_FACTOR = 4.0      # FMA contraction and a different order of a few additions (the margin of tests/adam_ref.py)
ACT_NONE, ACT_RELU, ACT_LRELU = "none", "relu", "lrelu"
U32 = 2.0 ** -24            # unit roundoff of float32


def stat_sum(base, off, C, rep=0, replicas=1):
    """sg_stat_sum for the channels [off, off + C): the copies added in order, in float64."""
    base = np.asarray(base, dtype=np.float64)
    v = base[off: off + C].copy()
    if rep:
        for r in range(1, replicas):
            v = v + base[off + r * rep: off + r * rep + C]
    return v


def mean_rstd(stats, count, eps, C, sq_stride=0, rep=0, replicas=1, out_dtype=np.float32):
    """sg_mean_rstd (sgan_common.h): float64 sums, var = max(q / M - m^2, 0), rstd = 1 / sqrt(var + eps), ALWAYS computed in float64
    (eps as the float the C ABI carries) and then cast to float32, as the kernel does.  out_dtype=np.float64 keeps the uncast pair:
    what the float64 reference of the functions below uses."""
    s = stat_sum(stats, 0, C, rep, replicas)
    q = stat_sum(stats, sq_stride if sq_stride else C, C, rep, replicas)
    inv = 1.0 / float(count)
    m = s * inv
    var = np.maximum(q * inv - m * m, 0.0)
    rstd = 1.0 / np.sqrt(var + float(np.float32(eps)))
    return m.astype(out_dtype), rstd.astype(out_dtype)


def _coef(C, stats, gamma, beta, count, eps, sq_stride, rep, replicas, dtype):
    """(mean, rstd, gamma, beta) in `dtype`; no statistics: (0, 1, 1, 0) -- the identity every kernel substitutes."""
    if stats is None:
        return np.zeros(C, dtype), np.ones(C, dtype), np.ones(C, dtype), np.zeros(C, dtype)
    mean, rstd = mean_rstd(stats, count, eps, C, sq_stride, rep, replicas, out_dtype=dtype)
    g = np.ones(C, dtype) if gamma is None else np.asarray(gamma, dtype=np.float32).astype(dtype)
    b = np.zeros(C, dtype) if beta is None else np.asarray(beta, dtype=np.float32).astype(dtype)
    return mean, rstd, g, b


def act_fwd(y, act, slope, dtype):
    if act == ACT_RELU:
        return np.where(y > 0, y, dtype(0))
    if act == ACT_LRELU:
        return np.where(y > 0, y, y * dtype(np.float32(slope)))
    return y


def act_grad(y, act, slope, dtype):
    if act == ACT_RELU:
        return np.where(y > 0, dtype(1), dtype(0))
    if act == ACT_LRELU:
        return np.where(y > 0, dtype(1), dtype(np.float32(slope)))
    return np.ones_like(y)


def refl(i, n):
    """nn.ReflectionPad2d's source index: -i for i < 0, 2 (n - 1) - i for i >= n."""
    i = np.asarray(i)
    return np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))


def pad_sources(H, W, pad):
    """(sy, sx): for every padded row / column the interior row / column it mirrors."""
    return refl(np.arange(H + 2 * pad) - pad, H), refl(np.arange(W + 2 * pad) - pad, W)


def ring(H, W, pad):
    """Boolean [H + 2 pad, W + 2 pad]: the padded rows and columns (the border ring around the interior)."""
    m = np.ones((H + 2 * pad, W + 2 * pad), dtype=bool)
    m[pad: pad + H, pad: pad + W] = False
    return m


def pad_reflect_fwd(x, pad, stats=None, gamma=None, beta=None, count=1, eps=1e-5, act=ACT_NONE, slope=0.0, mask=None, sq_stride=0,
                    rep=0, replicas=1, dtype=np.float64):
    """out[H + 2p, W + 2p, C] = mask[src] * act(x[src] * sc + sh), sc = gamma * rstd, sh = beta - mean * sc, as an explicit gather."""
    x = np.asarray(x, dtype=np.float32).astype(dtype)
    H, W, C = x.shape
    sy, sx = pad_sources(H, W, pad)
    v = x[sy[:, None], sx[None, :], :]
    if stats is not None:
        mean, rstd, g, b = _coef(C, stats, gamma, beta, count, eps, sq_stride, rep, replicas, dtype)
        sc = g * rstd
        sh = b - mean * sc
        v = v * sc + sh
    v = act_fwd(v, act, slope, dtype)
    if mask is not None:
        v = v * np.asarray(mask, dtype=np.float32).astype(dtype)[sy[:, None], sx[None, :], :]
    assert v.dtype == dtype
    return v


def xhat_y(x, C, stats, gamma, beta, count, eps, sq_stride, rep, replicas, dtype):
    """(xhat, y) as the backward kernels form them: xhat = (x - mean) * rstd, y = gamma * xhat + beta (no statistics: y = xhat = x)."""
    mean, rstd, g, b = _coef(C, stats, gamma, beta, count, eps, sq_stride, rep, replicas, dtype)
    xhat = (x - mean) * rstd
    y = g * xhat + b if stats is not None else x
    return xhat, y


def fold(dout, H, W, pad, dtype=np.float64):
    """The adjoint of the reflection gather as a scatter-add: every padded position adds its value to the interior pixel it mirrors."""
    dout = np.asarray(dout).astype(dtype)
    sy, sx = pad_sources(H, W, pad)
    d = np.zeros((H, W, dout.shape[2]), dtype=dtype)
    yy, xx = np.meshgrid(sy, sx, indexing="ij")
    np.add.at(d, (yy.reshape(-1), xx.reshape(-1)), dout.reshape(-1, dout.shape[2]))
    return d


def pad_reflect_bwd(dout, pad, x=None, stats=None, gamma=None, beta=None, count=1, eps=1e-5, act=ACT_NONE, slope=0.0, mask=None,
                    sq_stride=0, rep=0, replicas=1, dtype=np.float64):
    """(din, s1, s2, terms_abs): din = act'(y) * mask * fold(dout); s1 = sum din, s2 = sum din * xhat per channel (the products in
    `dtype`, the sums in float64 as the kernel's fp64 atomics); terms_abs = sum |dout| over the positions folded into each element
    (float64).  Without x there is no act' and s1 = s2 = None."""
    dout32 = np.asarray(dout, dtype=np.float32)
    Hp, Wp, C = dout32.shape
    H, W = Hp - 2 * pad, Wp - 2 * pad
    d = fold(dout32, H, W, pad, dtype)
    terms_abs = fold(np.abs(dout32), H, W, pad, np.float64)
    if mask is not None:
        d = d * np.asarray(mask, dtype=np.float32).astype(dtype)
    s1 = s2 = None
    if x is not None:
        x = np.asarray(x, dtype=np.float32).astype(dtype)
        xhat, y = xhat_y(x, C, stats, gamma, beta, count, eps, sq_stride, rep, replicas, dtype)
        d = d * act_grad(y, act, slope, dtype)
        s1 = d.astype(np.float64).sum((0, 1))
        s2 = (d * xhat).astype(np.float64).sum((0, 1))
    assert d.dtype == dtype
    return d, s1, s2, terms_abs


def norm_bwd(d, x, stats, gamma, count, eps, s1, s2, sq_stride=0, rep=0, replicas=1, dtype=np.float64):
    """(dx, dgamma, dbeta): dx = gamma * rstd * (d - s1 / M - xhat * s2 / M) with M the pixel count of d; dgamma = s2, dbeta = s1.
    s1 / M and s2 / M are formed in float64 and rounded once by the kernel (the yardstick does the same)."""
    d = np.asarray(d).astype(dtype)           # the kernel reads an fp32 buffer; a float64 d (the reference chain) is taken as it is
    x = np.asarray(x, dtype=np.float32).astype(dtype)
    H, W, C = d.shape
    mean, rstd, g, _ = _coef(C, stats, gamma, None, count, eps, sq_stride, rep, replicas, dtype)
    inv_m = 1.0 / float(H * W)
    c1 = (np.asarray(s1, dtype=np.float64) * inv_m).astype(dtype)
    c2 = (np.asarray(s2, dtype=np.float64) * inv_m).astype(dtype)
    a = g * rstd
    xhat = (x - mean) * rstd
    dx = a * (d - c1 - xhat * c2)
    assert dx.dtype == dtype
    return dx, np.asarray(s2, dtype=np.float64).astype(dtype), np.asarray(s1, dtype=np.float64).astype(dtype)


def norm_apply_fwd(u, stats, gamma, beta, count, eps, mask=None, noise=None, sigma=0.0, sq_stride=0, dtype=np.float64):
    """t = ((u - mean) * (gamma * rstd) + beta) * mask + sigma * noise."""
    u = np.asarray(u, dtype=np.float32).astype(dtype)
    C = u.shape[2]
    mean, rstd, g, b = _coef(C, stats, gamma, beta, count, eps, sq_stride, 0, 1, dtype)
    t = (u - mean) * (g * rstd) + b
    if mask is not None:
        t = t * np.asarray(mask, dtype=np.float32).astype(dtype)
    if noise is not None:
        t = t + dtype(np.float32(sigma)) * np.asarray(noise, dtype=np.float32).astype(dtype)
    assert t.dtype == dtype
    return t


def norm_apply_bwd_sums(dt, u, stats, count, eps, mask=None, sq_stride=0, dtype=np.float64):
    """(dt * mask, s1, s2, abs1, abs2): s1 = sum dt * mask, s2 = sum dt * mask * xhat per channel, summed in float64 from terms formed
    in `dtype`; abs1, abs2 = the sums of the terms' magnitudes (float64), for the a-priori bound of an fp32 summation in any grouping."""
    dt = np.asarray(dt, dtype=np.float32).astype(dtype)
    u = np.asarray(u, dtype=np.float32).astype(dtype)
    C = dt.shape[2]
    if mask is not None:
        dt = dt * np.asarray(mask, dtype=np.float32).astype(dtype)
    xhat, _ = xhat_y(u, C, stats, None, None, count, eps, sq_stride, 0, 1, dtype)
    t2 = dt * xhat
    assert t2.dtype == dtype
    d64, t64 = dt.astype(np.float64), t2.astype(np.float64)
    return dt, d64.sum((0, 1)), t64.sum((0, 1)), np.abs(d64).sum((0, 1)), np.abs(t64).sum((0, 1))


def kink_margin(x, stats=None, gamma=None, beta=None, count=1, eps=1e-5, sq_stride=0):
    """min |y| over all elements in float64, y = gamma * xhat + beta (no statistics: y = x): how far the data stays from the kink
    of ReLU / LeakyReLU, where two fp32 evaluations of y could fall on different sides."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    _, y = xhat_y(x, x.shape[2], stats, gamma, beta, count, eps, sq_stride, 0, 1, np.float64)
    return float(np.abs(y).min())


def add_act(a, b, tanh, dtype=np.float64):
    s = np.asarray(a, dtype=np.float32).astype(dtype) + np.asarray(b, dtype=np.float32).astype(dtype)
    return np.tanh(s) if tanh else s


def tanh_bwd(dy, y, dtype=np.float64):
    dy, y = np.asarray(dy, dtype=np.float32).astype(dtype), np.asarray(y).astype(dtype)
    return dy * (dtype(1) - y * y)


def stats_of(x, width=None, offset=0):
    """(sum, sum of squares) over H, W of the float32 values of x, float64, as the conv epilogues accumulate them: a 2 * width
    array (width: the channel count, or a wider arena) with the channels at `offset` -- read it as stats[offset:] with
    sq_stride = width."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    C = x.shape[2]
    width = C if width is None else width
    st = np.zeros(2 * width, dtype=np.float64)
    st[offset: offset + C] = x.sum((0, 1))
    st[width + offset: width + offset + C] = (x * x).sum((0, 1))
    return st


def deviation(a, b, sel=None):
    """max |a - b| in float64 (over the boolean / index selection `sel` when given)."""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    if sel is not None:
        d = d[sel]
    return float(d.max()) if d.size else 0.0


def within_yardstick(got, ref32, ref64, what, sel=None, floor=0.0):
    """The kernel's result must stay within YARDSTICK_FACTOR x the distance of the float32 restatement from float64, on the same
    inputs and the same elements (`floor`: a rounding the yardstick cannot contain, e.g. the order of fp64 atomics; stated by the
    caller).  Prints both figures and returns them."""
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got if sel is None else got[sel]).all(), f"{what}: not finite"
    dev, yard = deviation(got, ref64, sel), deviation(ref32, ref64, sel)
    print(f"{what}: kernel {dev:.3e} from fp64 | fp32 yardstick {yard:.3e}")
    assert dev <= YARDSTICK_FACTOR * yard + floor, f"{what}: {dev:.3e} from fp64, the fp32 yardstick is {yard:.3e} (floor {floor:.1e})"
    return dev, yard

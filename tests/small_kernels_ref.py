"""Plain numpy references of the small kernels of csrc/sgan_ew.hip that every trainer's step runs through: the layout boundary
(sg_to_nhwc_kernel, sg_planes_to_nhwc4_kernel, sg_concat_nhwc_kernel, sg_slice_nhwc_kernel), the elementwise kernels (sigmoid
forward / backward, tanh backward, add + activation), sg_bn_running_kernel and sg_sgd_kernel.  float64 where there is arithmetic,
index arithmetic where there is none; neither torch nor the library is imported.  tests/test_small_kernels_ref_host.py holds these
functions to torch on the CPU; tests/test_hip_small_kernels.py compares the kernels with them (Adam: tests/adam_ref.py).

Also here, because both of those files need the very same ones: the inputs of the two kernels whose error budget is measured on the
reference side (`sigmoid_inputs`, `add_tanh_inputs`), and the ulp arithmetic of that budget (`ulp_error`, `ulp_budget`)."""
import numpy as np

U = 2.0 ** -24                                   # unit roundoff of float32 (round to nearest)
MIN_NORMAL = float(np.finfo(np.float32).tiny)    # 2^-126: the absolute floor that allows a denormal flush on either side

# ---- layout -------------------------------------------------------------------------------------------------------------------


def to_nhwc_ref(src, Cstore):
    """Logical [C, H, W] array -> [H, W, Cstore], zeros in channels C .. Cstore - 1 (sgan_to_nhwc)."""
    src = np.asarray(src)
    C, H, W = src.shape
    assert C <= Cstore
    out = np.zeros((H, W, Cstore), dtype=src.dtype)
    for c in range(C):
        out[:, :, c] = src[c]
    return out


def concat_ref(a, Ca, b, Cb, Cstore):
    """Padded NHWC [..., >= Ca] and [..., >= Cb] -> [..., Cstore]: channels a[0:Ca], b[0:Cb], then zeros (sgan_concat_nhwc)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape[:-1] == b.shape[:-1] and a.shape[-1] >= Ca and b.shape[-1] >= Cb and Cstore >= Ca + Cb
    out = np.zeros(a.shape[:-1] + (Cstore,), dtype=a.dtype)
    for c in range(Ca):
        out[..., c] = a[..., c]
    for c in range(Cb):
        out[..., Ca + c] = b[..., c]
    return out


def slice_ref(src, c0, C, Cstore):
    """Channels [c0, c0 + C) of a padded NHWC array as [..., Cstore], zeros behind them (sgan_slice_nhwc)."""
    src = np.asarray(src)
    assert 0 <= c0 and c0 + C <= src.shape[-1] and Cstore >= C
    out = np.zeros(src.shape[:-1] + (Cstore,), dtype=src.dtype)
    for c in range(C):
        out[..., c] = src[..., c0 + c]
    return out


# ---- elementwise --------------------------------------------------------------------------------------------------------------
def _f64(a):
    return np.asarray(a, dtype=np.float64)


def sigmoid_ref(x):
    """1 / (1 + exp(-x)) in float64, written so that neither branch overflows."""
    x = _f64(x)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def sigmoid_bwd_ref(dp, p):
    dp, p = _f64(dp), _f64(p)
    return dp * p * (1.0 - p)


def tanh_bwd_ref(dy, y):
    dy, y = _f64(dy), _f64(y)
    return dy * (1.0 - y * y)


def add_act_ref(a, b, tanh):
    s = _f64(a) + _f64(b)
    return np.tanh(s) if tanh else s


# ---- BatchNorm running statistics ---------------------------------------------------------------------------------------------
def bn_running_ref(stats, C, count, sq_stride, rep_stride, replicas, rm, rv, momentum):
    """One momentum update of (running_mean, running_var), float64.  `stats`: the float64 arena as the kernel sees it from its
    first element on -- channel sums at [0, C), sums of squares at [sq, sq + C) with sq = sq_stride or C, and, when rep_stride > 0,
    `replicas` copies rep_stride doubles apart that are summed.  Returns (new running_mean, new running_var, mean, unbiased var)."""
    stats = _f64(stats)
    sq = sq_stride if sq_stride else C
    reps = replicas if rep_stride else 1
    s = np.zeros(C)
    q = np.zeros(C)
    for r in range(reps):
        s = s + stats[r * rep_stride: r * rep_stride + C]
        q = q + stats[r * rep_stride + sq: r * rep_stride + sq + C]
    mean = s / count
    var = np.maximum(q / count - mean * mean, 0.0)
    var = var * (count / (count - 1.0) if count > 1 else 1.0)
    mom = float(momentum)
    return (1.0 - mom) * _f64(rm) + mom * mean, (1.0 - mom) * _f64(rv) + mom * var, mean, var


# ---- SGD ----------------------------------------------------------------------------------------------------------------------
def sgd_step_ref(p, g, buf, lr, mu):
    """One step of torch.optim.SGD (dampening 0, no Nesterov, no weight decay) in float64 from the given state.  With mu != 0 and a
    buffer: g' = mu * buf + g, buf = g'; otherwise g' = g and the buffer (None or not) is returned as it came.  p - lr * g'.
    Returns (p, buf, g')."""
    p, g = _f64(p), _f64(g)
    if mu != 0 and buf is not None:
        g = mu * _f64(buf) + g
        buf = g
    return p - lr * g, buf, g


# ---- the budget of the kernels that go through expf / tanhf --------------------------------------------------------------------
SIGMOID_PLANTED = np.array([0.0, 1e-8, -1e-8, 17, -17, 30, -30, 88, -88, 89, -89, 104, -104, 1e30, -1e30], dtype=np.float32)
SIGMOID_NPIX = (1, 255, 257, 256 * 256 + 3)                                  # the last: past the 256-workgroup cap
EW_SIZES = (4, 1020, 1024, 1028, 4 * (2048 * 256) + 4)                       # the last: past the 2048-workgroup cap
TANH_PLANTED = np.array([0.0, 1e-8, -1e-8, 0.5, -0.5, 9.0, -9.0, 20.0, -20.0, 100.0, -100.0], dtype=np.float32)


def sigmoid_inputs(npix):
    """fp32 logits of a sigmoid case: normal * 4, as many of the planted values as fit in front."""
    rng = np.random.default_rng(1000 + npix)
    x = (rng.standard_normal(npix) * 4.0).astype(np.float32)
    k = min(npix, len(SIGMOID_PLANTED))
    x[:k] = SIGMOID_PLANTED[:k]
    return x


def add_tanh_inputs(n):
    """(a, b) of an add + tanh case: normal * 1.5 each; the planted sums in front (a = the value, b = 0)."""
    rng = np.random.default_rng(2000 + n)
    a = (rng.standard_normal(n) * 1.5).astype(np.float32)
    b = (rng.standard_normal(n) * 1.5).astype(np.float32)
    k = min(n, len(TANH_PLANTED))
    a[:k] = TANH_PLANTED[:k]
    b[:k] = 0.0
    return a, b


def ulp_error(got, ref):
    """|got - ref| in float32 ulps of the float64 reference, elementwise, after the absolute floor of one minimum normal has been
    taken off (so a result below 2^-126 may be flushed on either side at no cost)."""
    got, ref = _f64(got), _f64(ref)
    ulp = _f64(np.spacing(np.maximum(np.abs(ref), MIN_NORMAL).astype(np.float32)))
    return np.maximum(np.abs(got - ref) - MIN_NORMAL, 0.0) / ulp


def ulp_budget(f32_eval, ref):
    """The budget of a kernel that goes through the device's expf / tanhf: 4 x the largest error (ulp_error) that the float32
    evaluation `f32_eval` of the same expression by another implementation (torch on the CPU) shows against the float64 reference
    on the same inputs; at least 2 ulp.  Computed from the reference side only."""
    return max(2.0, 4.0 * float(ulp_error(f32_eval, ref).max()))

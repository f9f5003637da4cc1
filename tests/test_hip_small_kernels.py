"""The small kernels of csrc/sgan_ew.hip that every trainer's step runs through, each against the plain references of
tests/small_kernels_ref.py (Adam: tests/adam_ref.py): the layout boundary (sg_to_nhwc_kernel, both paths of
sg_planes_to_nhwc4_kernel -- also as the H2D copy of a pinned host batch --, sg_concat_nhwc_kernel, sg_slice_nhwc_kernel), the
elementwise kernels (sgan_scale, sgan_add_act_fwd, sgan_tanh_bwd, sgan_sigmoid_fwd / _bwd), sg_bn_running_kernel, sg_sgd_kernel
and the unfused sg_adam_kernel with its n & 3 tail.

Every output lies in storage that is larger than the kernel may touch and starts as a NaN sentinel (SENT): afterwards everything
beyond Cstore inside a pixel (dst_ld > Cstore) and beyond the last pixel still holds the sentinel's bits, and the padding channels
inside the write region are +0.0, bit for bit.  Every source ends in SLACK readable floats and carries NaN in the channels nobody
should read.

Bounds (u = 2^-24, the unit roundoff of fp32; none of them is measured on a kernel):
  layout, sgan_scale, sgan_add_act_fwd(ACT_NONE)   bit for bit (numpy.array_equal on the fp32 bytes)
  sgan_tanh_bwd      |out - ref| <= 4 u |dy|                      three roundings of quantities bounded by |dy|, since |y| <= 1
  sgan_sigmoid_bwd   |out - ref| <= 4 u |ref| + 2^-126            three roundings; the floor allows a denormal flush on either side
  running stats      |out - ref| <= 4 u (|old| + |new|)           one cast and three fp32 roundings, and that of 1 - momentum
  sgan_sgd_multi     |p - ref| <= 3 u (|p0| + lr |g'|),  |buf - ref| <= 2 u (|mu buf0| + |g|), each step from the read-back state.
                     Rounding by rounding the p error is at most u (|p0| + 3 lr |g'| + lr |mu buf0|) when no product is contracted
                     into an FMA, which is inside the bound wherever lr |mu buf0| <= 2 |p0|: the inputs keep |p0| >= 2 and the
                     test asserts that condition on every step's read-back state.
  sgan_adam_multi    adam_ref.assert_within_yardstick, the bound of tests/test_hip_adam_pack.py, unchanged
  sgan_sigmoid_fwd, sgan_add_act_fwd(ACT_TANH)   in fp32 ulps of the fp64 reference: 4 x the largest error of torch's CPU fp32
                     evaluation of the same expression on the same inputs, at least 2 ulp, plus the 2^-126 floor
                     (small_kernels_ref.ulp_budget; tests/test_small_kernels_ref_host.py keeps it <= 16 ulp).
Budgets as observed (pytest -s prints them beside the kernel's own error):
  sgan_sigmoid_fwd               npix 1: 2.00 (the floor)   255: 5.54   257: 5.33   65 539: 7.64 ulp;   the kernel itself: at most 2.01 ulp
  sgan_add_act_fwd(ACT_TANH)     n 4: 2.00 (the floor)   1020: 3.60   1024: 4.89   1028: 3.67   2 097 156: 5.73 ulp;   the kernel: at most 1.62 ulp
  (torch's CPU kernels differ between hosts: another CPU showed 6.97 for 255 pixels and 5.99 for the largest tanh case)

That the file can fail: one-line changes to a scratch copy of sgan_ew.hip, one at a time, each keeping every access in bounds, and
the tests of this file that fail with the library built from it:
  * fast path's store with pl[1][i] and pl[2][i] swapped: test_planes_fast_path_small (Creal 2, 3, 4; with one channel both planes
    are zero), test_planes_fast_path_stride_loop, test_planes_channel_slice_on_the_fast_path,
    test_pinned_host_batch_into_a_channel_slice[5-8-3] and [6-8-4]
  * fast path's stride gridDim.x * 257: test_planes_fast_path_stride_loop
  * fast path's stride gridDim.x * 255: NO test fails, and none can: a stride below the thread count skips nothing.  Thread t visits
    t + k S' with S' < S, S the number of threads; every integer is t + k S' for some t in [0, S), so every group is still written,
    some of them twice with the same value.  The result is bit-identical and only the run time differs; 257 is the neighbour that
    does skip groups.
  * sg_concat_nhwc_kernel reads pb[c] for pb[c - Ca]: all 48 cases of test_concat, test_concat_and_slice_past_the_block_cap, all 6
    of test_concat_slice_round_trip
  * running variance without `unb`: test_bn_running_update_16_layers[0.1] and [1.0]
  * rep_stride ignored, replica 0 only: test_bn_running_update_16_layers[0.1] and [1.0], test_bn_running_update_clamps_a_negative_variance
  * SGD writes S.m[e] before g is added: test_sgd_64_segments_some_without_a_buffer, test_sgd_64_segments_all_with_a_buffer,
    test_sgd_grid_stride_loop
  * Adam tail for threadIdx.x < ((S.n & 3) - 1): test_adam_multi_tails
  * sigmoid forward's padding loop from c = 2: the 24 cases of test_sigmoid_fwd with pld 4 or 5
"""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_ref as A
import small_kernels_ref as R

pytestmark = pytest.mark.gpu

U = R.U
SENT = 0x7FC5A5A5          # a quiet NaN with a payload: what every output byte holds before the call
POISON = 0x7FC1B2B3        # another: what source channels hold that nobody should read
TAIL = 1024                # sentinel floats behind the last pixel of every output
SLACK = 64                 # readable floats behind every source


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import _lib, ops
    _lib.lib()
    return ops


def _L():
    from supervised_gan_amd import _lib
    return _lib.lib()


def _P(t):
    return C.c_void_p(t.data_ptr())


def _ok(rc):
    assert rc == 0, _L().sgan_last_error()


def _filled(n, bits):
    return torch.full((n,), bits, dtype=torch.int32, device="cuda").view(torch.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def pad4(c):
    return (c + 3) // 4 * 4


class Out:
    """`npix` pixels of `ld` floats and TAIL more, all SENT."""

    def __init__(self, npix, ld):
        self.npix, self.ld = npix, ld
        self.flat = _filled(npix * ld + TAIL, SENT)

    def view(self, H, W, C0=None):
        assert H * W == self.npix
        return self.flat[: self.npix * self.ld].view(H, W, self.ld)[..., :C0]

    def read(self, Cstore, Creal):
        """[npix, Creal] fp32 as written, after the three region assertions: the sentinel beyond Cstore inside every pixel and beyond
        the last pixel, +0.0 in the padding channels Creal .. Cstore - 1."""
        torch.cuda.synchronize()
        got = self.flat.cpu().numpy().view(np.int32)
        body = got[: self.npix * self.ld].reshape(self.npix, self.ld)
        assert (got[self.npix * self.ld:] == SENT).all(), "written beyond the last pixel"
        assert (body[:, Cstore:] == SENT).all(), "written beyond Cstore inside a pixel"
        assert not body[:, Creal:Cstore].any(), "a padding channel is not +0.0"
        return np.ascontiguousarray(body[:, :Creal]).view(np.float32)

    def check_exact(self, want, Cstore, Creal):
        """want: [..., Cstore] reference; the Creal data channels bit for bit."""
        w = _bits(want).reshape(self.npix, Cstore)
        assert not w[:, Creal:].any()
        got = self.read(Cstore, Creal).view(np.int32)
        assert np.array_equal(got, w[:, :Creal]), f"{int((got != w[:, :Creal]).sum())} data words differ"


def _src(data, ld):
    """[..., C] host data -> device [..., ld] view of storage that holds POISON in channels C .. ld - 1 and SLACK floats behind."""
    data = np.asarray(data, dtype=np.float32)
    lead, Cn = data.shape[:-1], data.shape[-1]
    npix = int(np.prod(lead))
    host = np.full((npix * ld + SLACK,), POISON, dtype=np.int32).view(np.float32)
    host[: npix * ld].reshape(npix, ld)[:, :Cn] = data.reshape(npix, Cn)
    return _dev(host)[: npix * ld].view(*lead, ld)


def _normal(seed, *shape):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


# ---- sgan_to_nhwc -------------------------------------------------------------------------------------------------------------
def _takes_planes_kernel(src, out, Cstore):
    return src.stride(2) == 1 and Cstore == 4 and out.ld % 4 == 0 and out.flat.data_ptr() % 16 == 0


def _fast_conditions(src):
    """The four conditions of the 16-byte path of sg_planes_to_nhwc4_kernel, one flag each."""
    return (src.shape[2] % 4 == 0, src.stride(1) % 4 == 0, src.stride(0) % 4 == 0, src.data_ptr() % 16 == 0)


def _to_nhwc(ops, src, out, Cstore):
    """src: logical [C, H, W] tensor of any strides (device, or pinned host)."""
    Cr, H, W = src.shape
    _ok(_L().sgan_to_nhwc(_P(src), src.stride(0), src.stride(1), src.stride(2), H, W, Cr, _P(out.flat), out.ld, Cstore, ops._stream()))


def _check_to_nhwc(ops, src, dst_ld, Cstore, planes, fast=None):
    Cr, H, W = src.shape
    out = Out(H * W, dst_ld)
    assert _takes_planes_kernel(src, out, Cstore) == planes
    if planes:
        assert _fast_conditions(src) == fast, _fast_conditions(src)
    _to_nhwc(ops, src, out, Cstore)
    out.check_exact(R.to_nhwc_ref(src.cpu().numpy(), Cstore), Cstore, Cr)


ALL4 = (True, True, True, True)


@pytest.mark.parametrize("dst_ld", [4, 8])
@pytest.mark.parametrize("Creal", [1, 2, 3, 4])
def test_planes_fast_path_small(ops, Creal, dst_ld):
    _check_to_nhwc(ops, _dev(_normal(Creal, Creal, 5, 8)), dst_ld, 4, True, ALL4)


def test_planes_fast_path_stride_loop(ops):
    """1024 x 2052: 525 312 four-pixel groups for 2048 x 256 threads: the capped grid walks its stride loop."""
    H, W = 1024, 2052
    assert H * W > 4 * 2048 * 256
    _check_to_nhwc(ops, _dev(_normal(11, 3, H, W)), 4, 4, True, ALL4)


def test_planes_fast_path_broadcast_plane(ops):
    """An expanded source (plane stride 0): every channel reads the same plane."""
    src = _dev(_normal(12, 1, 5, 8)).expand(3, 5, 8)
    assert src.stride(0) == 0
    _check_to_nhwc(ops, src, 4, 4, True, ALL4)


def _scalar_case(name):
    """(source, the flags of _fast_conditions it must show): the scalar path reached one condition at a time."""
    if name == "W%4":
        return _dev(_normal(20, 3, 7, 11)), None
    if name == "row_stride":
        return _dev(_normal(21, 3, 6, 10))[..., :8], (True, False, True, True)
    if name == "plane_stride":
        base = _dev(_normal(22, 3 * 42 + 8))
        return base.as_strided((3, 5, 8), (42, 8, 1)), (True, True, False, True)
    if name == "misaligned":
        return _dev(_normal(23, 3, 5, 12))[..., 1:9], (True, True, True, False)
    if name == "channel_slice":
        return _dev(_normal(24, 1, 4, 7, 11))[0, 1:3], None
    if name == "stride_loop":
        return _dev(_normal(25, 2, 725, 725)), None
    raise KeyError(name)


@pytest.mark.parametrize("dst_ld", [4, 8])
@pytest.mark.parametrize("name", ["W%4", "row_stride", "plane_stride", "misaligned", "channel_slice", "stride_loop"])
def test_planes_scalar_path(ops, name, dst_ld):
    src, flags = _scalar_case(name)
    if flags is None:
        flags = _fast_conditions(src)
        assert not flags[0]                       # W % 4 != 0 (the channel slice of a 7 x 11 batch is misaligned as well)
    if name == "stride_loop":
        assert src.shape[1] * src.shape[2] > 2048 * 256
    _check_to_nhwc(ops, src, dst_ld, 4, True, flags)


def test_planes_channel_slice_on_the_fast_path(ops):
    """t[:, 1:3] of a batch whose planes are a multiple of 16 bytes: the slice starts aligned and stays on the 16-byte path."""
    _check_to_nhwc(ops, _dev(_normal(26, 1, 4, 6, 8))[0, 1:3], 4, 4, True, ALL4)


@pytest.mark.parametrize("H,W,Creal", [(5, 8, 3), (7, 11, 2), (6, 8, 4), (33, 64, 1)])
def test_pinned_host_batch_into_a_channel_slice(ops, H, W, Creal):
    """ops.host_batch_to_nhwc of a pinned host batch (the kernel is the H2D copy) into channels 0..3 of an [H, W, 8] buffer:
    dst_ld = 8, channels 4..7 keep the sentinel."""
    t = torch.empty(1, Creal, H, W, dtype=torch.float32).pin_memory()
    t.copy_(torch.from_numpy(_normal(30 + H, 1, Creal, H, W)))
    assert t.is_pinned()
    out = Out(H * W, 8)
    ops.host_batch_to_nhwc(t, out.view(H, W, 4))
    out.check_exact(R.to_nhwc_ref(t[0].numpy(), 4), 4, Creal)


def _generic_source(kind, Cr, H, W):
    if kind == "permuted":          # [H, W, C] storage seen as [C, H, W]: sw = C
        src = _dev(_normal(40 + Cr, H, W, Cr + 1))[..., :Cr].permute(2, 0, 1)
    elif kind == "transposed":      # [C, W, H] storage: sw = H, sh = 1
        src = _dev(_normal(41 + Cr, Cr, W, H)).permute(0, 2, 1)
    else:                           # expanded along W: sw = 0
        src = _dev(_normal(42 + Cr, Cr, H, 1)).expand(Cr, H, W)
        assert src.stride(2) == 0
    assert src.stride(2) != 1
    return src


@pytest.mark.parametrize("dst_ld", [8, 11])
@pytest.mark.parametrize("kind", ["permuted", "transposed", "expanded"])
@pytest.mark.parametrize("Cr", [1, 5, 8])
@pytest.mark.parametrize("H,W", [(7, 11), (363, 362)])
def test_generic_to_nhwc(ops, H, W, Cr, kind, dst_ld):
    """sg_to_nhwc_kernel, Cstore = 8; 363 x 362 x 8 = 1 051 248 elements for 4096 x 256 threads: the stride loop."""
    if (H, W) == (363, 362):
        assert H * W * 8 > 4096 * 256
    _check_to_nhwc(ops, _generic_source(kind, Cr, H, W), dst_ld, 8, False)


def test_generic_to_nhwc_unit_stride_sources_that_miss_the_planes_kernel(ops):
    """sw == 1 but Cstore != 4, or a destination stride that is no multiple of 4: the generic kernel, same result."""
    _check_to_nhwc(ops, _dev(_normal(50, 5, 9, 11)), 8, 8, False)
    _check_to_nhwc(ops, _dev(_normal(51, 3, 9, 11)), 5, 4, False)
    _check_to_nhwc(ops, _dev(_normal(52, 3, 9, 11)), 3, 3, False)


# ---- sgan_concat_nhwc / sgan_slice_nhwc ---------------------------------------------------------------------------------------
PAIRS = [(1, 1), (1, 3), (3, 1), (2, 3), (4, 4), (3, 6)]


def _concat(ops, a, Ca, b, Cb, npix, out, Cstore):
    _ok(_L().sgan_concat_nhwc(_P(a), a.stride(-2), Ca, _P(b), b.stride(-2), Cb, npix, _P(out.flat), out.ld, Cstore, ops._stream()))


def _slice(ops, src, c0, Cn, npix, out, Cstore):
    _ok(_L().sgan_slice_nhwc(_P(src), src.stride(-2), c0, Cn, npix, _P(out.flat), out.ld, Cstore, ops._stream()))


@pytest.mark.parametrize("wide_a,extra", [(False, 0), (True, 0), (False, 3), (True, 4)])
@pytest.mark.parametrize("npix", [35, 323])
@pytest.mark.parametrize("Ca,Cb", PAIRS)
def test_concat(ops, Ca, Cb, npix, wide_a, extra):
    """Source pixel strides larger than the channel counts (b's at least Ca + Cb), dst_ld = Cstore + extra."""
    ha, hb = _normal(60 + Ca, npix, Ca), _normal(70 + Cb, npix, Cb)
    a, b = _src(ha, Ca + 3 if wide_a else pad4(Ca)), _src(hb, Ca + Cb + 1)
    Cs = pad4(Ca + Cb)
    out = Out(npix, Cs + extra)
    _concat(ops, a, Ca, b, Cb, npix, out, Cs)
    out.check_exact(R.concat_ref(ha, Ca, hb, Cb, Cs), Cs, Ca + Cb)


@pytest.mark.parametrize("extra", [0, 4])
@pytest.mark.parametrize("c0", [0, 1, 3])
@pytest.mark.parametrize("npix", [35, 323])
@pytest.mark.parametrize("Ca,Cb", PAIRS)
def test_slice(ops, Ca, Cb, npix, c0, extra):
    total = Ca + Cb
    if c0 >= total:
        c0 = total - 1                       # (1, 1) has no channel 3: its last one
    Cn = min(max(Ca, Cb), total - c0)
    hs = _normal(80 + total, npix, total)
    src = _src(hs, total + 2)
    Cs = pad4(Cn)
    out = Out(npix, Cs + extra)
    _slice(ops, src, c0, Cn, npix, out, Cs)
    out.check_exact(R.slice_ref(hs, c0, Cn, Cs), Cs, Cn)


def test_slice_into_a_callers_wider_out(ops):
    """ops.slice_nhwc(out=...): an `out` wider than pad4(Cn) is zero-filled to its width; an `out` that is itself the channel slice
    of a wider buffer leaves the rest of that buffer alone."""
    H, W, Cn, c0 = 9, 13, 3, 2
    hs = _normal(90, H, W, 7)
    src = _src(hs, 8)
    wide = Out(H * W, 12)
    ops.slice_nhwc(src, c0, Cn, out=wide.view(H, W))
    wide.check_exact(R.slice_ref(hs, c0, Cn, 12), 12, Cn)
    part = Out(H * W, 12)
    ops.slice_nhwc(src, c0, Cn, out=part.view(H, W, 8))
    part.check_exact(R.slice_ref(hs, c0, Cn, 8), 8, Cn)


def test_concat_and_slice_past_the_block_cap(ops):
    """npix = 1025 x 1024 for 4096 x 256 threads: both kernels walk their stride loop."""
    npix = 1025 * 1024
    assert npix > 4096 * 256
    ha, hb = _normal(91, npix, 2), _normal(92, npix, 3)
    a, b = _src(ha, 4), _src(hb, 6)
    out = Out(npix, 12)
    _concat(ops, a, 2, b, 3, npix, out, 8)
    out.check_exact(R.concat_ref(ha, 2, hb, 3, 8), 8, 5)
    del out
    sl = Out(npix, 4)
    _slice(ops, b, 1, 2, npix, sl, 4)
    sl.check_exact(R.slice_ref(hb, 1, 2, 4), 4, 2)


@pytest.mark.parametrize("Ca,Cb", PAIRS)
def test_concat_slice_round_trip(ops, Ca, Cb):
    """Through the ops wrappers on padded buffers as the discriminators hold them: slice(concat(a, b)) is a and b, bit for bit."""
    H, W = 17, 19
    ha, hb = _normal(100 + Ca, H, W, Ca), _normal(110 + Cb, H, W, Cb)
    a, b = _src(ha, pad4(Ca)), _src(hb, pad4(Cb))
    cat = ops.concat_nhwc(a, Ca, b, Cb)
    assert cat.shape == (H, W, pad4(Ca + Cb))
    sa, sb = ops.slice_nhwc(cat, 0, Ca), ops.slice_nhwc(cat, Ca, Cb)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(cat.cpu().numpy()), _bits(R.concat_ref(ha, Ca, hb, Cb, pad4(Ca + Cb))))
    assert np.array_equal(_bits(sa.cpu().numpy()), _bits(R.slice_ref(ha, 0, Ca, pad4(Ca))))
    assert np.array_equal(_bits(sb.cpu().numpy()), _bits(R.slice_ref(hb, 0, Cb, pad4(Cb))))


# ---- elementwise: flat kernels ------------------------------------------------------------------------------------------------
def _flat_out(n):
    o = Out(n, 1)
    return o, o.flat[:n]


@pytest.mark.parametrize("gout", [0.7, -1.3, 0.0, 1e-40], ids=["pos", "neg", "zero", "denormal"])
@pytest.mark.parametrize("n", R.EW_SIZES)
def test_scale_bit_exact(ops, n, gout):
    """One correctly rounded product per element: bit for bit against numpy fp32 (a denormal factor gives denormal products)."""
    g = _normal(120 + n % 97, n)
    s = np.float32(gout)
    assert gout != 1e-40 or (s != 0 and abs(s) < np.finfo(np.float32).tiny)
    out, dx = _flat_out(n)
    ops.scale(_dev(np.array(s)), _dev(g), dx)
    out.check_exact((g * s).reshape(n, 1), 1, 1)


@pytest.mark.parametrize("n", R.EW_SIZES)
def test_add_bit_exact(ops, n):
    a, b = _normal(130 + n % 97, n), _normal(131 + n % 97, n)
    a[:3], b[:3] = (1e-40, -1.0, 0.0), (2e-40, 1.0, -0.0)
    out, o = _flat_out(n)
    ops.add_act_fwd(_dev(a), _dev(b), o, act=0)
    out.check_exact((a + b).reshape(n, 1), 1, 1)


def _cpu_f32_add_tanh(a, b):
    return torch.tanh(torch.from_numpy(a) + torch.from_numpy(b)).numpy()


def _cpu_f32_sigmoid(x):
    t = torch.from_numpy(x)
    return (1.0 / (1.0 + torch.exp(-t))).numpy()


@pytest.mark.parametrize("n", R.EW_SIZES)
def test_add_tanh_within_the_reference_side_budget(ops, n):
    a, b = R.add_tanh_inputs(n)
    ref = R.add_act_ref(a, b, True)
    budget = R.ulp_budget(_cpu_f32_add_tanh(a, b), ref)
    out, o = _flat_out(n)
    ops.add_act_fwd(_dev(a), _dev(b), o)
    got = out.read(1, 1)[:, 0]
    err = R.ulp_error(got, ref)
    print(f"add+tanh n={n}: kernel {err.max():.2f} ulp, budget {budget:.2f} ulp")
    assert budget <= 16.0 and np.isfinite(got).all() and err.max() <= budget, (int(err.argmax()), float(err.max()), budget)
    assert np.abs(got).max() <= 1.0


@pytest.mark.parametrize("n", R.EW_SIZES)
def test_tanh_bwd(ops, n):
    rng = np.random.default_rng(140 + n % 97)
    y = rng.uniform(-1, 1, n).astype(np.float32)
    dy = (rng.standard_normal(n) * 3).astype(np.float32)
    planted = np.array([1.0, -1.0, 1 - 2.0 ** -24, -(1 - 2.0 ** -24), 0.0], dtype=np.float32)
    k = min(n, len(planted))
    y[:k] = planted[:k]
    if n > 8:
        y[-3:] = (0.0, -1.0, 1.0)          # the last chunk as well
    out, dx = _flat_out(n)
    ops.tanh_bwd(_dev(dy), _dev(y), dx)
    got = out.read(1, 1)[:, 0]
    ref = R.tanh_bwd_ref(dy, y)
    assert (np.abs(got.astype(np.float64) - ref) <= 4 * U * np.abs(dy.astype(np.float64))).all()
    assert (got[np.abs(y) == 1.0] == 0.0).all() and (np.abs(y) == 1.0).sum() >= 2
    assert np.array_equal(got[y == 0.0], dy[y == 0.0])


# ---- elementwise: the standalone sigmoid on strided one-channel maps ------------------------------------------------------------
def _strided(vals, ld):
    """A [1, npix, 1] view with pixel stride ld over storage that holds POISON everywhere else (and SLACK floats behind)."""
    n = len(vals)
    host = np.full((n * ld + SLACK,), POISON, dtype=np.int32).view(np.float32)
    host[: n * ld: ld] = vals
    return _dev(host).as_strided((1, n, 1), (n * ld, ld, 1))


def _pixels(out):
    return out.flat.as_strided((1, out.npix, 1), (out.npix * out.ld, out.ld, 1))


@pytest.mark.parametrize("pld", [1, 4, 5])
@pytest.mark.parametrize("ld", [1, 4, 5])
@pytest.mark.parametrize("npix", R.SIGMOID_NPIX)
def test_sigmoid_fwd(ops, npix, ld, pld):
    """The whole pld floats of every pixel are the write region: channel 0, then zeros.  65 539 pixels: past the 256-block cap."""
    x = R.sigmoid_inputs(npix)
    ref = R.sigmoid_ref(x)
    budget = R.ulp_budget(_cpu_f32_sigmoid(x), ref)
    out = Out(npix, pld)
    ops.sigmoid_fwd(_strided(x, ld), _pixels(out))
    got = out.read(pld, 1)[:, 0]
    err = R.ulp_error(got, ref)
    print(f"sigmoid npix={npix} ld={ld} pld={pld}: kernel {err.max():.2f} ulp, budget {budget:.2f} ulp")
    assert budget <= 16.0 and np.isfinite(got).all() and err.max() <= budget, (int(err.argmax()), float(err.max()), budget)
    assert (got[x <= -104] == 0.0).all()
    assert (np.abs(got[x >= 17].astype(np.float64) - 1.0) <= budget * 2.0 ** -23).all() and got.max() <= 1.0 and got.min() >= 0.0


def test_sigmoid_fwd_every_planted_logit(ops):
    """All of x in {0, +-1e-8, +-17, +-30, +-88, +-89, +-104, +-1e30} are among the inputs of the 255-pixel case and up."""
    for npix in R.SIGMOID_NPIX[1:]:
        assert np.array_equal(R.sigmoid_inputs(npix)[: len(R.SIGMOID_PLANTED)], R.SIGMOID_PLANTED)
    assert (R.sigmoid_ref(np.float64(-104.0)) < 2.0 ** -150) and R.sigmoid_inputs(1)[0] == 0.0


P_PLANTED = np.array([0.0, 1.0, 0.5, 2.0 ** -30, 1 - 2.0 ** -24], dtype=np.float32)
BWD_CASES = [(257, a, b, c) for a in (1, 4, 5) for b in (1, 4, 5) for c in (1, 4, 5)] + [(256 * 256 + 3, 1, 1, 1), (256 * 256 + 3, 5, 4, 5)]


@pytest.mark.parametrize("npix,dpld,pld,dxld", BWD_CASES)
def test_sigmoid_bwd(ops, npix, dpld, pld, dxld):
    rng = np.random.default_rng(150 + npix + 9 * dpld + 3 * pld + dxld)
    p = rng.uniform(0, 1, npix).astype(np.float32)
    dp = (rng.standard_normal(npix) * 2).astype(np.float32)
    p[: len(P_PLANTED)] = P_PLANTED
    p[-len(P_PLANTED):] = P_PLANTED
    out = Out(npix, dxld)
    ops.sigmoid_bwd(_strided(dp, dpld), _strided(p, pld), _pixels(out))
    got = out.read(dxld, 1)[:, 0]
    ref = R.sigmoid_bwd_ref(dp, p)
    assert (np.abs(got.astype(np.float64) - ref) <= 4 * U * np.abs(ref) + R.MIN_NORMAL).all()
    assert (got[(p == 0.0) | (p == 1.0)] == 0.0).all()


# ---- sgan_bn_running_update ---------------------------------------------------------------------------------------------------
BN_C = [1, 3, 8, 255, 256, 257, 513] * 2 + [8, 513]
BN_COUNTS = [1, 2, 256, 262144]


def _exact_parts(rng, total, reps):
    """`total` (multiples of 1/64, small) as `reps` addends that are multiples of 1/64 themselves: every partial sum is exact."""
    parts = rng.integers(-64, 65, size=(reps,) + total.shape) / 64.0
    parts[-1] = total - parts[:-1].sum(0)
    return parts


def _bn_layers(reps_built):
    """16 layers: (C, count, sq_stride, rep_stride, reps, float64 stats arena, has_counter)."""
    rng = np.random.default_rng(77)
    layers = []
    for i, Cn in enumerate(BN_C):
        count = BN_COUNTS[(i + i // 4) % 4]
        sq = 0 if i % 2 == 0 else Cn + 5
        sqe = sq or Cn
        rep = 0 if i % 5 == 4 else 2 * sqe + 3
        reps = reps_built if rep else 1
        stats = rng.standard_normal((reps - 1) * rep + 2 * sqe) * 1e3          # whatever lies between the live slots is junk
        if count == 1:         # one value per channel: sum^2 == sumsq exactly, so that the variance is exactly 0 on both sides
            mean = rng.integers(-256, 257, Cn) / 8.0
            s_parts, q_parts = _exact_parts(rng, mean, reps), _exact_parts(rng, mean * mean, reps)
        else:
            mean, var = rng.standard_normal(Cn) * 2 + 1, rng.uniform(0.5, 4.0, Cn)
            w = rng.dirichlet(np.ones(reps))[:, None] if reps > 1 else np.ones((1, 1))
            s_parts, q_parts = w * (count * mean), w[::-1] * (count * (var + mean * mean))
        for r in range(reps):
            stats[r * rep: r * rep + Cn] = s_parts[r]
            stats[r * rep + sqe: r * rep + sqe + Cn] = q_parts[r]
        layers.append((Cn, count, sq, rep, reps, stats, i % 3 != 0))
    return layers


def _bn_state(layers):
    rng = np.random.default_rng(78)
    rms, rvs, nbts = [], [], []
    for i, (Cn, *_rest, has_nbt) in enumerate(layers):
        rm, rv = _flat_out(Cn), _flat_out(Cn)
        rm[1].copy_(_dev(rng.standard_normal(Cn).astype(np.float32)))
        rv[1].copy_(_dev(rng.uniform(0.5, 2.0, Cn).astype(np.float32)))
        rms.append(rm)
        rvs.append(rv)
        nbts.append(torch.tensor([1000 * i + 5, 0x5A5A5A5A], dtype=torch.int64, device="cuda") if has_nbt else None)
    return rms, rvs, nbts


def _bn_check(what, got, old, blend, new, mom):
    if mom == 0.0:
        assert np.array_equal(_bits(got), _bits(old)), f"{what}: momentum 0 changed the buffer"
    elif mom == 1.0:
        assert np.array_equal(got, new.astype(np.float32)), f"{what}: momentum 1 is not the cast of the new value"
    bound = 4 * U * (np.abs(old.astype(np.float64)) + np.abs(new))
    bad = np.abs(got.astype(np.float64) - blend) > bound
    assert not bad.any(), f"{what}: channel {int(bad.argmax())} is {got[bad.argmax()]} for {blend[bad.argmax()]}"


@pytest.mark.parametrize("momentum", [0.0, 0.1, 1.0])
def test_bn_running_update_16_layers(ops, momentum):
    """One launch over a full table, three times: every layer against bn_running_ref from the read-back state of that launch."""
    reps = ops.stat_replicas()
    assert reps > 1
    layers = _bn_layers(reps)
    assert len(layers) == 16 and {la[1] for la in layers} == set(BN_COUNTS) and {la[0] for la in layers} == set(BN_C)
    assert any(la[3] == 0 for la in layers) and any(la[2] for la in layers) and any(not la[6] for la in layers)
    mom = float(np.float32(momentum))                 # what crosses the C ABI
    stats = [_dev(la[5]) for la in layers]
    rms, rvs, nbts = _bn_state(layers)
    for launch in range(3):
        old = [(rm[1].cpu().numpy(), rv[1].cpu().numpy()) for rm, rv in zip(rms, rvs)]
        ops.bn_running_update([(st, rm[1], rv[1], nbt, la[0], la[1], la[2], la[3])
                               for st, rm, rv, nbt, la in zip(stats, rms, rvs, nbts, layers)], momentum)
        for i, (la, rm, rv, nbt) in enumerate(zip(layers, rms, rvs, nbts)):
            Cn, count, sq, rep, _, host, _ = la
            want_m, want_v, mean, var = R.bn_running_ref(host, Cn, count, sq, rep, reps, old[i][0], old[i][1], mom)
            what = f"launch {launch} layer {i} (C={Cn}, count={count}, sq={sq}, rep={rep})"
            _bn_check(what + " mean", rm[0].read(1, 1)[:, 0], old[i][0], want_m, mean, mom)
            _bn_check(what + " var", rv[0].read(1, 1)[:, 0], old[i][1], want_v, var, mom)
            if nbt is not None:
                assert nbt.cpu().tolist() == [1000 * i + 5 + launch + 1, 0x5A5A5A5A], what


def test_bn_running_update_clamps_a_negative_variance(ops):
    """sumsq / count = mean^2 - 100 (mean = 1e4: 1e-6 below, relatively): variance 0, not -100."""
    reps = ops.stat_replicas()
    Cn, count = 3, 256
    rep = 2 * Cn + 1
    rng = np.random.default_rng(79)
    host = np.zeros((reps - 1) * rep + 2 * Cn)
    s_parts = _exact_parts(rng, np.full(Cn, count * 1e4), reps)                  # integers and 64ths: every sum is exact
    q_parts = _exact_parts(rng, np.full(Cn, count * (1e8 - 100.0)), reps)
    for r in range(reps):
        host[r * rep: r * rep + Cn] = s_parts[r]
        host[r * rep + Cn: r * rep + 2 * Cn] = q_parts[r]
    st = _dev(host)
    rm, rv = _flat_out(Cn), _flat_out(Cn)
    for mom in (0.1, 1.0):
        rm[1].fill_(0.5)
        rv[1].fill_(1.0)
        ops.bn_running_update([(st, rm[1], rv[1], None, Cn, count, 0, rep)], mom)
        m32 = float(np.float32(mom))
        want_m, want_v, mean, var = R.bn_running_ref(host, Cn, count, 0, rep, reps, np.full(Cn, 0.5), np.ones(Cn), m32)
        assert np.array_equal(mean, np.full(Cn, 1e4)) and not var.any()
        _bn_check(f"clamp mean, momentum {mom}", rm[0].read(1, 1)[:, 0], np.full(Cn, 0.5, np.float32), want_m, mean, m32)
        _bn_check(f"clamp var, momentum {mom}", rv[0].read(1, 1)[:, 0], np.ones(Cn, np.float32), want_v, var, m32)
    assert not _bits(rv[0].read(1, 1)).any()          # momentum 1: the running variance is the clamped variance, +0.0


# ---- sgan_sgd_multi -----------------------------------------------------------------------------------------------------------
SGD_LENGTHS = [1, 2, 3, 5, 255, 256, 257, 1023, 1025, 4099]


def _cut(lengths):
    """Segment offsets inside one arena, none a multiple of 4, at least two dead floats between neighbours."""
    offs, cur = [], 1
    for n in lengths:
        offs.append(cur)
        cur += n + 2
        if cur % 4 == 0:
            cur += 1
    return offs, cur + 8


def _arena(total, live, values):
    a = np.full(total, SENT, dtype=np.int32).view(np.float32)
    a[live] = values
    return a


def _run_sgd(ops, lengths, has_buf, mu, steps, seed):
    lr_h, mu_h = A.as_f32(0.05, mu)
    offs, total = _cut(lengths)
    assert all(o % 4 for o in offs)
    live, mom, seg_of = np.zeros(total, dtype=bool), np.zeros(total, dtype=bool), np.full(total, -1)
    for i, (o, n, hb) in enumerate(zip(offs, lengths, has_buf)):
        live[o: o + n] = True
        mom[o: o + n] = hb and mu_h != 0
        seg_of[o: o + n] = i
    nl = int(live.sum())
    rng = np.random.default_rng(seed)
    p0 = _arena(total, live, (np.where(rng.random(nl) < 0.5, -1, 1) * (2 + np.abs(rng.standard_normal(nl)))).astype(np.float32))
    b0 = _arena(total, live, rng.standard_normal(nl).astype(np.float32))
    p, buf, g = _dev(p0), _dev(b0), _filled(total, SENT)
    lr = _dev(np.full(1, lr_h, dtype=np.float32))
    segs = [(p[o: o + n], g[o: o + n], buf[o: o + n] if hb else None, n) for o, n, hb in zip(offs, lengths, has_buf)]
    hp, hb_ = p0, b0
    for s in range(steps):
        hg = _arena(total, live, rng.standard_normal(nl).astype(np.float32))
        g.copy_(_dev(hg))
        ops.sgd_multi(segs, lr, mu)
        torch.cuda.synchronize()
        gp, gb = p.cpu().numpy(), buf.cpu().numpy()
        assert np.array_equal(_bits(gp)[~live], _bits(hp)[~live]) and np.array_equal(_bits(gb)[~mom], _bits(hb_)[~mom]), \
            f"step {s}: a dead float, or a buffer that takes no part, was written"
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(hg)), "the gradient was written"
        # the condition under which the p bound is derived (module docstring)
        assert (lr_h * np.abs(mu_h * hb_[mom].astype(np.float64)) <= 2 * np.abs(hp[mom])).all()
        for sel, m_sel in ((mom, mu_h), (live & ~mom, 0.0)):
            if not sel.any():
                continue
            p_old, b_old, gs = hp[sel].astype(np.float64), hb_[sel].astype(np.float64), hg[sel].astype(np.float64)
            rp, rb, gq = R.sgd_step_ref(p_old, gs, b_old if m_sel else None, lr_h, m_sel)
            bad = np.abs(gp[sel] - rp) > 3 * U * (np.abs(p_old) + lr_h * np.abs(gq))
            assert not bad.any(), f"step {s}: p of segment {seg_of[sel][bad.argmax()]} (mu {m_sel})"
            if m_sel:
                bad = np.abs(gb[sel] - rb) > 2 * U * (np.abs(m_sel * b_old) + np.abs(gs))
                assert not bad.any(), f"step {s}: buf of segment {seg_of[sel][bad.argmax()]}"
            assert np.abs(rp - p_old).max() > 1e-3        # the step is far above the bound
        hp, hb_ = gp, gb


def _lengths64():
    rng = np.random.default_rng(64)
    ln = SGD_LENGTHS * 6 + SGD_LENGTHS[:4]
    rng.shuffle(ln)
    return [int(n) for n in ln]


def test_sgd_64_segments_some_without_a_buffer(ops):
    """mu = 0.9, every third segment passes buf = None: plain descent there, its slice of the buffer arena untouched."""
    ln = _lengths64()
    assert len(ln) == 64 and set(ln) == set(SGD_LENGTHS)
    _run_sgd(ops, ln, [i % 3 != 0 for i in range(64)], 0.9, 3, 200)


def test_sgd_64_segments_all_with_a_buffer(ops):
    ln = _lengths64()
    _run_sgd(ops, ln, [True] * 64, 0.9, 3, 201)


def test_sgd_momentum_zero_leaves_a_given_buffer_alone(ops):
    """mu == 0 with buffers present: p -= lr * g, every buffer bit-identical afterwards (_run_sgd compares the bits)."""
    _run_sgd(ops, _lengths64(), [True] * 64, 0.0, 3, 202)


def test_sgd_grid_stride_loop(ops):
    """1024 x 1024 + 1029 elements for a grid of 1024 x 256 threads, next to a 3-element segment."""
    n = 1024 * 1024 + 1029
    assert n > 1024 * 256 * 4
    _run_sgd(ops, [n, 3], [True, True], 0.9, 2, 203)


# ---- sgan_adam_multi: the n & 3 tail -------------------------------------------------------------------------------------------
ADAM_N = [1, 3, 6, 1027, 40029]
LR, B1, B2, EPS = A.as_f32(2e-4, 0.5, 0.999, 1e-8)


def test_adam_multi_tails(ops):
    """Five 16-byte aligned segments in one launch, three steps with gradient scales 1e-2, 1e-1, 1: every segment against fp64
    within the project's Adam bound (adam_ref.assert_within_yardstick, and the same figures segment by segment), the step counter
    and the two floats behind it, the sentinel behind each segment's n."""
    offs, cur = [], 0
    for n in ADAM_N:
        offs.append(cur)
        cur += (n + 3) // 4 * 4 + 4
    live = np.zeros(cur, dtype=bool)
    for o, n in zip(offs, ADAM_N):
        live[o: o + n] = True
    nl = int(live.sum())
    rng = np.random.default_rng(300)
    p0 = _arena(cur, live, rng.standard_normal(nl).astype(np.float32))
    z0 = _arena(cur, live, np.zeros(nl, dtype=np.float32))
    grads = [_arena(cur, live, (rng.standard_normal(nl) * 10.0 ** (s - 2)).astype(np.float32)) for s in range(3)]
    p, m, v, g = _dev(p0), _dev(z0), _dev(z0), _filled(cur, SENT)
    state = torch.tensor([0, 0, 0, 0x5A5A5A5A], dtype=torch.int32, device="cuda")
    lr = _dev(np.full(1, LR, dtype=np.float32))
    segs = [(p[o: o + n], g[o: o + n], m[o: o + n], v[o: o + n], n) for o, n in zip(offs, ADAM_N)]
    assert all(t.data_ptr() % 16 == 0 for s in segs for t in s[:4])
    for s in range(3):
        g.copy_(_dev(grads[s]))
        ops.adam_multi(segs, lr, B1, B2, EPS, state)
        torch.cuda.synchronize()
        assert int(state[0]) == s + 1
    step_size, inv = A.bias_corrections(3, LR, B1, B2)
    assert state.cpu().tolist() == [3, int(np.float32(step_size).view(np.int32)), int(np.float32(inv).view(np.int32)), 0x5A5A5A5A]
    gl = [x[live] for x in grads]
    ref = A.adam_run(A.adam_step, p0[live].astype(np.float64), gl, LR, B1, B2, EPS)
    f32 = A.adam_run(A.adam_step_f32, p0[live], gl, LR, B1, B2, EPS)
    hp, hm, hv = (t.cpu().numpy() for t in (p, m, v))
    got = (hp[live], hm[live], hv[live])
    dev, yard = A.assert_within_yardstick(got, f32, ref, "adam_multi tails")
    pos = np.cumsum([0] + ADAM_N)
    for i, n in enumerate(ADAM_N):
        sl = slice(pos[i], pos[i + 1])
        assert np.abs(got[0][sl] - ref[0][sl]).max() <= A.YARDSTICK_FACTOR * yard[0], (i, n)
        assert np.abs(got[1][sl] - ref[1][sl]).max() <= A.YARDSTICK_FACTOR * yard[1] * np.abs(ref[1]).max(), (i, n)
        assert np.abs(got[2][sl] - ref[2][sl]).max() <= A.YARDSTICK_FACTOR * yard[2] * np.abs(ref[2]).max(), (i, n)
        tail = slice(pos[i + 1] - (n & 3), pos[i + 1])      # the n & 3 elements behind the last full 16 bytes: each moved far beyond the bound
        assert (np.abs(ref[0][tail] - p0[live][tail]) > 25 * A.YARDSTICK_FACTOR * yard[0]).all(), (i, n)
    for name, h, h0 in (("p", hp, p0), ("m", hm, z0), ("v", hv, z0)):
        assert np.array_equal(_bits(h)[~live], _bits(h0)[~live]), f"{name}: a float behind a segment's n was written"
    assert np.array_equal(_bits(g.cpu().numpy()), _bits(grads[-1]))

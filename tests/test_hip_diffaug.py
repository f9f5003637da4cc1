"""GPU tests of the augmentation kernels (csrc/sgan_diffaug.hip) against the host yardsticks of util.py
(diffaug_params, diffaug_ref, diffaug_bwd_ref), on records the test writes.

Bounds, u = 2^-24, for an element of a colour channel that the record shows (every other element must be equal to the bit):
  forward   the device forms m^ = fl32(m64), t = fl(v - m^), y1 = fl(a t + m^) (one fma), y = fl(y1 + b).  Against the exact
            y* = a (v - m*) + m* + b:  |y - y*| <= |1 - a| dm + u (|a| |v - m*| + |a (v - m*) + m*| + |y*|) (1 + 1e-3), where
            dm = u |m*| (1 + 1e-4) + 2.02 * 2^-53 * sum|x| covers the rounding of m to fp32 and the fp64 sums of the device and of
            NumPy, each at most (n - 1) 2^-53 sum|x| / n off whatever their order; the 1e-3 holds the second-order terms.
  backward  c^ = fl32((1 - a) S64 / n), dx = fl(a K dy + c^) (one fma).  Against dx* = a K dy + c*:
            |dx - dx*| <= u |dx*| (1 + 1e-3) + dc,  dc = u |c*| (1 + 1e-4) + |1 - a| / n * 2.02 * 2^-53 * sum|K dy|.
  adjoint   <fwd(x) - fwd(0), dy> - <x, bwd(dy)> is 0 for the exact maps; on device outputs it is at most
            sum |dy| (bound_fwd(x) + bound_fwd(0)) + sum |x| bound_bwd."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hip_utils import _guard_intact, _guarded  # noqa: E402

from supervised_gan_amd import _lib as L  # noqa: E402
from supervised_gan_amd import ops, util  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(1, 1, 1, 4), (7, 9, 3, 4), (33, 31, 3, 4), (64, 64, 6, 8), (130, 67, 3, 4)]      # the last: 9 workgroups in the reduction
IDS = ["%dx%dx%d" % s[:3] for s in SHAPES]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")


def colour_mask(C):
    """The last channel of a 1- or 3-channel image (rg | b), channels 2 and 5 of the 6-channel one: colour and plain channels mix
    inside one 16-byte group and across two."""
    return {1: 0b1, 3: 0b100, 6: 0b100100}[C]


def geometry_records(H, W):
    Sy, Sx = int(np.floor(H * 0.125 + 0.5)), int(np.floor(W * 0.125 + 0.5))
    qh, qw = (H + 3) // 4, (W + 3) // 4
    g = [(0, 0, 0, 0, 0, 0),                                                            # the identity
         (Sy, 0, 0, 0, 0, 0), (-Sy, 0, 0, 0, 0, 0), (0, Sx, 0, 0, 0, 0), (0, -Sx, 0, 0, 0, 0),      # the largest drawn shift, four ways
         (H - 1, 0, 0, 0, 0, 0), (-(H - 1), 0, 0, 0, 0, 0), (0, W - 1, 0, 0, 0, 0), (0, -(W - 1), 0, 0, 0, 0),      # one row / column left
         (H, W, 0, 0, 0, 0),                                                            # nothing left
         (0, 0, 0, qh, 0, qw), (0, 0, 0, qh, W - qw, W), (0, 0, H - qh, H, 0, qw), (0, 0, H - qh, H, W - qw, W),      # clipped at the corners
         (0, 0, 0, H, 0, W),                                                            # the whole image
         (0, 0, H // 2, H // 2, 0, W), (0, 0, 0, 0, 0, 0),                              # empty rectangles
         (min(2, H - 1), -min(1, W - 1), 0, qh, W - qw, W)]                             # a shift and a cutout
    return [(0.0, 1.0) + r for r in g]


def colour_records(H, W):
    qh, qw = (H + 3) // 4, (W + 3) // 4
    recs = [(b, a, 0, 0, 0, 0, 0, 0) for a in (0.5, 1.0, 1.5) for b in (0.5, -0.5)]
    recs += [(-0.5, 1.5, min(1, H - 1), -min(2, W - 1), H - qh, H, 0, qw), (0.25, 0.75, -(H - 1), 0, 0, 0, 0, 0),
             (0.125, 1.25, 0, 0, 0, H, 0, W), (0.0, 0.5, H, 0, 0, 0, 0, 0)]
    return recs


def rec_tensor(recs):
    arr = np.zeros((len(recs), 8), dtype=np.int32)
    arr[:, :2] = np.array([r[:2] for r in recs], dtype=np.float32).view(np.int32)
    arr[:, 2:] = np.array([r[2:] for r in recs], dtype=np.int64)
    return torch.from_numpy(arr).cuda()


def rec_tuples(t):
    arr = t.cpu().numpy()
    return [tuple(float(v) for v in row[:2].view(np.float32)) + tuple(int(v) for v in row[2:]) for row in arr]


def image(H, W, C, Cs, seed, pad=float("nan")):
    """(x [H, W, C] float32 numpy, its padded device buffer whose padding channels hold `pad`)."""
    x = np.random.default_rng(seed).standard_normal((H, W, C)).astype(np.float32)
    buf = torch.full((H, W, Cs), pad, dtype=torch.float32)
    buf[..., :C] = torch.from_numpy(x)
    return x, buf.cuda()


def run(fn, src, C, mask, recs, workspace):
    """fn = ops.diffaug_multi_fwd / _bwd on one source under every record, 8 jobs a call; each destination is NaN on entry and has
    NaN guards behind it.  Returns the [H, W, Cs] results as numpy."""
    outs = []
    for k in range(0, len(recs), ops.DIFFAUG_MAX_JOBS):
        chunk = recs[k: k + ops.DIFFAUG_MAX_JOBS]
        pairs = [_guarded(torch.full(tuple(src.shape), float("nan"), dtype=torch.float32)) for _ in chunk]
        fn([src] * len(chunk), [d for d, _ in pairs], [C] * len(chunk), mask, rec_tensor(chunk), workspace)
        torch.cuda.synchronize()
        assert all(_guard_intact(g) for _, g in pairs)
        outs += [d.cpu().numpy() for d, _ in pairs]
    return outs


def fwd_bound(x, rec, mask):
    """Per-element bound of the forward, and the exact result (fp64)."""
    H, W, C = x.shape
    b, a = rec[:2]
    col = np.array([(mask >> c) & 1 for c in range(C)], dtype=bool)
    x = x.astype(np.float64)
    y = util.diffaug_ref(x, rec, mask)
    bound = np.zeros_like(y)
    if col.any():
        xc = x[:, :, col]
        m = xc.mean()
        dm = U * abs(m) * (1 + 1e-4) + 2.02 * 2.0 ** -53 * np.abs(xc).sum()
        g = np.zeros_like(x)
        g[:, :, col] = abs(1 - a) * dm + U * (abs(a) * np.abs(xc - m) + np.abs(a * (xc - m) + m) + np.abs(a * (xc - m) + m + b)) * (1 + 1e-3)
        bound = util._diffaug_visible(rec, H, W)[:, :, None] * util._diffaug_shift(g, rec[2], rec[3])
    return bound, y


def bwd_bound(dy, rec, mask):
    H, W, C = dy.shape
    b, a = rec[:2]
    col = np.array([(mask >> c) & 1 for c in range(C)], dtype=bool)
    dy = dy.astype(np.float64)
    dx = util.diffaug_bwd_ref(dy, rec, mask)
    bound = np.zeros_like(dx)
    if col.any() and a != 1.0:
        kdy = util._diffaug_visible(rec, H, W)[:, :, None] * dy[:, :, col]
        n = int(col.sum()) * H * W
        c = (1 - a) * kdy.sum() / n
        dc = U * abs(c) * (1 + 1e-4) + abs(1 - a) / n * 2.02 * 2.0 ** -53 * np.abs(kdy).sum()
        bound[:, :, col] = U * np.abs(dx[:, :, col]) * (1 + 1e-3) + dc
    return bound, dx


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_geometry_alone_is_exact(shape):
    """Translation and cutout without a colour operation: forward and backward equal the yardstick bit for bit, through the
    one-launch form and through the two-launch form (whose records all have a == 1); padding channels come out 0 although the source
    holds NaN there."""
    _need_gpu()
    H, W, C, Cs = shape
    mask = colour_mask(C)
    x, src = image(H, W, C, Cs, 1)
    recs = geometry_records(H, W)
    ws = ops.diffaug_workspace(ops.DIFFAUG_MAX_JOBS, "cuda")
    for fn, ref in ((ops.diffaug_multi_fwd, util.diffaug_ref), (ops.diffaug_multi_bwd, util.diffaug_bwd_ref)):
        for workspace in (None, ws):
            outs = run(fn, src, C, mask, recs, workspace)
            for rec, out in zip(recs, outs):
                want = ref(x, rec, 0).astype(np.float32)      # a == 1, b == 0: g is the identity on every channel
                assert np.array_equal(out[..., :C], want), rec
                assert np.array_equal(out[..., C:], np.zeros((H, W, Cs - C), dtype=np.float32)), rec


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_colour_within_the_derived_bound(shape):
    """Brightness and contrast, alone and over a shift and a cutout: per element within the bound of the module docstring, plain
    channels and hidden pixels to the bit, the adjoint identity on the device outputs, and two runs bit-identical."""
    _need_gpu()
    H, W, C, Cs = shape
    mask = colour_mask(C)
    col = np.array([(mask >> c) & 1 for c in range(C)], dtype=bool)
    x, src = image(H, W, C, Cs, 2)
    dy, dsrc = image(H, W, C, Cs, 3)
    zero = torch.zeros_like(src)
    recs = colour_records(H, W)
    ws = ops.diffaug_workspace(ops.DIFFAUG_MAX_JOBS, "cuda")
    ys, y0s, dxs = (run(ops.diffaug_multi_fwd, src, C, mask, recs, ws), run(ops.diffaug_multi_fwd, zero, C, mask, recs, ws),
                    run(ops.diffaug_multi_bwd, dsrc, C, mask, recs, ws))
    again = run(ops.diffaug_multi_fwd, src, C, mask, recs, ws), run(ops.diffaug_multi_bwd, dsrc, C, mask, recs, ws)
    worst = [0.0, 0.0, 0.0]
    for i, rec in enumerate(recs):
        y, y0, dx = ys[i], y0s[i], dxs[i]
        assert np.array_equal(y.view(np.int32), again[0][i].view(np.int32)) and np.array_equal(dx.view(np.int32), again[1][i].view(np.int32))
        for out in (y, y0, dx):
            assert np.array_equal(out[..., C:], np.zeros((H, W, Cs - C), dtype=np.float32)), rec
        bf, yref = fwd_bound(x, rec, mask)
        bf0, y0ref = fwd_bound(np.zeros_like(x), rec, mask)
        bb, dxref = bwd_bound(dy, rec, mask)
        for got, ref, bound, what in ((y, yref, bf, "forward"), (y0, y0ref, bf0, "forward of 0"), (dx, dxref, bb, "backward")):
            dev = np.abs(got[..., :C].astype(np.float64) - ref)
            assert (dev <= bound).all(), (what, rec, float(dev.max()), float(bound.max()))
            assert np.array_equal(got[..., :C][..., ~col], ref[..., ~col].astype(np.float32)), (what, rec)      # plain channels: to the bit
            k = 0 if what != "backward" else 1
            if bound.max() > 0:
                worst[k] = max(worst[k], float((dev / np.where(bound > 0, bound, 1)).max()))
        lhs = np.sum((y[..., :C].astype(np.float64) - y0[..., :C].astype(np.float64)) * dy.astype(np.float64))
        rhs = np.sum(x.astype(np.float64) * dx[..., :C].astype(np.float64))
        adj = np.sum(np.abs(dy) * (bf + bf0)) + np.sum(np.abs(x) * bb)
        assert abs(lhs - rhs) <= adj, (rec, lhs - rhs, adj)
        if adj > 0:
            worst[2] = max(worst[2], abs(lhs - rhs) / adj)
    print(f"{H}x{W}x{C}: largest deviation as a share of its bound: forward {worst[0]:.3f}, backward {worst[1]:.3f}, adjoint {worst[2]:.3f}")


def test_one_launch_form_takes_contrast_as_one():
    """workspace None is the caller's statement that no record carries a contrast: brightness is applied, `a` is not read."""
    _need_gpu()
    H, W, C, Cs = 7, 9, 3, 4
    x, src = image(H, W, C, Cs, 4)
    out, = run(ops.diffaug_multi_fwd, src, C, 0b100, [(0.25, 1.5, 1, 0, 0, 0, 0, 0)], None)
    want = util.diffaug_ref(x, (0.25, 1.0, 1, 0, 0, 0, 0, 0), 0b100)
    assert np.abs(out[..., :C] - want).max() <= U * np.abs(want).max() and np.array_equal(out[..., :2], want[..., :2].astype(np.float32))


def test_colour_only_record_passes_plain_channels():
    _need_gpu()
    H, W, C, Cs = 33, 31, 6, 8
    x, src = image(H, W, C, Cs, 5)
    ws = ops.diffaug_workspace(1, "cuda")
    rec = (0.25, 1.5, 0, 0, 0, 0, 0, 0)
    y, = run(ops.diffaug_multi_fwd, src, C, 0b100100, [rec], ws)
    dx, = run(ops.diffaug_multi_bwd, src, C, 0b100100, [rec], ws)
    plain = [0, 1, 3, 4]
    assert np.array_equal(y[..., plain].view(np.int32), x[..., plain].view(np.int32))
    assert np.array_equal(dx[..., plain].view(np.int32), x[..., plain].view(np.int32))
    assert not np.array_equal(y[..., [2, 5]], x[..., [2, 5]])


@pytest.mark.parametrize("policy", [("translation", "cutout", "brightness", "contrast"), ("cutout", "brightness"), ()],
                         ids=["all", "cutout_brightness", "none"])
def test_draw_equals_the_yardstick(policy):
    _need_gpu()
    shapes = [(128, 128), (7, 9), (33, 31)]
    bits = sum(ops.DIFFAUG_BITS[p] for p in policy)
    seed, off0 = 5 + 7919, 6
    offset = torch.full((1,), off0, dtype=torch.int64, device="cuda")
    recs = torch.full((4, 8), -1, dtype=torch.int32, device="cuda")
    ops.diffaug_draw(recs, shapes, bits, 0.125, 0.5, seed, offset)
    torch.cuda.synchronize()
    assert rec_tuples(recs[:3]) == util.diffaug_params(seed, off0, shapes, policy, 0.125, 0.5)
    assert int(offset.item()) == off0 + 2 * 3 and recs[3].eq(-1).all()
    ops.diffaug_draw(recs, shapes, bits, 0.125, 0.5, seed, offset)      # the next call draws the next records
    assert rec_tuples(recs[:3]) == util.diffaug_params(seed, off0 + 6, shapes, policy, 0.125, 0.5)
    assert int(offset.item()) == off0 + 12
    ops.diffaug_draw(recs, shapes[:1], bits, 0.3, 0.7, seed, offset, advance=False)
    assert rec_tuples(recs[:1]) == util.diffaug_params(seed, off0 + 12, shapes[:1], policy, 0.3, 0.7) and int(offset.item()) == off0 + 12
    ops.diffaug_draw(recs, shapes[:1], bits, 0.125, 0.5, seed, None)      # no offset word: counter 0
    assert rec_tuples(recs[:1]) == util.diffaug_params(seed, 0, shapes[:1], policy, 0.125, 0.5)


def test_unsupported_shapes_are_refused_and_write_nothing():
    _need_gpu()
    recs = rec_tensor([(0.0, 1.0, 0, 0, 0, 0, 0, 0)])
    src = torch.zeros((4, 4, 6), dtype=torch.float32, device="cuda")
    dst, guard = _guarded(torch.full((4, 4, 6), float("nan"), dtype=torch.float32))
    for fn in (ops.diffaug_multi_fwd, ops.diffaug_multi_bwd):
        with pytest.raises(L.SganError, match="multiple of 4"):
            fn([src], [dst], [3], 0b100, recs, None)
    job = (L.DiffaugJob * 1)(L.DiffaugJob(src.data_ptr(), dst.data_ptr(), 4, 4, 3, 6, 0b100))
    assert L.lib().sgan_diffaug_multi_fwd(job, 1, recs.data_ptr(), None, None) == 1
    src4 = torch.zeros((4, 4, 4), dtype=torch.float32, device="cuda")
    dst4, guard4 = _guarded(torch.full((4, 4, 4), float("nan"), dtype=torch.float32))
    with pytest.raises(L.SganError, match="colour mask"):
        ops.diffaug_multi_fwd([src4], [dst4], [3], 0b1000, recs, None)
    with pytest.raises(L.SganError, match="two different"):
        ops.diffaug_multi_fwd([src4], [src4], [3], 0b100, recs, None)
    with pytest.raises(L.SganError, match="njobs"):
        ops.diffaug_multi_fwd([src4] * 9, [torch.empty_like(src4) for _ in range(9)], [3] * 9, 0b100, rec_tensor([(0.0, 1.0, 0, 0, 0, 0, 0, 0)] * 9), None)
    with pytest.raises(L.SganError, match="ratios"):
        ops.diffaug_draw(recs, [(4, 4)], 15, 1.5, 0.5, 0, None)
    torch.cuda.synchronize()
    assert torch.isnan(dst).all() and torch.isnan(dst4).all() and _guard_intact(guard) and _guard_intact(guard4)


class _State:
    def __init__(self, recs, mask, workspace):
        self.records, self.colour_mask, self.workspace = rec_tensor(recs), mask, workspace


def test_autograd_function():
    """ops.diffaug over logical views: the backward is sgan_diffaug_multi_bwd under the forward's records; the list form transforms
    two tensors in one call, each under its own record; a tensor that needs no gradient records no backward."""
    _need_gpu()
    H, W, C, Cs = 33, 31, 3, 4
    recs = [(0.25, 1.5, 2, -3, 0, 8, 20, 31), (-0.5, 0.5, -4, 1, 10, 20, 0, 9)]
    st = _State(recs, 0b100, ops.diffaug_workspace(2, "cuda"))
    (xa, ba), (xb, bb) = image(H, W, C, Cs, 6, pad=0.0), image(H, W, C, Cs, 7, pad=0.0)
    dy, dbuf = image(H, W, C, Cs, 8, pad=0.0)
    ta, tb = ops.logical_view(ba, C).requires_grad_(True), ops.logical_view(bb, C)
    ya, yb = ops.diffaug([ta, tb], st)
    assert ya.grad_fn is not None and ya.shape == (1, C, H, W)
    for y, x, rec in ((ya, xa, recs[0]), (yb, xb, recs[1])):
        bound, ref = fwd_bound(x, rec, 0b100)
        assert (np.abs(y.detach()[0].permute(1, 2, 0).cpu().numpy().astype(np.float64) - ref) <= bound).all()
    ya.backward(ops.logical_view(dbuf, C))
    want, = run(ops.diffaug_multi_bwd, dbuf, C, 0b100, recs[:1], st.workspace)
    assert np.array_equal(ta.grad[0].permute(1, 2, 0).cpu().numpy(), want[..., :C]) and tb.grad is None
    # slot 1 alone, and no gradient wanted: plain tensors out
    y1 = ops.diffaug(tb, st, slot=1)
    assert y1.grad_fn is None and not y1.requires_grad and torch.equal(y1, yb.detach())

"""GPU tests of the signed squared distance map (sgan_signed_edt_sq) bit for bit against the host yardstick util.signed_edt_sq: every
value is an exact integer.  Shapes: those of tests/test_hip_seg_terms.py plus a plane below one 32-row segment of the transform and
one that crosses two segment boundaries."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

PLANES = ((5, 7), (33, 31), (257, 3), (64, 64), (9, 7), (1, 1), (31, 33), (65, 5))
SENTINEL = -7777


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")


def cell_map(H, W):
    """Thin walls: every 8th row and column, one gap per wall segment."""
    m = np.zeros((H, W), np.float32)
    m[::8, :] = 1.0
    m[:, ::8] = 1.0
    m[::8, 3::16] = 0.0
    return m


def planes(H, W):
    rng = np.random.default_rng(100 * H + W)
    out = {"d%g" % d: (rng.random((H, W)) < d).astype(np.float32) for d in (0.02, 0.5, 0.98)}
    out["cells"] = cell_map(H, W)
    out["empty"], out["full"] = np.zeros((H, W), np.float32), np.ones((H, W), np.float32)
    one = np.zeros((H, W), np.float32)
    one[H // 2, W // 2] = 1.0
    out["one_inside"], out["one_outside"] = one, 1.0 - one
    odd = (rng.random((H, W)) < 0.5).astype(np.float32)
    odd[0, 0], odd[H - 1, W - 1] = np.nan, 0.5      # both outside
    out["nan_and_half"] = odd
    return out


def device_map(plane, stride=1, twice=True):
    """ops.signed_edt_sq of the host plane into a sentinel-filled output; stride 4: the plane is channel 1 of an NHWC buffer whose
    other channels hold the complement."""
    from supervised_gan_amd import ops
    dev = torch.device("cuda", 0)
    H, W = plane.shape
    if stride == 1:
        t = torch.from_numpy(plane).to(dev)
    else:
        buf = torch.from_numpy(np.repeat((1.0 - np.nan_to_num(plane))[:, :, None], stride, axis=2).astype(np.float32)).to(dev)
        buf[:, :, 1] = torch.from_numpy(plane).to(dev)
        t = buf[:, :, 1]
        assert t.stride() == (W * stride, stride)
    out = torch.full((H, W), SENTINEL, dtype=torch.int32, device=dev)
    ops.signed_edt_sq(t, out=out)
    first = out.cpu().numpy()
    if twice:
        out.fill_(SENTINEL)
        ops.signed_edt_sq(t, out=out)
        assert np.array_equal(out.cpu().numpy(), first)
    return first


@pytest.mark.parametrize("shape", PLANES)
def test_bit_for_bit_against_the_yardstick(shape):
    _need_gpu()
    from supervised_gan_amd.util import signed_edt_sq
    H, W = shape
    for name, plane in planes(H, W).items():
        want = signed_edt_sq(plane)
        got = device_map(plane)
        assert got.dtype == np.int32 and np.array_equal(got, want), (shape, name, int(np.abs(got.astype(np.int64) - want).max()))
        inside = plane > 0.5
        if inside.any() and not inside.all():
            assert (got[inside] <= -1).all() and (got[~inside] >= 1).all(), (shape, name)
        else:
            assert not got.any(), (shape, name)
    for name in ("d0.5", "cells", "nan_and_half", "full"):
        plane = planes(H, W)[name]
        assert np.array_equal(device_map(plane, stride=4, twice=False), signed_edt_sq(plane)), (shape, name, "strided")


def test_graph_replay_on_another_plane():
    _need_gpu()
    from supervised_gan_amd import ops
    from supervised_gan_amd.util import signed_edt_sq
    dev = torch.device("cuda", 0)
    for H, W in ((65, 5), (33, 31)):
        ps = planes(H, W)
        src = torch.from_numpy(ps["d0.5"]).to(dev)
        out = torch.full((H, W), SENTINEL, dtype=torch.int32, device=dev)
        ops.signed_edt_sq(src, out=out)      # the workspace exists before the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ops.signed_edt_sq(src, out=out)
        for name in ("cells", "empty", "d0.02", "full", "nan_and_half"):
            src.copy_(torch.from_numpy(ps[name]).to(dev))
            out.fill_(SENTINEL)
            g.replay()
            torch.cuda.synchronize()
            replayed = out.cpu().numpy()
            assert np.array_equal(replayed, signed_edt_sq(ps[name])), (H, W, name)
            assert np.array_equal(replayed, device_map(ps[name], twice=False)), (H, W, name)      # the eager call's bits


def test_refusals_launch_nothing():
    _need_gpu()
    from supervised_gan_amd import _lib, ops
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    H, W = 8, 8
    plane = torch.zeros((H, W), device=dev)
    out = torch.full((H, W), SENTINEL, dtype=torch.int32, device=dev)
    ws = ops.signed_edt_workspace(H, W, dev)
    err = ops.metric_err(dev)
    nbytes = ws.numel() * 8
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    assert lib.sgan_signed_edt_workspace(0, 8) < 0 and lib.sgan_signed_edt_workspace(40000, 8) < 0
    assert lib.sgan_signed_edt_workspace(H, W) > lib.sgan_edt_workspace(H, W) + 8 * H * W - 1
    for args, why in (((None, 1, H, W, P(out), P(ws), nbytes, P(err), None), b"null"),
                      ((P(plane), 1, H, W, None, P(ws), nbytes, P(err), None), b"null"),
                      ((P(plane), 1, H, W, P(out), P(ws), nbytes, None, None), b"null"),
                      ((P(plane), 0, H, W, P(out), P(ws), nbytes, P(err), None), b"pixel stride"),
                      ((P(plane), 1, 0, W, P(out), P(ws), nbytes, P(err), None), b"bad shape"),
                      ((P(plane), 1, H, W, P(out), P(ws), lib.sgan_signed_edt_workspace(H, W) - 1, P(err), None), b"workspace"),
                      ((P(plane), 1, H, W, P(out), ctypes.c_void_p(ws.data_ptr() + 8), nbytes - 8, P(err), None), b"aligned")):
        assert lib.sgan_signed_edt_sq(*args) == 1 and why in lib.sgan_last_error(), why
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())

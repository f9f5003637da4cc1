"""Host tests of the geometry of whole-image inference (util.tile_plan / tile_window / prep_tile_ref / blend_tiles_ref):
the yardsticks the device kernels and SegmentationModel.test() are checked against, and the refusals of options.check_tile_options."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from supervised_gan_amd import util  # noqa: E402
from supervised_gan_amd.options import TestOptions as _TestOptions, check_tile_options  # noqa: E402

PLANS = [(40, 16, 3, 4, 6), (16, 16, 0, 1, 16), (17, 16, 0, 1, 16), (53, 16, 5, 2, 6), (21, 16, 7, 1, 2)]      # (L, T, M, R, S)


@pytest.mark.parametrize("L,T,M,R,S", PLANS)
def test_tile_plan_origins_and_weight_sum(L, T, M, R, S):
    oy, ox, Wy, Wx = util.tile_plan(L, L, T, M, R, S)
    assert oy == ox and oy[0] == -M and oy[-1] == L + M - T and len(set(oy)) == len(oy) and oy == sorted(oy)
    assert all(b - a <= S for a, b in zip(oy, oy[1:]))
    win = util.tile_window(T, M, R)
    assert win.dtype == np.int64 and (win == win[::-1]).all() and (win[:M] == 0).all() and win.max() <= R
    brute = np.zeros(L, dtype=np.int64)
    for Y in range(L):
        for o in oy:
            i = Y - o
            if 0 <= i < T:
                brute[Y] += max(0, min(min(i + 1, T - i) - M, R))
    assert np.array_equal(Wy, brute) and np.array_equal(Wx, brute)
    assert (Wy > 0).all()


def test_tile_plan_is_per_axis():
    oy, ox, Wy, Wx = util.tile_plan(40, 53, 16, 3, 4, 6)
    assert (oy, ox) == (util.tile_plan(40, 40, 16, 3, 4, 6)[0], util.tile_plan(53, 53, 16, 3, 4, 6)[0])
    assert Wy.shape == (40,) and Wx.shape == (53,)
    assert util.tile_passes([0, 4], [1], True)[:9] == [(0, 1, 0, 0), (0, 1, 0, 1), (0, 1, 0, 2), (0, 1, 0, 3), (0, 1, 1, 0), (0, 1, 1, 1),
                                                       (0, 1, 1, 2), (0, 1, 1, 3), (4, 1, 0, 0)]
    assert util.tile_passes([0, 4], [1, 2], False) == [(0, 1, 0, 0), (0, 2, 0, 0), (4, 1, 0, 0), (4, 2, 0, 0)]


def _opt(*extra):
    argv = ["--model", "segmentation", "--dataset_mode", "single", "--dataroot", "/nonexistent/folder", "--gpu_ids", "-1", "--fineSize", "16",
            "--whole_image"] + list(extra)
    return _TestOptions().parse(argv, save=False, verbose=False)


def test_check_tile_options_defaults_and_refusals(capsys):
    o = _opt("--tile", "64")
    assert o.tiling and (o.tile, o.tile_margin, o.tile_ramp, o.tile_stride) == (64, 16, 16, 16)
    o = _opt("--tile", "40", "--tile_margin", "16", "--tile_ramp", "16")
    assert o.tile_stride == 1                                         # T - 2 M - R = -8: at least 1
    o = _TestOptions().parse(["--model", "segmentation", "--dataset_mode", "single", "--dataroot", "/nonexistent/folder", "--gpu_ids", "-1",
                              "--fineSize", "32", "--tta", "d4"], save=False, verbose=False)
    assert o.tiling and (o.tile, o.tile_margin, o.tile_ramp, o.tile_stride) == (32, 0, 1, 32)      # the crop as one tile
    o = _TestOptions().parse(["--model", "segmentation", "--gpu_ids", "-1"], save=False, verbose=False)
    assert not o.tiling
    # at parse time, through parser.error: S > T - 2 M, R outside 1..64, the synthetic feeder, another model
    for bad in (["--tile", "16", "--tile_margin", "3", "--tile_stride", "11"], ["--tile", "16", "--tile_margin", "8"],
                ["--tile_ramp", "0", "--tile_margin", "0"], ["--tile_ramp", "65", "--tile_margin", "0"], ["--tile_stride", "0", "--tile_margin", "0"],
                ["--dataroot", "synthetic", "--tile_margin", "0"], ["--model", "segmentation_cycle", "--tile_margin", "0"],
                ["--dataset_mode", "aligned", "--tile_margin", "0"]):
        with pytest.raises(SystemExit):
            _opt(*bad)
    assert "--tile" in capsys.readouterr().err
    # with the image: M >= L, L + 2 M < T
    o = _opt("--tile", "16", "--tile_margin", "3", "--tile_ramp", "4", "--tile_stride", "6")
    check_tile_options(o, size=(40, 53))
    with pytest.raises(ValueError, match="tile_margin"):
        check_tile_options(o, size=(3, 53))
    with pytest.raises(ValueError, match="tile_margin"):
        check_tile_options(o, size=(40, 2))
    o = _opt("--tile", "16", "--tile_margin", "2", "--tile_ramp", "4", "--tile_stride", "6")
    with pytest.raises(ValueError, match="does not fit"):
        check_tile_options(o, size=(11, 40))
    check_tile_options(o, size=(12, 40))
    for L, T, M, R, S in [(40, 16, 3, 4, 11), (3, 16, 3, 4, 6), (9, 16, 3, 4, 6), (40, 16, 3, 0, 6), (40, 16, 3, 65, 6)]:
        with pytest.raises(ValueError):
            util.tile_plan(L, 40, T, M, R, S)
        with pytest.raises(ValueError):
            util.tile_plan(40, L, T, M, R, S)


def _image(H, W, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=(H, W, 3), dtype=np.uint8)


def test_prep_tile_ref_reflects_like_pad_reflect_and_d4_inverts():
    img = _image(11, 14)
    full = util.prep_tile_ref(img, 0, 0, 11, 14, 0, 0)
    want = ((img.astype(np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(0.5)).transpose(2, 0, 1)
    assert full.dtype == np.float32 and np.array_equal(full, want)
    padded = np.pad(full, ((0, 0), (4, 4), (5, 5)), mode="reflect")      # F.pad(mode='reflect'): the edge is not repeated
    for y0, x0 in [(-4, -5), (-4, 14 + 5 - 8), (11 + 4 - 8, -5), (11 + 4 - 8, 14 + 5 - 8), (2, 3), (-1, 4)]:
        win = padded[:, y0 + 4: y0 + 12, x0 + 5: x0 + 13]
        for flip in (0, 1):
            for rot in range(4):
                t = util.prep_tile_ref(img, y0, x0, 8, 8, flip, rot)
                assert np.array_equal(util.d4_inverse(t, flip, rot), win), (y0, x0, flip, rot)      # the inverse of blend_tiles_ref: identity
                # sg_image_prep_kernel's convention, spelled out: R[i][j] = F[j][n-1-i] (rot 1) of the flipped window F
                F = win[:, :, ::-1] if flip else win
                n = 8
                R = {0: F, 1: np.array([[[F[c, j, n - 1 - i] for j in range(n)] for i in range(n)] for c in range(3)]),
                     2: F[:, ::-1, ::-1], 3: np.array([[[F[c, n - 1 - j, i] for j in range(n)] for i in range(n)] for c in range(3)])}[rot]
                assert np.array_equal(t, R), (flip, rot)
    # the 8 elements are distinct on an asymmetric image
    seen = {util.prep_tile_ref(img, 1, 2, 8, 8, f, r).tobytes() for f in (0, 1) for r in range(4)}
    assert len(seen) == 8
    with pytest.raises(AssertionError):
        util.prep_tile_ref(img, -11, 0, 8, 8, 0, 0)


A_MAP = np.array([[1.5, -2.0, 0.25], [-0.75, 0.5, 3.0], [2.0, 1.0, -1.0]])      # "logits" = A x + b of the three pixel values in [-1, 1]
B_MAP = np.array([0.1, -0.2, 0.3])


def _pixelwise(x):
    return np.einsum("kc,chw->khw", A_MAP, x.astype(np.float64)) + B_MAP[:, None, None]


@pytest.mark.parametrize("L,T,M,R,S", PLANS)
@pytest.mark.parametrize("tta", [False, True])
@pytest.mark.parametrize("sigmoid", [False, True])
def test_blend_of_a_pixelwise_network_is_the_untiled_prediction(L, T, M, R, S, tta, sigmoid):
    """A network without context predicts every pixel from that pixel alone, so tiling, mirroring, the 8 orientations and the blend
    must return exactly what it gives on the untiled image: reflection, origins, the inverse D4 and the normalisation, pinned together."""
    H, W = L, L + 5
    img = _image(H, W, seed=L)
    z = _pixelwise(util.prep_tile_ref(img, 0, 0, H, W, 0, 0))
    if sigmoid:
        want = 1.0 / (1.0 + np.exp(-z))
    else:
        e = np.exp(z - z.max(axis=0, keepdims=True))
        want = e / e.sum(axis=0, keepdims=True)
    calls = []

    def net(k, y0, x0, flip, rot):
        calls.append((y0, x0, flip, rot))
        return _pixelwise(util.prep_tile_ref(img, y0, x0, T, T, flip, rot))

    P, count = util.blend_tiles_ref(net, H, W, T, M, R, S, tta=tta, sigmoid=sigmoid, return_count=True)
    oy, ox, _, _ = util.tile_plan(H, W, T, M, R, S)
    assert calls == util.tile_passes(oy, ox, tta) and len(calls) == len(oy) * len(ox) * (8 if tta else 1)
    assert P.shape == (3, H, W) and float(np.abs(P - want).max()) <= 1e-12
    assert count.min() >= (8 if tta else 1) and count.max() <= len(calls)
    # the same from a list of per-pass arrays
    P2 = util.blend_tiles_ref([net(k, *p) for k, p in enumerate(util.tile_passes(oy, ox, tta))], H, W, T, M, R, S, tta=tta, sigmoid=sigmoid)
    assert np.array_equal(P, P2)

"""The NumPy yardstick of the elastic deformation (util.elastic_field, util.elastic_prep) against independent
statements of what it should compute, the option checks, and the order of the feeders' random draws -- all on the host.

Bound of the fp32 field (test_linear_control_points_give_a_linear_field, and tests/test_hip_elastic.py for the device): with u =
2^-24, a correctly rounded fp32 operation has relative error at most u.  t and s are one rounded division each of exact integers.
Every Catmull-Rom weight is a product of sums of POSITIVE terms (util._catmull_rom_weights), so relative errors add and never
amplify: s^2, s t, t^2 carry 3 roundings (two operands, one product); 3 s t carries 4; (s^2 + 3 s t) + t^2 / 2 carries 4 + 2 = 6;
times s: 6 + 1 + 1 = 8 for w1 and w2, and 1 + 3 + 1 = 5 for w0 and w3.  A row sum ((w0 c0 + w1 c1) + w2 c2) + w3 c3 adds one
rounding per product and one per addition, each at most u times sum |w c|: 8 + 1 + 3 = 12.  The column stage repeats this on
the row sums: 12 + (8 + 1 + 3) = 24.  So |field32 - exact| <= K u sum_rs |w_r w_s c_rs| with K = 24 to first order in u (the
second-order terms are 2^-19 of that).  A fused multiply-add only removes roundings; the clamp is 1-Lipschitz."""
import itertools
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from supervised_gan_amd import util  # noqa: E402

K_FIELD = 24
U32 = 2.0 ** -24
WINDOWS = [(0, 0, 70), (61, 0, 70), (17, 9, 48), (130, 69, 1)]      # (x0, y0, n) in a 70 x 131 image (H0 = 70, W0 = 131)


def source(h=70, w=131, seed=0):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3), dtype=np.uint8)


def test_zero_control_points_are_the_plain_prep():
    import image_prep as IP
    img = source()
    for (x0, y0, n), flip, rot in itertools.product(WINDOWS, (False, True), range(4)):
        want = IP.prep_pil(img, x0, y0, n, flip, rot)
        for G, mask in ((1, 0), (3, 3), (13, 7)):
            got = util.elastic_prep(img, x0, y0, n, flip, rot, np.zeros((G + 3, G + 3, 2), np.float32), G, mask)
            assert got.dtype == np.float32 and np.array_equal(got, want), (x0, y0, n, flip, rot, G, mask)


def test_constant_integer_control_points_shift_the_window():
    """weights that sum to one, and the sign convention: the crop at (x0, y0) displaced by (3, -2) is the crop at (x0 + 3, y0 - 2)."""
    import image_prep as IP
    img = source()
    x0, y0, n = 17, 9, 48
    for G, mask, flip, rot in itertools.product((1, 3, 13), (0, 3, 7), (False, True), range(4)):
        ctrl = np.empty((G + 3, G + 3, 2), np.float32)
        ctrl[..., 0], ctrl[..., 1] = 3.0, -2.0
        got = util.elastic_prep(img, x0, y0, n, flip, rot, ctrl, G, mask)
        assert np.array_equal(got, IP.prep_pil(img, x0 + 3, y0 - 2, n, flip, rot)), (G, mask, flip, rot)


def test_linear_control_points_give_a_linear_field():
    """Catmull-Rom reproduces linear functions: control values linear in (r, s) give the field alpha + beta u G / n + gamma v G / n.
    The fp32 field within K u sum |w w c| of it (module docstring), the fp64 field within the same form at 2^-53."""
    worst = 0.0
    for n, G in ((70, 3), (70, 13), (48, 1), (1, 5), (33, 7)):
        r, s = np.meshgrid(np.arange(G + 3, dtype=np.float64), np.arange(G + 3, dtype=np.float64), indexing='ij')
        ctrl = np.stack([1.5 + 2.25 * (s - 1) - 0.75 * (r - 1), -3.0 + 0.5 * (s - 1) + 1.125 * (r - 1)], axis=-1)      # exact in fp32
        v, u = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing='ij')
        want = np.stack([1.5 + 2.25 * (u * G / n) - 0.75 * (v * G / n), -3.0 + 0.5 * (u * G / n) + 1.125 * (v * G / n)], axis=-1)
        assert np.abs(want).max() < 127
        # the analytic value is itself formed in fp64: three roundings per term and two additions, relative to the terms' magnitudes
        floor = 8 * 2.0 ** -53 * np.stack([1.5 + 2.25 * (u * G / n) + 0.75 * (v * G / n), 3.0 + 0.5 * (u * G / n) + 1.125 * (v * G / n)], axis=-1)
        f32, mag = util.elastic_field(ctrl.astype(np.float32), n, G, np.float32, return_abs=True)
        f64 = util.elastic_field(ctrl, n, G, np.float64)
        assert f32.dtype == np.float32 and f64.dtype == np.float64 and f32.shape == (n, n, 2)
        assert (np.abs(f64 - want) <= K_FIELD * 2.0 ** -53 * mag + floor).all()
        err = np.abs(f32.astype(np.float64) - want)
        assert (err <= K_FIELD * U32 * mag + floor).all(), (n, G, float((err / (U32 * mag)).max()))
        worst = max(worst, float((err / (U32 * mag)).max()))
    print(f"worst fp32 field error: {worst:.2f} of the allowed {K_FIELD} units of 2^-24 sum |w w c|")


def test_the_field_is_clamped():
    ctrl = np.full((4, 4, 2), 300.0, np.float32)
    ctrl[..., 1] = -300.0
    f = util.elastic_field(ctrl, 9, 1)
    assert np.array_equal(f[..., 0], np.full((9, 9), 127.0, np.float32)) and np.array_equal(f[..., 1], np.full((9, 9), -127.0, np.float32))


def _own_mirror(i, N):
    """reflection written independently of util: walk a triangle wave table."""
    if N == 1:
        return np.zeros_like(i)
    wave = np.concatenate([np.arange(N), np.arange(N - 2, 0, -1)])
    return wave[np.mod(i, len(wave))]


def _random_positions(img, x0, y0, n, G, sigma, seed):
    rng = np.random.RandomState(seed)
    ctrl = (rng.randn(G + 3, G + 3, 2) * sigma).astype(np.float32)
    return util.elastic_positions(util.elastic_field(ctrl, n, G), x0, y0)


@pytest.mark.parametrize("shape,window,G,sigma", [((70, 131), (17, 9, 48), 3, 10.0), ((70, 131), (61, 0, 70), 13, 10.0),
                                                  ((20, 20), (2, 3, 16), 3, 200.0), ((5, 1), (0, 2, 1), 1, 200.0)])
def test_integer_bilinear_against_scipy(shape, window, G, sigma):
    """scipy.ndimage.map_coordinates(order=1, mode='mirror') in fp64 at X / 256, Y / 256, rounded half up, is the integer result;
    only an exact tie of the numerator may differ, by one level, and ties are rare."""
    from scipy import ndimage
    img = source(*shape, seed=3)
    x0, y0, n = window
    X, Y = _random_positions(img, x0, y0, n, G, sigma, seed=4)
    if sigma > 100 and n > 1:
        assert (np.abs(X - (x0 + np.arange(n)[None, :]) * 256) == 127 * 256).any()      # the clamp is reached
        assert X.min() < -2 * 256 * (shape[1] - 1) or X.max() > 3 * 256 * (shape[1] - 1)      # more than one fold
    got = util.elastic_sample(img, X, Y, 0).astype(np.int64)
    ix, iy, fx, fy = X >> 8, Y >> 8, X & 255, Y & 255
    H0, W0 = shape
    p = lambda yy, xx: img[_own_mirror(yy, H0), _own_mirror(xx, W0)].astype(np.int64)      # noqa: E731
    num = (((256 - fx) * (256 - fy))[..., None] * p(iy, ix) + (fx * (256 - fy))[..., None] * p(iy, ix + 1)
           + ((256 - fx) * fy)[..., None] * p(iy + 1, ix) + (fx * fy)[..., None] * p(iy + 1, ix + 1))
    tie = num % 65536 == 32768
    assert tie.mean() < 0.01, tie.mean()
    for c in range(3):
        ref = ndimage.map_coordinates(img[..., c].astype(np.float64), [Y / 256.0, X / 256.0], order=1, mode='mirror')
        ref = np.floor(ref + 0.5).astype(np.int64)
        diff = np.abs(ref - got[..., c])
        assert (diff[~tie[..., c]] == 0).all() and (diff <= 1).all(), (c, int(diff.max()))


def test_nearest_channels_hold_source_values_only():
    img = source(seed=5)
    img[..., 0] = np.where(img[..., 0] > 127, 255, 0)      # a label channel
    img[..., 1] = (img[..., 1] // 64) * 64                 # four levels
    X, Y = _random_positions(img, 17, 9, 48, 3, 10.0, seed=6)
    out = util.elastic_sample(img, X, Y, 3)
    assert set(np.unique(out[..., 0])) <= {0, 255} and set(np.unique(out[..., 1])) <= set(np.unique(img[..., 1]))
    assert len(np.unique(out[..., 2])) > 4                 # the image channel is interpolated
    near = img[_own_mirror((Y + 128) >> 8, 70), _own_mirror((X + 128) >> 8, 131)]
    assert np.array_equal(out[..., :2], near[..., :2])
    binary = np.where(source(seed=7) > 127, 255, 0).astype(np.uint8)
    for G, sigma in ((3, 10.0), (13, 200.0)):
        ctrl = (np.random.RandomState(8).randn(G + 3, G + 3, 2) * sigma).astype(np.float32)
        t = util.elastic_prep(binary, 17, 9, 48, True, 1, ctrl, G, 7)
        assert set(np.unique(t)) <= {-1.0, 1.0}
    assert not set(np.unique(util.elastic_prep(binary, 17, 9, 48, True, 1, ctrl, G, 0))) <= {-1.0, 1.0}      # bilinear would not


@pytest.mark.parametrize("shape,window", [((20, 20), (2, 3, 16)), ((5, 1), (0, 2, 1)), ((1, 7), (3, 0, 1))])
def test_mirroring_over_several_folds(shape, window):
    """against np.pad(mode='reflect'), which folds as often as it takes and does not repeat the edge."""
    img = source(*shape, seed=9)
    H0, W0 = shape
    x0, y0, n = window
    X, Y = _random_positions(img, x0, y0, n, 2, 200.0, seed=10)
    P = 130
    padded = np.pad(img, ((P, P), (0, 0), (0, 0)), mode='reflect' if H0 > 1 else 'edge')
    padded = np.pad(padded, ((0, 0), (P, P), (0, 0)), mode='reflect' if W0 > 1 else 'edge')
    want = padded[((Y + 128) >> 8) + P, ((X + 128) >> 8) + P]
    assert np.array_equal(util.elastic_sample(img, X, Y, 7), want)
    whole = ((X >> 8) << 8), ((Y >> 8) << 8)      # integer positions: bilinear is the pixel itself
    assert np.array_equal(util.elastic_sample(img, whole[0], whole[1], 0), padded[(Y >> 8) + P, (X >> 8) + P])
    if n > 1:
        assert (X >> 8).min() < -(W0 - 1) and (X >> 8).max() > 2 * (W0 - 1)


def test_a_given_field_replaces_the_control_points():
    img = source(seed=11)
    ctrl = (np.random.RandomState(12).randn(6, 6, 2) * 10).astype(np.float32)
    field = util.elastic_field(ctrl, 48, 3)
    a = util.elastic_prep(img, 17, 9, 48, True, 3, ctrl, 3, 3)
    assert np.array_equal(a, util.elastic_prep(img, 17, 9, 48, True, 3, None, 3, 3, field=field))
    assert not np.array_equal(a, util.elastic_prep(img, 17, 9, 48, True, 3, None, 3, 3, field=np.zeros_like(field)))


# ------------------------------------------------------------------------------------------------------------------------------
# options and feeders
# ------------------------------------------------------------------------------------------------------------------------------
def _parse(extra, dataroot="/nowhere"):
    from supervised_gan_amd.options import TrainOptions
    return TrainOptions().parse(["--name", "t", "--gpu_ids", "-1", "--dataroot", dataroot] + extra, save=False, verbose=False)


def test_check_elastic_options():
    from supervised_gan_amd.options import TestOptions, elastic_nearest_mask
    opt = _parse([])
    assert opt.elastic is None and opt.elastic_label_channels == "rg"
    opt = _parse(["--elastic", "3", "10"])
    assert opt.elastic == (3, 10.0) and isinstance(opt.elastic[0], int) and elastic_nearest_mask(opt) == 3
    assert _parse(["--elastic", "13", "0"]).elastic == (13, 0.0)
    assert elastic_nearest_mask(_parse(["--elastic", "1", "2", "--elastic_label_channels", "b"])) == 4
    assert elastic_nearest_mask(_parse(["--elastic", "1", "2", "--elastic_label_channels", ""])) == 0
    for bad, msg in ((["--elastic", "0", "10"], "1..13"), (["--elastic", "14", "10"], "1..13"), (["--elastic", "2.5", "10"], "1..13"),
                     (["--elastic", "3", "-1"], "SIGMA"), (["--elastic", "3", "10", "--elastic_label_channels", "rx"], "letters")):
        with pytest.raises(AssertionError, match=msg):
            _parse(bad)
    with pytest.raises(AssertionError, match="synthetic feeder"):
        _parse(["--elastic", "3", "10"], dataroot="synthetic")
    assert "--elastic" in TrainOptions_help() and "not in the reference" in TrainOptions_help()
    with pytest.raises(SystemExit):      # the test drivers have no such option: they never deform
        TestOptions().parse(["--name", "t", "--gpu_ids", "-1", "--elastic", "3", "10"], save=False, verbose=False)


def TrainOptions_help():
    from supervised_gan_amd.options import TrainOptions
    to = TrainOptions()
    to.initialize()
    return " ".join(to.parser.format_help().split())


def test_validation_options_switch_elastic_off():
    import train_ss
    opt = _parse(["--elastic", "3", "10"])
    val = train_ss.validation_options(opt)
    assert val.elastic is None and opt.elastic == (3, 10.0) and val.no_flip and val.no_rotate


class _Recorder:
    """Stands in for the device ops of data.py on the host: records every call, returns an [n, n, 4] CPU buffer."""

    def __init__(self):
        self.calls = []

    def image_prep(self, dev, x0, y0, n, flip, rot):
        import torch
        self.calls.append(("plain", x0, y0, n, bool(flip), rot))
        return torch.zeros(n, n, 4)

    def image_prep_elastic(self, dev, x0, y0, n, flip, rot, ctrl, nearest_mask):
        import torch
        self.calls.append(("elastic", x0, y0, n, bool(flip), rot, ctrl.clone(), nearest_mask))
        return torch.zeros(n, n, 4)


def _write_png(path, w, h, seed):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.random.RandomState(seed).randint(0, 256, size=(h, w, 3), dtype=np.uint8), "RGB").save(path)


@pytest.mark.parametrize("mode", ["single", "aligned", "unaligned"])
def test_elastic_draws_come_after_the_existing_draws(tmp_path, monkeypatch, mode):
    """a seeded feeder draws the same crop, flip and rot with and without --elastic; the control values are the NEXT 2 (G + 3)^2
    random.gauss(0, SIGMA) draws, row-major with dx before dy; aligned halves share one field, unaligned images get one each; a feeder
    that does not train draws none.  The device ops are replaced by a recorder, so this runs on CPU tensors."""
    import torch
    from supervised_gan_amd import data, ops
    rec = _Recorder()
    monkeypatch.setattr(ops, "image_prep", rec.image_prep)
    monkeypatch.setattr(ops, "image_prep_elastic", rec.image_prep_elastic)
    root = tmp_path / mode
    if mode == "unaligned":
        _write_png(str(root / "trainA" / "a.png"), 50, 44, 1)
        _write_png(str(root / "trainB" / "b.png"), 47, 52, 2)
    else:
        _write_png(str(root / "train" / "a.png"), 80 if mode == "aligned" else 50, 40 if mode == "aligned" else 44, 1)
    size = ["--loadSize", "40", "--fineSize", "32"] + ([] if mode == "aligned" else ["--resize_or_crop", "crop"])
    base = ["--dataset_mode", mode, "--nThreads", "0", "--serial_batches"] + size

    def item0(extra, train=True):
        opt = _parse(base + extra, dataroot=str(root))
        opt.isTrain = train
        del rec.calls[:]
        random.seed(17)
        data.create_dataset(opt, device=torch.device("cpu"))[0]
        return list(rec.calls), random.random()      # the calls, and where the generator stands afterwards

    plain, after_plain = item0([])
    deformed, after_deformed = item0(["--elastic", "3", "10", "--elastic_label_channels", "gb"])
    assert len(plain) == len(deformed) == (1 if mode == "single" else 2)
    assert [c[0] for c in plain] == ["plain"] * len(plain) and [c[0] for c in deformed] == ["elastic"] * len(deformed)
    assert [c[1:6] for c in plain] == [c[1:6] for c in deformed]
    assert all(c[7] == 6 for c in deformed)
    # replay: the existing draws, then the fields
    random.seed(17)
    data.create_dataset(_parse(base, dataroot=str(root)), device=torch.device("cpu"))[0]
    fields = 2 if mode == "unaligned" else 1
    want = [torch.tensor([random.gauss(0.0, 10.0) for _ in range(72)], dtype=torch.float32).view(6, 6, 2) for _ in range(fields)]
    assert random.random() == after_deformed != after_plain
    assert torch.equal(deformed[0][6], want[0]) and torch.equal(deformed[-1][6], want[-1])
    if mode == "unaligned":
        assert not torch.equal(want[0], want[1])
    # a feeder that does not train makes no elastic draw and calls the plain kernel
    off, after_off = item0(["--elastic", "3", "10"], train=False)
    ref, after_ref = item0([], train=False)
    assert [c[0] for c in off] == ["plain"] * len(off) and off == ref and after_off == after_ref

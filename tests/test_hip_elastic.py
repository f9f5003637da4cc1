"""GPU tests of sgan_image_prep_elastic (csrc/sgan_elastic.hip) against the host yardsticks util.elastic_field and
util.elastic_prep, of the feeders that call it under --elastic, and of train_ss.py with it.

The field.  |field_out - elastic_field(float64)| <= K 2^-24 sum_rs |w_r w_s c_rs| per pixel and component, K = 24, the sum taken by
the yardstick in fp64.  K counts the roundings on the longest path of the kernel as written, each a relative 2^-24 of a quantity
bounded by the sum (tests/test_elastic_host.py derives it): t and s are one rounded division each; s s, s t, t t: 3 (two operands,
one product); 3 s t: 4; (s s + 3 s t) + t t / 2: 6; w1 = s (...): 8 (w0 = (-t / 2) s s: 5); a row ((w0 c0 + w1 c1) + w2 c2) + w3 c3:
8 + 1 product + 3 additions = 12; the column stage on the row sums: 12 + 8 + 1 + 3 = 24.  Every term inside a weight is positive, so
nothing amplifies; a contraction into a fused multiply-add removes a rounding; the clamp is 1-Lipschitz; second-order terms are
2^-19 of the bound.  The worst observed ratio is printed (run with -s).

The sampling.  From the float that was written everything is integer, so the output equals util.elastic_prep on the device's own
field read back, bit for bit.

Shapes: a 70 x 131 source with the windows (0, 0, 70), (61, 0, 70), (17, 9, 48), (130, 69, 1) -- 70 is not divisible by 3 or 13, 4900
pixels are 20 workgroups, the last one ragged -- every flip and rot, G in {1, 3, 13}, nearest_mask in {0, 3, 7}, SIGMA 10; a 20 x 20
source with SIGMA 200 (the clamp and several folds of the mirror); 5 x 1 and 1 x 5 sources with n = 1.  The output buffers cycle
through the 16-byte-store layouts (4 channels dense; 4 channels inside a 12 wide buffer) and the scalar ones (3, 5 and 8 channels)."""
import ctypes
import functools
import itertools
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from supervised_gan_amd import util  # noqa: E402

pytestmark = pytest.mark.gpu

K_FIELD = 24
U32 = 2.0 ** -24
WINDOWS = [(0, 0, 70), (61, 0, 70), (17, 9, 48), (130, 69, 1)]
LAYOUTS = [(4, False), (4, True), (3, False), (8, True), (5, True)]      # (stored channels, sliced out of a 3 C wide buffer)


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def source(h, w, seed=0):
    img = np.random.RandomState(seed).randint(0, 256, size=(h, w, 3), dtype=np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def control(G, sigma, seed):
    c = (np.random.RandomState(seed).randn(G + 3, G + 3, 2) * sigma).astype(np.float32)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference_field(G, sigma, seed, n):
    """(fp64 field, sum |w w c|) of control(G, sigma, seed) over an n x n crop: computed once, shared, never written."""
    f, mag = util.elastic_field(control(G, sigma, seed), n, G, np.float64, return_abs=True)
    f.setflags(write=False)
    mag.setflags(write=False)
    return f, mag


def run(img_dev, window, flip, rot, ctrl_dev, mask, layout=(4, False), want_field=True):
    """-> (out [n, n, C] numpy, field [n, n, 2] numpy or None); asserts the guards around both buffers."""
    from hip_utils import Guarded
    from supervised_gan_amd import ops
    x0, y0, n = window
    C, sliced = layout
    out = Guarded(n, n, C, sliced=sliced)
    fld = Guarded(n, n, 2) if want_field else None
    ops.image_prep_elastic(img_dev, x0, y0, n, flip, rot, ctrl_dev, mask, out=out.t, field_out=fld.t if fld else None)
    torch.cuda.synchronize()
    assert out.outside_intact() and out.finite_inside(), (window, flip, rot, mask, layout)
    if fld is not None:
        assert fld.outside_intact() and fld.finite_inside(), (window, flip, rot, mask, layout)
    return out.numpy(), (fld.numpy() if fld else None)


def check_case(img, img_dev, window, flip, rot, G, sigma, seed, mask, layout, ctrl_dev):
    """One launch against both yardsticks; returns the worst field error in units of 2^-24 sum |w w c|."""
    x0, y0, n = window
    got, field = run(img_dev, window, flip, rot, ctrl_dev, mask, layout)
    want_f, mag = reference_field(G, sigma, seed, n)
    err = np.abs(field.astype(np.float64) - want_f)
    ratio = float((err / np.maximum(U32 * mag, 1e-300)).max())
    assert (err <= K_FIELD * U32 * mag).all(), ("field", window, G, ratio)
    assert np.abs(field).max() <= 127.0
    want = util.elastic_prep(img, x0, y0, n, flip, rot, None, G, mask, field=field)
    assert np.array_equal(got[..., :3].transpose(2, 0, 1), want), ("sampling", window, flip, rot, G, mask, layout)
    assert (got[..., 3:] == 0).all(), ("padding channels", layout)
    return ratio


@pytest.mark.parametrize("G", [1, 3, 13])
def test_field_and_sampling_against_the_yardsticks(G):
    dev = _dev()
    img = source(70, 131)
    img_dev = torch.from_numpy(img.copy()).to(dev)
    sigma, seed = 10.0, 20 + G
    ctrl_dev = torch.from_numpy(control(G, sigma, seed).copy()).to(dev)
    worst, moved = 0.0, 0
    cases = itertools.product(WINDOWS, (False, True), range(4), (0, 3, 7))
    for k, (window, flip, rot, mask) in enumerate(cases):
        worst = max(worst, check_case(img, img_dev, window, flip, rot, G, sigma, seed, mask, LAYOUTS[k % len(LAYOUTS)], ctrl_dev))
        moved += 1
    assert np.abs(reference_field(G, sigma, seed, 70)[0]).max() > 3.0      # the crops really are deformed
    print(f"G = {G}: {moved} launches, worst field error {worst:.2f} of the allowed {K_FIELD} units of 2^-24 sum |w w c|")


@pytest.mark.parametrize("shape,window", [((20, 20), (2, 3, 16)), ((20, 20), (0, 0, 20)), ((5, 1), (0, 2, 1)), ((1, 5), (3, 0, 1))])
def test_clamp_and_several_folds(shape, window):
    dev = _dev()
    img = source(*shape, seed=1)
    img_dev = torch.from_numpy(img.copy()).to(dev)
    worst, k = 0.0, 0
    for G, flip, rot, mask in itertools.product((1, 3, 13), (False, True), (0, 1, 3), (0, 3, 7)):
        sigma, seed = 200.0, 40 + G
        ctrl_dev = torch.from_numpy(control(G, sigma, seed).copy()).to(dev)
        worst = max(worst, check_case(img, img_dev, window, flip, rot, G, sigma, seed, mask, LAYOUTS[k % len(LAYOUTS)], ctrl_dev))
        k += 1
    if window[2] > 1:
        f = reference_field(3, 200.0, 43, window[2])[0]
        assert (np.abs(f) == 127.0).any() and np.abs(f).max() * 256 > 3 * 256 * (shape[1] - 1)      # clamped; more than one fold
    print(f"{shape} {window}: worst field error {worst:.2f} of the allowed {K_FIELD} units")


def test_zero_control_points_are_image_prep_bit_for_bit():
    from supervised_gan_amd import ops
    dev = _dev()
    img_dev = torch.from_numpy(source(70, 131).copy()).to(dev)
    for k, ((x0, y0, n), flip, rot) in enumerate(itertools.product(WINDOWS, (False, True), range(4))):
        G, mask = (1, 3, 13)[k % 3], (0, 3, 7)[(k // 3) % 3]
        ctrl_dev = torch.zeros(G + 3, G + 3, 2, dtype=torch.float32, device=dev)
        plain = ops.image_prep(img_dev, x0, y0, n, flip, rot)
        got, field = run(img_dev, (x0, y0, n), flip, rot, ctrl_dev, mask)
        assert np.array_equal(got.view(np.int32), plain.cpu().numpy().view(np.int32)), ((x0, y0, n), flip, rot, G, mask)
        assert not field.any()


def test_without_field_out_the_output_is_the_same_and_the_kernel_is_recorded():
    from supervised_gan_amd import _lib as L
    dev = _dev()
    img_dev = torch.from_numpy(source(70, 131).copy()).to(dev)
    ctrl_dev = torch.from_numpy(control(3, 10.0, 23).copy()).to(dev)
    for window, layout, mask in (((61, 0, 70), (4, False), 3), ((17, 9, 48), (3, False), 0), ((17, 9, 48), (4, True), 7)):
        with_field, _ = run(img_dev, window, True, 1, ctrl_dev, mask, layout)
        assert b"image_prep_elastic" in L.lib().sgan_last_kernel()
        without, none = run(img_dev, window, True, 1, ctrl_dev, mask, layout, want_field=False)
        assert none is None and np.array_equal(with_field.view(np.int32), without.view(np.int32))


def test_refusals():
    from hip_utils import Guarded
    from supervised_gan_amd import _lib as L
    from supervised_gan_amd import ops
    dev = _dev()
    lib = L.lib()
    img_dev = torch.from_numpy(source(70, 131).copy()).to(dev)
    out = Guarded(48, 48, 4)
    ctrl = torch.zeros(17, 17, 2, dtype=torch.float32, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)      # noqa: E731

    def call(x0, y0, n, G, ctrl_t, rot=0):
        return lib.sgan_image_prep_elastic(P(img_dev), 70, 131, x0, y0, n, 0, rot, P(ctrl_t), G, 3, P(out.t), 4, 4, None, None)

    for args, msg in (((17, 9, 48, 0, ctrl), b"G = 0"), ((17, 9, 48, 14, ctrl), b"G = 14"), ((17, 9, 48, 3, None), b"control array"),
                      ((84, 9, 48, 3, ctrl), b"outside"), ((17, 23, 48, 3, ctrl), b"outside"), ((-1, 9, 48, 3, ctrl), b"outside"),
                      ((17, 9, 48, 3, ctrl, 4), b"rot")):
        assert call(*args) != 0 and msg in lib.sgan_last_error(), (args, lib.sgan_last_error())
    torch.cuda.synchronize()
    assert out.untouched()      # nothing was launched
    with pytest.raises(L.SganError, match="1..13"):
        ops.image_prep_elastic(img_dev, 17, 9, 48, False, 0, torch.zeros(3, 3, 2, dtype=torch.float32, device=dev), 3)
    with pytest.raises(L.SganError, match="MI355X"):
        ops.image_prep_elastic(img_dev.cpu(), 17, 9, 48, False, 0, ctrl, 3)
    assert call(17, 9, 48, 13, torch.zeros(16, 16, 2, dtype=torch.float32, device=dev)) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------------------
# feeders and driver
# ------------------------------------------------------------------------------------------------------------------------------
def _write_png(path, arr):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr, "RGB").save(path)


def _parse(argv):
    from supervised_gan_amd.options import TrainOptions
    return TrainOptions().parse(["--name", "t", "--gpu_ids", "0", "--nThreads", "0", "--serial_batches"] + argv, save=False, verbose=False)


def _device_field(img, window, ctrl, dev):
    """the field the device computes for these control points (the kernel is deterministic: the feeder's launch computed the same)."""
    return run(torch.from_numpy(img.copy()).to(dev), window, False, 0, torch.from_numpy(ctrl).to(dev), 0)[1]


def _gauss_ctrl(G, sigma):
    return np.array([random.gauss(0.0, sigma) for _ in range(2 * (G + 3) ** 2)], dtype=np.float32).reshape(G + 3, G + 3, 2)


def test_feeders_deform_with_the_documented_draws(tmp_path):
    from supervised_gan_amd.data import create_dataset
    dev = _dev()
    single, pair, ua, ub = source(44, 50, 2), source(40, 80, 3), source(44, 50, 4), source(52, 47, 5)
    _write_png(str(tmp_path / "single" / "train" / "a.png"), single)
    _write_png(str(tmp_path / "aligned" / "train" / "a.png"), pair)
    _write_png(str(tmp_path / "unaligned" / "trainA" / "a.png"), ua)
    _write_png(str(tmp_path / "unaligned" / "trainB" / "b.png"), ub)
    el = ["--elastic", "3", "10"]
    n = 32

    def item(mode, extra, train=True, seed=9):
        size = ["--loadSize", "40", "--fineSize", str(n)] + ([] if mode == "aligned" else ["--resize_or_crop", "crop"])
        opt = _parse(["--dataset_mode", mode, "--dataroot", str(tmp_path / mode)] + size + extra)
        opt.isTrain = train
        random.seed(seed)
        d = create_dataset(opt)[0]
        torch.cuda.synchronize()
        return {k: v[0].cpu().numpy() for k, v in d.items() if not k.endswith("paths")}

    def expect(img, x0, y0, flip, rot, ctrl):
        field = _device_field(img, (x0, y0, n), ctrl, dev)
        assert np.abs(field).max() > 1.0
        return util.elastic_prep(img, x0, y0, n, flip, rot, None, 3, 3, field=field)      # --elastic_label_channels rg: mask 3

    # single: x, y, flip, rot, then the field
    got = item("single", el)
    random.seed(9)
    x0, y0 = random.randint(0, 50 - n), random.randint(0, 44 - n)
    flip, rot = random.random() < 0.5, random.randint(0, 3)
    assert np.array_equal(got["A"], expect(single, x0, y0, flip, rot, _gauss_ctrl(3, 10.0)))
    assert not np.array_equal(got["A"], item("single", [])["A"])

    # aligned: the offsets and the flip, then ONE field for both halves
    got = item("aligned", el)
    random.seed(9)
    wo, ho = random.randint(0, 40 - n - 1), random.randint(0, 40 - n - 1)
    flip = random.random() < 0.5
    ctrl = _gauss_ctrl(3, 10.0)
    assert np.array_equal(got["A"], expect(pair, wo, ho, flip, 0, ctrl))
    assert np.array_equal(got["B"], expect(pair, 40 + wo, ho, flip, 0, ctrl))

    # unaligned: A's draws, B's draws, then A's field and B's field
    got = item("unaligned", el)
    random.seed(9)
    ax, ay = random.randint(0, 50 - n), random.randint(0, 44 - n)
    aflip, arot = random.random() < 0.5, random.randint(0, 3)
    bx, by = random.randint(0, 47 - n), random.randint(0, 52 - n)
    bflip, brot = random.random() < 0.5, random.randint(0, 3)
    ca, cb = _gauss_ctrl(3, 10.0), _gauss_ctrl(3, 10.0)
    assert np.array_equal(got["A"], expect(ua, ax, ay, aflip, arot, ca))
    assert np.array_equal(got["B"], expect(ub, bx, by, bflip, brot, cb))

    # a feeder that does not train never deforms
    for mode in ("single", "aligned", "unaligned"):
        off, ref = item(mode, el, train=False), item(mode, [], train=False)
        assert off.keys() == ref.keys() and all(np.array_equal(off[k], ref[k]) for k in off), mode


def _cell_image(h, w, seed):
    """the reference's data convention: r and g hold the labels (r = wall, g = cell interior, one-hot), b the image."""
    yy, xx = np.mgrid[:h, :w]
    wall = ((yy + seed) % 23 < 2) | ((xx + 2 * seed) % 19 < 2)
    img = np.zeros((h, w, 3), np.uint8)
    img[..., 0] = np.where(wall, 255, 0)
    img[..., 1] = 255 - img[..., 0]
    img[..., 2] = np.random.RandomState(seed).randint(0, 256, size=(h, w))
    return img


def test_train_ss_with_elastic_and_border_weight(tmp_path):
    import train_ss
    from supervised_gan_amd.data import create_dataset
    from supervised_gan_amd.options import TrainOptions
    _dev()
    root = tmp_path / "cells"
    for i in range(2):
        _write_png(str(root / "train" / ("t%d.png" % i)), _cell_image(140, 140, i))
    _write_png(str(root / "val" / "v0.png"), _cell_image(128, 128, 7))
    net = ["--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "single", "--loadSize", "140", "--fineSize", "128",
           "--valSize", "128", "--which_model_netG", "resnet_6blocks", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg",
           "--gpu_ids", "0", "--no_dropout", "--dataroot", str(root), "--manualSeed", "4", "--which_model_netD", "None", "--weights", "1", "2",
           "--border_weight", "10", "5", "--print_freq", "1", "--save_epoch_freq", "100", "--nThreads", "0", "--name", "el",
           "--checkpoints_dir", str(tmp_path / "ckpt")]
    model, _ = train_ss.main(net + ["--elastic", "3", "10", "--niter", "1", "--niter_decay", "0", "--max_steps", "2"])
    torch.cuda.synchronize()
    assert model.opt.elastic == (3, 10.0)
    loss = model.get_current_errors()["G_CE"]
    lines = [l for l in (tmp_path / "ckpt" / "el" / "loss_log.txt").read_text().splitlines() if l.startswith("(epoch:")]
    print(f"two steps with --elastic 3 10 --border_weight 10 5: last G_CE {loss!r}; {lines}")
    assert len(lines) == 2 and np.isfinite(loss)
    # the labels stayed one-hot through the deformation: the last TRAINING crop is not visible here (the validation pass came
    # after it), so draw one item of the same feeder
    opt = TrainOptions().parse(net + ["--elastic", "3", "10"], save=False, verbose=False)
    random.seed(1)
    rg = create_dataset(opt)[0]["A"][0, :2].cpu().numpy()
    assert set(np.unique(rg)) == {-1.0, 1.0} and (rg.sum(axis=0) == 0).all()
    # the validation feeder of the run is undeformed: its item is the plain feeder's
    val, plain = train_ss.validation_options(opt), train_ss.validation_options(TrainOptions().parse(net, save=False, verbose=False))
    assert val.elastic is None and val.isTrain
    random.seed(2)
    a = create_dataset(val)[0]["A"].clone()
    random.seed(2)
    b = create_dataset(plain)[0]["A"].clone()
    whole = util.elastic_prep(_cell_image(128, 128, 7), 0, 0, 128, False, 0, np.zeros((4, 4, 2), np.float32), 1, 0)      # = the plain prep
    assert torch.equal(a, b) and np.array_equal(a[0].cpu().numpy(), whole)

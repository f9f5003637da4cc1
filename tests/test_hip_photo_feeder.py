"""GPU tests of --photo_aug in the image-folder feeders (data.py) and in train_ss.py.

A seeded feeder with the option must yield util.photo_ref -- within util.photo_bounds, the counted interval of tests/test_hip_photo.py
-- of what the same feeder yields without it, under the record that util.photo_draw makes from the generator state the plain feeder
leaves behind, with noise planes that ops.normal_fill draws from the record's seed.  Without the option the feeder is the parent's:
the same bits as the prep kernels called directly, and `random` left in the state the documented draws leave it in."""
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

ALL = ["--photo_aug", "blur,gamma,contrast,brightness,noise,occlude", "--photo_prob", "1"]
SEED = 11


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def _cell_image(h, w, seed):
    """the reference's data convention: r and g hold the labels (r = wall, g = cell interior, one-hot), b the image."""
    yy, xx = np.mgrid[:h, :w]
    wall = ((yy + seed) % 23 < 2) | ((xx + 2 * seed) % 19 < 2)
    img = np.zeros((h, w, 3), np.uint8)
    img[..., 0] = np.where(wall, 255, 0)
    img[..., 1] = 255 - img[..., 0]
    img[..., 2] = np.random.RandomState(seed).randint(0, 256, size=(h, w))
    return img


def _write_png(path, arr):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr, "RGB").save(path)


def _folder(tmp_path):
    root = tmp_path / "cells"
    for i in range(2):
        _write_png(str(root / "train" / ("t%d.png" % i)), _cell_image(64, 64, i))
    return root


def _parse(argv):
    from supervised_gan_amd.options import TrainOptions
    return TrainOptions().parse(["--name", "t", "--gpu_ids", "0", "--nThreads", "0", "--serial_batches"] + argv, save=False, verbose=False)


def _item(opt, seed=SEED):
    """(item 0 of a fresh feeder as {key: [H, W, 3] numpy}, the state `random` is left in)."""
    from supervised_gan_amd.data import create_dataset
    random.seed(seed)
    d = create_dataset(opt)[0]
    torch.cuda.synchronize()
    return {k: v[0].permute(1, 2, 0).contiguous().cpu().numpy() for k, v in d.items() if not k.endswith("paths")}, random.getstate()


def _noise_halves(seed, halves, n):
    """the N(0, 1) planes of the halves of one item: ONE fill of halves * n * n values from stream offset 0 -- n * n is a multiple of
    4, so the second half of that fill is the stream from the offset that follows the first half."""
    from supervised_gan_amd import ops
    assert (n * n) % 4 == 0
    buf = torch.empty(halves, 1, n, n, dtype=torch.float32, device="cuda")
    ops.normal_fill(buf, seed, None, advance=False)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _inside(got, plain, rec, noise, what):
    lo, hi = util.photo_bounds(plain, rec, 0b100, noise)
    g = got.astype(np.float64)
    assert ((lo <= g) & (g <= hi)).all(), (what, float(np.maximum(lo - g, g - hi).max()))
    assert np.array_equal(got[..., :2].view(np.int32), plain[..., :2].view(np.int32)), ("labels", what)
    ref = util.photo_ref(plain, rec, 0b100, noise)
    assert np.abs(ref[..., 2] - plain[..., 2]).max() > 0.05, "the record changes the image"


@pytest.mark.parametrize("mode", ["single", "aligned"])
def test_feeder_applies_the_drawn_record(tmp_path, mode):
    _dev()
    root = _folder(tmp_path)
    n = 48 if mode == "single" else 24
    size = ["--resize_or_crop", "crop", "--fineSize", "48"] if mode == "single" else ["--loadSize", "32", "--fineSize", "24"]
    base = ["--dataset_mode", mode, "--dataroot", str(root)] + size
    plain, state = _item(_parse(base))
    opt = _parse(base + ALL)
    got, state_after = _item(opt)
    # the record: photo_draw on the state the plain draws leave behind; the feeder's own state afterwards says it drew the same
    random.setstate(state)
    rec = util.photo_draw(opt, n)
    assert random.getstate() == state_after != state
    assert rec.R >= 2 and rec.gamma != 1.0 and rec.contrast != 1.0 and rec.brightness != 0.0 and rec.sigma_n > 0.0 and len(rec.boxes) == 2
    keys = ["A"] if mode == "single" else ["A", "B"]
    assert sorted(got) == sorted(plain) == keys
    noise = _noise_halves(rec.seed, len(keys), n)
    for i, k in enumerate(keys):
        _inside(got[k], plain[k], rec, noise[i], (mode, k))
    if mode == "aligned":
        assert not np.array_equal(noise[0], noise[1])
    # the other seed, the other record
    other, _ = _item(opt, seed=SEED + 1)
    assert not np.array_equal(other["A"], got["A"])


@pytest.mark.parametrize("mode", ["single", "aligned"])
def test_without_the_option_the_feeder_is_unchanged(tmp_path, mode):
    """the prep kernels called directly with the documented draws give the feeder's 'A' bit for bit, and `random` stands where those
    draws leave it: no line of the feature ran."""
    from PIL import Image
    from supervised_gan_amd import ops
    dev = _dev()
    root = _folder(tmp_path)
    img = np.array(Image.open(str(root / "train" / "t0.png")).convert("RGB"), dtype=np.uint8)
    if mode == "single":
        opt = _parse(["--dataset_mode", "single", "--dataroot", str(root), "--resize_or_crop", "crop", "--fineSize", "48"])
        got, state = _item(opt)
        random.seed(SEED)
        x0, y0 = random.randint(0, 64 - 48), random.randint(0, 64 - 48)
        flip, rot = random.random() < 0.5, random.randint(0, 3)
        want = {"A": ops.image_prep(torch.from_numpy(img).to(dev), x0, y0, 48, flip, rot)}
    else:
        opt = _parse(["--dataset_mode", "aligned", "--dataroot", str(root), "--loadSize", "32", "--fineSize", "24"])
        got, state = _item(opt)
        random.seed(SEED)
        wo, ho = random.randint(0, 32 - 24 - 1), random.randint(0, 32 - 24 - 1)
        flip = random.random() < 0.5
        small = ops.image_resize(torch.from_numpy(img).to(dev), 64, 32, "bicubic")
        want = {"A": ops.image_prep(small, wo, ho, 24, flip, 0), "B": ops.image_prep(small, 32 + wo, ho, 24, flip, 0)}
    assert random.getstate() == state
    assert opt.photo_aug is None
    for k, v in want.items():
        assert np.array_equal(got[k].view(np.int32), v[..., :3].cpu().numpy().view(np.int32)), (mode, k)


@pytest.mark.parametrize("mode", ["single", "aligned"])
def test_a_validation_feeder_makes_no_photometric_draw(tmp_path, mode):
    import train_ss
    _dev()
    root = _folder(tmp_path)
    _write_png(str(root / "val" / "v0.png"), _cell_image(64, 64, 7))
    base = ["--dataset_mode", mode, "--dataroot", str(root), "--loadSize", "32", "--fineSize", "24", "--valSize", "32"]
    val, ref = train_ss.validation_options(_parse(base + ALL)), train_ss.validation_options(_parse(base))
    assert val.photo_aug is None and val.isTrain
    (a, state_a), (b, state_b) = _item(val), _item(ref)
    assert state_a == state_b and a.keys() == b.keys() and all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)
    # and a feeder that does not train at all: the option is still set, nothing is drawn
    opt = _parse(base + ALL)
    opt.isTrain = False
    plain = _parse(base)
    plain.isTrain = False
    (a, state_a), (b, state_b) = _item(opt), _item(plain)
    assert state_a == state_b and all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)


def test_train_ss_two_graphed_steps_with_every_stage(tmp_path):
    import train_ss
    _dev()
    root = _folder(tmp_path)
    _write_png(str(root / "val" / "v0.png"), _cell_image(64, 64, 7))
    net = ["--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "single", "--loadSize", "64", "--fineSize", "64",
           "--valSize", "64", "--which_model_netG", "resnet_6blocks", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg",
           "--gpu_ids", "0", "--no_dropout", "--dataroot", str(root), "--manualSeed", "4", "--which_model_netD", "None", "--weights", "1", "2",
           "--print_freq", "1", "--save_epoch_freq", "100", "--nThreads", "0", "--name", "photo", "--checkpoints_dir", str(tmp_path / "ckpt")]
    model, _ = train_ss.main(net + ALL + ["--graph", "--niter", "1", "--niter_decay", "0", "--max_steps", "2"])
    torch.cuda.synchronize()
    assert model.opt.photo_aug == util.PHOTO_STAGES and model.opt.photo_prob == 1.0
    loss = model.get_current_errors()["G_CE"]
    lines = [l for l in (tmp_path / "ckpt" / "photo" / "loss_log.txt").read_text().splitlines() if l.startswith("(epoch:")]
    print(f"two graphed steps with every photometric stage: last G_CE {loss!r}; {lines}")
    assert len(lines) == 2 and np.isfinite(loss)
    for l in lines:
        assert "nan" not in l.lower() and "inf" not in l.lower(), l

"""Host tests of the photometric augmentation (--photo_aug); no GPU: the taps, the float64 yardstick util.photo_ref
against scipy and against three-line formulas, the interval of util.photo_bounds, the parameter draw util.photo_draw and its place in
the feeders' sequence of draws (a recording stub stands in for `random`), and the option checks."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from supervised_gan_amd import util  # noqa: E402
from supervised_gan_amd.util import PhotoRec  # noqa: E402


def crop(h, w, c=4, seed=0):
    """[h, w, c] fp32 in [-1, 1] on the grid of sgan_image_prep (v / 255 * 2 - 1), the last channel zero like a padding channel."""
    x = (np.random.RandomState(seed).randint(0, 256, size=(h, w, c)).astype(np.float32) / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)
    x[..., -1] = 0.0
    return x


@pytest.mark.parametrize("sigma", [0.2, 0.5, 1.0, 1.7, 2.0, 3.99, 4.0, 10.0])
def test_taps_follow_the_rule_and_sum_to_one(sigma):
    w = util.photo_taps(sigma)
    R = len(w) - 1
    assert w.dtype == np.float32 and R == min(12, int(np.ceil(3 * sigma))) and 1 <= R <= util.PHOTO_MAX_R
    # 2 R + 1 values, each rounded once: the sum is within (2 R + 1) half-ulps of the largest tap, itself below 1
    assert abs(float(w[0].astype(np.float64) + 2.0 * w[1:].astype(np.float64).sum()) - 1.0) <= (2 * R + 1) * 2.0 ** -25
    k = np.arange(R + 1, dtype=np.float64)
    want = np.exp(-k * k / (2 * sigma * sigma))
    want /= want[0] + 2 * want[1:].sum()
    assert np.array_equal(w, want.astype(np.float32)) and (np.diff(w) < 0).all() and (w > 0).all()


@pytest.mark.parametrize("shape,sigma", [((13, 13), 4.0), ((33, 47), 1.3), ((9, 30), 2.5)])
def test_blur_is_scipy_correlate1d_mirror_twice(shape, sigma):
    from scipy import ndimage
    x = crop(*shape)
    w = util.photo_taps(sigma)
    if len(w) - 1 > min(shape) - 1:
        w = w[: min(shape)]
    rec = PhotoRec(taps=w)
    got = util.photo_ref(x, rec, 0b101)
    full = np.concatenate([w[:0:-1], w]).astype(np.float64)
    for c in (0, 2):
        rows = ndimage.correlate1d(x[..., c].astype(np.float64), full, axis=1, mode="mirror")
        want = ndimage.correlate1d(rows, full, axis=0, mode="mirror")
        assert np.abs(got[..., c] - want).max() <= 1e-14
    assert np.array_equal(got[..., 1], x[..., 1].astype(np.float64)) and np.array_equal(got[..., 3], x[..., 3].astype(np.float64))


def test_each_point_stage_is_its_formula():
    x = crop(21, 18)
    s = x[..., 2].astype(np.float64)
    yy, xx = np.mgrid[:21, :18]
    noise = np.random.RandomState(3).randn(1, 21, 18).astype(np.float32)
    g, c, b, sn = (float(np.float32(v)) for v in (0.7, 1.2, -0.05, 0.04))
    cases = [
        (PhotoRec(gamma=g), None, np.clip(2 * np.clip(0.5 * s + 0.5, 0, 1) ** g - 1, -1, 1)),
        (PhotoRec(contrast=c), None, np.clip(c * s, -1, 1)),
        (PhotoRec(brightness=b), None, np.clip(s + 2 * b, -1, 1)),
        (PhotoRec(contrast=c, brightness=b), None, np.clip(c * s + 2 * b, -1, 1)),
        (PhotoRec(sigma_n=sn), noise, np.clip(s + sn * noise[0].astype(np.float64), -1, 1)),
        (PhotoRec(sigma_n=sn), None, s),                                    # no planes: the stage is neutral
        (PhotoRec(boxes=[(2, 9, 3, 30, 0.25), (-4, 4, 0, 5, -1.0), (7, 7, 0, 18, 0.5)]), None,
         np.where((yy < 4) & (xx < 5), -1.0, np.where((yy >= 2) & (yy < 9) & (xx >= 3), 0.25, s))),
    ]
    for rec, nz, want in cases:
        got = util.photo_ref(x, rec, 0b100, nz)
        assert np.abs(got[..., 2] - want).max() <= 1e-15, rec
        assert np.array_equal(got[..., [0, 1, 3]], x[..., [0, 1, 3]].astype(np.float64)), rec
        lo, hi = util.photo_bounds(x, rec, 0b100, nz)
        assert (lo <= got).all() and (got <= hi).all() and (hi - lo).max() <= 64 * 2.0 ** -24, rec
        assert np.array_equal(lo[..., [0, 1, 3]], hi[..., [0, 1, 3]])


def test_all_neutral_returns_its_input_and_a_point_interval():
    x = crop(13, 17)
    for mask, nz in ((0b101, None), (0b100, np.ones((1, 13, 17), np.float32)), (0, None)):
        got = util.photo_ref(x, PhotoRec(), mask, nz)
        lo, hi = util.photo_bounds(x, PhotoRec(), mask, nz)
        assert np.array_equal(got, x.astype(np.float64)) and np.array_equal(lo, got) and np.array_equal(hi, got)


def test_bounds_hold_an_fp32_evaluation_and_stay_narrow():
    """The interval contains a plain NumPy fp32 evaluation of the same expressions (not the device's, which may fuse where NumPy
    rounds twice, but inside the same count), and is a few hundred roundings wide at most -- near u = 0 with gamma < 1 too, where
    the interval of pow maps end points instead of scaling an error."""
    x = crop(40, 33, seed=5)
    x[:6, :, 2] = -1.0      # u = 0 under the gamma stage
    x[6:9, :, 2] = np.float32(-1.0 + 2.0 ** -20)
    noise = np.random.RandomState(6).randn(1, 40, 33).astype(np.float32)
    rec = PhotoRec(taps=util.photo_taps(1.5), gamma=0.5, contrast=1.2, brightness=0.03, sigma_n=0.05, boxes=[(30, 35, 2, 9, 0.5)])
    lo, hi = util.photo_bounds(x, rec, 0b100, noise)
    f = np.float32
    s = x[..., 2]
    for axis in (1, 0):
        idx = np.arange(s.shape[axis])
        acc = rec.w[0] * s
        for k in range(1, rec.R + 1):
            acc = f(rec.w[k]) * (np.take(s, util._mirror_index(idx - k, len(idx)), axis=axis)
                                 + np.take(s, util._mirror_index(idx + k, len(idx)), axis=axis)) + acc
        s = acc.astype(f)
    u = np.clip(f(0.5) * s + f(0.5), 0, 1).astype(f)
    s = f(2) * np.power(u.astype(np.float64), rec.gamma).astype(f) - f(1)
    s = f(rec.contrast) * s + f(2 * rec.brightness)
    s = np.clip(f(rec.sigma_n) * noise[0] + s, -1, 1).astype(f)
    s[30:35, 2:9] = 0.5
    assert s.dtype == np.float32 and (lo[..., 2] <= s).all() and (s <= hi[..., 2]).all()
    ref = util.photo_ref(x, rec, 0b100, noise)
    assert (lo <= ref).all() and (ref <= hi).all()
    # the square root near zero turns an input interval of ~2^-22 into ~2^-11: end points are mapped, nothing is scaled
    assert (hi - lo)[..., 2].max() < 2e-3 and np.median((hi - lo)[9:, :, 2]) < 300 * 2.0 ** -24


class _Opt:
    photo_aug = util.PHOTO_STAGES
    photo_prob, photo_blur, photo_gamma, photo_contrast, photo_brightness, photo_noise, photo_occlude = 0.5, 2.0, 1.5, 0.25, 0.1, 0.05, (2, 0.25)


class _Counting(random.Random):
    """random.Random that records (method, value) of every draw made through random() or getrandbits()."""

    def __init__(self, seed):
        super().__init__(seed)
        self.log = []

    def random(self):
        v = super().random()
        self.log.append(("random", v))
        return v

    def getrandbits(self, k):
        v = super().getrandbits(k)
        self.log.append(("getrandbits", v))
        return v


def test_photo_draw_is_deterministic_counts_its_draws_and_stays_in_range():
    n, opt = 64, _Opt()
    extra = {"blur": 1, "gamma": 1, "contrast": 1, "brightness": 1, "noise": 2, "occlude": 5 * opt.photo_occlude[0]}
    fired_any = {s: 0 for s in util.PHOTO_STAGES}
    for seed in range(60):
        rng = _Counting(seed)
        rec = util.photo_draw(opt, n, rng=rng)
        again = util.photo_draw(opt, n, rng=_Counting(seed))
        assert repr(rec) == repr(again) and np.array_equal(rec.w, again.w)
        # replay the gates from the log: a gate, then the stage's own draws when it fired
        pos, fired = 0, []
        for stage in util.PHOTO_STAGES:
            assert rng.log[pos][0] == "random"
            hit = rng.log[pos][1] < opt.photo_prob
            pos += 1 + (extra[stage] if hit else 0)
            fired += [stage] if hit else []
        assert pos == len(rng.log) == 6 + sum(extra[s] for s in fired), (seed, fired, len(rng.log))
        assert [m for m, _ in rng.log].count("getrandbits") == ("noise" in fired)
        for s in fired:
            fired_any[s] += 1
        assert (rec.R > 0) == ("blur" in fired) and rec.R <= min(12, int(np.ceil(3 * opt.photo_blur)))
        assert (1 / 1.5) * (1 - 1e-6) <= rec.gamma <= 1.5 * (1 + 1e-6) and 0.75 <= rec.contrast <= 1.25 and abs(rec.brightness) <= 0.1
        assert 0.0 <= rec.sigma_n <= 0.05 and 0 <= rec.seed < 2 ** 64 and len(rec.boxes) == (2 if "occlude" in fired else 0)
        for y0, y1, x0, x1, v in rec.boxes:
            assert 0 <= y0 < y1 <= n and 0 <= x0 < x1 <= n and 1 <= y1 - y0 <= 16 and 1 <= x1 - x0 <= 16 and -1.0 <= v <= 1.0
        if not fired:
            assert repr(rec) == repr(PhotoRec())
    assert all(10 <= v <= 50 for v in fired_any.values()), fired_any
    # a stage that is not listed draws nothing, not even its gate; prob 0 and 1
    only = _Opt()
    only.photo_aug, only.photo_prob = ("gamma", "noise"), 1.0
    rng = _Counting(1)
    rec = util.photo_draw(only, n, rng=rng)
    assert [m for m, _ in rng.log] == ["random", "random", "random", "random", "getrandbits"] and rec.R == 0 and not rec.boxes
    only.photo_prob = 0.0
    rng = _Counting(1)
    assert repr(util.photo_draw(only, n, rng=rng)) == repr(PhotoRec()) and len(rng.log) == 2


# ------------------------------------------------------------------------------------------------------------------------------
# options and feeders
# ------------------------------------------------------------------------------------------------------------------------------
def _parse(extra, dataroot="/nowhere"):
    from supervised_gan_amd.options import TrainOptions
    return TrainOptions().parse(["--name", "t", "--gpu_ids", "-1", "--dataroot", dataroot] + extra, save=False, verbose=False)


def test_check_photo_options():
    from supervised_gan_amd.options import TestOptions, photo_channel_mask
    opt = _parse([])
    assert opt.photo_aug is None and opt.photo_prob == 0.5 and opt.photo_channels == "b"
    opt = _parse(["--photo_aug", "noise,blur, gamma"])
    assert opt.photo_aug == ("blur", "gamma", "noise") and opt.photo_occlude == (2, 0.25) and isinstance(opt.photo_occlude[0], int)
    assert (opt.photo_blur, opt.photo_gamma, opt.photo_contrast, opt.photo_brightness, opt.photo_noise) == (2.0, 1.5, 0.25, 0.1, 0.05)
    assert photo_channel_mask(opt) == 4
    both = _parse(["--photo_aug", "blur,gamma,contrast,brightness,noise,occlude", "--photo_channels", "rb", "--elastic_label_channels", "g"])
    assert both.photo_aug == util.PHOTO_STAGES and photo_channel_mask(both) == 5
    assert _parse(["--photo_aug", "blur", "--photo_blur", "4", "--fineSize", "13"]).photo_blur == 4.0      # R = 12 = fineSize - 1
    on = ["--photo_aug", "blur,occlude"]
    for bad, msg in ((["--photo_aug", "blur,sharpen"], "comma list"), (["--photo_aug", "blur,blur"], "comma list"), (["--photo_aug", ""], "comma list"),
                     (on + ["--photo_prob", "1.5"], "probability"), (on + ["--photo_prob", "-0.1"], "probability"),
                     (on + ["--photo_blur", "4.5"], "SMAX"), (on + ["--photo_blur", "0.25"], "SMAX"),
                     (on + ["--photo_gamma", "2.5"], "G <= 2"), (on + ["--photo_gamma", "0.9"], "G <= 2"),
                     (on + ["--photo_contrast", "1"], "C < 1"), (on + ["--photo_contrast", "-0.1"], "C < 1"),
                     (on + ["--photo_brightness", "-1"], "negative"), (on + ["--photo_noise", "-1"], "negative"),
                     (on + ["--photo_noise", "nan"], "finite"), (on + ["--photo_brightness", "inf"], "finite"),
                     (on + ["--photo_occlude", "5", "0.25"], "K boxes"), (on + ["--photo_occlude", "0", "0.25"], "K boxes"),
                     (on + ["--photo_occlude", "1.5", "0.25"], "K boxes"), (on + ["--photo_occlude", "2", "0"], "K boxes"),
                     (on + ["--photo_occlude", "2", "1.5"], "K boxes"),
                     (on + ["--photo_channels", "bx"], "letters"), (on + ["--photo_channels", ""], "letters"),
                     (on + ["--photo_channels", "gb"], "share a channel"),
                     (on + ["--photo_blur", "4", "--fineSize", "12"], "reaches 12 pixels"),
                     (on + ["--photo_blur", "2", "--fineSize", "6"], "reaches 6 pixels")):
        with pytest.raises(AssertionError, match=msg):
            _parse(bad)
    assert _parse(["--photo_aug", "gamma", "--fineSize", "6"]).photo_aug == ("gamma",)      # no blur: the crop need not hold its reach
    assert _parse(["--photo_channels", "gb"]).photo_aug is None                            # option off: nothing is checked
    with pytest.raises(AssertionError, match="synthetic feeder"):
        _parse(on, dataroot="synthetic")
    to = __import__("supervised_gan_amd.options", fromlist=["TrainOptions"]).TrainOptions()
    to.initialize()
    assert "--photo_aug" in to.parser.format_help() and "--photo_occlude" in to.parser.format_help()
    with pytest.raises(SystemExit):      # the test drivers have no such option
        TestOptions().parse(["--name", "t", "--gpu_ids", "-1", "--photo_aug", "blur"], save=False, verbose=False)


def test_validation_options_switch_photo_aug_off():
    import train_ss
    opt = _parse(["--photo_aug", "blur,noise", "--elastic", "3", "10"])
    val = train_ss.validation_options(opt)
    assert val.photo_aug is None and val.elastic is None and opt.photo_aug == ("blur", "noise")


class _RandomLog:
    """Stands in for the `random` module inside data.py: one seeded random.Random whose every call is recorded by name and result."""

    def __init__(self, seed):
        self._r = random.Random(seed)
        self.log = []

    def __getattr__(self, name):
        fn = getattr(self._r, name)

        def call(*a, **k):
            v = fn(*a, **k)
            self.log.append((name, a, v))
            return v
        return call


class _Device:
    """Stands in for the device ops of data.py on the host: records every call, returns [n, n, 4] CPU buffers."""

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

    def normal_fill(self, dst, seed, offset_dev=None, advance=True):
        self.calls.append(("normal_fill", tuple(dst.shape), seed, offset_dev is not None, advance))

    def image_photo(self, src, rec, mask, noise=None, out=None):
        import torch
        self.calls.append(("photo", repr(rec), mask, None if noise is None else tuple(noise.shape)))
        return torch.ones_like(src)


def _write_png(path, w, h, seed):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.random.RandomState(seed).randint(0, 256, size=(h, w, 3), dtype=np.uint8), "RGB").save(path)


ALL = ["--photo_aug", "blur,gamma,contrast,brightness,noise,occlude", "--photo_prob", "1"]


@pytest.mark.parametrize("mode", ["single", "aligned", "unaligned"])
@pytest.mark.parametrize("elastic", [[], ["--elastic", "3", "10"]])
def test_photo_draws_come_after_every_other_draw(tmp_path, monkeypatch, mode, elastic):
    """The feeder's calls into `random`, recorded by a stub: with --photo_aug the sequence BEGINS with the sequence without it, call
    for call -- crop, flip, rot and the elastic field keep their draws -- and what follows is photo_draw's sequence, once per item
    (single, aligned) or once per image (unaligned).  The prep calls are the same; one photo call per crop follows them, an aligned
    pair sharing the record with a noise fill per half.  A feeder that does not train makes no photometric draw."""
    import torch
    from supervised_gan_amd import data, ops
    dev = _Device()
    for name in ("image_prep", "image_prep_elastic", "normal_fill", "image_photo"):
        monkeypatch.setattr(ops, name, getattr(dev, name))
    root = tmp_path / mode
    if mode == "unaligned":
        _write_png(str(root / "trainA" / "a.png"), 50, 44, 1)
        _write_png(str(root / "trainB" / "b.png"), 47, 52, 2)
    else:
        _write_png(str(root / "train" / "a.png"), 80 if mode == "aligned" else 50, 40 if mode == "aligned" else 44, 1)
    size = ["--loadSize", "40", "--fineSize", "32"] + ([] if mode == "aligned" else ["--resize_or_crop", "crop"])
    base = ["--dataset_mode", mode, "--nThreads", "0", "--serial_batches"] + size + elastic

    def item0(extra, train=True):
        opt = _parse(base + extra, dataroot=str(root))
        opt.isTrain = train
        del dev.calls[:]
        stub = _RandomLog(17)
        monkeypatch.setattr(data, "random", stub)
        item = data.create_dataset(opt, device=torch.device("cpu"))[0]
        return list(dev.calls), stub.log, item, opt

    plain_calls, plain_log, plain_item, _ = item0([])
    calls, log, item, opt = item0(ALL)
    assert log[: len(plain_log)] == plain_log and len(plain_log) >= 3
    records = 2 if mode == "unaligned" else 1
    tail = log[len(plain_log):]
    per_record = 6 + 1 + 1 + 1 + 1 + 2 + 5 * 2
    assert len(tail) == records * per_record and [t[0] for t in tail].count("getrandbits") == records
    # replaying the tail through photo_draw gives the records the kernel was called with
    replay = random.Random(17)
    for name, a, v in plain_log:
        assert getattr(replay, name)(*a) == v
    want = [repr(util.photo_draw(opt, 32, rng=replay)) for _ in range(records)]
    preps = [c for c in calls if c[0] in ("plain", "elastic")]
    photos = [c for c in calls if c[0] == "photo"]
    fills = [c for c in calls if c[0] == "normal_fill"]
    assert [c[:6] for c in preps] == [c[:6] for c in plain_calls] and len(photos) == len(preps) == (1 if mode == "single" else 2)
    assert [c[1] for c in photos] == (want if mode != "aligned" else want * 2) and all(c[2] == 4 and c[3] == (1, 32, 32) for c in photos)
    assert len(fills) == len(photos) and all(c[1] == (1, 32, 32) and c[3] and c[4] for c in fills)
    assert all((v == 1).all() for k, v in item.items() if not k.endswith("paths")) and all((v == 0).all() for k, v in plain_item.items() if not k.endswith("paths"))
    # a feeder that does not train draws nothing photometric and calls nothing new
    off_calls, off_log, _, _ = item0(ALL, train=False)
    ref_calls, ref_log, _, _ = item0([], train=False)
    assert off_calls == ref_calls and off_log == ref_log and not [c for c in off_calls if c[0] in ("photo", "normal_fill")]

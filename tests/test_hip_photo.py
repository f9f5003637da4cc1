"""GPU tests of sgan_image_photo (csrc/sgan_photo.hip) against the host yardsticks util.photo_ref / util.photo_bounds.

Every value the kernel computes must lie in the interval photo_bounds derives by counting roundings -- (2 R + 2) per blur pass, one
per fused multiply-add of a point stage, PHOTO_POW_ULP ulps for powf, end points mapped through the monotone stages -- and every
channel it only copies must come back bit for bit; there is no tolerance to tune.  The share of the interval that was used is
printed (run with -s).

Shapes, the smallest at which the kernel can go wrong: 13 x 13 with R = 12 (the reach is the side minus one: every halo pixel is a
mirrored one, some folded twice over the ragged tile), 33 x 47 (rectangular, no multiple of the 32 x 32 tile, four workgroups),
64 x 64 (exact tiles), 65 x 31 (three tile rows, one ragged column).  Layouts: 4 stored channels dense (the 16-byte path), and 4
channels at pixel stride 5 read / 8 written (the scalar path; stride 5 is not 16-byte aligned).  Masks 0b100 (the default: b holds
the image) and 0b101.  One 8-channel case with five masked channels walks the scalar path's second group of LDS planes."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from supervised_gan_amd import util  # noqa: E402
from supervised_gan_amd.util import PhotoRec  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(13, 13), (33, 47), (64, 64), (65, 31)]
LAYOUTS = [("vec4", None, None), ("scalar", 5, 8)]      # (name, src pixel stride, dst pixel stride); None: dense
MASKS = [0b100, 0b101]


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def crop(h, w, c=4, seed=0):
    """[h, w, c] fp32: the image channels on sgan_image_prep's grid in [-1, 1] with both ends and a value just above -1 present (u = 0
    and u ~ 2^-21 under the gamma stage); channel 1 and the last channel hold arbitrary BIT PATTERNS (NaNs and denormals among them):
    a channel that is only copied must come back with its bits."""
    rs = np.random.RandomState(seed)
    x = ((rs.randint(0, 256, size=(h, w, c)).astype(np.float32) / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5))
    x[0, :, :] = -1.0
    x[1, :, :] = 1.0
    x[2, :, :] = np.float32(-1.0 + 2.0 ** -20)
    for ch in (1, c - 1):
        x[..., ch] = rs.randint(-2 ** 31, 2 ** 31, size=(h, w), dtype=np.int64).astype(np.int32).view(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def planes(p, h, w, seed=1):
    z = np.random.RandomState(seed).randn(p, h, w).astype(np.float32)
    z.setflags(write=False)
    return z


def records(h, w):
    """name -> PhotoRec: each stage alone, then all together."""
    taps = util.photo_taps(4.0 if min(h, w) > 12 else 0.3 * (min(h, w) - 1))
    assert len(taps) - 1 == min(12, min(h, w) - 1)
    boxes = [(2, h // 2, 3, w // 2 + 1, 0.25), (h // 3, h // 3 + 4, -2, w + 5, -0.5)]
    return {
        "blur R=%d" % (len(taps) - 1): PhotoRec(taps=taps),
        "blur R=1": PhotoRec(taps=util.photo_taps(0.3)),
        "gamma 0.5": PhotoRec(gamma=0.5),
        "gamma 2": PhotoRec(gamma=2.0),
        "gamma 1.37": PhotoRec(gamma=1.37),
        "contrast": PhotoRec(contrast=1.25),
        "brightness": PhotoRec(brightness=-0.1),
        "noise": PhotoRec(sigma_n=0.05),
        "occlude": PhotoRec(boxes=boxes),
        "all": PhotoRec(taps=util.photo_taps(1.7), gamma=0.61, contrast=0.8, brightness=0.07, sigma_n=0.04, boxes=boxes),
    }


def run(x, rec, mask, noise, src_ld=None, dst_ld=None):
    """One launch on guarded buffers -> the [H, W, C] result; the memory around both views must keep its bits."""
    from hip_utils import Guarded
    from supervised_gan_amd import ops
    H, W, C = x.shape
    src = Guarded(H, W, C, ld=src_ld or C, off=0)
    src.t.view(torch.int32).copy_(torch.from_numpy(x.view(np.int32).copy()))      # the bits, not a float conversion
    src.snap = src.store.view(torch.int32).clone()
    dst = Guarded(H, W, C, ld=dst_ld or C, off=0)
    nz = None if noise is None else torch.from_numpy(noise.copy()).cuda()
    ops.image_photo(src.t, rec, mask, noise=nz, out=dst.t)
    torch.cuda.synchronize()
    assert src.untouched() and dst.outside_intact(), (x.shape, rec, mask)
    return dst.numpy()


def check(x, rec, mask, noise, got, what):
    """got inside photo_bounds, copied channels bit for bit -> the largest used share of the interval's half width."""
    lo, hi = util.photo_bounds(x, rec, mask, noise)
    C = x.shape[2]
    copied = [c for c in range(C) if not (mask >> c) & 1]
    assert np.array_equal(got[..., copied].view(np.int32), x[..., copied].view(np.int32)), ("copied channels", what)
    masked = [c for c in range(C) if (mask >> c) & 1]
    g, l, h = got[..., masked].astype(np.float64), lo[..., masked], hi[..., masked]
    bad = ~((l <= g) & (g <= h))
    assert not bad.any(), (what, int(bad.sum()), float(np.max(np.maximum(l - g, g - h))))
    ref = util.photo_ref(x, rec, mask, noise)[..., masked]
    half = np.maximum(np.maximum(h - ref, ref - l), 1e-300)
    exact = h == l
    assert np.array_equal(g[exact], ref[exact])
    return float((np.abs(g - ref) / half)[~exact].max()) if (~exact).any() else 0.0


@pytest.mark.parametrize("shape", SHAPES)
def test_every_stage_alone_and_all_together_inside_the_bounds(shape):
    _dev()
    h, w = shape
    x = crop(h, w)
    worst = {}
    for (lname, sld, dld), mask in ((l, m) for l in LAYOUTS for m in MASKS):
        noise = planes(bin(mask).count("1"), h, w)
        for name, rec in records(h, w).items():
            nz = noise if rec.sigma_n else None
            got = run(x, rec, mask, nz, sld, dld)
            share = check(x, rec, mask, nz, got, (shape, lname, bin(mask), name))
            worst[name] = max(worst.get(name, 0.0), share)
            if name == "all" and lname == "vec4":
                again = run(x, rec, mask, nz, sld, dld)
                assert np.array_equal(got.view(np.int32), again.view(np.int32)), "two runs, two results"
    print(f"{h} x {w}: largest share of the allowed interval used, per case: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


@pytest.mark.parametrize("shape", SHAPES)
def test_all_neutral_copies_every_bit(shape):
    from supervised_gan_amd import _lib as L
    _dev()
    h, w = shape
    x = crop(h, w)
    for (lname, sld, dld), mask in ((l, m) for l in LAYOUTS for m in MASKS + [0, 0b1111]):
        nz = planes(bin(mask).count("1"), h, w) if mask else None
        for rec, noise in ((PhotoRec(), None), (PhotoRec(), nz), (PhotoRec(boxes=[(3, 3, 0, w, 0.5), (5, 2, 1, 4, 0.5)]), None)):
            got = run(x, rec, mask, noise, sld, dld)      # sigma_n == 0 with planes given, and empty boxes, are neutral too
            assert np.array_equal(got.view(np.int32), x.view(np.int32)), (shape, lname, bin(mask))
            assert b"sg_image_photo_kernel" in L.lib().sgan_last_kernel()


def test_boxes_hold_their_value_exactly():
    _dev()
    h, w = 33, 47
    x = crop(h, w)
    yy, xx = np.mgrid[:h, :w]
    v = [float(np.float32(t)) for t in (0.3, -0.7, 1.0, 0.123456789)]
    cases = [
        ([(4, 4, 0, w, v[0])], np.zeros((h, w), bool), None),                                            # empty
        ([(0, h, 0, w, v[1])], np.ones((h, w), bool), np.full((h, w), v[1])),                             # the whole crop
        ([(-5, 6, w - 3, w + 40, v[2])], (yy < 6) & (xx >= w - 3), np.full((h, w), v[2])),                # across two borders
        ([(2, 20, 2, 30, v[0]), (10, 33, 20, 40, v[3])], ((yy >= 2) & (yy < 20) & (xx >= 2) & (xx < 30)) | ((yy >= 10) & (xx >= 20) & (xx < 40)),
         np.where((yy >= 10) & (xx >= 20) & (xx < 40), v[3], v[0])),                                      # the later box wins
        ([(0, 9, 0, 9, v[0]), (0, 9, 0, 9, v[1]), (40, 50, 0, 9, v[2]), (31, 34, 31, 34, v[3])],
         ((yy < 9) & (xx < 9)) | ((yy >= 31) & (xx >= 31) & (xx < 34)), np.where(yy < 9, v[1], v[3])),    # four, one outside the crop
    ]
    for (lname, sld, dld), mask in ((l, m) for l in LAYOUTS for m in MASKS):
        for boxes, inside, value in cases:
            for extra in ({}, {"taps": util.photo_taps(1.0), "gamma": 0.8, "contrast": 1.1}):
                rec = PhotoRec(boxes=boxes, **extra)
                got = run(x, rec, mask, None, sld, dld)
                check(x, rec, mask, None, got, (lname, bin(mask), boxes))
                for c in range(4):
                    if (mask >> c) & 1:
                        assert inside.any() == (value is not None)
                        if value is not None:
                            assert np.array_equal(got[..., c][inside], value[inside].astype(np.float32)), (lname, bin(mask), boxes, c)
                        if not extra:
                            assert np.array_equal(got[..., c][~inside].view(np.int32), x[..., c][~inside].view(np.int32))


def test_a_constant_image_stays_inside_the_blur_bound():
    _dev()
    for (h, w), value in (((13, 13), 0.3), ((65, 31), -1.0), ((33, 47), 1.0), ((64, 64), 0.7372549)):
        x = np.zeros((h, w, 4), np.float32)
        x[..., 2] = value
        x[..., 0] = -value
        rec = PhotoRec(taps=util.photo_taps(4.0))
        for lname, sld, dld in LAYOUTS:
            got = run(x, rec, 0b101, None, sld, dld)
            share = check(x, rec, 0b101, None, got, ("constant", (h, w), lname))
            # the bound itself is tight here: two passes of (2 R + 2) roundings around a value the taps reproduce to their own rounding
            lo, hi = util.photo_bounds(x, rec, 0b101)
            assert (hi - lo)[..., 2].max() <= 2 * 2 * (2 * rec.R + 2) * 2.0 ** -24 * 1.01 and share <= 1.0


def test_five_masked_channels_of_eight_walk_two_groups_of_planes():
    _dev()
    h, w = 33, 47
    x = crop(h, w, c=8, seed=3)
    mask = 0b01011101      # channel 1 and 7 are copied (arbitrary bits), 5 is copied too
    x = x.copy()
    x[..., 5] = crop(h, w, c=8, seed=4)[..., 1]
    noise = planes(5, h, w, seed=9)
    for name, rec in records(h, w).items():
        nz = noise if rec.sigma_n else None
        for sld, dld in ((8, 8), (9, 24)):
            check(x, rec, mask, nz, run(x, rec, mask, nz, sld, dld), ("8 channels", name, sld, dld))


def test_refusals():
    from hip_utils import Guarded
    from supervised_gan_amd import _lib as L
    from supervised_gan_amd import ops
    _dev()
    lib = L.lib()
    h, w = 16, 20
    src = Guarded(h, w, 4, data=np.zeros((h, w, 4), np.float32))
    dst = Guarded(h, w, 4)
    noise = torch.zeros(1, h, w, device="cuda")
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off if t is not None else 0)      # noqa: E731
    NAN, INF = float("nan"), float("inf")

    def call(rec=PhotoRec(), s=P(src.t), d=P(dst.t), H=h, W=w, Cs=4, mask=0b100, sld=4, dld=4, patch=None, norec=False):
        r = ops.photo_record(rec)
        for k, v in (patch or {}).items():
            if isinstance(k, tuple):
                getattr(r, k[0])[k[1]] = v
            else:
                setattr(r, k, v)
        return lib.sgan_image_photo(s, sld, d, dld, H, W, Cs, mask, None if norec else ctypes.byref(r), P(noise), None)

    taps13 = util.photo_taps(4.0)
    cases = [
        (dict(s=P(None)), b"null"), (dict(d=P(None)), b"null"), (dict(norec=True), b"null"),
        (dict(d=P(src.t)), b"overlap"), (dict(d=P(src.t, 16 * 7)), b"overlap"), (dict(s=P(dst.t, 4 * (h * w * 4 - 1))), b"overlap"),
        (dict(patch={"R": 13}), b"radius 13"), (dict(patch={"R": -1}), b"radius -1"),
        (dict(rec=PhotoRec(taps=taps13), H=12), b"radius 12"), (dict(rec=PhotoRec(taps=taps13), W=12), b"radius 12"),
        (dict(patch={"gamma": 0.4999}), b"gamma"), (dict(patch={"gamma": 2.0001}), b"gamma"), (dict(patch={"gamma": NAN}), b"not finite"),
        (dict(patch={"contrast": 0.0}), b"contrast"), (dict(patch={"contrast": -1.0}), b"contrast"), (dict(patch={"contrast": INF}), b"not finite"),
        (dict(patch={"brightness": NAN}), b"not finite"), (dict(patch={"brightness": -INF}), b"not finite"),
        (dict(patch={"sigma_n": -0.1}), b"sigma_n"), (dict(patch={"sigma_n": INF}), b"not finite"),
        (dict(rec=PhotoRec(taps=util.photo_taps(1.0)), patch={("w", 2): NAN}), b"tap 2"),
        (dict(rec=PhotoRec(boxes=[(0, 1, 0, 1, 0.0)]), patch={("box_value", 0): NAN}), b"box 0"),
        (dict(patch={"nbox": 5}), b"5 boxes"), (dict(patch={"nbox": -1}), b"-1 boxes"),
        (dict(mask=0b10000), b"mask"), (dict(mask=-1), b"mask"), (dict(mask=0b1000, Cs=3, sld=4, dld=4), b"mask"),
        (dict(H=(1 << 22) + 1, W=1), b"sides"), (dict(H=1, W=(1 << 22) + 1), b"sides"), (dict(H=0), b"sides"),
        (dict(sld=3), b"stride"), (dict(Cs=0), b"stored channels"),
    ]
    for kw, msg in cases:
        assert call(**kw) == 1 and msg in lib.sgan_last_error(), (kw, lib.sgan_last_error())
    torch.cuda.synchronize()
    assert dst.untouched() and src.untouched()      # nothing was launched
    with pytest.raises(L.SganError, match="gamma"):
        ops.image_photo(src.t, PhotoRec(gamma=3.0), 0b100, out=dst.t)
    with pytest.raises(L.SganError, match="boxes"):
        ops.image_photo(src.t, PhotoRec(boxes=[(0, 1, 0, 1, 0.0)] * 5), 0b100, out=dst.t)
    with pytest.raises(L.SganError, match="MI355X"):
        ops.image_photo(src.t.cpu(), PhotoRec(), 0b100)
    assert dst.untouched()
    # the edge of every range is accepted: R = 12 = min(H, W) - 1, gamma 0.5 and 2, four boxes, a tap beyond R that is not finite
    assert call(rec=PhotoRec(taps=taps13, gamma=0.5, boxes=[(0, 1, 0, 1, 0.0)] * 4), H=13, W=13) == 0
    assert call(rec=PhotoRec(taps=util.photo_taps(0.3), gamma=2.0), patch={("w", 5): NAN}) == 0
    torch.cuda.synchronize()
    assert dst.finite_inside()

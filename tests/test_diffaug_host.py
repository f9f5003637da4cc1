"""--diffaug without a GPU: the parameter draw of util.diffaug_params against a restatement made directly with philox_ref, the forward
and backward yardsticks (util.diffaug_ref, util.diffaug_bwd_ref) against torch fp64 and its autograd, the options, the exported
symbols, and that a trainer without the option never builds the augmentation state."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_ref as P  # noqa: E402

from supervised_gan_amd import util  # noqa: E402

ALL = ("translation", "cutout", "brightness", "contrast")


def restated(seed, offset, shapes, policy, rt, rc):
    """The issue's definition, word by word, on philox_ref.philox4x32_10."""
    out = []
    for j, (H, W) in enumerate(shapes):
        w = []
        for blk in (0, 1):
            ctr = (offset + 2 * j + blk) & (2 ** 64 - 1)
            w += [int(v[0]) for v in P.philox4x32_10(ctr & 0xFFFFFFFF, ctr >> 32, 0, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)]
        b = (w[0] >> 8) * 2.0 ** -24 - 0.5 if "brightness" in policy else 0.0
        a = float(np.float32((w[1] >> 8) * 2.0 ** -24 + 0.5)) if "contrast" in policy else 1.0      # an fp32 sum: rounded from 1 up
        ty = tx = cy0 = cy1 = cx0 = cx1 = 0
        if "translation" in policy:
            Sy, Sx = int(np.floor(H * rt + 0.5)), int(np.floor(W * rt + 0.5))
            ty, tx = -Sy + w[2] % (2 * Sy + 1), -Sx + w[3] % (2 * Sx + 1)
        if "cutout" in policy:
            ch, cw = int(np.floor(H * rc + 0.5)), int(np.floor(W * rc + 0.5))
            oy, ox = w[4] % (H + 1 - ch % 2), w[5] % (W + 1 - cw % 2)
            cy0, cy1, cx0, cx1 = max(0, oy - ch // 2), min(H, oy - ch // 2 + ch), max(0, ox - cw // 2), min(W, ox - cw // 2 + cw)
        out.append((b, a, ty, tx, cy0, cy1, cx0, cx1))
    return out


@pytest.mark.parametrize("seed,offset", [(0, 0), (5 + 7919, 6), (2 ** 40 + 3, 2 ** 32 - 1), (2 ** 64 - 1, 2 ** 64 - 2)])
@pytest.mark.parametrize("policy", [ALL, ("translation",), ("cutout", "contrast"), ("brightness",), ()])
def test_params_equal_the_restatement(seed, offset, policy):
    shapes = [(128, 128), (7, 9), (33, 31)]
    got = util.diffaug_params(seed, offset, shapes, policy, 0.125, 0.5)
    assert got == restated(seed, offset, shapes, policy, 0.125, 0.5)
    for b, a, *_ in got:      # fp32 values
        assert float(np.float32(b)) == b and float(np.float32(a)) == a and -0.5 <= b < 0.5 and 0.5 <= a <= 1.5


def test_switching_an_operation_off_leaves_the_others():
    shapes = [(64, 48), (9, 8)]
    full = util.diffaug_params(11, 40, shapes, ALL)
    idx = {"brightness": [0], "contrast": [1], "translation": [2, 3], "cutout": [4, 5, 6, 7]}
    neutral = {"brightness": [0.0], "contrast": [1.0], "translation": [0, 0], "cutout": [0, 0, 0, 0]}
    for off in ALL:
        part = util.diffaug_params(11, 40, shapes, [p for p in ALL if p != off])
        for rf, rp in zip(full, part):
            for op in ALL:
                want = neutral[op] if op == off else [rf[i] for i in idx[op]]
                assert [rp[i] for i in idx[op]] == want, (off, op)


def test_offset_use_is_two_blocks_per_job():
    shapes = [(16, 16)] * 3
    a = util.diffaug_params(3, 100, shapes, ALL)
    assert util.diffaug_params(3, 102, shapes[:2], ALL) == a[1:]      # job j of a call at `offset` is job 0 of a call at offset + 2 j
    assert util.diffaug_params(3, 100 + 2 * 3, shapes[:1], ALL)[0] not in a
    assert len(set(a)) == 3


@pytest.mark.parametrize("H", [1, 2, 7, 8, 9])
@pytest.mark.parametrize("W", [1, 2, 7, 8, 9])
def test_ranges(H, W):
    for rt, rc in ((0.125, 0.5), (1.0, 1.0), (0.3, 0.7), (0.0, 0.0)):
        Sy, Sx = int(np.floor(H * rt + 0.5)), int(np.floor(W * rt + 0.5))
        ch, cw = int(np.floor(H * rc + 0.5)), int(np.floor(W * rc + 0.5))
        seen = set()
        for off in range(0, 80, 2):
            b, a, ty, tx, cy0, cy1, cx0, cx1 = util.diffaug_params(1, off, [(H, W)], ALL, rt, rc)[0]
            assert -Sy <= ty <= Sy and -Sx <= tx <= Sx
            assert 0 <= cy0 <= cy1 <= H and 0 <= cx0 <= cx1 <= W and cy1 - cy0 <= ch and cx1 - cx0 <= cw
            seen.add(ty)
        assert seen == {0} if Sy == 0 else len(seen) > 1      # 40 draws over 2 Sy + 1 >= 3 values


# ---- forward and backward yardsticks against torch fp64 ------------------------------------------------------------------------------
def torch_diffaug(x, rec, col):
    """DiffAugment's operations in its order on x [1, C, H, W] fp64: brightness, contrast about the mean, zero-padded translate,
    cutout mask -- F.pad and slicing, none of util's code."""
    b, a, ty, tx, cy0, cy1, cx0, cx1 = rec
    _, C, H, W = x.shape
    col = torch.tensor(col, dtype=torch.bool)
    if col.any():
        xc = x[:, col] + b
        mean = xc.mean(dim=[1, 2, 3], keepdim=True)
        xc = (xc - mean) * a + mean
        parts, k = [], 0
        for c in range(C):
            if col[c]:
                parts.append(xc[:, k:k + 1])
                k += 1
            else:
                parts.append(x[:, c:c + 1])
        x = torch.cat(parts, 1)
    xp = F.pad(x, (W, W, H, H))      # out[h][w] = x[h + ty][w + tx], zeros outside
    x = xp[:, :, H + ty: 2 * H + ty, W + tx: 2 * W + tx] if abs(ty) <= H and abs(tx) <= W else torch.zeros_like(x)
    mask = torch.ones(H, W, dtype=x.dtype)
    mask[cy0:cy1, cx0:cx1] = 0
    return x * mask


RECS = [(0.0, 1.0, 0, 0, 0, 0, 0, 0), (0.25, 1.5, 2, -3, 0, 0, 0, 0), (-0.5, 0.5, -6, 8, 1, 4, 0, 5), (0.1, 1.25, 0, 0, 0, 7, 0, 9),
        (0.3, 0.75, 7, 0, 0, 0, 0, 0), (0.0, 1.0, 1, 1, 5, 7, 6, 9)]


@pytest.mark.parametrize("rec", RECS)
@pytest.mark.parametrize("mask", [0b100, 0b011, 0b000, 0b111])
def test_forward_and_backward_equal_torch(rec, mask):
    rng = np.random.default_rng(7)
    H, W, C = 7, 9, 3
    x = rng.standard_normal((H, W, C))
    dy = rng.standard_normal((H, W, C))
    col = [(mask >> c) & 1 for c in range(C)]
    xt = torch.tensor(x.transpose(2, 0, 1)[None], dtype=torch.float64, requires_grad=True)
    yt = torch_diffaug(xt, rec, col)
    y = util.diffaug_ref(x, rec, mask)
    assert np.abs(y - yt.detach()[0].permute(1, 2, 0).numpy()).max() <= 1e-12
    yt.backward(torch.tensor(dy.transpose(2, 0, 1)[None]))
    dx = util.diffaug_bwd_ref(dy, rec, mask)
    assert np.abs(dx - xt.grad[0].permute(1, 2, 0).numpy()).max() <= 1e-12
    # the adjoint identity of the linear part
    assert abs(np.sum((y - util.diffaug_ref(np.zeros_like(x), rec, mask)) * dy) - np.sum(x * dx)) <= 1e-10


# ---- options ---------------------------------------------------------------------------------------------------------------------------
CGAN = ["--model", "cgan", "--which_channel", "rg_b"]


def _parse(argv):
    from supervised_gan_amd.options import TrainOptions
    return TrainOptions().parse(argv, save=False, verbose=False)


def test_options_default_is_off():
    opt = _parse(CGAN)
    assert opt.diffaug is None and opt.diffaug_policy is None
    assert opt.diffaug_translation == 0.125 and opt.diffaug_cutout == 0.5 and opt.diffaug_color_channels == "b"


def test_color_expands_and_order_is_fixed():
    from supervised_gan_amd import diffaug
    opt = _parse(CGAN + ["--diffaug", "color,cutout"])
    assert opt.diffaug_policy == ("cutout", "brightness", "contrast")
    assert _parse(CGAN + ["--diffaug", "translation,cutout,color"]).diffaug_policy == ALL
    assert diffaug.policy_bits(ALL) == 15 and diffaug.policy_bits(("cutout",)) == 2
    assert diffaug.parse_policy("contrast, translation") == ("translation", "contrast")


def test_colour_mask_follows_the_discriminator_input():
    from supervised_gan_amd import diffaug
    mk = lambda argv: (lambda o: diffaug.colour_mask(diffaug.input_letters(o), o.diffaug_color_channels))(_parse(argv))      # noqa: E731
    assert mk(CGAN) == 0b100                                          # cat(r, g | b): the image is position 2
    assert mk(CGAN + ["--no_cgan"]) == 0b001                          # the discriminators see b alone
    assert mk(["--model", "segmentation", "--which_channel", "b_rg"]) == 0b001      # cat(b | class scores)
    assert mk(["--model", "fcgan", "--which_channel", "rg_b"]) == 0b100
    assert mk(["--model", "fcgan", "--which_channel", "rg", "--diffaug_color_channels", "g"]) == 0b010


@pytest.mark.parametrize("argv,message", [
    (CGAN + ["--diffaug", "translation,rotate"], "unknown operation 'rotate'"),
    (CGAN + ["--diffaug", ","], "a comma list of"),
    (["--model", "fcgan", "--which_channel", "rg", "--diffaug", "color"], "none of the channels 'b'"),
    (["--model", "segmentation", "--which_channel", "b_rg", "--no_cgan", "--diffaug", "brightness"], "none of the channels 'b'"),
    (["--model", "cgan_cycle", "--diffaug", "cutout"], "fcgan, cgan, cgan2, segmentation"),
    (["--model", "twostage", "--diffaug", "cutout"], "fcgan, cgan, cgan2, segmentation"),
    (["--model", "segmentation", "--which_channel", "b_rg", "--which_model_netD", "None", "--diffaug", "cutout"], "--which_model_netD None"),
    (CGAN + ["--diffaug", "cutout", "--diffaug_cutout", "1.5"], "a ratio of 0 .. 1 (got 1.5)"),
    (CGAN + ["--diffaug", "translation", "--diffaug_translation", "nan"], "a ratio of 0 .. 1 (got nan)"),
], ids=["unknown", "empty", "fcgan_no_colour", "segm_no_cgan_no_colour", "cycle", "twostage", "no_netD", "ratio", "nan"])
def test_options_refuse(argv, message, capsys):
    with pytest.raises(SystemExit):
        _parse(argv)
    err = capsys.readouterr().err
    assert message in err and "unrecognized" not in err


def test_geometry_only_policy_needs_no_colour_channel():
    assert _parse(["--model", "fcgan", "--which_channel", "rg", "--diffaug", "translation,cutout"]).diffaug_policy == ("translation", "cutout")


def test_unsupported_trainer_refuses_at_construction():
    """A trainer outside the supported set refuses the option even for an options object that skipped the parser's check."""
    from supervised_gan_amd.base_model import BaseModel
    from supervised_gan_amd.cgan_cycle_model import CGANCycleModel
    from supervised_gan_amd.cgan_model import CGANModel
    from supervised_gan_amd.fcgan_model import FCGANModel
    from supervised_gan_amd.segm_model import SegmentationModel
    opt = _parse(CGAN + ["--diffaug", "cutout", "--gpu_ids", "-1"])
    opt.model = "cgan_cycle"
    with pytest.raises(NotImplementedError, match="fcgan, cgan, cgan2, segmentation"):
        BaseModel.initialize(CGANCycleModel(), opt)
    assert not BaseModel.supports_diffaug and not CGANCycleModel.supports_diffaug
    assert FCGANModel.supports_diffaug and CGANModel.supports_diffaug and SegmentationModel.supports_diffaug


def test_without_the_option_no_state_is_built(monkeypatch):
    """_init_diffaug and _augment of a trainer whose options lack --diffaug: DiffAugment is never constructed, the tensors pass as
    they are; with the option the constructor is reached."""
    from supervised_gan_amd import diffaug
    from supervised_gan_amd.cgan_model import CGANModel
    built = []
    monkeypatch.setattr(diffaug.DiffAugment, "__init__", lambda self, *a, **k: built.append(a))
    for extra, n in (([], 0), (["--diffaug", "translation"], 1)):
        opt = _parse(CGAN + ["--gpu_ids", "-1"] + extra)
        m = CGANModel()
        from supervised_gan_amd.base_model import BaseModel
        BaseModel.initialize(m, opt)
        m._rng_seed = 5
        m._init_diffaug(True)
        assert len(built) == n and (m.diffaug is None) == (n == 0)
        if n == 0:
            ts = [object(), object()]
            assert m._augment(ts, 0) is ts
    with pytest.raises(ValueError, match="which_model_netD None"):
        m._init_diffaug(False)


# ---- library -----------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_entries(built_lib):
    lib = ctypes.CDLL(built_lib)
    from supervised_gan_amd import _lib
    for name in ("sgan_diffaug_draw", "sgan_diffaug_multi_fwd", "sgan_diffaug_multi_bwd", "sgan_diffaug_workspace"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert ctypes.sizeof(_lib.DiffaugJob) == 40
    lib.sgan_diffaug_workspace.restype = ctypes.c_int64
    assert lib.sgan_diffaug_workspace(2) == 2 * 256 * 8 and lib.sgan_diffaug_workspace(0) < 0 and lib.sgan_diffaug_workspace(9) < 0

"""GPU tests of whole-image inference in SegmentationModel.test() (--whole_image / --tile / --tile_margin / --tile_ramp / --tta d4,
DESIGN.md R21): the geometry end to end with a context-free stub in place of the generator, the one-tile plan against the plain test()
of the same network, and a many-tile image through the accuracies.  Inputs are handed to set_input() as the single-image feeder hands
them over: 'A' (the whole image, ops.image_prep_tile over the full window) and 'A_u8' (the uint8 device image)."""
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

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
E_P = 1e-6                       # the per-element bound of the softmax kernel tests (tests/test_hip_ops.py:1036), as in tests/test_hip_tile.py


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def _net_argv(ckpt, channels="b_rg", extra=()):
    return ["--name", "tile", "--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "single", "--fineSize", "128",
            "--which_model_netG", "unet_128", "--ngf", "4", "--norm", "instance", "--which_channel", channels, "--gpu_ids", "0", "--no_dropout",
            "--checkpoints_dir", str(ckpt), "--manualSeed", "4"] + list(extra)


def _checkpoint(ckpt, channels="b_rg", extra=()):
    """A freshly initialised unet_128 saved as `latest`, for the evaluation models to load."""
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    opt = TrainOptions().parse(_net_argv(ckpt, channels, extra) + ["--dataroot", "synthetic", "--which_model_netD", "None"], save=False, verbose=False)
    create_model(opt).save("latest")


def _eval_model(ckpt, channels="b_rg", extra=()):
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TestOptions
    opt = TestOptions().parse(_net_argv(ckpt, channels, extra) + ["--dataroot", str(ckpt / "images")], save=False, verbose=False)
    return create_model(opt)


def _feed(img):
    """What data.SingleFolderDataset yields under --whole_image for the uint8 image `img` [H, W, 3]."""
    from supervised_gan_amd import ops
    u8 = torch.from_numpy(np.ascontiguousarray(img)).to(_dev())
    H, W = img.shape[:2]
    return {"A": ops.logical_view(ops.image_prep_tile(u8, 0, 0, H, W, False, 0), 3), "A_u8": u8, "A_paths": ["image.png"]}


def _walls(H, W, seed):
    """r: a wall grid (255 / 0), g: its complement, b: noise -- a label map with cells for the label-based scores."""
    yy, xx = np.mgrid[:H, :W]
    wall = ((yy % 16 < 2) | (xx % 20 < 2)).astype(np.uint8) * 255
    return np.stack([wall, 255 - wall, np.random.RandomState(seed).randint(0, 256, size=(H, W), dtype=np.uint8)], axis=2)


class _Pixelwise:
    """In place of netG: logits_k = sum_c x_c A[k][c] + b_k per pixel, in fp32 with one rounding per operation -- no conv, no
    statistics, so tiling cannot change what a pixel gets."""

    def __init__(self, A, b):
        self.A, self.b = A, b

    def forward(self, x, noise=None, activation=None):
        rows = []
        for k in range(len(self.b)):
            z = x[:, 0:1] * self.A[k][0]
            for c in range(1, x.shape[1]):
                z = z + x[:, c:c + 1] * self.A[k][c]
            rows.append(z + self.b[k])
        return torch.cat(rows, dim=1)

    def host(self, x):
        """The same operations on a float32 [cin, H, W] numpy array -> float32 [K, H, W]."""
        rows = []
        for k in range(len(self.b)):
            z = x[0] * np.float32(self.A[k][0])
            for c in range(1, x.shape[0]):
                z = z + x[c] * np.float32(self.A[k][c])
            rows.append(z + np.float32(self.b[k]))
        return np.stack(rows).astype(np.float32)


@pytest.mark.parametrize("tta", [False, True])
@pytest.mark.parametrize("channels,extra,picked", [("b_rg", (), [2]), ("rb_g", ("--add_background_onehot",), [0, 2])])
def test_geometry_end_to_end_with_a_pixelwise_stub(tmp_path, channels, extra, picked, tta):
    H, W, T, M, R = 72, 100, 32, 4, 4
    _checkpoint(tmp_path, channels, extra)
    flags = ["--whole_image", "--tile", str(T), "--tile_margin", str(M), "--tile_ramp", str(R)] + (["--tta", "d4"] if tta else [])
    model = _eval_model(tmp_path, channels, tuple(extra) + tuple(flags))
    assert model.opt.tile_stride == T - 2 * M - R and model.num_classes == 2
    stub = _Pixelwise([[1.5, -0.75][:len(picked)], [-2.0, 0.5][:len(picked)]], [0.25, -0.5])
    model.netG = stub
    img = np.random.RandomState(5).randint(0, 256, size=(H, W, 3), dtype=np.uint8)
    model.set_input(_feed(img))
    model.test()
    torch.cuda.synchronize()
    z = stub.host(util.prep_tile_ref(img, 0, 0, H, W, 0, 0)[picked]).astype(np.float64)
    e = np.exp(z - z.max(axis=0, keepdims=True))
    want = e / e.sum(axis=0, keepdims=True)
    _, n = util.blend_tiles_ref(lambda *a: np.zeros((2, T, T)), H, W, T, M, R, model.opt.tile_stride, tta=tta, return_count=True)
    k = (n + 2).astype(np.float64)
    bound = k * U32 / (1.0 - k * U32) + E_P
    got = model.fake_B.detach().cpu().numpy()[0].astype(np.float64)
    err = np.abs(got - want)
    print("stub %s tta %d: max |fake_B - softmax| %.3e, worst err / bound %.3f, passes per pixel up to %d" % (channels, tta, err.max(), (err / bound).max(), n.max()))
    assert got.shape == (2, H, W) and (err <= bound).all()
    assert tuple(model.real_A.shape) == (1, len(picked), H, W) and tuple(model.real_B.shape) == (1, 2, H, W) and tuple(model.label.shape) == (1, H, W)
    assert tuple(model.logit.shape) == (1, 2, H, W) and torch.equal(model.logit.argmax(dim=1), model.fake_B.argmax(dim=1))
    assert np.array_equal(model.real_A.cpu().numpy()[0], util.prep_tile_ref(img, 0, 0, H, W, 0, 0)[picked])
    ce = float(model.compute_cross_entropy_loss())
    lab = model.label.cpu().numpy()[0]
    want_ce = float(np.mean(-np.log(np.take_along_axis(want, lab[None], axis=0))))
    assert abs(ce - want_ce) <= 1e-5 * max(1.0, want_ce), (ce, want_ce)      # -log P[label], the mean over the whole image
    vis = model.get_current_visuals()
    assert tuple(vis["prediction"].shape[2:]) == (H, W) and tuple(vis["image"].shape[2:]) == (H, W)


def test_one_tile_is_the_plain_test_of_the_same_network(tmp_path):
    from supervised_gan_amd import ops
    _checkpoint(tmp_path)
    img = _walls(128, 128, 1)
    u8 = torch.from_numpy(img).to(_dev())
    plain = _eval_model(tmp_path)
    assert not plain._tiling
    plain.set_input({"A": ops.logical_view(ops.image_prep(u8, 0, 0, 128, False, 0), 3), "A_paths": ["image.png"]})
    plain.test()
    first = plain.fake_B.detach().clone()
    plain.test()
    again = plain.fake_B.detach().clone()
    d = float((first - again).abs().max())
    tiled = _eval_model(tmp_path, extra=("--whole_image", "--tile", "128", "--tile_margin", "0", "--tile_ramp", "1"))
    assert tiled._tiling and tiled.opt.tile_stride == 127
    tiled.set_input(_feed(img))
    tiled.test()
    got = tiled.fake_B.detach()
    diff = float((got - again).abs().max())
    print("two plain test() calls differ by %.3e; the one-tile prediction differs from the plain one by %.3e" % (d, diff))
    assert got.shape == again.shape == (1, 2, 128, 128)
    if d == 0.0:
        assert torch.equal(got, again)
    else:
        assert diff <= 2.0 * d
    # --tta d4 alone: the crop as one tile of weight 1, eight passes
    tta = _eval_model(tmp_path, extra=("--tta", "d4"))
    assert tta._tiling and (tta.opt.tile, tta.opt.tile_margin, tta.opt.tile_ramp, tta.opt.tile_stride) == (128, 0, 1, 128)
    tta.set_input(_feed(img))
    tta.test()
    p = tta.fake_B.detach()
    assert p.shape == (1, 2, 128, 128) and bool(torch.isfinite(p).all()) and float((p.sum(dim=1) - 1).abs().max()) < 1e-5


@pytest.mark.parametrize("clean", [False, True])
def test_many_tiles_through_the_accuracies(tmp_path, clean):
    from supervised_gan_amd import ops
    H, W = 160, 200
    _checkpoint(tmp_path)
    extra = ["--whole_image", "--tile", "128", "--tile_margin", "16", "--which_metric", "RandScore", "meanIU", "BoundF"]
    model = _eval_model(tmp_path, extra=tuple(extra + (["--clean_close", "1.5"] if clean else [])))
    model.set_input(_feed(_walls(H, W, 2)))
    model.test()
    assert len(model._tile_st["passes"]) == 2 * 3
    ce = float(model.compute_cross_entropy_loss())
    model.accum_accs()
    accs = model.get_current_accs()                      # synchronises and raises if a metric kernel flagged its result (metric_err)
    ops.check_metric_err(model.device)
    assert list(accs) == ["RandScore", "meanIU", "BoundF"] and all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in accs.values()), accs
    assert model.numAveragedPixels == H * W and model.numAveragedImages == 1 and np.isfinite(ce) and ce > 0
    p = model.fake_B.detach()
    assert p.shape == (1, 2, H, W) and float((p.sum(dim=1) - 1).abs().max()) < 1e-5
    vis = model.get_current_visuals()
    assert ("fake_B_clean" in vis) == clean and tuple(vis["prediction"].shape[2:]) == (H, W)
    model.test()                                         # the persistent buffers are reused, the canvas starts from zero again
    assert model.fake_B.data_ptr() == p.data_ptr() and float((model.fake_B.sum(dim=1) - 1).abs().max()) < 1e-5

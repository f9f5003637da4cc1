"""CPU tests of the options of the Tversky / focal loss terms: defaults, that a weight of 0 checks and changes nothing, what is
accepted, and every refusal of options.check_dice_options / check_focal_options."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse(tmp_path, extra, model="segmentation"):
    from supervised_gan_amd.options import TrainOptions
    base = ["--name", "t", "--gpu_ids", "-1", "--checkpoints_dir", str(tmp_path), "--model", model]
    return TrainOptions().parse(base + extra.split(), save=False, verbose=False)


def test_defaults_and_off(tmp_path):
    opt = parse(tmp_path, "")
    assert (opt.dice_weight, opt.dice_classes, opt.tversky, opt.dice_smooth, opt.tversky_power) == (0.0, [0], [0.5, 0.5], 1.0, 1.0)
    assert (opt.focal_weight, opt.focal_gamma) == (0.0, 2.0)
    # with the weights at 0 nothing is checked and nothing is filled in, whatever the other flags hold
    off = parse(tmp_path, "--dice_weight 0 --dice_classes -3 -3 --tversky 0 0 --tversky_power 9 --dice_smooth -1 --focal_weight 0 --focal_gamma 99")
    keys = ("dice_classes", "tversky", "tversky_power", "dice_smooth", "focal_gamma")
    rest = lambda o: {k: v for k, v in vars(o).items() if k not in keys}      # noqa: E731
    assert rest(off) == rest(opt)
    parse(tmp_path, "--dice_weight 0 --focal_weight 0", model="cgan")      # off: any model


def test_accepted(tmp_path):
    on = parse(tmp_path, "--dice_weight 0.5 --dice_classes 1 0 --tversky 0.3 0.7 --dice_smooth 0 --tversky_power 0.75 --which_model_netD None")
    assert (on.dice_weight, on.dice_classes, on.tversky, on.dice_smooth, on.tversky_power) == (0.5, [1, 0], [0.3, 0.7], 0.0, 0.75)
    on = parse(tmp_path, "--focal_weight 0.25 --focal_gamma 0 --use_sigmoid_ss --weights 1 2")
    assert (on.focal_weight, on.focal_gamma) == (0.25, 0.0)
    parse(tmp_path, "--dice_weight 1 --tversky 0 1 --tversky_power 4 --focal_weight 1 --focal_gamma 8 --cldice_weight 0.25 --lovasz_weight 0.5")


@pytest.mark.parametrize("bad, why", [
    ("--dice_weight -1", "weight >= 0"), ("--dice_weight nan", "weight >= 0"),
    ("--dice_weight 1 --dice_classes 0 1 2 3 4 5 6 7 8", "1..8 classes"), ("--dice_weight 1 --dice_classes -1", "class indices"),
    ("--dice_weight 1 --dice_classes 1 1", "distinct"),
    ("--dice_weight 1 --tversky 0 0", "A \\+ B == 0"), ("--dice_weight 1 --tversky -0.5 1", "both >= 0"),
    ("--dice_weight 1 --tversky nan 0.5", "both >= 0"), ("--dice_weight 1 --tversky 0.5 nan", "both >= 0"),
    ("--dice_weight 1 --tversky inf 0.5", "finite"),
    ("--dice_weight 1 --dice_smooth -0.5", "S >= 0"), ("--dice_weight 1 --dice_smooth nan", "S >= 0"),
    ("--dice_weight 1 --tversky_power 0", "0 < E <= 4"), ("--dice_weight 1 --tversky_power 4.5", "0 < E <= 4"),
    ("--dice_weight 1 --tversky_power nan", "0 < E <= 4"),
    ("--focal_weight -1", "weight >= 0"), ("--focal_weight nan", "weight >= 0"),
    ("--focal_weight 1 --focal_gamma -0.5", "0 <= G <= 8"), ("--focal_weight 1 --focal_gamma 8.5", "0 <= G <= 8"),
    ("--focal_weight 1 --focal_gamma nan", "0 <= G <= 8")])
def test_refusals(tmp_path, bad, why):
    with pytest.raises(AssertionError, match=why):
        parse(tmp_path, bad)


@pytest.mark.parametrize("flag", ["--dice_weight", "--focal_weight"])
def test_other_models_refuse(tmp_path, flag):
    with pytest.raises(AssertionError, match="--model segmentation"):
        parse(tmp_path, flag + " 1", model="cgan")


def test_bare_options_pass():
    from supervised_gan_amd.options import check_dice_options, check_focal_options

    class Bare:
        pass
    check_dice_options(Bare())
    check_focal_options(Bare())

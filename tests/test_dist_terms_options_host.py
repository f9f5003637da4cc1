"""CPU tests of the options of the distance-map loss terms (--boundary_loss_weight, --hausdorff_weight, --hausdorff_alpha,
--dist_class): defaults, that weights of 0 check and change nothing, what is accepted, every refusal of options.check_dist_options,
and that a trainer built with both weights at 0 holds nothing of the term."""
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
    assert (opt.boundary_loss_weight, opt.hausdorff_weight, opt.hausdorff_alpha, opt.dist_class) == (0.0, 0.0, 2.0, 0)
    # with the weights at 0 nothing is checked and nothing is filled in, whatever the other flags hold
    off = parse(tmp_path, "--boundary_loss_weight 0 --hausdorff_weight 0 --hausdorff_alpha 99 --dist_class -3")
    keys = ("hausdorff_alpha", "dist_class")
    rest = lambda o: {k: v for k, v in vars(o).items() if k not in keys}      # noqa: E731
    assert rest(off) == rest(opt)
    parse(tmp_path, "--boundary_loss_weight 0 --hausdorff_weight 0", model="cgan")      # off: any model


def test_accepted(tmp_path):
    on = parse(tmp_path, "--boundary_loss_weight 0.01 --hausdorff_weight 0.001 --hausdorff_alpha 1 --dist_class 1 --which_model_netD None")
    assert (on.boundary_loss_weight, on.hausdorff_weight, on.hausdorff_alpha, on.dist_class) == (0.01, 0.001, 1.0, 1)
    on = parse(tmp_path, "--hausdorff_weight 0.5 --hausdorff_alpha 4 --use_sigmoid_ss")
    assert (on.boundary_loss_weight, on.hausdorff_weight, on.hausdorff_alpha) == (0.0, 0.5, 4.0)
    parse(tmp_path, "--boundary_loss_weight 1 --hausdorff_alpha 99")      # the exponent belongs to the Hausdorff term: off, not looked at
    parse(tmp_path, "--boundary_loss_weight 1 --hausdorff_weight 1 --cldice_weight 0.25 --lovasz_weight 0.5 --dice_weight 1 --focal_weight 1")


@pytest.mark.parametrize("bad, why", [
    ("--boundary_loss_weight -1", "weight >= 0"), ("--boundary_loss_weight nan", "weight >= 0"),
    ("--hausdorff_weight -1", "weight >= 0"), ("--hausdorff_weight nan", "weight >= 0"),
    ("--boundary_loss_weight 1 --hausdorff_weight -1", "weight >= 0"),
    ("--hausdorff_weight 1 --hausdorff_alpha 0", "0 < A <= 4"), ("--hausdorff_weight 1 --hausdorff_alpha 4.5", "0 < A <= 4"),
    ("--hausdorff_weight 1 --hausdorff_alpha -2", "0 < A <= 4"), ("--hausdorff_weight 1 --hausdorff_alpha nan", "0 < A <= 4"),
    ("--boundary_loss_weight 1 --dist_class -1", "class index"), ("--hausdorff_weight 1 --dist_class -1", "class index")])
def test_refusals(tmp_path, bad, why):
    with pytest.raises(AssertionError, match=why):
        parse(tmp_path, bad)


@pytest.mark.parametrize("flag", ["--boundary_loss_weight", "--hausdorff_weight"])
@pytest.mark.parametrize("model", ["cgan", "fcgan"])
def test_other_models_refuse(tmp_path, flag, model):
    with pytest.raises(AssertionError, match="--model segmentation"):
        parse(tmp_path, flag + " 1", model=model)


def test_bare_options_pass():
    from supervised_gan_amd.options import check_dist_options

    class Bare:
        pass
    check_dist_options(Bare())


def test_weights_zero_create_nothing_of_the_term(tmp_path):
    """The trainer on the CPU (nothing is launched by building it): with both weights at 0 it holds no buffer and no loss attribute
    of the term and logs no error of it; a class index past the class count is refused when the trainer is built."""
    from supervised_gan_amd.models import create_model
    net = ("--which_direction AtoB --dataset_mode aligned --fineSize 64 --which_model_netG resnet_6blocks --ngf 8 --which_channel b_rg "
           "--no_dropout --which_model_netD None")
    m = create_model(parse(tmp_path, net + " --boundary_loss_weight 0 --hausdorff_weight 0 --dist_class 7"))
    assert m.distterms is None
    assert not [k for k in vars(m) if k.startswith("_dl_") or k in ("loss_G_Boundary", "loss_G_Hausdorff")]
    assert m._with_dist_terms("the loss") == "the loss"
    with pytest.raises(AssertionError, match="batch 1 on the device|there are 2 classes"):
        create_model(parse(tmp_path, net + " --boundary_loss_weight 1 --dist_class 7"))

"""shape_stats.py on a tiny fcgan checkpoint (nothing is trained): the two files, the image ordinals, and for --shape_source real the
table of util.region_table on the same synthetic images."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NET = ["--model", "fcgan", "--which_direction", "A", "--dataset_mode", "single", "--fineSize", "64", "--input_nc", "2",
       "--which_model_netG", "deconv", "--n_layers_G", "3", "--ngf", "8", "--noise_nc", "8", "--noiseSize", "4", "--norm", "instance",
       "--no_dropout", "--which_channel", "rg", "--gpu_ids", "0", "--dataroot", "synthetic", "--manualSeed", "3"]


def _load(npz, txt):
    assert os.path.exists(npz) and os.path.exists(txt)
    z = np.load(npz, allow_pickle=False)
    table, props = z["table"], z["props"]
    assert table.dtype == np.int64 and table.shape[1] == 16 and props.shape == (len(table), len(z["prop_names"]))
    assert int(z["images"]) == 3 and z["shape"].tolist() == [64, 64]
    assert sorted(set(table[:, 12].tolist())) == [0, 1, 2] and np.all(np.diff(table[:, 12]) >= 0)
    text = open(txt).read()
    assert "images: 3" in text and "regions per image: mean" in text
    assert all(("\n%s: " % name) in text for name in ("area", "eccentricity", "compactness"))
    return table, props, z


def test_fake_and_real(tmp_path, capsys):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    import shape_stats
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TestOptions, TrainOptions
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    from supervised_gan_amd.util import REGION_PROPS, region_props, region_table
    net = ["--name", "drv_shape", "--checkpoints_dir", str(tmp_path / "ckpt")] + NET
    opt = TrainOptions().parse(net + ["--which_model_netD", "n_layers", "--n_layers_D", "3", "--ndf", "8", "--scale_factor", "1",
                                      "--lambda_D", "1", "--no_lsgan"], save=False, verbose=False)
    create_model(opt).save("latest")                           # a generator as initialised: the driver needs a checkpoint, not a good one
    res = ["--results_dir", str(tmp_path / "res"), "--how_many", "3"]

    npz, txt = shape_stats.main(net + res + ["--shape_source", "fake"])
    assert npz == str(tmp_path / "res" / "drv_shape" / "test_latest" / "shape_stats.npz")
    table, props, z = _load(npz, txt)
    assert [str(n) for n in z["prop_names"]] == list(REGION_PROPS)
    assert table[:, 0].sum() <= 3 * 64 * 64

    npz, txt = shape_stats.main(net + res + ["--shape_source", "real", "--shape_channel", "1", "--shape_objects", "wall",
                                             "--phase", "val"])
    assert npz == str(tmp_path / "res" / "drv_shape" / "val_latest" / "shape_stats.npz")
    table, props, _ = _load(npz, txt)
    topt = TestOptions().parse(net + res, save=False, verbose=False)
    want = []
    for i, data in enumerate(SyntheticDataset(topt, 3, device=torch.device("cpu"))):
        plane = shape_stats.object_plane(data["A"][0, 1], "wall")                # channel 1 of 'rg' is g
        want.append(region_table(~(plane > 0.5).numpy(), i))
    want = np.concatenate(want)
    assert len(want) > 3 and np.array_equal(table, want)
    ref = region_props(want, (64, 64))
    assert np.array_equal(props, np.stack([ref[n].astype(np.float64) for n in REGION_PROPS], axis=1), equal_nan=True)
    capsys.readouterr()


def test_refusals(tmp_path):
    import shape_stats
    for extra in (["--model", "cgan", "--shape_source", "fake"], ["--model", "fcgan", "--which_channel", "rg", "--shape_channel", "2"]):
        with pytest.raises(SystemExit) as e:
            shape_stats.main(["--name", "x", "--dataroot", "synthetic", "--gpu_ids", "0", "--checkpoints_dir", str(tmp_path)] + extra)
        assert e.value.code == 2

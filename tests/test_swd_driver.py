"""swd.py on a tiny fcgan checkpoint (nothing is trained): the two files, the per-level scores against util.swd_ref on the very
images the driver scored, a set split against itself, and the same file from the same seed.

The yardstick takes the driver's images (main's `keep`), their pyramid from ops.lap_pyramid (held to util.lap_pyramid_ref in
test_hip_swd.py; the same launches give the same bits), and from there only host code: swd_descriptors_ref, swd_normalise_ref on
the float64 statistics, swd_ref.  The bound per direction is test_hip_swd.py's: gamma_K (max_i sum_k |nA_ik d_jk| + max_i sum_k
|nB_ik d_jk|) + (N + 2) 2^-53 ref_j; a level's score is the mean of its directions, so it is held to the mean of their bounds."""
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
SWD = ["--how_many", "4", "--swd_patches", "16", "--swd_dirs", "8", "--swd_seed", "5"]
U32 = 2.0 ** -24


def _yardstick(keep, seed, same_positions):
    """Per-level (distances [J], bound [J]) of the kept images."""
    from supervised_gan_amd import ops
    from supervised_gan_amd import util as U
    pyr = {s: [[l.cpu().numpy() for l in ops.lap_pyramid(x)] for x in keep[s]] for s in "AB"}
    out = []
    for l in range(len(pyr["A"][0])):
        C, h, w = pyr["A"][0][l].shape
        K, n = C * 49, []
        for si, s in enumerate("AB"):
            pos, dirs = U.swd_draw(seed, l, 4, 16, h, w, K, 8, set_index=0 if same_positions else si)
            desc, mean, std = U.swd_descriptors_ref([p[l] for p in pyr[s]], pos)
            n.append(U.swd_normalise_ref(desc, mean, std))
        ref = U.swd_ref(n[0], n[1], dirs)
        ad = np.abs(dirs.astype(np.float64))
        g = K * U32 / (1 - K * U32)
        bound = g * sum((np.abs(v.astype(np.float64)) @ ad.T).max(axis=0) for v in n) + (64 + 2) * 2.0 ** -53 * ref
        out.append((ref, bound))
    return out


def test_real_fake_and_real_real(tmp_path, capsys):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    import swd
    from PIL import Image
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    net = ["--name", "drv_swd", "--checkpoints_dir", str(tmp_path / "ckpt")] + NET
    opt = TrainOptions().parse(net + ["--which_model_netD", "n_layers", "--n_layers_D", "3", "--ndf", "8", "--scale_factor", "1",
                                      "--lambda_D", "1", "--no_lsgan"], save=False, verbose=False)
    create_model(opt).save("latest")                           # a generator as initialised: the driver needs a checkpoint, not a good one
    res = ["--results_dir", str(tmp_path / "res")]

    keep = {}
    npz, txt = swd.main(net + res + SWD, keep=keep)
    assert npz == str(tmp_path / "res" / "drv_swd" / "test_latest" / "swd.npz") and os.path.exists(npz) and os.path.exists(txt)
    assert len(keep["A"]) == len(keep["B"]) == 4 and tuple(keep["A"][0].shape) == tuple(keep["B"][3].shape) == (2, 64, 64)
    z = np.load(npz, allow_pickle=False)
    assert z["sizes"].tolist() == [[64, 64], [32, 32], [16, 16]] and z["distances"].shape == (3, 8) and z["distances"].dtype == np.float64
    assert dict(zip(z["option_names"].tolist(), z["option_values"].tolist()))["swd_patches"] == "16"
    for l, (ref, bound) in enumerate(_yardstick(keep, 5, False)):
        err = np.abs(z["distances"][l] - ref)
        print("level %d: score %.6e, max err %.3e, bound there %.3e" % (l, ref.mean(), err.max(), bound[err.argmax()]))
        assert np.all(err <= bound) and ref.mean() > 0
        assert abs(z["scores"][l] - ref.mean()) <= bound.mean() + 4 * 2.0 ** -53 * ref.mean()
    text = open(txt).read()
    lines = text.splitlines()
    assert [l.split(":")[0] for l in lines] == ["64x64", "32x32", "16x16", "average"]
    assert [float(l.split(":")[1]) for l in lines[:3]] == [float("%.6f" % (s * 1e3)) for s in z["scores"]]
    assert text in capsys.readouterr().out

    # the same seed: the same file; another seed: other patches and directions
    first = open(txt, "rb").read()
    npz2, txt2 = swd.main(net + res + SWD)
    z2 = np.load(npz2, allow_pickle=False)
    assert open(txt2, "rb").read() == first and np.array_equal(z2["distances"], z["distances"])
    swd.main(net + res + SWD[:-1] + ["6"])
    assert open(txt, "rb").read() != first

    # real against real: even files against odd files, the same positions in both halves
    keep = {}
    npz, txt = swd.main(net + res + SWD + ["--swd_pair", "real_real", "--swd_channels", "1", "--phase", "val"], keep=keep)
    assert npz == str(tmp_path / "res" / "drv_swd" / "val_latest" / "swd.npz")
    z = np.load(npz, allow_pickle=False)
    assert z["channels"].tolist() == [1] and tuple(keep["A"][0].shape) == (1, 64, 64)
    for l, (ref, bound) in enumerate(_yardstick(keep, 5, True)):
        assert np.all(np.abs(z["distances"][l] - ref) <= bound) and ref.mean() > 0

    # a set split against itself -- every file twice, so the even and the odd files are the same images -- scores exactly 0
    folder = tmp_path / "twice" / "test"
    os.makedirs(str(folder))
    rng = np.random.RandomState(0)
    for i in range(4):
        img = Image.fromarray(rng.randint(0, 256, size=(64, 64, 3), dtype=np.uint8), "RGB")
        for copy in "ab":
            img.save(str(folder / ("img_%02d%s.png" % (i, copy))))
    argv = [a for a in net if a != "synthetic"]
    argv.insert(argv.index("--dataroot") + 1, str(tmp_path / "twice"))
    npz, txt = swd.main(argv + res + SWD + ["--swd_pair", "real_real", "--loadSize", "64", "--name", "drv_swd_twice"])
    z = np.load(npz, allow_pickle=False)
    assert np.array_equal(z["distances"], np.zeros((3, 8)))
    assert open(txt).read() == "64x64: 0.000000\n32x32: 0.000000\n16x16: 0.000000\naverage: 0.000000\n"
    capsys.readouterr()


def test_refusals(tmp_path, capsys):
    import swd
    base = ["--name", "x", "--dataroot", "synthetic", "--gpu_ids", "0", "--checkpoints_dir", str(tmp_path), "--which_channel", "rg"]
    for extra, word in ((["--model", "segmentation"], "--model"), (["--model", "fcgan", "--how_many", "1025", "--swd_patches", "16"], "16384")):
        with pytest.raises(SystemExit) as e:
            swd.main(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err

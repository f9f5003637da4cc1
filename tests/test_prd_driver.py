"""swd.py --prd_k on a tiny fcgan checkpoint (nothing is trained): prd.npz against util.prd_scores_ref on the very images the driver
scored, a dataset whose odd files copy the even ones, and --prd_k 0 leaving the run as it was.

The yardstick takes the driver's images (main's `keep`), their pyramid from ops.lap_pyramid (held to util.lap_pyramid_ref in
test_hip_swd.py; the same launches give the same bits), and from there only host code: swd_descriptors_ref, swd_normalise_ref of BOTH
sets on set A's float64 statistics, knn_radii_ref with group = the patches of one image, prd_rows_ref, prd_scores_ref.  The device's
squared distances differ from the yardstick's by at most gamma_{K+2} d2 per pair (the direct form, tests/test_hip_prd.py); the four
integer counts must equal the yardstick's unless a pair sits within that bound of a ball's surface (then the test says so and fails:
the seed is a bad one), and the two medians are held to the largest bound of their rows."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NET = ["--model", "fcgan", "--which_direction", "A", "--dataset_mode", "single", "--fineSize", "64", "--input_nc", "2",
       "--which_model_netG", "deconv", "--n_layers_G", "3", "--ngf", "8", "--noise_nc", "8", "--noiseSize", "4", "--norm", "instance",
       "--no_dropout", "--which_channel", "rg", "--gpu_ids", "0", "--dataroot", "synthetic", "--manualSeed", "3"]
SWD = ["--how_many", "4", "--swd_patches", "16", "--swd_dirs", "8", "--swd_seed", "5"]
U32 = 2.0 ** -24
KEYS = ("precision", "recall", "density", "coverage", "nn_fake_real", "nn_real_real", "nn_ratio")


def test_arguments(tmp_path, capsys):
    """CPU: argument handling only."""
    import swd
    sargs, rest = swd._swd_args(["--prd_k", "3", "--name", "x"])
    assert sargs.prd_k == 3 and rest == ["--name", "x"] and swd._swd_args([])[0].prd_k == 0
    base = ["--name", "x", "--dataroot", "synthetic", "--gpu_ids", "-1", "--checkpoints_dir", str(tmp_path), "--which_channel", "rg", "--model", "fcgan"]
    with pytest.raises(SystemExit) as e:
        swd.main(base + SWD + ["--prd_k", "8", "--how_many", "1"])
    assert e.value.code == 2 and "N - swd_patches = 16 - 16 = 0" in capsys.readouterr().err


def _yardstick(keep, seed, same_positions, k):
    """Per level: (prd_scores_ref's dict, ambiguous pairs, bound of the medians)."""
    from supervised_gan_amd import ops
    from supervised_gan_amd import util as U
    pyr = {s: [[l.cpu().numpy() for l in ops.lap_pyramid(x)] for x in keep[s]] for s in "AB"}
    out = []
    for l in range(len(pyr["A"][0])):
        C, h, w = pyr["A"][0][l].shape
        K, desc = C * 49, []
        for si, s in enumerate("AB"):
            pos, _ = U.swd_draw(seed, l, 4, 16, h, w, K, 8, set_index=0 if same_positions else si)
            desc.append(U.swd_descriptors_ref([p[l] for p in pyr[s]], pos))
        mean, std = desc[0][1], desc[0][2]
        nA, nB = U.swd_normalise_ref(desc[0][0], mean, std), U.swd_normalise_ref(desc[1][0], mean, std)
        g = (K + 2) * U32 / (1 - (K + 2) * U32)
        dAA, dBB, dBA = U._prd_d2(nA, nA), U._prd_d2(nB, nB), U._prd_d2(nB, nA)
        knnA, knnB = U.knn_radii_ref(nA, k, 16, d2=dAA), U.knn_radii_ref(nB, k, 16, d2=dBB)
        rowsB, rowsA = U.prd_rows_ref(nB, nA, knnA[0], d2=dBA), U.prd_rows_ref(nA, nB, knnB[0], d2=dBA.T)
        amb = int((np.abs(dBA - knnA[0][None, :]) <= g * (dBA + dAA.max())).sum() + (np.abs(dBA.T - knnB[0][None, :]) <= g * (dBA.T + dBB.max())).sum()
                  + (np.abs(rowsA[1] - knnA[0]) <= g * (dBA.max() + dAA.max())).sum())
        out.append((U.prd_scores_ref(rowsB, rowsA, knnA, knnB, k), amb, g * max(dBA.max(), dAA.max())))
    return out


@pytest.mark.gpu
def test_real_fake_real_real_and_off(tmp_path, capsys):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    import swd
    from PIL import Image
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    net = ["--name", "drv_prd", "--checkpoints_dir", str(tmp_path / "ckpt")] + NET
    opt = TrainOptions().parse(net + ["--which_model_netD", "n_layers", "--n_layers_D", "3", "--ndf", "8", "--scale_factor", "1",
                                      "--lambda_D", "1", "--no_lsgan"], save=False, verbose=False)
    create_model(opt).save("latest")                           # a generator as initialised: the driver needs a checkpoint, not a good one
    res = ["--results_dir", str(tmp_path / "res")]
    out_dir = tmp_path / "res" / "drv_prd" / "test_latest"

    # off: no prd.* and the swd files of a run that never heard of the flag
    npz, txt = swd.main(net + res + SWD)
    plain = dict(np.load(npz, allow_pickle=False))
    plain_txt = open(txt, "rb").read()
    npz, txt = swd.main(net + res + SWD + ["--prd_k", "0"])
    off = dict(np.load(npz, allow_pickle=False))
    assert sorted(off) == sorted(plain) and all(np.array_equal(off[key], plain[key]) for key in plain) and open(txt, "rb").read() == plain_txt
    assert "prd_k" not in off["option_names"].tolist()
    assert not os.path.exists(str(out_dir / "prd.npz")) and not os.path.exists(str(out_dir / "prd.txt"))
    capsys.readouterr()

    keep = {}
    npz, txt = swd.main(net + res + SWD + ["--prd_k", "3"], keep=keep)
    z0 = np.load(npz, allow_pickle=False)
    assert np.array_equal(z0["distances"], plain["distances"])      # the distances do not move
    assert open(txt, "rb").read() == plain_txt
    z = np.load(str(out_dir / "prd.npz"), allow_pickle=False)
    assert z["sizes"].tolist() == [[64, 64], [32, 32], [16, 16]] and int(z["k"]) == 3 and int(z["N"]) == 64 and int(z["group"]) == 16
    assert z["counts"].shape == (3, 4) and z["counts"].dtype == np.int64
    assert dict(zip(z["option_names"].tolist(), z["option_values"].tolist()))["prd_k"] == "3"
    for l, (ref, amb, bound) in enumerate(_yardstick(keep, 5, False, 3)):
        print("level %d: counts %s (yardstick %s), ambiguous pairs %d, medians %.6e %.6e (yardstick %.6e %.6e, bound %.3e)"
              % (l, z["counts"][l].tolist(), ref["counts"].tolist(), amb, z["nn_fake_real"][l], z["nn_real_real"][l], ref["nn_fake_real"],
                 ref["nn_real_real"], bound))
        assert amb == 0, "a bad seed: a pair sits on a ball's surface"
        assert np.array_equal(z["counts"][l], ref["counts"])
        for key in KEYS[:4]:
            assert z[key][l] == ref[key], key
        assert abs(z["nn_fake_real"][l] - ref["nn_fake_real"]) <= bound and abs(z["nn_real_real"][l] - ref["nn_real_real"]) <= bound
        assert z["nn_ratio"][l] == z["nn_fake_real"][l] / z["nn_real_real"][l]
    text = open(str(out_dir / "prd.txt")).read()
    lines = text.splitlines()
    assert [l.split(":")[0] for l in lines] == ["64x64", "32x32", "16x16", "average"]
    assert lines[0] == "64x64: " + " ".join("%s %.6f" % (key, z[key][0]) for key in KEYS)
    assert text in capsys.readouterr().out

    # odd files copy the even ones: the two halves are the same images at the same positions
    folder = tmp_path / "twice" / "test"
    os.makedirs(str(folder))
    rng = np.random.RandomState(0)
    for i in range(4):
        img = Image.fromarray(rng.randint(0, 256, size=(64, 64, 3), dtype=np.uint8), "RGB")
        for copy in "ab":
            img.save(str(folder / ("img_%02d%s.png" % (i, copy))))
    argv = [a for a in net if a != "synthetic"]
    argv.insert(argv.index("--dataroot") + 1, str(tmp_path / "twice"))
    swd.main(argv + res + SWD + ["--swd_pair", "real_real", "--loadSize", "64", "--name", "drv_prd_twice", "--prd_k", "3"])
    z = np.load(str(tmp_path / "res" / "drv_prd_twice" / "test_latest" / "prd.npz"), allow_pickle=False)
    for key in ("precision", "recall", "coverage"):
        assert np.array_equal(z[key], np.ones(3)), key
    assert np.array_equal(z["nn_fake_real"], np.zeros(3)) and np.all(z["density"] >= 1.0)
    capsys.readouterr()

"""GPU tests of the boundary scores on the device (sgan_edt_sq and sgan_boundary_accumulate in sgan_edt.hip): the distance transform
against the host yardstick util.edt_sq with integer equality on every named plane of every shape, repeatability, the counts against
util.boundary_counts, pooling, the refusals, graph capture, the trainers' BoundF / HausD / ASSD and the train_ss.py / test_ss.py
drivers.

Tolerance: the integers are equal.  The three fp64 sums are sums of n correctly rounded square roots (clang's fp64 sqrt on gfx950 is
the correctly rounded one unless fast-math asks otherwise, and the library is built without it), added in another order than the
yardstick's correctly rounded sum: max(2, n) 2^-52 relative (boundary_ref.sums_close)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import boundary_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def _garbage_ws(ws):
    ws = ws.clone()
    ws.fill_(-1)
    return ws


def _edt_checked(dev, H, W, names):
    """ops.edt_sq on the named planes of one shape, twice each into a garbage workspace, against the yardstick."""
    from supervised_gan_amd import ops
    ws = _garbage_ws(ops.edt_workspace(H, W, dev))
    for name in names:
        plane = torch.from_numpy(np.array(R.planes(H, W)[name])).to(dev)
        ws.fill_(-1)                                           # garbage on entry: the call initialises what it uses
        first = ops.edt_sq(plane, workspace=ws)
        second = ops.edt_sq(plane, workspace=ws)               # and what the first call left behind is garbage too
        assert first.dtype == torch.int32 and tuple(first.shape) == (H, W)
        got, again = first.cpu().numpy(), second.cpu().numpy()
        want = R.want_edt(H, W, name)
        assert np.array_equal(got, want), (H, W, name, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())
        assert np.array_equal(got, again), (H, W, name)
    ops.check_metric_err(dev)


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_edt_equals_the_host_yardstick(H, W):
    _edt_checked(_dev(), H, W, R.NAMES)


@pytest.mark.parametrize("H,W", R.CHUNK_SHAPES)
def test_edt_rows_longer_than_a_chunk(H, W):
    _edt_checked(_dev(), H, W, R.CHUNK_NAMES)


def test_edt_512_sparse_and_noise():
    _edt_checked(_dev(), *R.BIG, R.BIG_NAMES)


@pytest.mark.parametrize("H,W", ((37, 53), (65, 130)))
def test_edt_reads_channel_0_of_an_nhwc_map(H, W):
    """The same content as channel 0 of a 2-channel NHWC map (pixel stride 2), the other channel all wall."""
    from supervised_gan_amd import ops
    dev = _dev()
    for name in R.NAMES:
        nhwc = torch.ones((H, W, 2), dtype=torch.float32, device=dev)
        nhwc[:, :, 0] = torch.from_numpy(np.array(R.planes(H, W)[name])).to(dev)
        view = nhwc[:, :, 0]
        assert view.stride(1) == 2
        got = ops.edt_sq(view).cpu().numpy()
        assert np.array_equal(got, R.want_edt(H, W, name)), (H, W, name)
    out = torch.full((H, W), 7, dtype=torch.int32, device=dev)
    assert ops.edt_sq(view, out=out) is out and np.array_equal(out.cpu().numpy(), R.want_edt(H, W, R.NAMES[-1]))


def _dsq_pair(dev, H, W, s_name, t_name):
    from supervised_gan_amd import ops
    p = R.planes(H, W)
    return (ops.edt_sq(torch.from_numpy(np.array(p[t_name])).to(dev)), ops.edt_sq(torch.from_numpy(np.array(p[s_name])).to(dev)))


def _fresh(dev):
    return torch.zeros(80, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.float64, device=dev)


@pytest.mark.parametrize("H,W", R.SHAPES + (R.BIG,))
def test_counts_equal_the_host_yardstick(H, W):
    from supervised_gan_amd import ops
    dev = _dev()
    ws = _garbage_ws(ops.boundary_workspace(H, W, dev))
    for s_name, t_name in (R.PAIRS if (H, W) != R.BIG else (("dense", "sparse"), ("sparse", "dense"), ("no_wall", "dense"))):
        t_dsq, s_dsq = _dsq_pair(dev, H, W, s_name, t_name)
        acc_i, acc_f = _fresh(dev)
        counts, sums = torch.full((80,), 5, dtype=torch.int64, device=dev), torch.full((4,), 5.0, dtype=torch.float64, device=dev)
        ws.fill_(-1)
        ops.boundary_accumulate(t_dsq, s_dsq, acc_i, acc_f, counts_out=counts, sums_out=sums, workspace=ws)
        want_c, want_s = R.want_counts(H, W, s_name, t_name)
        got_c, got_s = acc_i.cpu().tolist(), acc_f.cpu().tolist()
        print("%dx%d %s/%s: N_s %d N_t %d max %d %d sums %r want %r" % (H, W, s_name, t_name, got_c[64], got_c[65], got_c[70], got_c[71],
                                                                     got_s, want_s))
        assert got_c == want_c, (H, W, s_name, t_name, [(k, a, b) for k, (a, b) in enumerate(zip(got_c, want_c)) if a != b])
        assert counts.cpu().tolist() == want_c
        assert R.sums_close(got_s, want_s, want_c) and R.sums_close(sums.cpu().tolist(), want_s, want_c), (got_s, want_s)
        again_i, again_f = _fresh(dev)
        ops.boundary_accumulate(t_dsq, s_dsq, again_i, again_f, workspace=ws)
        assert again_i.cpu().tolist() == got_c and R.sums_close(again_f.cpu().tolist(), want_s, want_c)
    ops.check_metric_err(dev)


def test_several_pairs_pool():
    """Four pairs (one of them without a predicted wall) into one pair of accumulators: the sums of their counts_out, the maxima following the max."""
    from supervised_gan_amd import ops
    dev = _dev()
    H, W = 65, 130
    acc_i, acc_f = _fresh(dev)
    total_c, total_s = np.zeros(80, dtype=np.int64), np.zeros(4)
    maxima = []
    for s_name, t_name in (("centre", "equidistant"), ("corner_tl", "corner_br"), ("no_wall", "sparse"), ("dense", "sparse")):
        t_dsq, s_dsq = _dsq_pair(dev, H, W, s_name, t_name)
        counts, sums = _fresh(dev)
        ops.boundary_accumulate(t_dsq, s_dsq, acc_i, acc_f, counts_out=counts, sums_out=sums)
        c = counts.cpu().numpy()
        assert c.tolist() == R.want_counts(H, W, s_name, t_name)[0]
        total_c[:70] += c[:70]
        total_c[70:72] = np.maximum(total_c[70:72], c[70:72])
        total_s += np.array(R.want_counts(H, W, s_name, t_name)[1])
        maxima.append(c[70:72].tolist())
    got = acc_i.cpu().numpy()
    assert got.tolist() == total_c.tolist() and got[66] == 4 and got[67] == 3
    assert maxima[1] == [(H - 1) ** 2 + (W - 1) ** 2] * 2 and got[70:72].tolist() == maxima[1] and maxima[3][0] < maxima[1][0]
    assert R.sums_close(acc_f.cpu().tolist(), total_s.tolist(), total_c)
    ops.check_metric_err(dev)


def test_malformed_calls_are_refused_before_any_launch():
    from supervised_gan_amd import _lib, ops
    dev = _dev()
    l = _lib.lib()
    H, W = 37, 53
    need = l.sgan_edt_workspace(H, W)
    assert need > 0
    ws = torch.full((need // 8 + 1,), 7, dtype=torch.int64, device=dev)
    plane = torch.zeros((H, W), dtype=torch.float32, device=dev)
    dsq = torch.full((H, W), 7, dtype=torch.int32, device=dev)
    err = ops.metric_err(dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    for args, message in (((None, 1, H, W, P(dsq), P(ws), need, P(err), None), b"null pointer"),
                          ((P(plane), 1, H, W, None, P(ws), need, P(err), None), b"null pointer"),
                          ((P(plane), 1, H, W, P(dsq), None, need, P(err), None), b"null pointer"),
                          ((P(plane), 1, H, W, P(dsq), P(ws), need, None, None), b"null pointer"),
                          ((P(plane), 1, 0, W, P(dsq), P(ws), need, P(err), None), b"bad shape"),
                          ((P(plane), 1, H, -1, P(dsq), P(ws), need, P(err), None), b"bad shape"),
                          ((P(plane), 1, 1, 32769, P(dsq), P(ws), 1 << 40, P(err), None), b"bad shape"),
                          ((P(plane), 1, 32769, 1, P(dsq), P(ws), 1 << 40, P(err), None), b"bad shape"),
                          ((P(plane), 0, H, W, P(dsq), P(ws), need, P(err), None), b"pixel stride"),
                          ((P(plane), 1, H, W, P(dsq), P(ws), need - 16, P(err), None), b"nothing was launched")):
        assert l.sgan_edt_sq(*args) == 1 and message in l.sgan_last_error(), (message, l.sgan_last_error())
    bneed = l.sgan_boundary_workspace(H, W)
    assert bneed > 0
    bws = torch.full((bneed // 8 + 1,), 7, dtype=torch.int64, device=dev)
    acc_i, acc_f = _fresh(dev)
    for args, message in (((None, P(dsq), H, W, P(bws), bneed, P(acc_i), P(acc_f), None, None, P(err), None), b"null pointer"),
                          ((P(dsq), None, H, W, P(bws), bneed, P(acc_i), P(acc_f), None, None, P(err), None), b"null pointer"),
                          ((P(dsq), P(dsq), H, W, None, bneed, P(acc_i), P(acc_f), None, None, P(err), None), b"null pointer"),
                          ((P(dsq), P(dsq), H, W, P(bws), bneed, None, P(acc_f), None, None, P(err), None), b"null pointer"),
                          ((P(dsq), P(dsq), H, W, P(bws), bneed, P(acc_i), None, None, None, P(err), None), b"null pointer"),
                          ((P(dsq), P(dsq), H, W, P(bws), bneed, P(acc_i), P(acc_f), None, None, None, None), b"null pointer"),
                          ((P(dsq), P(dsq), H, 0, P(bws), bneed, P(acc_i), P(acc_f), None, None, P(err), None), b"bad shape"),
                          ((P(dsq), P(dsq), H, W, P(bws), bneed - 8, P(acc_i), P(acc_f), None, None, P(err), None), b"nothing was launched")):
        assert l.sgan_boundary_accumulate(*args) == 1 and message in l.sgan_last_error(), (message, l.sgan_last_error())
    torch.cuda.synchronize()
    assert bool((ws == 7).all()) and bool((bws == 7).all()) and bool((dsq == 7).all())      # untouched
    assert acc_i.cpu().tolist() == [0] * 80 and acc_f.cpu().tolist() == [0.0] * 4
    assert l.sgan_edt_workspace(1, 32769) < 0 and l.sgan_edt_workspace(0, 5) < 0 and l.sgan_boundary_workspace(5, 0) < 0
    with pytest.raises(_lib.SganError, match="workspace"):
        ops.edt_sq(plane, workspace=ws[:4])
    with pytest.raises(_lib.SganError, match="workspace"):
        ops.boundary_accumulate(dsq, dsq, acc_i, acc_f, workspace=bws[:4])


def test_capture_replays_on_another_pair():
    """edt_sq twice and boundary_accumulate captured on one pair and replayed on another whose prediction has no wall: a single
    chain of launches that depends on the shape alone."""
    from supervised_gan_amd import ops
    dev = _dev()
    H, W = 65, 130
    p = R.planes(H, W)
    first, second = R.want_counts(H, W, "dense", "sparse"), R.want_counts(H, W, "no_wall", "last_row")
    t_plane, s_plane = torch.from_numpy(np.array(p["sparse"])).to(dev), torch.from_numpy(np.array(p["dense"])).to(dev)
    dsq = torch.empty((2, H, W), dtype=torch.int32, device=dev)
    acc_i, acc_f = _fresh(dev)
    counts, sums = _fresh(dev)

    def run():
        ops.edt_sq(t_plane, out=dsq[0])
        ops.edt_sq(s_plane, out=dsq[1])
        ops.boundary_accumulate(dsq[0], dsq[1], acc_i, acc_f, counts_out=counts, sums_out=sums)

    run()                                                      # the workspaces and dev_err exist before the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    acc_i.zero_()
    acc_f.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == first[0] and R.sums_close(sums.cpu().tolist(), first[1], first[0])
    t_plane.copy_(torch.from_numpy(np.array(p["last_row"])))
    s_plane.copy_(torch.from_numpy(np.array(p["no_wall"])))
    g.replay()
    torch.cuda.synchronize()
    ops.check_metric_err(dev)
    assert np.array_equal(dsq[0].cpu().numpy(), R.want_edt(H, W, "last_row")) and bool((dsq[1] == -1).all())
    assert counts.cpu().tolist() == second[0] and sums.cpu().tolist() == second[1] == [0.0] * 4
    pooled = [a + b for a, b in zip(first[0], second[0])]
    pooled[70:72] = [max(a, b) for a, b in zip(first[0][70:72], second[0][70:72])]
    assert acc_i.cpu().tolist() == pooled and acc_i[67].item() == 1


def _net_argv(ckpt, metrics, name="boundary"):
    return ["--name", name, "--model", "segmentation", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "64",
            "--which_model_netG", "resnet_6blocks", "--ngf", "8", "--norm", "instance", "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout",
            "--checkpoints_dir", str(ckpt), "--dataroot", "synthetic", "--manualSeed", "4", "--which_metric", *metrics]


_TRAIN = ["--which_model_netD", "n_layers", "--n_layers_D", "2", "--ndf", "8", "--scale_factor", "1", "--lambda_D", "1.0", "--weights", "1", "2",
          "--no_lsgan", "--print_freq", "1", "--valSize", "64"]
ASKED = ["RandScore", "BoundF", "HausD", "ASSD"]


def _pooled(pairs, tolerance, thin=False):
    """util.boundary_scores of the yardstick's pooled counts on (fake_B, real_B) tensors, and the pooled numbers themselves."""
    from supervised_gan_amd import util
    counts, sums = np.zeros(80, dtype=np.int64), np.zeros(4, dtype=np.float64)
    for fb, rb in pairs:
        s = fb[0, 0].cpu().numpy() > 0.5
        c, f = util.boundary_counts(util.thin(s)[0] if thin else s, rb[0, 0].cpu().numpy())
        counts[:70] += c[:70]
        counts[70:72] = np.maximum(counts[70:72], c[70:72])
        sums += f
    return util.boundary_scores(counts, sums, tolerance), counts, sums


def _scores_match(accs, want, counts):
    """BoundF comes from equal integers through one function; HausD and ASSD carry the sums' bound over the pooled terms."""
    bound = max(2, int(counts[68]) + int(counts[69])) * 2.0 ** -52
    return accs["BoundF"] == want["BoundF"] and all(abs(accs[k] - want[k]) <= bound * abs(want[k]) for k in ("HausD", "ASSD"))


def test_trainer_scores_and_key_order(tmp_path, monkeypatch):
    from supervised_gan_amd import ops
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    _dev()
    opt = TrainOptions().parse(_net_argv(tmp_path, ASKED) + _TRAIN, save=False, verbose=False)
    model = create_model(opt)
    thinnings = []
    real_thin = ops.thin
    monkeypatch.setattr(ops, "thin", lambda *a, **k: (thinnings.append(1), real_thin(*a, **k))[1])
    seen = []
    for data in SyntheticDataset(opt, 3):
        model.set_input(data)
        model.optimize_parameters()
        model.accum_accs()
        seen.append((model.fake_B.detach().clone(), model.real_B.detach().clone()))
    accs = model.get_current_accs()
    assert list(accs) == ASKED and model.numAveragedImages == 3 and not thinnings
    want, counts, sums = _pooled(seen, 2)
    pooled = model.get_boundary_counts()
    print("trainer: device %r, host %r" % (dict(accs), dict(want)))
    assert list(pooled) == list(ops.BOUNDARY_COUNTS) + list(ops.BOUNDARY_SUMS)
    assert [pooled[k] for k in ops.BOUNDARY_COUNTS] == counts.tolist() and counts[66] == 3 and counts[65] > 0
    assert _scores_match(accs, want, counts)
    rand = accs["RandScore"]

    def again(metrics, **options):
        model.opt.which_metric = metrics
        for k, v in options.items():
            setattr(model.opt, k, v)
        model.reset_accs()
        assert model.get_boundary_counts()["images"] == 0
        thinnings.clear()
        for fb, rb in seen:
            model.fake_B, model.real_B = fb, rb
            model.accum_accs()
        return model.get_current_accs()

    # another tolerance; the keys come in BOUNDARY_METRICS order whatever order they were asked in
    at0 = again(["ASSD", "BoundF"], boundary_tolerance=0)
    assert list(at0) == ["BoundF", "ASSD"] and at0["BoundF"] == _pooled(seen, 0)[0]["BoundF"] <= accs["BoundF"]
    # the thinned prediction: util.thin's, thinned once per image
    thin = again(ASKED, boundary_tolerance=2, boundary_thin=True)
    want_thin, counts_thin, _ = _pooled(seen, 2, thin=True)
    assert len(thinnings) == 3 and thin["RandScore"] == rand
    assert [model.get_boundary_counts()[k] for k in ops.BOUNDARY_COUNTS] == counts_thin.tolist()
    assert _scores_match(thin, want_thin, counts_thin) and counts_thin[64] <= counts[64]
    # with RandScoreThin in the same accum_accs the thinned plane is reused: still one thinning per image, the same numbers
    both = again(ASKED + ["RandScoreThin"], boundary_thin=True)
    assert len(thinnings) == 3 and list(both) == ["RandScore", "RandScoreThin", "BoundF", "HausD", "ASSD"]
    assert [model.get_boundary_counts()[k] for k in ops.BOUNDARY_COUNTS] == counts_thin.tolist()
    assert all(both[k] == thin[k] for k in ("BoundF", "RandScore")) and _scores_match(both, want_thin, counts_thin)


def test_segmentation_cycle_borrows_the_boundary_scores(tmp_path):
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    from supervised_gan_amd.synthetic_data import SyntheticDataset
    _dev()
    argv = ["--name", "bndc", "--model", "segmentation_cycle", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "64",
            "--which_model_netG1", "resnet_6blocks", "--ngf1", "8", "--which_model_netG2", "resnet_6blocks", "--ngf2", "8", "--norm", "instance",
            "--which_channel", "b_rg", "--gpu_ids", "0", "--no_dropout1", "--no_dropout2", "--checkpoints_dir", str(tmp_path),
            "--dataroot", "synthetic", "--manualSeed", "4", "--which_metric", *ASKED, "--boundary_tolerance", "3",
            "--which_model_netD2", "n_layers", "--n_layers_D2", "2", "--ndf2", "8", "--scale_factor2", "1", "--lambda_D2", "1.0", "--no_lsgan2",
            "--print_freq", "1", "--valSize", "64"]
    opt = TrainOptions().parse(argv, save=False, verbose=False)
    model = create_model(opt)
    for data in SyntheticDataset(opt, 1):
        model.set_input(data)
        model.optimize_parameters()
        model.accum_accs()
    accs = model.get_current_accs()
    assert list(accs) == ASKED and model.numAveragedImages == 1
    want, counts, _ = _pooled([(model.fake_B.detach(), model.real_B.detach())], 3)
    print("cycle: device %r, host %r" % (dict(accs), dict(want)))
    assert [model.get_boundary_counts()[k] for k in ("N_s", "N_t", "max_dsq_s", "max_dsq_t")] == [int(counts[k]) for k in (64, 65, 70, 71)]
    assert _scores_match(accs, want, counts)


@pytest.mark.parametrize("graph", (False, True))
def test_drivers_carry_the_boundary_scores(tmp_path, graph):
    """train_ss.py in a fresh process (eager, and with --graph) keeps its `best` checkpoint by BoundF and logs the three scores;
    test_ss.py on that checkpoint prints them and the per-tolerance line."""
    _dev()
    argv = _net_argv(tmp_path / "ckpt", ASKED) + _TRAIN + ["--best_metric", "BoundF", "--max_steps", "3" if graph else "2", "--val_epoch_size", "1"]
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "train_ss.py")] + argv + (["--graph"] if graph else []),
                         cwd=ROOT, capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    log = (tmp_path / "ckpt" / "boundary" / "acc_log.txt").read_text().splitlines()
    assert sum(l.startswith("(train,") for l in log) >= 2 and sum(l.startswith("(val,") for l in log) == 1, log
    assert all("RandScore:" in l and "BoundF:" in l and "HausD:" in l and "ASSD:" in l for l in log), log
    values = {key: [float(l.split(key + ":")[1].split()[0]) for l in log] for key in ("BoundF", "HausD", "ASSD")}
    assert all(0.0 <= v <= 1.0 for v in values["BoundF"]) and all(0.0 <= v <= 64 * 2 ** 0.5 for v in values["HausD"] + values["ASSD"]), values
    assert "saving the best model (epoch 1, BoundF" in run.stdout
    assert (tmp_path / "ckpt" / "boundary" / "best_net_G.pth").exists()
    if graph:
        return
    run = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "test_ss.py")]
                         + _net_argv(tmp_path / "ckpt", ASKED) + ["--results_dir", str(tmp_path / "res"), "--how_many", "2"],
                         cwd=ROOT, capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    line = [l for l in run.stdout.splitlines() if l.startswith("boundary: P/R/F at tolerance 0 .. 5:")]
    assert len(line) == 1 and "worst distance" in line[0], run.stdout[-2000:]
    prf = [[float(v) for v in w.split("/")] for w in line[0].split(":")[2].split(",")[0].split()]
    assert len(prf) == 6 and all(len(v) == 3 for v in prf) and all(a[0] <= b[0] and a[1] <= b[1] for a, b in zip(prf, prf[1:])), line
    assert "BoundF: " in run.stdout and "HausD: " in run.stdout and "ASSD: " in run.stdout

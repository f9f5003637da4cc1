"""The finalised normalisation statistics: a loss launch turns a tensor's fp64 (sum, sum of squares) into float
(mean, rstd) pairs once, and the backward kernels of the pass load those instead of deriving them per workgroup.

  * the table against the in-kernel path (bit for bit) and against float64 (<= 1 float ulp, derived in tests/norm_table_ref.py);
  * every reader family with the table and without, from the same inputs, on results that no cross-workgroup float atomic touches:
    bit for bit;
  * one fcgan step at the fcgan_step_small shape with SGAN_NO_NORM_TABLE on and off: the rule for two runs of one build
    (tests/test_hip_segm_nod.py: 1e-4 of a tensor's maximum), and the walk's bookkeeping: every backward reader got a table;
  * stale tables: at every backward walk of two steps with different inputs -- eager, launch by launch through the graphed step's
    prefetch path (a kept forward refilled in place), InstanceNorm and BatchNorm -- each table equals what its statistics give NOW."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import norm_table_ref as R      # noqa: E402


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import _lib, ops
    _lib.lib()
    return ops


class _Owner:
    pass


def finalise(ops, jobs):
    """The tables of `jobs` = [(stats, C, count, eps, sq_stride, rep_stride)] from the loss launch that carries them."""
    own = _Owner()
    ops.norm_tables_register(own, jobs)
    logits = torch.zeros(3, 3, 4, device="cuda")
    each, total = torch.empty(1, device="cuda"), torch.empty((), device="cuda")
    ops.gan_loss_multi_fwd([logits], [1.0], [1.0], 0, each, total)
    torch.cuda.synchronize()
    assert abs(float(total) - float(np.log(2.0))) < 1e-6      # the loss rows of the launch are untouched by the extra rows
    assert own.norm_tables is not None
    return [own.norm_tables[j[0].data_ptr()] for j in jobs]


def probe(ops, desc, Cs):
    """(mean, rstd) of every channel as a kernel reading `desc` derives them."""
    from supervised_gan_amd import _lib
    out = torch.full((2 * Cs,), float("nan"), device="cuda")
    _lib.check(_lib.lib().sgan_norm_mean_rstd_probe(C.byref(desc), Cs, out.data_ptr(), torch.cuda.current_stream().cuda_stream), "probe")
    torch.cuda.synchronize()
    return out


def _samples(kind, count, Cs, rng):
    if kind == "cancel":      # large mean, tiny variance: q / n - m^2 cancels nearly everything
        return 1000.0 + 1e-3 * rng.standard_normal((count, Cs))
    return rng.standard_normal((count, Cs)) * rng.uniform(0.1, 30.0, Cs) + rng.uniform(-5, 5, Cs)


TABLE_CASES = [(Cs, rep, sq, count, kind) for Cs in (4, 32, 200, 256) for rep, sq in ((0, 0), (1, 0), (1, 1)) for count, kind in ((4096, "plain"),)]
TABLE_CASES += [(32, 0, 0, 1, "plain"), (200, 1, 1, 1, "plain"), (32, 0, 0, 4096, "cancel"), (256, 1, 1, 4096, "cancel"), (200, 0, 1, 289, "plain")]


@pytest.mark.parametrize("Cs,rep,sq,count,kind", TABLE_CASES)
def test_table_equals_in_kernel_path_and_float64(ops, Cs, rep, sq, count, kind):
    rng = np.random.default_rng(Cs * 7 + count + rep + 2 * sq)
    x = _samples(kind, count, Cs, rng)
    sq_stride = Cs + 24 if sq else 0                      # the sums of squares further off: a slice of a wider concat buffer's statistics
    rep_stride = (sq_stride or Cs) + Cs + 16 if rep else 0
    split = None
    if rep:      # unequal copies, three of them empty (all zero)
        owner = rng.choice([0, 1, 3, 4, 6], size=count, p=[0.5, 0.2, 0.15, 0.1, 0.05])
        split = [np.nonzero(owner == r)[0] for r in range(R.REPLICAS)]
    buf = R.make_stats(x, sq_stride, rep_stride, split, pad=0.0 if rep else 1e30)
    if rep:      # the empty copies and the gaps of a replicated arena are zero, what lies between a slice's halves is not
        for r in range(R.REPLICAS):
            buf[r * rep_stride + Cs: r * rep_stride + (sq_stride or Cs)] = 1e30
    eps = 1e-5
    ref = R.mean_rstd_f64(buf, Cs, count, eps, sq_stride, rep_stride)
    stats = torch.from_numpy(buf).cuda()
    table, = finalise(ops, [(stats, Cs, count, eps, sq_stride, rep_stride)])
    old = probe(ops, ops.norm_desc(stats, None, None, count, eps, 0, 0.0, sq_stride, rep_stride), Cs)
    assert torch.equal(table.view(torch.int32), old.view(torch.int32))                                  # bit for bit the in-kernel path
    new = probe(ops, ops.norm_desc(stats, None, None, count, eps, 0, 0.0, sq_stride, rep_stride, table), Cs)
    assert torch.equal(new.view(torch.int32), table.view(torch.int32))                                  # and a reader loads just that
    u = R.ulps(table.cpu().numpy().reshape(Cs, 2), ref)
    print(f"C {Cs} rep {rep_stride} sq {sq_stride} count {count} {kind}: max ulp mean {u[:, 0].max():.3f} rstd {u[:, 1].max():.3f}")
    assert u.max() <= 1.0
    if count == 1:
        assert np.all(table.cpu().numpy().reshape(Cs, 2)[:, 1] == np.float32(1.0 / np.sqrt(np.float64(np.float32(eps)))))


# ---- readers --------------------------------------------------------------------------------------------------------------------
def _layer(ops, kind, k, stride, pad, hin, cin, cout, cin_l=None, cout_l=None, seed=0):
    """One layer's backward inputs: x (forward input, normalised on load), its statistics, dout, weights with every derived copy."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    hout = (hin + 2 * pad - k) // stride + 1 if kind == ops.CONV else (hin - 1) * stride - 2 * pad + k
    desc = ops.conv_desc(kind, k, stride, pad, hin, hin, cin, hout, hout, cout, cin_l or cin, cout_l or cout)
    x = torch.randn(hin, hin, cin, device="cuda", generator=g) * 3 + 1
    dout = torch.randn(hout, hout, cout, device="cuda", generator=g)
    n = k * k * cout * cin
    flat = torch.randn(n, device="cuda", generator=g) * 0.05
    der = [torch.zeros_like(flat) for _ in range(4)]
    ops.pack_weights(flat, der[0], der[1], der[2], [(0, k * k, cout, cin)], der[3])
    wt = ops.with_packed(der[0], der[2], der[3])
    x64 = x.double().reshape(-1, cin)
    stats = torch.cat([x64.sum(0), (x64 * x64).sum(0)])
    return dict(desc=desc, x=x, dout=dout, wt=wt, stats=stats, count=hin * hin, cin=cin, cout=cout, k=k, hin=hin)


def _both(ops, Ld, run):
    """run(norm descriptor) with the table and without: the two result tuples."""
    table, = finalise(ops, [(Ld["stats"], Ld["cin"], Ld["count"], 1e-5, 0, 0)])
    res = []
    for t in (None, table):
        nd = ops.norm_desc(Ld["stats"], None, None, Ld["count"], 1e-5, ops.ACT_LRELU, 0.2, 0, 0, t)
        res.append(run(nd))
        torch.cuda.synchronize()
    return res


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# 16 x 16 / 8 x 8: the shapes of the issue (maps under 256 pixels run the exact-fp32 kernels in either mode); 32 x 32: the same layers
# where the split 16-bit-plane kernels and the fused launch take them
@pytest.mark.parametrize("math,hin", [("f32", 16), ("bf16x3", 16), ("bf16x3", 32)])
def test_backward_data_reader(ops, math, hin):
    Ld = _layer(ops, ops.CONV, 4, 2, 1, hin, 32, 64, seed=1)

    def run(nd):
        din = torch.empty_like(Ld["x"])
        sums = torch.zeros(2 * Ld["cin"], dtype=torch.float64, device="cuda")
        with ops.math_scope(math):
            ops.conv_dgrad_grouped([(Ld["desc"], Ld["dout"], Ld["wt"], din, Ld["x"], nd, sums, 0, False, True, 0)])
        return din, sums, ops.L.lib().sgan_last_kernel().decode()
    (d0, s0, k0), (d1, s1, k1) = _both(ops, Ld, run)
    print("backward-data ran", k0)
    assert k0 == k1 and (hin < 32 or "igemm3" in k0)
    assert _same_bits(d0, d1)
    # The norm-backward sums s1_c = sum_p dY, s2_c = sum_p dY * xhat: the terms are the same floats in both runs (same dY, same mean
    # and rstd), the workgroups add their parts to the fp64 sums in the order they arrive.  Two orders of an fp64 sum of n terms t
    # differ by at most 2 (n - 1) 2^-53 sum|t|; 1 % on top for parts a workgroup may have pre-summed in a fixed order of its own.
    tab = finalise(ops, [(Ld["stats"], Ld["cin"], Ld["count"], 1e-5, 0, 0)])[0].double().reshape(-1, 2)
    dy = d0.double().reshape(-1, Ld["cin"])
    xhat = (Ld["x"].double().reshape(-1, Ld["cin"]) - tab[:, 0]) * tab[:, 1]
    mass = torch.cat([dy.abs().sum(0), (dy * xhat).abs().sum(0)])
    bound = 2 * dy.shape[0] * 2.0 ** -53 * mass * 1.01
    assert float(s0.abs().max()) > 0 and bool(((s0 - s1).abs() <= bound).all()), float(((s0 - s1).abs() / bound).max())


def _one_pixel_split(ops, monkeypatch):
    """The split 16-bit-plane backward-weight kernels (alone and inside the fused launch) cut a problem's pixels into splits that add
    their parts with float atomics; SGAN_WGRAD3_WANT (read per call) sets how many workgroups the split aims at.  One workgroup wanted:
    one split, every dW element has one writer and the two paths can be compared bit for bit."""
    monkeypatch.setenv("SGAN_WGRAD3_WANT", "1")


def _variant(ops):
    return ops.L.lib().sgan_last_variant().decode()


@pytest.mark.parametrize("math,hin", [("f32", 8), ("bf16x3", 8), ("bf16x3", 32)])
def test_backward_weight_reader(ops, monkeypatch, math, hin):
    _one_pixel_split(ops, monkeypatch)
    Ld = _layer(ops, ops.CONV, 4, 2, 1, hin, 64, 32, seed=2)      # 8: 4 x 4 output pixels, one pixel chunk, one writer per dW element

    def run(nd):
        dw = torch.zeros(Ld["k"] ** 2 * Ld["cout"] * Ld["cin"], device="cuda")
        db = torch.zeros(Ld["cout"], device="cuda")
        with ops.math_scope(math):
            ops.conv_wgrad_grouped([(Ld["desc"], Ld["x"], nd, Ld["dout"], dw, db)])
        return dw, db, ops.L.lib().sgan_last_kernel().decode(), _variant(ops)
    (w0, b0, k0, v0), (w1, b1, k1, v1) = _both(ops, Ld, run)
    print("backward-weight ran", k0, v0)
    assert float(w0.abs().max()) > 0 and (k0, v0) == (k1, v1)
    if hin == 32:
        assert "wgrad3" in k0 and v0.endswith("nsplit 1"), (k0, v0)
    assert _same_bits(w0, w1) and _same_bits(b0, b1)


def _pair(ops, Ld):
    def run(nd):
        din = torch.empty_like(Ld["x"])
        sums = torch.zeros(2 * Ld["cin"], dtype=torch.float64, device="cuda")
        dw = torch.zeros(Ld["k"] ** 2 * Ld["cout"] * Ld["cin"], device="cuda")
        db = torch.zeros(Ld["cout"], device="cuda")
        one = ops.conv_bwd_grouped([(Ld["desc"], Ld["dout"], Ld["wt"], din, Ld["x"], nd, sums, 0, False, True, 0)],
                                   [(Ld["desc"], Ld["x"], nd, Ld["dout"], dw, db)])
        return din, dw, one, ops.L.lib().sgan_last_kernel().decode(), _variant(ops)
    return _both(ops, Ld, run)


@pytest.mark.parametrize("hin", [8, 32])
def test_fused_pair_reader(ops, monkeypatch, hin):
    """8 x 8 (the issue's layer): the pair call answers with the two grouped launches.  32 x 32: sg_bwd_fused_kernel takes the pair, its
    backward-weight half with one pixel split.  One writer per dW element either way: dX and dW bit for bit."""
    _one_pixel_split(ops, monkeypatch)
    (d0, w0, one0, k0, v0), (d1, w1, one1, k1, v1) = _pair(ops, _layer(ops, ops.CONV, 4, 2, 1, hin, 64, 32, seed=3))
    print("fused pair ran", k0, v0, one0)
    assert (one0, k0, v0) == (one1, k1, v1)
    if hin == 32:
        assert one0 and "sg_bwd_fused" in k0 and v0.endswith("nsplit 1"), (k0, v0)
    assert _same_bits(d0, d1) and _same_bits(w0, w1)


def test_thin_pair_reader(ops):
    """4 <-> 32 at 16 x 16: the generator's output ConvTranspose2d(32, 2 -> 4 stored).  The thin backward-weight half walks the 8 x 8
    input pixels and splits a problem only above 256 of them: one split here (the variant says so), one writer per dW element, and dX
    and dW are both compared bit for bit."""
    (d0, w0, one0, k0, v0), (d1, w1, one1, k1, v1) = _pair(ops, _layer(ops, ops.CONVT, 4, 2, 1, 8, 32, 4, cout_l=2, seed=4))
    print("thin pair ran", k0, v0, one0)
    assert (one0, k0, v0) == (one1, k1, v1)
    assert one0 and "thin_pair" in k0 and v0.endswith("nsplit 1"), (k0, v0)
    assert float(w0.abs().max()) > 0
    assert _same_bits(d0, d1) and _same_bits(w0, w1)


def test_norm_bwd_apply_reader(ops):
    g = torch.Generator(device="cuda").manual_seed(5)
    Cs, H = 200, 9
    x = torch.randn(H, H, Cs, device="cuda", generator=g) * 2 - 1
    dy = torch.randn(H, H, Cs, device="cuda", generator=g)
    x64 = x.double().reshape(-1, Cs)
    stats = torch.cat([x64.sum(0), (x64 * x64).sum(0)])
    sums = torch.randn(2 * Cs, device="cuda", generator=g).double()
    table, = finalise(ops, [(stats, Cs, H * H, 1e-5, 0, 0)])
    res = []
    for t in (None, table):
        d = dy.clone()
        ops.norm_bwd_apply(d, x, ops.norm_desc(stats, None, None, H * H, 1e-5, 0, 0.0, 0, 0, t), sums)
        torch.cuda.synchronize()
        res.append(d)
    assert not torch.equal(res[0], dy)
    assert _same_bits(res[0], res[1])


# ---- whole steps ----------------------------------------------------------------------------------------------------------------
def _fresh_tables_checked(ops, monkeypatch, seen):
    """Every backward walk first checks each table it is about to hand out against the statistics as they are NOW (the in-kernel
    path on the fp64 sums): a table left over from an earlier forward of the same buffers fails here."""
    from supervised_gan_amd import chain
    walk = chain._grouped_backward

    def checked(nets, xs, outs, stats, *a, **kw):
        if torch.cuda.is_current_stream_capturing():      # the probe synchronises: the captured pass itself is checked launch by launch
            return walk(nets, xs, outs, stats, *a, **kw)
        for j, net in enumerate(nets):
            geo = net._geometry(xs[j].shape[0], xs[j].shape[1])
            tabs = stats[j][-1].norm_tables
            for li, Lr in enumerate(net.layers):
                if Lr.norm and tabs is not None:
                    nd = net._norm_of(li, stats[j], geo[li][3] * geo[li][4])
                    now = probe(ops, nd, Lr.cout_s)
                    assert torch.equal(now.view(torch.int32), tabs[stats[j][li].data_ptr()].view(torch.int32)), (type(net).__name__, li)
                    seen[0] += 1
        return walk(nets, xs, outs, stats, *a, **kw)
    monkeypatch.setattr(chain, "_grouped_backward", checked)


def _reset_log(ops):
    ops.NORM_TABLE_LOG.update({k: 0 for k in ops.NORM_TABLE_LOG})


def _within_the_rule(ga, gb):
    """tests/test_hip_segm_nod.py: 1e-4 of the tensor's maximum; a bias in front of an InstanceNorm (an analytically zero gradient)
    is held to its layer's weight gradient."""
    for k, g in ga.items():
        scale = ga.get(k.replace(".bias", ".weight"), g)
        assert float((g - gb[k]).abs().max()) <= 1e-4 * float(scale.abs().max()) + 1e-12, k


def test_step_with_and_without_tables(ops, monkeypatch):
    import sgan_oracle as O
    from test_hip_step import build_model, real3, step1_with_captures
    cfg = O.FCGANConfig(ngf=8, ndf=8, noiseSize=2, n_update_G=2)      # the fcgan_step_small shape
    caps, logs = {}, {}
    for off in (True, False):
        monkeypatch.setattr(ops, "NO_NORM_TABLE", off)
        seen = [0]
        with monkeypatch.context() as mp:
            _fresh_tables_checked(ops, mp, seen)
            m = build_model(cfg, 0)
            _reset_log(ops)
            caps[off] = step1_with_captures(m, real3(cfg, 0))
            torch.cuda.synchronize()
        logs[off] = (dict(ops.NORM_TABLE_LOG), seen[0])
    print("bookkeeping (switch on, switch off):", logs[True], logs[False])
    assert (logs[True][0]["finalised"], logs[True][0]["with_table"], logs[True][1]) == (0, 0, 0) and logs[False][0]["dropped"] == 0
    assert logs[True][0]["without_table"] > 0
    # every normalised tensor a backward kernel read came with its table, and as many were read as without the switch
    assert logs[False][0]["without_table"] == 0 and logs[False][0]["with_table"] == logs[True][0]["without_table"]
    assert logs[False][0]["finalised"] >= logs[False][1] > 0
    a, b = caps[True], caps[False]
    assert torch.equal(a["fake"], b["fake"])      # the forward pass reads no table
    for la, lb in zip(a["loss_D"] + [a["loss_G"]], b["loss_D"] + [b["loss_G"]]):
        assert abs(la - lb) <= 1e-5 * max(1.0, abs(la))
    for ga, gb in zip(a["gradD"], b["gradD"]):
        _within_the_rule(ga, gb)
    _within_the_rule(a["gradG"], b["gradG"])


@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_tables_follow_their_statistics_over_two_steps(ops, monkeypatch, norm):
    """Two steps on different inputs, launch by launch through the graphed step (n_update_G 2: a second forward of the generator per
    step; the prefetch path refills the kept forward in place; then two eager steps of a second trainer): every table handed to a
    backward walk equals what the statistics behind it give at that moment."""
    import gc
    from supervised_gan_amd.graph_step import GraphedStep
    from test_graph_step import FCGAN, _build, _ring
    ring = _ring(128)
    seen = [0]
    _fresh_tables_checked(ops, monkeypatch, seen)
    _reset_log(ops)
    random.seed(11)
    m = _build(FCGAN + ["--norm", norm])
    gs = GraphedStep(m)
    gs.capture(ring[0])
    at_capture = seen[0]
    for i in (1, 2):
        gs.step(ring[i], replay=False)
    torch.cuda.synchronize()
    assert gs._prefetch and seen[0] > at_capture > 0
    gs.step(ring[3])      # and a replay still runs
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for v in m.get_current_errors().values())
    e = _build(FCGAN + ["--norm", norm])
    before = seen[0]
    for i in (0, 1):
        e.set_input(ring[i])
        e.optimize_parameters()
    torch.cuda.synchronize()
    assert seen[0] > before
    assert ops.NORM_TABLE_LOG["without_table"] == 0 and ops.NORM_TABLE_LOG["with_table"] > 0
    del gs, m, e
    gc.collect()


def test_graphed_step_with_and_without_tables(ops, monkeypatch):
    """The graphed half of the whole-step case, at the fcgan_step_small shape (test_graph_step.FCGAN: 128 x 128, ngf = ndf = 8,
    noiseSize 2, n_update_G 2, prefetch on).  Two trainers are captured from the same seed, one with tables and one under the switch;
    the state of the first after its capture (tests/graph_state.py) is written into the second, so both replay ONE step from one
    state.  A replay runs what the capture recorded: the loss launches with the finalise jobs that were pending then, the backward
    launches with the table addresses handed out then -- for the kept generator forward, ChainNet._kept_tab, which is filled with
    NaN before the replay, so a captured loss launch that did not carry the kept forward's jobs shows.  Compared, as in the eager
    half: the output, the losses, and the gradients handed to the optimizers of the discriminator update and of the first generator
    update, by the rule for two runs of one build.  Bookkeeping: the capture (two warm-up steps and the captured pass, every walk of
    them) read as many normalised tensors with a table as the switched-off trainer read without, and none the other way."""
    import gc
    from graph_state import restore, snapshot
    from supervised_gan_amd.graph_step import GraphedStep
    from test_graph_step import FCGAN, _build, _ring
    from test_graph_step_snapshot import _install_probes
    ring = _ring(128)
    gss, logs = {}, {}
    for off in (False, True):
        monkeypatch.setattr(ops, "NO_NORM_TABLE", off)
        random.seed(11)
        m = _build(FCGAN)
        gs = GraphedStep(m)
        _install_probes(m)
        _reset_log(ops)
        gs.capture(ring[0])
        torch.cuda.synchronize()
        logs[off] = dict(ops.NORM_TABLE_LOG)
        assert gs._prefetch
        gss[off] = gs
    print("bookkeeping of the captures (tables, switch):", logs[False], logs[True])
    assert logs[False]["without_table"] == 0 and logs[False]["dropped"] == 0
    assert logs[True]["with_table"] == 0 and logs[True]["finalised"] == 0
    assert logs[False]["with_table"] == logs[True]["without_table"] > 0
    S = snapshot(gss[False])
    restore(gss[True], S)
    kept_tab = gss[False].m.netG._kept_tab
    kept_tab.fill_(float("nan"))
    assert getattr(gss[True].m.netG, "_kept_tab", None) is None
    rec = {}
    for off in (False, True):
        monkeypatch.setattr(ops, "NO_NORM_TABLE", off)
        gs = gss[off]
        gs.step(ring[1])
        torch.cuda.synchronize()
        rec[off] = dict(errors=[float(v) for v in gs.m.get_current_errors().values()], out=gs.m.fake.detach().clone(),
                        probes={k: t.clone() for k, t in gs.m._probes.items()})
    assert bool(torch.isfinite(kept_tab).all())      # the replayed loss launch refilled the kept forward's table
    a, b = rec[False], rec[True]
    # G_GAN, D_real, D_fake as the trainer reports them after the step (G_GAN: of the second generator update, behind two optimizer
    # steps): 1e-3, the tolerance of tests/test_hip_step.py
    for x, y in zip(a["errors"], b["errors"]):
        assert np.isfinite(x) and abs(x - y) <= 1e-3 * max(1.0, abs(y)), (a["errors"], b["errors"])
    names = [k for k in a["probes"] if k.startswith(("probe.0.", "probe.1."))]
    assert len(names) >= 2 and list(a["probes"]) == list(b["probes"])
    for k in names:
        d, ref = float((a["probes"][k] - b["probes"][k]).abs().max()), float(b["probes"][k].abs().max())
        print(f"{k}: max |difference| {d:.3e} of max {ref:.3e}")
        assert ref > 0 and d <= 1e-4 * ref, k
    del gss, gs, m
    gc.collect()

"""The library's own random streams on the MI355X against the numpy reference (tests/philox_ref.py, itself held to the Random123
vectors by tests/test_philox_host.py).

The network and step tests inject the reference's masks and noise, so sg_dropout_mask_kernel, sg_normal_fill_kernel and
sg_normal_fill_pair_kernel (csrc/sgan_ew.hip) never run under a parity check there.  Here:

A. dropout masks, bit for bit (every step of the mask is exact float32 arithmetic);
B. normal fills, elementwise |z_gpu - z_ref| <= TOL * max(1, rad) against the float64 Box-Muller of the same Philox words;
C. the host bookkeeping: over two training steps of every stochastic generator and trainer no two draws of one (c2, key) stream
   share a counter, and every network moves its offset once per forward by its longest draw.

TOL.  Measured on an MI355X: the largest |z_gpu - z_ref| / max(1, rad) over the 1 049 607-value fill (seed 7, offset 11) is
1.975e-07 = 2^-22.27 (1.959e-07 for the other seed / offset; 0.9e-07 .. 1.7e-07 for the small fills).  TOL is four times that,
rounded up to a power of two: 2^-20 (the factor covers other seeds), and has to stay <= 2^-18: a wrong word, a wrong pairing or
swapped sin / cos give errors of order 1, a few ulp of float32 are about 2^-21.

What each case is there to catch: a wrong round count, constant or key schedule changes every word (A fails everywhere); c1
dropped: the offsets 2^32 - 5 (carry in mid-fill) and 2^40 + 3; k1 dropped: the seed with a high word; masks on c2 = 0: every
mask, and the separate-streams test; sin / cos swapped or words paired otherwise: errors of order 1 in B; the pair's second
latent at offset + n / 4: n = 105 (26 instead of 27 blocks); a grid-stride loop that does not stride: the 1 049 607-value fills."""
import functools
import math

import numpy as np
import pytest
import torch

import philox_ref as P

pytestmark = pytest.mark.gpu

MEASURED_MAX_ERR = 1.975e-07     # MI355X, the N_BIG fill of seed 7 at offset 11
TOL = 2.0 ** -20
TOL_CAP = 2.0 ** -18

SEED_A, SEED_B = 7, 0x9E3779B97F4A7C15          # the second has a nonzero high word (k1)
N_BIG = 4 * 262144 + 4 * 257 + 3                # 1 049 607: 262 402 blocks of four > 1024 workgroups x 256: a second, partial grid-stride trip
GUARD = -7.0


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import ops
    from supervised_gan_amd import _lib
    _lib.lib()   # raises if libsgan_hip.so is missing -- no fallback
    return ops


def test_tolerance_respects_its_cap():
    assert TOL <= TOL_CAP and math.log2(TOL) == int(math.log2(TOL))
    assert 4 * MEASURED_MAX_ERR <= TOL < 8 * MEASURED_MAX_ERR


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def dev_offset(value):
    return None if value is None else torch.tensor([value], dtype=torch.int64, device="cuda")


def read_offset(off):
    return None if off is None else int(off.item())


def check_offset(off, start, n, advance, times=1):
    if off is not None:
        assert read_offset(off) == (start + times * P.blocks(n) if advance else start)


@functools.lru_cache(maxsize=None)
def normal_ref(n, seed, offset):
    """(z, rad) of philox_ref.normal_ref, computed once per (n, seed, offset) and shared read-only."""
    z, rad = P.normal_ref(n, seed, offset or 0)
    z.setflags(write=False)
    rad.setflags(write=False)
    return z, rad


def check_normal(got, z, rad, what=""):
    """got: float32 values from the device, any shape matching z / rad."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == z.shape
    assert np.isfinite(got).all(), what
    assert np.abs(got).max() <= P.ZMAX * (1 + 2.0 ** -20), what
    err = np.abs(got - z) / np.maximum(1.0, rad)
    worst = float(err.max())
    print(f"normal fill {what}: max |z_gpu - z_ref| / max(1, rad) = {worst:.3e} = 2^{math.log2(worst) if worst else -math.inf:.2f}")
    assert worst <= TOL, (what, worst, int(err.argmax()))
    return worst


def guarded(n, fill=GUARD):
    """(n-element contiguous view the kernel writes, the n + 1 element allocation behind it)."""
    whole = torch.full((n + 1,), fill, dtype=torch.float32, device="cuda")
    return whole[:n], whole


# (n, seed, offset, advance): tails 1, 2, 3, 5, 43; one block 1024 / two blocks 1028; the grid-stride case; offset None (read as 0),
# 0, 11, 2^32 - 5 with n = 43 (11 blocks: the carry into c1 falls inside the fill), 2^40 + 3; both seeds; both advance modes
EDGES = [(1, SEED_A, None, True),
         (2, SEED_A, 0, True),
         (3, SEED_B, 11, False),
         (5, SEED_A, 11, True),
         (43, SEED_A, 2 ** 32 - 5, True),
         (43, SEED_B, 2 ** 32 - 5, False),
         (1024, SEED_B, 2 ** 40 + 3, True),
         (1024, SEED_A, None, False),
         (1028, SEED_A, 11, True),
         (1028, SEED_B, 0, False),
         (N_BIG, SEED_A, 11, True),
         (N_BIG, SEED_B, 2 ** 40 + 3, False)]
P_OF_CASE = [0.5, 0.2, 0.5, 0.0, 0.5, 0.2, 0.5, 0.0, 0.5, 0.2, 0.5, 0.2]


def _id(case):
    n, seed, offset, advance = case[:4]
    o = "none" if offset is None else {2 ** 32 - 5: "2p32m5", 2 ** 40 + 3: "2p40p3"}.get(offset, str(offset))
    return f"n{n}-{'A' if seed == SEED_A else 'B'}-off{o}-{'adv' if advance else 'keep'}"


# ------------------------------------------------------------------------------------------------
# A. dropout masks
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c + (p,) for c, p in zip(EDGES, P_OF_CASE)], ids=_id)
def test_dropout_mask_bit_for_bit(hip, case):
    n, seed, offset, advance, p = case
    mask, whole = guarded(n)
    off = dev_offset(offset)
    hip.dropout_mask(mask, p, seed, off, advance=advance)
    torch.cuda.synchronize()
    got = whole.cpu().numpy()
    ref = P.dropout_ref(n, p, seed, offset or 0)
    assert np.array_equal(got[:n], ref), int(np.flatnonzero(got[:n] != ref)[0])
    assert got[n] == GUARD
    check_offset(off, offset, n, advance)
    if p == 0.0:
        assert (got[:n] == 1.0).all()


# ------------------------------------------------------------------------------------------------
# B. normal fills
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EDGES, ids=_id)
def test_normal_fill_against_reference(hip, case):
    """n <= 1024 is one workgroup, which moves the offset itself; 1028 and the grid-stride case take the separate advance launch."""
    n, seed, offset, advance = case
    dst, whole = guarded(n)
    off = dev_offset(offset)
    hip.normal_fill(dst, seed, off, advance=advance)
    torch.cuda.synchronize()
    got = whole.cpu().numpy()
    z, rad = normal_ref(n, seed, offset)
    check_normal(got[:n], z, rad, _id(case))
    assert got[n] == GUARD
    check_offset(off, offset, n, advance)


NHWC_SHAPES = [(3, 7, 5, 4),      # 105 values: a tail of one, quads straddle the channel planes (35 values each), one pad channel
               (6, 8, 5, 8)]      # 240 values, two pad channels


@pytest.mark.parametrize("C,H,W,Cs", NHWC_SHAPES)
@pytest.mark.parametrize("advance", [True, False])
def test_normal_fill_nhwc_against_reference(hip, C, H, W, Cs, advance):
    n, seed, offset = C * H * W, SEED_B, 2 ** 32 - 5
    flat, whole = guarded(H * W * Cs, 7.0)
    buf = flat.view(H, W, Cs)
    off = dev_offset(offset)
    hip.normal_fill_nhwc(buf, C, seed, off, advance=advance)
    torch.cuda.synchronize()
    got = whole.cpu().numpy()
    z, rad = normal_ref(n, seed, offset)
    g = got[:-1].reshape(H, W, Cs)
    check_normal(g[:, :, :C], P.to_nhwc(z, C, H, W, C, 0.0), P.to_nhwc(rad, C, H, W, C, 0.0), f"nhwc {C}x{H}x{W}/{Cs}")
    assert (g[:, :, C:] == 7.0).all() and got[-1] == 7.0
    check_offset(off, offset, n, advance)


@pytest.mark.parametrize("C,H,W,Cs", NHWC_SHAPES)
@pytest.mark.parametrize("offset", [11, 2 ** 32 - 30])
def test_normal_fill_nhwc_pair_against_reference(hip, C, H, W, Cs, offset):
    """The second latent starts at offset + ceil(n / 4) (n = 105: + 27 blocks, not + 26.25), the offset moves by twice that, the
    arena is zeroed and nothing behind it is touched."""
    n, seed = C * H * W, SEED_A
    nq = P.blocks(n)
    fa, wa = guarded(H * W * Cs, 7.0)
    fb, wb = guarded(H * W * Cs, 7.0)
    arena = torch.full((8,), 3.0, dtype=torch.float64, device="cuda")
    off = dev_offset(offset)
    hip.normal_fill_nhwc_pair(fa.view(H, W, Cs), fb.view(H, W, Cs), C, seed, off, arena[:6])
    torch.cuda.synchronize()
    for which, (whole, start) in enumerate([(wa, offset), (wb, offset + nq)]):
        got = whole.cpu().numpy()
        z, rad = normal_ref(n, seed, start)
        g = got[:-1].reshape(H, W, Cs)
        check_normal(g[:, :, :C], P.to_nhwc(z, C, H, W, C, 0.0), P.to_nhwc(rad, C, H, W, C, 0.0), f"pair[{which}] {C}x{H}x{W}/{Cs}")
        assert (g[:, :, C:] == 7.0).all() and got[-1] == 7.0
    assert read_offset(off) == offset + 2 * nq
    assert arena.cpu().tolist() == [0.0] * 6 + [3.0] * 2


@pytest.mark.parametrize("n,seed,offset", [(43, SEED_A, 11), (1028, SEED_B, 2 ** 32 - 5)])
def test_mask_and_noise_of_one_seed_and_offset_are_separate_streams(hip, n, seed, offset):
    """c2 = 1 for masks, 0 for normal fills: a mask and a noise tensor of one level (same key, same offset) use different words."""
    mask, _ = guarded(n)
    noise, _ = guarded(n)
    off = dev_offset(offset)
    hip.dropout_mask(mask, 0.5, seed, off, advance=False)
    hip.normal_fill(noise, seed, off, advance=False)
    torch.cuda.synchronize()
    assert np.array_equal(mask.cpu().numpy(), P.dropout_ref(n, 0.5, seed, offset))
    check_normal(noise.cpu().numpy(), *normal_ref(n, seed, offset), "beside a mask")
    assert not np.array_equal(P.words(seed, offset, 4, P.C2_DROPOUT), P.words(seed, offset, 4, P.C2_NORMAL))
    assert read_offset(off) == offset


# Counters of seed 0 among the first 2^26 whose word 0 or word 2 has its top 24 bits all ones (u1 = 1: rad = 0, both outputs exactly
# 0) or all zeros (u1 = 2^-24: the largest radius, sqrt(48 ln 2)); found once on the CPU with philox_ref.words.  (counter, index of
# the word, the four words)
U1_ONES = [(2330056, 2, "58004768 9e5a72af ffffff45 f1d970a6"), (18082804, 2, "c91a526d 5004285b ffffff05 dd768ac4"),
           (24962728, 2, "4021e51e f3800b02 ffffffb9 24c7a892"), (35333089, 2, "2b98d599 61a50729 ffffffde 76c4170c"),
           (38471471, 0, "ffffffec bb5882e5 b46d5b9b 1e7126e9"), (54165442, 2, "1f63dc0d 3cce4bac ffffff37 4fa31e22"),
           (58912592, 0, "ffffff56 8c78f0f5 05cba755 76bac4e7"), (64966008, 2, "ae07730c b8a5d21c ffffffab ca9dd45e")]
U1_ZEROS = [(14883995, 0, "00000093 9f72220c e0d8a663 7890953d"), (17758991, 0, "00000079 bb39fbf9 9f0c1457 2e25dd96"),
            (21603008, 2, "5de317ae de4c58b2 000000bc 6c0df501"), (32952608, 0, "000000e8 9f3b929d 01db4b1f df05df34"),
            (34829342, 0, "000000d3 69b276f7 4c652eba 86f62567"), (48643752, 0, "00000015 5002e164 5a5c2f86 9040ba85"),
            (55573990, 0, "0000002d 6e3cf48f d19ec300 b834810c"), (65593969, 2, "853f28e3 54c5babb 000000db 6ae3f70b"),
            (66601073, 2, "295c1112 20a3931c 00000044 5dac7a0a")]


def test_u1_edges(hip):
    """Both ends of u1 = ((w >> 8) + 1) 2^-24 turned up in the first 2^26 counters of seed 0 (8 and 9 of them).  u1 = 1: log 1 = 0, the
    pair is exactly (0, 0); u1 = 2^-24: the radius is sqrt(48 ln 2) and the values stay finite and inside the bound."""
    for table, ones in ((U1_ONES, True), (U1_ZEROS, False)):
        for ctr, wi, text in table:
            w = P.words(0, ctr, 1, P.C2_NORMAL)[0]
            assert [int(x, 16) for x in text.split()] == w.tolist()
            assert int(w[wi]) >> 8 == (0xFFFFFF if ones else 0)
            dst, whole = guarded(4)
            off = dev_offset(ctr)
            hip.normal_fill(dst, 0, off)
            got = whole.cpu().numpy()
            z, rad = normal_ref(4, 0, ctr)
            check_normal(got[:4], z, rad, f"u1 edge at counter {ctr}")
            pair = got[wi: wi + 2]
            if ones:
                assert rad[wi] == 0.0 and (pair == 0.0).all(), (ctr, pair)
            else:
                assert abs(rad[wi] - P.ZMAX) < 1e-12 and abs(float(np.hypot(*pair.astype(np.float64))) - P.ZMAX) <= TOL * P.ZMAX, (ctr, pair)
            assert got[4] == GUARD and read_offset(off) == ctr + 1


# ------------------------------------------------------------------------------------------------
# C. host bookkeeping: no two live streams overlap, one advance per pass
# ------------------------------------------------------------------------------------------------
class StreamLog:
    """Wraps the four drawing entry points of ops: every call is recorded as (c2, key mod 2^64, offset read back before the call,
    blocks of four drawn) and then runs.  The read-back synchronises: not for use under graph capture."""

    def __init__(self, ops, monkeypatch):
        self.records = []

        def wrap(name, c2, blocks_of, seed_at, off_at):
            inner = getattr(ops, name)

            def call(*a, **k):
                assert not k or set(k) <= {"advance", "zero"}, k
                off = a[off_at] if len(a) > off_at else None
                self.records.append((c2, int(a[seed_at]) & (2 ** 64 - 1), 0 if off is None else int(off.item()), blocks_of(a), name))
                return inner(*a, **k)
            monkeypatch.setattr(ops, name, call)
        wrap("dropout_mask", P.C2_DROPOUT, lambda a: P.blocks(a[0].numel()), 2, 3)                       # (mask, p, seed, offset_dev)
        wrap("normal_fill", P.C2_NORMAL, lambda a: P.blocks(a[0].numel()), 1, 2)                         # (dst, seed, offset_dev)
        wrap("normal_fill_nhwc", P.C2_NORMAL, lambda a: P.blocks(a[0].shape[0] * a[0].shape[1] * a[1]), 2, 3)      # (buf, C, seed, offset_dev)
        wrap("normal_fill_nhwc_pair", P.C2_NORMAL, lambda a: 2 * P.blocks(a[0].shape[0] * a[0].shape[1] * a[2]), 3, 4)   # (a, b, C, seed, off)

    def assert_disjoint(self, at_least):
        assert len(self.records) >= at_least, (len(self.records), at_least)
        streams = {}
        for c2, key, off, nq, name in self.records:
            streams.setdefault((c2, key), []).append((off, off + nq, name))
        for (c2, key), spans in streams.items():
            spans.sort()
            for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
                assert a1 <= b0, f"stream (c2={c2}, key={key:#x}): {an} draws counters [{a0}, {a1}) and {bn} draws [{b0}, {b1})"


def watch_advance(net, expected_blocks, seen):
    """Every run_forward of `net` has to move the net's offset by expected_blocks(H of its input): once, by the longest draw."""
    inner = net.run_forward

    def run(x, *a, **k):
        H = (x["label"] if isinstance(x, dict) else x).shape[0]
        before = 0 if net._rng_offset is None else int(net._rng_offset.item())
        r = inner(x, *a, **k)
        seen.append((type(net).__name__, int(net._rng_offset.item()) - before, expected_blocks(H)))
        return r
    net.run_forward = run


# longest draw of one forward, from the architectures (the reference's models/networks.py), in Philox blocks of four values
def unet_blocks(ngf, n, dropout, noise):
    """Level l = 1 .. n-1 of the decoder emits [ngf min(2^(l-1), 8), H / 2^l, W / 2^l]; Gaussian noise on every level, dropout on
    levels 4 .. n-2."""
    def f(H):
        sizes = [ngf * min(2 ** (l - 1), 8) * (H >> l) ** 2 for l in range(1, n) if noise or (dropout and 4 <= l <= n - 2)]
        return P.blocks(max(sizes))
    return f


def resnet_blocks(ngf):
    return lambda H: P.blocks(4 * ngf * (H // 4) ** 2)          # every block masks a [4 ngf, H/4, W/4] tensor


def crn_blocks(ngf):
    return lambda H: P.blocks(ngf * (H // 2) ** 2)              # noise on the upsampled tensor of stages 5 .. 1: the largest is [ngf, H/2, W/2]


def rand(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def check_advances(seen, at_least):
    assert len(seen) >= at_least, seen
    for name, moved, want in seen:
        assert moved == want and want > 0, seen


@pytest.mark.parametrize("which", ["unet_128", "resnet_6blocks", "crn"])
def test_generator_streams_do_not_overlap(hip, monkeypatch, which):
    from supervised_gan_amd import networks as N
    log, seen = StreamLog(hip, monkeypatch), []
    if which == "unet_128":
        G, S = N.define_G(2, 1, 8, which, "instance", True, add_gaussian_noise=True, gpu_ids=[0]), 128
        watch_advance(G, unet_blocks(8, 7, True, True), seen)
        draws = 2 + 6         # masks on levels 4, 5; noise on levels 1 .. 6
    elif which == "resnet_6blocks":
        G, S = N.define_G(2, 1, 8, which, "instance", True, gpu_ids=[0]), 32
        watch_advance(G, resnet_blocks(8), seen)
        draws = 6
    else:
        G, S = N.define_G(2, 1, 8, which, "instance", False, n_layers_G=5, noise_nc=8, upsample_mode="convt", n_layers_CRN_block=1,
                          share_label_weights=True, add_gaussian_noise=True, gaussian_sigma=0.1, gpu_ids=[0]), 64
        watch_advance(G, crn_blocks(8), seen)
        draws = 5
    for step in range(2):
        x = rand(10 + step, 1, 2, S, S).cuda().requires_grad_(True)
        y = G.forward(x, rand(20 + step, 1, 8, S // 64, S // 64).cuda()) if which == "crn" else G.forward(x)
        (y * rand(30 + step, *y.shape).cuda()).sum().backward()
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    log.assert_disjoint(2 * draws)
    check_advances(seen, 2)


def _model(argv):
    from supervised_gan_amd.models import create_model
    from supervised_gan_amd.options import TrainOptions
    common = ["--name", "t", "--norm", "instance", "--gpu_ids", "0", "--checkpoints_dir", "/tmp/sgan_ckpt"]
    return create_model(TrainOptions().parse(common + argv, save=False, verbose=False))


def _batch(step, S):
    return {"A": rand(100 + step, 1, 3, S, S), "B": rand(200 + step, 1, 3, S, S), "A_paths": ["synthetic"], "B_paths": ["synthetic"]}


D1 = ["--which_model_netD1", "n_layers", "--n_layers_D1", "3", "--ndf1", "8", "--scale_factor1", "1", "--lambda_D1", "1.0"]
D2 = ["--which_model_netD2", "n_layers", "--n_layers_D2", "3", "--ndf2", "8", "--scale_factor2", "1", "--lambda_D2", "1.0"]
NOISY = ["--add_gaussian_noise", "--gaussian_sigma", "0.1"]
TRAINERS = {
    "cgan": (["--model", "cgan", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "128", "--which_model_netG", "unet_128",
              "--ngf", "8", "--which_model_netD", "n_layers", "--n_layers_D", "3", "--ndf", "8", "--scale_factor", "1", "--lambda_D", "1.0",
              "--which_channel", "rg_b"] + NOISY, 128, ["netG"]),
    "cgan_cycle": (["--model", "cgan_cycle", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "128", "--which_channel", "rg_b",
                    "--which_model_netG1", "unet_128", "--ngf1", "8", "--which_model_netG2", "unet_128", "--ngf2", "8"] + D1 + NOISY,
                   128, ["netG1", "netG2"]),
    "twostage_cycle": (["--model", "twostage_cycle", "--which_direction", "AtoB", "--dataset_mode", "aligned", "--fineSize", "128",
                        "--transform_1to2", "bilinear_2", "--which_channel", "rg_b", "--which_model_netG1", "fcgan", "--n_layers_G1", "4",
                        "--ngf1", "8", "--noise_nc1", "8", "--noiseSize1", "2", "--no_dropout1", "--which_model_netG2", "unet_128", "--ngf2", "8",
                        "--which_model_netF2", "unet_128", "--nff2", "8"] + D1 + D2 + NOISY, 128, ["netG2", "netF2"]),
}


@pytest.mark.parametrize("name", list(TRAINERS))
def test_trainer_streams_do_not_overlap(hip, monkeypatch, name):
    """Two optimisation steps with the trainer's and the generators' own draws (nothing injected).  The generators of cgan_cycle and
    twostage_cycle have the same architecture and widths: they must still draw from different streams."""
    argv, S, nets = TRAINERS[name]
    log, seen = StreamLog(hip, monkeypatch), []
    m = _model(argv)
    for attr in nets:
        G = getattr(m, attr)
        assert G.use_dropout and G.add_gauss
        watch_advance(G, unet_blocks(8, 7, True, True), seen)
    forwards = {"cgan": 1, "cgan_cycle": 3, "twostage_cycle": 5}[name]          # generator calls of one forward() that draw
    for step in range(2):
        m.set_input(_batch(step, S))
        m.optimize_parameters()
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in m.get_current_errors().values())
    log.assert_disjoint(2 * 8 * forwards)
    check_advances(seen, 2 * forwards)
    keys = {attr: getattr(m, attr)._rng_seed for attr in nets}
    assert len(set(keys.values())) == len(nets), keys


def test_fcgan_trainer_streams_do_not_overlap(hip, monkeypatch):
    """--model fcgan: the latent of every forward() / sample_noise() continues one stream (key = the seed, counters in order)."""
    log = StreamLog(hip, monkeypatch)
    m = _model(["--model", "fcgan", "--which_direction", "A", "--fineSize", "128", "--input_nc", "2", "--which_model_netG", "deconv",
                "--n_layers_G", "5", "--ngf", "8", "--which_model_netD", "n_layers", "--n_layers_D", "3", "--ndf", "8", "--scale_factor", "1",
                "--lambda_D", "1.0", "--noise_nc", "8", "--noiseSize", "2", "--no_dropout", "--n_update_G", "2", "--no_lsgan",
                "--which_channel", "rg", "--manualSeed", "3"])
    for step in range(2):
        m.set_input({"A": rand(100 + step, 1, 3, 128, 128), "A_paths": ["synthetic"]})
        m.optimize_parameters()
    torch.cuda.synchronize()
    assert all(np.isfinite(v) for v in m.get_current_errors().values())
    log.assert_disjoint(2 * 3)          # forward() and two re-draws per step
    assert {(c2, key) for c2, key, *_ in log.records} == {(P.C2_NORMAL, 3)}
    spans = sorted((off, off + nq) for _, _, off, nq, _ in log.records)
    assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:]))         # one stream, no gaps: 8 x 2 x 2 values = 8 blocks each
    assert all(b - a in (8, 16) for a, b in spans)
    assert int(m._rng_offset.item()) == spans[-1][1]

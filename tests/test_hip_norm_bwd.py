"""sgan_norm_bwd_apply_multi, sgan_norm_apply_bwd_sums and sgan_norm_apply_fwd on their own: the kernels are fed d, x, the forward
statistics and the two backward sums, all computed in float64 on the host from d and x; no conv runs.  dy is updated in place
inside NaN-filled storage (hip_utils.Guarded).  Reference and yardstick: tests/pad_norm_ref.py (pinned on the CPU by
tests/test_pad_norm_ref_host.py); the bound is max |kernel - fp64| <= 4 x max |fp32 restatement - fp64| on the same inputs.

The heterogeneous table (jobs A-D) reaches: workgroups that return early (blockIdx.x >= blocks of their job), a partial last trip of
the four-chunk loop, a channel slice, the affine gradients added exactly once by four workgroups (bit-equal to one fp32 add), the
coefficient loop running twice (C = 260), and -- with the published maximum -- the wave maxima that reuse cA[0..3] at C = 4.

The published max |dy| is bit-equal to the maximum of the job's own result; against the reference it is held to the yardstick of
that result, since |max |a| - max |b|| <= max |a - b|.

sgan_norm_apply_bwd_sums: dt * mask is bit-equal.  The grouping of its fp32 partial sums (per thread, then LDS atomics in any
order, then fp64 atomics) cannot be restated, so the sums are held to the a-priori bound of an fp32 summation of n = H W terms in
any grouping, n 2^-24 sum |terms| (plus the fp64 floor n 2^-53 (|base| + sum |terms|) for the accumulator's own rounding); the
sequential fp32 restatement is printed beside it.

Figures of the run on an MI355X, kernel deviation from fp64 | fp32 yardstick (pytest -s prints them per test):
    norm_bwd_apply_multi, dx       A (35 x 4) 1.8e-07 | 1.8e-07   B (221 x 24 in 32, BN) 3.5e-07 | 3.5e-07
                                   C (1600 x 8, BN) 3.0e-07 | 3.0e-07   D (9 x 260) 3.4e-07 | 3.4e-07
    nine jobs, dx                  8.0e-08 .. 3.5e-07, each equal to its yardstick but job 1 (1.9e-07 | 2.1e-07)
    replicated sums / statistics   B 3.5e-07 | 3.5e-07, C 3.0e-07 | 3.0e-07; 0.00 ulp from the plain-array run
    published maximum              A 1.92953873 (fp64 1.92953881): off by 8.8e-08 | 1.8e-07; C with the planted element 29.2808132
                                   (fp64 29.2808118): off by 1.5e-06 | 1.5e-06; both modes alike
    norm_apply_bwd_sums            kernel from fp64 | sequential fp32 restatement | a-priori bound (worst over mask / no mask)
                                   C = 12   s1 9.2e-06 | 0 | 1.3e-03      s2 6.6e-06 | 2.8e-06 | 1.1e-03
                                   C = 40   s1 7.6e-06 | 0 | 1.4e-03      s2 1.3e-05 | 2.6e-06 | 1.2e-03
                                   C = 16   s1 6.4e-06 | 0 | 1.4e-03      s2 8.8e-06 | 1.8e-06 | 1.2e-03
                                   C = 256  s1 3.4e-06 | 0 | 1.5e-03      s2 4.4e-06 | 3.4e-06 | 1.2e-03      (worst err / bound 0.011)
    norm_apply_fwd, x_res + BN(c)  2.5e-07 | 3.3e-07
"""
import ctypes as C

import numpy as np
import pytest
import torch

import pad_norm_ref as R
from hip_utils import Guarded

pytestmark = pytest.mark.gpu

EPS = float(np.float32(1e-5))
U32 = R.U32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import _lib, ops
    _lib.lib()
    return ops


@pytest.fixture
def math_mode(ops, request):
    """Sets the arithmetic mode named by the test's parameter and puts the previous one back."""
    prev = ops.get_math()
    ops.set_math(request.param)
    yield request.param
    ops.set_math(prev)


def _cuda(a, dtype):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


class Job:
    """One norm-backward job with its host data, float64 reference and float32 yardstick.  `slice_of`: the channels sit at
    `c0` of a `slice_of`-wide buffer, statistics and sums at the same offset of a `slice_of`-wide arena."""

    def __init__(self, name, H, W, Cn, bn, seed, slice_of=0, c0=0, plant=None):
        rng = np.random.default_rng(seed)
        self.name, self.H, self.W, self.C, self.bn, self.slice_of, self.c0 = name, H, W, Cn, bn, slice_of, c0
        self.x = (rng.standard_normal((H, W, Cn)) * 1.5 + 0.5).astype(np.float32)
        self.d = rng.standard_normal((H, W, Cn)).astype(np.float32)
        if plant is not None:      # (pixel, channel): one element a hundred times larger, so that the maximum is known to sit there
            self.d.reshape(H * W, Cn)[plant] *= 100.0
        self.gamma = (rng.uniform(0.5, 1.5, Cn) * rng.choice([-1.0, 1.0], Cn)).astype(np.float32) if bn else None
        self.beta = (rng.standard_normal(Cn) * 0.3).astype(np.float32) if bn else None
        self.width = slice_of if slice_of else Cn
        self.sq = slice_of
        self.stats = R.stats_of(self.x)
        mean, rstd = R.mean_rstd(self.stats, H * W, EPS, Cn, out_dtype=np.float64)
        d64 = self.d.astype(np.float64)
        self.s1, self.s2 = d64.sum((0, 1)), (d64 * ((self.x.astype(np.float64) - mean) * rstd)).sum((0, 1))
        self.ref64, self.dg64, self.db64 = R.norm_bwd(self.d, self.x, self.stats, self.gamma, H * W, EPS, self.s1, self.s2)
        self.ref32, _, _ = R.norm_bwd(self.d, self.x, self.stats, self.gamma, H * W, EPS, self.s1, self.s2, dtype=np.float32)
        assert self.ref32.dtype == np.float32
        self.gbase = np.concatenate([0.5 + 0.25 * np.arange(Cn), -1.0 + 0.125 * np.arange(Cn)]).astype(np.float32)

    def _arena(self, values, other):
        """(2 * width doubles with the job's own entries set and `other` elsewhere, which entries are the job's own)."""
        host, own = np.full(2 * self.width, other, dtype=np.float64), np.zeros(2 * self.width, dtype=bool)
        for half in (0, 1):
            lo = half * self.width + self.c0
            host[lo: lo + self.C] = values[half * self.C: (half + 1) * self.C]
            own[lo: lo + self.C] = True
        return host, own

    def upload(self, ops, replicate=0, rng=None):
        """Device buffers and the job tuple of ops.norm_bwd_apply_multi.  replicate = R: statistics and sums are split at random
        over R copies `rep` doubles apart that add up to the plain arrays."""
        H, W, Cn = self.H, self.W, self.C
        self.dy = _SliceGuard(H, W, Cn, self.slice_of, self.c0, self.d)
        self.xg = _SliceGuard(H, W, Cn, self.slice_of, self.c0, self.x)
        (st, own), (sm, _) = self._arena(self.stats, np.nan), self._arena(np.concatenate([self.s1, self.s2]), 1.0)
        rep = 0
        if replicate:
            rep = 2 * self.width
            st, sm = _split(st, own, replicate, rng), _split(sm, own, replicate, rng)
        self.st_dev, self.sm_dev = torch.from_numpy(st).cuda(), torch.from_numpy(sm).cuda()
        self.sm_host = sm
        self.g_dev, self.dg_dev, self.db_dev = _cuda(self.gamma, torch.float32), None, None
        if self.bn:
            self.dg_dev, self.db_dev = _cuda(self.gbase[:Cn], torch.float32), _cuda(self.gbase[Cn:], torch.float32)
        self.nd = ops.norm_desc(self.st_dev[self.c0:], self.g_dev, _cuda(self.beta, torch.float32), H * W, EPS, sq_stride=self.sq, rep_stride=rep)
        return (self.dy.t, self.xg.t, self.nd, self.sm_dev[self.c0:], self.dg_dev, self.db_dev, self.sq, rep)

    def check(self, what=""):
        """The result within the yardstick, nothing outside the job's rows and channels written, inputs left alone."""
        assert self.dy.outside_intact() and self.dy.finite_inside() and self.xg.untouched()
        assert np.array_equal(self.sm_dev.cpu().numpy().view(np.int64), self.sm_host.view(np.int64))
        got = self.dy.numpy()
        R.within_yardstick(got, self.ref32, self.ref64, f"{what}job {self.name} dx")
        return got


class _SliceGuard(Guarded):
    """Guarded with the view at channels [c0, c0 + C) of a `width`-wide buffer (width 0: plain)."""

    def __init__(self, H, W, Cn, width, c0, data, tail=1024):
        ld = width if width else Cn
        self.store = torch.full((H * W * ld + tail,), float("nan"), dtype=torch.float32, device="cuda")
        self.t = self.store[: H * W * ld].view(H, W, ld)[..., c0: c0 + Cn]
        self.t.copy_(torch.as_tensor(data, dtype=torch.float32))
        self.inside = torch.zeros_like(self.store, dtype=torch.bool)
        self.inside.as_strided(self.t.shape, self.t.stride(), self.t.storage_offset()).fill_(True)
        self.snap = self.store.view(torch.int32).clone()


def _split(plain, own, copies, rng):
    """`copies` arrays len(plain) apart whose `own` entries add up to those of `plain` (the others: kept in the first copy, 0 after)."""
    parts = np.zeros((copies, plain.size))
    parts[1:, own] = rng.standard_normal((copies - 1, int(own.sum()))) * np.abs(plain[own])
    parts[0] = plain
    parts[0, own] = plain[own] - parts[1:, own].sum(0)
    return parts.reshape(-1)


def _table(plant=False):
    return [Job("A", 5, 7, 4, False, 11),                                                   # 35 chunks: most of one workgroup idle
            Job("B", 13, 17, 24, True, 12, slice_of=32, c0=4),                              # slice + affine gradients
            Job("C", 40, 40, 8, True, 13, plant=(1500, 1) if plant else None),              # 3200 chunks -> 4 workgroups; chunk 3000 = pixel 1500 belongs to the last
            Job("D", 3, 3, 260, False, 14)]                                                 # coefficient loop runs twice


def test_heterogeneous_table_in_one_launch(ops):
    from supervised_gan_amd import _lib
    jobs = _table()
    tuples = [j.upload(ops) for j in jobs]
    ops.tanh_bwd(*(torch.zeros(4, device="cuda") for _ in range(3)))
    calls = []
    real = ops.L.check
    try:
        ops.L.check = lambda rc, what: (calls.append(what), real(rc, what))[1]
        ops.norm_bwd_apply_multi(tuples)
    finally:
        ops.L.check = real
    torch.cuda.synchronize()
    assert calls == ["sgan_norm_bwd_apply_multi"] and _lib.lib().sgan_last_kernel().decode() == "sg_norm_bwd_apply_kernel"
    for j in jobs:
        j.check()
        assert not hasattr(j.dy.t, "_sgan_amax") or j.dy.t._sgan_amax is None
    for j in jobs:
        if j.bn:      # one fp32 add per channel, exactly once, however many workgroups ran: bit-equal to the host's fp32 add
            Cn = j.C
            want_g = j.gbase[:Cn] + j.s2.astype(np.float32)
            want_b = j.gbase[Cn:] + j.s1.astype(np.float32)
            assert want_g.dtype == np.float32
            assert np.array_equal(j.dg_dev.cpu().numpy(), want_g) and np.array_equal(j.db_dev.cpu().numpy(), want_b), j.name
    assert np.abs(jobs[2].s2.astype(np.float32)).min() > 1e-3      # job C: a second add would show in every channel


def _nine():
    shapes = [(3, 5, 4), (4, 4, 8), (2, 9, 12), (5, 5, 4), (6, 3, 16), (3, 3, 20), (7, 2, 8), (4, 6, 4), (5, 3, 24)]
    return [Job(str(i), H, W, Cn, i % 2 == 1, 100 + i) for i, (H, W, Cn) in enumerate(shapes)]


def test_nine_jobs_make_two_launches(ops):
    jobs = _nine()
    tuples = [j.upload(ops) for j in jobs]
    calls = []
    real = ops.L.check
    try:
        ops.L.check = lambda rc, what: (calls.append(what), real(rc, what))[1]
        ops.norm_bwd_apply_multi(tuples)
    finally:
        ops.L.check = real
    torch.cuda.synchronize()
    assert calls == ["sgan_norm_bwd_apply_multi"] * 2
    for j in jobs:
        j.check("nine: ")


@pytest.mark.parametrize("n", [9, 0])
def test_c_abi_refuses_nine_and_zero_jobs(ops, n):
    from supervised_gan_amd import _lib as L
    jobs = _nine()
    arr = (L.NormBwdJob * 9)()
    for i, j in enumerate(jobs):
        dy, x, nd, sums, dg, db, sq, rep = j.upload(ops)
        arr[i] = L.NormBwdJob(dy.data_ptr(), dy.stride(1), x.data_ptr(), x.stride(1), j.H * j.W, j.C, C.pointer(nd), sums.data_ptr(), sq,
                              dg.data_ptr() if dg is not None else 0, db.data_ptr() if db is not None else 0, rep, 0)
    rc = L.lib().sgan_norm_bwd_apply_multi(arr, n, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc != 0 and b"jobs" in L.lib().sgan_last_error()
    for j in jobs:
        assert j.dy.untouched() and j.xg.untouched()
        if j.bn:
            assert np.array_equal(j.dg_dev.cpu().numpy(), j.gbase[:j.C]) and np.array_equal(j.db_dev.cpu().numpy(), j.gbase[j.C:])


def test_replicated_sums_and_statistics(ops):
    """Sums (sums_rep) and forward statistics (rep_stride) split at random over stat_replicas() copies that add up to the plain
    arrays: within the yardstick, and within 2 ulp of the run on the plain arrays."""
    copies = ops.stat_replicas()
    assert copies >= 2
    rng = np.random.default_rng(77)
    plain_jobs, rep_jobs = [_table()[1], _table()[2]], [_table()[1], _table()[2]]
    ops.norm_bwd_apply_multi([j.upload(ops) for j in plain_jobs])
    ops.norm_bwd_apply_multi([j.upload(ops, replicate=copies, rng=rng) for j in rep_jobs])
    torch.cuda.synchronize()
    for p, r in zip(plain_jobs, rep_jobs):
        a, b = p.check("plain: "), r.check("replicated: ")
        ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
        worst = float((np.abs(a.astype(np.float64) - b) / ulp).max())
        print(f"job {p.name}: replicated vs plain, worst {worst:.2f} ulp")
        assert worst <= 2.0
        for got, base in ((r.dg_dev, r.gbase[:r.C]), (r.db_dev, r.gbase[r.C:])):
            assert np.array_equal(got.cpu().numpy() != base, np.ones(r.C, dtype=bool))      # the affine gradients were added


@pytest.mark.parametrize("math_mode", ["bf16x3", "bf16x1"], indirect=True)
def test_published_maximum(ops, math_mode):
    """max |dy| of jobs A and C, published by one launch: a one-element fp32 view, bit-equal to the maximum of the job's own result.
    Job A (C = 4) is where the four wave maxima fill cA[0..3] exactly; job C's maximum sits at a pixel of the last workgroup."""
    table = _table(plant=True)
    jobs = [table[0], table[2]]
    tuples = [j.upload(ops) for j in jobs]
    with ops.arena_scope(ops.ArenaPool()):      # the slots of the maxima come from a pool of this test's own, not the process-wide one
        ops.norm_bwd_apply_multi(tuples, publish_amax=True)
    torch.cuda.synchronize()
    for j, t in zip(jobs, tuples):
        got = j.check(f"{math_mode} amax: ")
        assert ops.has_amax(t[0])
        am = t[0]._sgan_amax
        assert am.dtype == torch.float32 and am.numel() == 1
        mine = np.abs(got).max()
        assert np.array_equal(am.cpu().numpy().view(np.int32), np.array([mine], dtype=np.float32).view(np.int32)), (j.name, float(am), mine)
        ref_max, yard = float(np.abs(j.ref64).max()), R.deviation(j.ref32, j.ref64)
        print(f"job {j.name}: published max {float(am):.9g}, fp64 {ref_max:.9g}, off by {abs(float(am) - ref_max):.3e} | yardstick {yard:.3e}")
        assert abs(float(am) - ref_max) <= R.YARDSTICK_FACTOR * yard
    at = np.unravel_index(np.abs(jobs[1].ref64).argmax(), jobs[1].ref64.shape)
    assert at[0] * 40 + at[1] == 1500 and at[2] == 1      # the planted element: chunk 3000 of 3200, last workgroup, third chunk of its trip


def test_no_maximum_in_f32_mode(ops):
    prev = ops.get_math()
    ops.set_math("f32")
    try:
        j = _table()[0]
        t = j.upload(ops)
        ops.norm_bwd_apply_multi([t], publish_amax=True)
        torch.cuda.synchronize()
        j.check("f32: ")
        assert not ops.has_amax(t[0])
    finally:
        ops.set_math(prev)


# ---- sgan_norm_apply_bwd_sums ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("Cn", [12, 40, 16, 256])      # 12, 40: generic LDS-atomic path (256 % (C / 4) != 0); 16, 256: register path
def test_norm_apply_bwd_sums(ops, Cn, masked):
    H, W = 15, 11                                        # 165 pixels: the chunk count is no multiple of the grid stride
    rng = np.random.default_rng(1000 + Cn + masked)
    u = (rng.standard_normal((H, W, Cn)) * 1.5 + 0.5).astype(np.float32)
    dt = rng.standard_normal((H, W, Cn)).astype(np.float32)
    m = (rng.integers(0, 2, (H, W, Cn)) * 2).astype(np.float32) if masked else None
    stats = R.stats_of(u)
    base = np.concatenate([3.0 + 0.01 * np.arange(Cn), -2.0 - 0.01 * np.arange(Cn)])
    dg, ug = Guarded(H, W, Cn, True, dt), Guarded(H, W, Cn, False, u)
    st_dev, sums = torch.from_numpy(stats).cuda(), torch.from_numpy(base.copy()).cuda()
    nd = ops.norm_desc(st_dev, None, None, H * W, EPS)
    ops.norm_apply_bwd_sums(dg.t, ug.t, nd, sums, _cuda(m, torch.float32))
    torch.cuda.synchronize()
    assert dg.outside_intact() and ug.untouched()
    d64, s1, s2, a1, a2 = R.norm_apply_bwd_sums(dt, u, stats, H * W, EPS, m)
    d32, t1, t2, _, _ = R.norm_apply_bwd_sums(dt, u, stats, H * W, EPS, m, dtype=np.float32)
    assert np.array_equal(dg.numpy().view(np.int32), d32.view(np.int32))      # dt * mask: one exact product (or dt itself), bit-equal
    got = sums.cpu().numpy()
    n = H * W
    for name, lo, s64, s32, mag in (("s1", 0, s1, t1, a1), ("s2", Cn, s2, t2, a2)):
        g, bs = got[lo: lo + Cn], base[lo: lo + Cn]
        err = np.abs(g - (bs + s64))
        bound = n * U32 * mag + n * 2.0 ** -53 * (np.abs(bs) + mag)
        print(f"C={Cn} {'mask' if masked else 'nomask'} {name}: kernel {float(err.max()):.3e} from fp64 | sequential fp32 restatement "
              f"{float(np.abs(s32 - s64).max()):.3e} | a-priori bound {float(bound.max()):.3e}, worst err/bound {float((err / bound).max()):.4f}")
        assert np.isfinite(g).all() and (err <= bound).all()
        assert float(np.abs(s64).max()) > 4 * float(bound.max())
        assert float(np.abs(g - (bs + 2 * s64)).max()) > float(bound.max()) and float(np.abs(g - s64).max()) > float(bound.max())


def test_norm_apply_fwd_resnet_block_tail(ops):
    """The ResNet block's use: t = residual + BN(c), i.e. noise = residual, sigma = 1, gamma / beta, C = 12, into a slice."""
    H, W, Cn = 9, 7, 12
    rng = np.random.default_rng(21)
    c = (rng.standard_normal((H, W, Cn)) * 1.5 + 0.5).astype(np.float32)
    res = rng.standard_normal((H, W, Cn)).astype(np.float32)
    gamma, beta = rng.uniform(0.5, 1.5, Cn).astype(np.float32), (rng.standard_normal(Cn) * 0.3).astype(np.float32)
    stats = R.stats_of(c)
    cg, tg = Guarded(H, W, Cn, True, c), Guarded(H, W, Cn, True)
    st_dev = torch.from_numpy(stats).cuda()
    nd = ops.norm_desc(st_dev, _cuda(gamma, torch.float32), _cuda(beta, torch.float32), H * W, EPS)
    ops.norm_apply_fwd(cg.t, nd, tg.t, None, _cuda(res, torch.float32), 1.0)
    torch.cuda.synchronize()
    assert tg.outside_intact() and tg.finite_inside() and cg.untouched()
    ref64 = R.norm_apply_fwd(c, stats, gamma, beta, H * W, EPS, noise=res, sigma=1.0)
    ref32 = R.norm_apply_fwd(c, stats, gamma, beta, H * W, EPS, noise=res, sigma=1.0, dtype=np.float32)
    assert ref32.dtype == np.float32
    R.within_yardstick(tg.numpy(), ref32, ref64, "x_res + BN(c)")

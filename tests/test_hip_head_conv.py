"""The three kernels of the one-channel stride-1 head -- sg_conv_head2_kernel<K,R>, sg_conv_head_kernel<TH>, sg_head_bwd_kernel<K> --
against the float64 reference of tests/thin_conv_ref.py, row by row of tests/head_conv_cases.py (pinned on the CPU by
tests/test_head_conv_host.py).

Per row: the kernel's name through sgan_last_kernel() and its variant ("K4 R2 nrg1", "TH4", "K4 tiles9 gy4") through
sgan_last_variant(); every element of the forward result, of dX, dW and dbias within the derived bound of its operation
((L + 1) u M_a + 8 u M_A forward, (L + 4) u M backward-data, (L + 1) u M_a + 11 u M_A backward-weight -- the kernel forms its operand
from xhat --, (L + 3) u M bias gradient, u = 2^-24; tanh 4 u |tanh| on top), reported over the whole tensor and over the outermost two
rows and columns; the two norm-backward sums within bound_sum with the kernel's fp32 runs of 8; padded channels exactly zero;
overwritten outputs start NaN-filled; every operand stands in front of a NaN guard that must be intact afterwards.  SGAN_HEAD2_R,
SGAN_HEAD_TH and SGAN_NO_HEAD2 are set around the row's own launch only.  Every backward row is also run through the generic pair
(conv_wgrad_grouped + conv_dgrad_grouped) and that result held to fp64 as well, and so is what runs after sgan_conv_head_bwd
declined (the tile limit, accumulate, two job lists that read the forward tensor differently).

The old tests (tests/test_hip_ops.py) reached head2 <4,2> and <3,2> at nch 1 / 2 / 4 / 8 with pads 1 and 2, the backward kernel at
C 64 .. 512 on maps of 9 x 9 and more, and sg_conv_head_kernel not at all, against fp32 torch in one norm over the tensor.

Measured on an MI355X (pytest -s prints every row), worst |kernel - fp64| / bound: head2 <4,2> 0.005, <4,4> 0.001, <3,2> 0.008,
<3,4> 0.002; sg_conv_head_kernel <2> 0.004, <4> 0.006, <8> 0.003; sg_head_bwd_kernel<4> dX 0.202, dW 0.132, dbias 0.057, sums 0.050;
<3> dX 0.124, dW 0.108, dbias 0.026, sums 0.043; the generic pair on the same rows dX 0.202, dW 0.170.  No kernel needed a fix.
This file: 56 tests in 3.0 s.

Scratch builds with one value changed each turned these rows red (nothing else): `pok` dropped from the backward-weight operand --
the 13 backward rows with a dW, pad > 0 and W % 16 != 0; head2's zero padding applied before the activation -- the 9 head2 rows with
a norm and pad > 0; rows = RW in the dW accumulation alone -- 14 backward rows (hb_k4p2_c64_1x1 .. hb_rep_sums_c256_17x33_in_lrelu:
those with pad > 0 whose last tile row has a wave below the map); ky / kx swapped in head2's tap
index -- all 17 head2 rows; swapped in the backward kernel -- all 19 backward rows; the job-list comparison removed from
sgan_conv_head_bwd -- hb_norm_mismatch_c64_9x16_lrelu and hb_ld_mismatch_c64_9x16.
"""
import contextlib
import os

import pytest
import torch

import head_conv_cases as HC
import thin_conv_cases as K
import thin_conv_gpu as T
import thin_conv_ref as R
from hip_utils import from_buf, from_master, master_weight, pad_vec, to_buf
from thin_conv_ref import pad4

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import _lib, ops
    _lib.lib()
    yield ops
    print("\nworst ratio to the bound, per kernel: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(T.WORST.items())))


@contextlib.contextmanager
def knobs(env):
    """The row's per-call knobs for the launches inside; all three popped on the way out."""
    for k in HC.KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k in HC.KNOBS:
            os.environ.pop(k, None)


@pytest.mark.parametrize("case", HC.FWD, ids=HC.IDS)
def test_forward(ops, case):
    G = T.Guards()
    jobs, _ = T.build_fwd(ops, case, G)
    with knobs(case.env):
        ops.conv_fwd_grouped(jobs, ops.ACT_TANH if case.tanh else ops.ACT_NONE)
    torch.cuda.synchronize()
    T.launched(case.kernel, case.variant)
    assert (case.kernel in HC.HEAD_KERNELS) == (not case.name.startswith("hk_lds_decline"))
    key = case.kernel + " " + case.variant.split(" nrg")[0]      # per instantiation: "K4 R2", "TH4"
    for i, (job, ref) in enumerate(zip(jobs, HC.fwd_reference(case))):
        ob = job[5]
        T.held(from_buf(ob, 1)[0], ref["ref"], ref["bound"], f"{case.name}[{i}] forward", key)
        assert float(ob[..., 1:].abs().max()) == 0.0, "padded channels must stay exactly zero"
    assert not G.broken(), G.broken()


# ---- backward -------------------------------------------------------------------------------------------------------------------------
class Pass:
    """The two job lists of a row over one set of guarded operands, with fresh outputs."""

    def __init__(self, ops, row, G, shared=None):
        d, L = HC.bwd_data(row), row.layer
        C = pad4(L.cin)
        self.row, self.C = row, C
        if shared is None:
            wm, wt = T.weights(ops, d["w"], False, G)
            gam, bet = (G(pad_vec(d["gamma"])), G(pad_vec(d["beta"]))) if row.norm == "bn" else (None, None)
            shared = dict(w=wt if row.wt else wm, xs=[], dys=[], nd=[], nw=[])
            for p in d["probs"]:
                xb = to_buf(p["x"][None])
                if row.wide:      # x in the first C channels of a 2 C wide pixel; backward-data is told the pixel stride C all the same
                    wide = G(torch.cat([xb, torch.zeros_like(xb)], dim=2))
                    shared["xs"].append((torch.as_strided(wide, xb.shape, (p["W"] * C, C, 1)), wide[..., :C]))
                else:
                    xg = G(xb)
                    shared["xs"].append((xg, xg))
                shared["dys"].append(G(to_buf(p["dy"][None])))
                mk = lambda n: ops.norm_desc(G(R.stats_of(p["x"])) if n else None, gam, bet, p["H"] * p["W"], 1e-5, row.act, R.SLOPE)      # noqa: E731
                nd = mk(row.norm)
                shared["nd"].append(nd)
                shared["nw"].append(nd if row.wnorm == row.norm else mk(row.wnorm))
        self.shared = shared
        n = len(d["probs"])
        zw = torch.zeros(L.wshape())
        self.dws = [G(master_weight(zw, False).clone()) for _ in range(n if row.own_dw else 1)]
        self.dbs = [G(torch.zeros(4)) if row.bias else None for _ in self.dws]
        self.dins, self.sums, self.djobs, self.wjobs = [], [], [], []
        for i, p in enumerate(d["probs"]):
            din = G(to_buf(p["prev"][None])) if row.accum else G(torch.full((p["H"], p["W"], C), NAN))
            arena = G(torch.zeros((8 if row.rep else 1) * 2 * C, dtype=torch.float64)) if row.stats else None
            self.dins.append(din), self.sums.append(arena)
            xd, xw = shared["xs"][i]
            self.djobs.append((T._desc(ops, L, p), shared["dys"][i], shared["w"], din, xd, shared["nd"][i], arena[: 2 * C] if row.stats else None, 0,
                               row.accum, row.wt, 2 * C if row.rep else 0))
            j = i if row.own_dw else 0
            self.wjobs.append((self.djobs[-1][0], xw, shared["nw"][i], shared["dys"][i], self.dws[j], self.dbs[j]))

    def check(self, key, head):
        """head: the result of sg_head_bwd_kernel (its backward-weight bound and fp32 runs), else of the generic kernels."""
        row, C, L = self.row, self.C, self.row.layer
        dg, wg = HC.bwd_reference(row)
        for i, (din, arena, ref) in enumerate(zip(self.dins, self.sums, dg)):
            T.held(from_buf(din, C)[0], ref["ref"], ref["bound"], f"{row.name}[{i}] backward-data", key)
            if arena is not None:
                v, vb, xh, run = ref["own"], ref["own_bound"], ref["xhat"], 8 if head else 1
                T.sums_held(arena.view(-1, 2 * C).sum(0), C, (v.sum((1, 2)), (v * xh).sum((1, 2))),
                            (R.bound_sum(v, vb, run=run), R.bound_sum(v, vb, xh, run=run)), f"{row.name}[{i}] norm-backward", key)
        if not row.wj:
            return
        for j, (dw, db, ref) in enumerate(zip(self.dws, self.dbs, wg)):
            bound = HC.head_dw_bound(row, ref) if head else ref["dw_bound"]
            T.held(from_master(dw, L.k, L.cin, 1, False).double(), ref["dw"], bound, f"{row.name}[{j}] backward-weight", key + " dw")
            m = dw.detach().cpu().view(L.k, L.k, 4, C)
            assert float(m[:, :, 1:].abs().max()) == 0.0, "padded rows of dw must stay exactly zero"
            if db is not None:
                T.held(db.cpu()[:1].double(), ref["db"], ref["db_bound"], f"{row.name}[{j}] bias gradient", key + " dbias")
                assert float(db[1:].abs().max()) == 0.0


def _generic(ops, row, G, first):
    """The generic pair on fresh outputs over the same operands, held to the same reference."""
    P = Pass(ops, row, G, shared=first.shared)
    if row.wj:
        ops.conv_wgrad_grouped(P.wjobs)
        assert T.last_kernel() != HC.HB
    ops.conv_dgrad_grouped(P.djobs)
    torch.cuda.synchronize()
    assert T.last_kernel() != HC.HB
    P.check("generic pair", head=False)


@pytest.mark.parametrize("row", HC.BWD, ids=HC.IDS)
def test_backward_one_launch(ops, row):
    from supervised_gan_amd import _lib
    G = T.Guards()
    P = Pass(ops, row, G)
    if row.wj:
        assert ops.conv_bwd_grouped(P.djobs, P.wjobs) is True
    else:
        assert _lib.lib().sgan_conv_head_bwd(ops._dgrad_array(P.djobs), None, len(P.djobs), ops._stream()) == 0
    torch.cuda.synchronize()
    T.launched(HC.HB, row.variant)
    P.check(f"{HC.HB}<{row.layer.k}>", head=True)
    if row.rep:      # 9 tiles over 8 copies: more than one copy took part
        used = (P.sums[0].view(8, -1).abs().sum(1) > 0).sum()
        assert int(used) == 8, int(used)
    _generic(ops, row, G, P)
    assert not G.broken(), G.broken()


@pytest.mark.parametrize("row", HC.DECLINED, ids=HC.IDS)
def test_backward_declined(ops, row):
    """sgan_conv_head_bwd answers 1 (nothing written), conv_bwd_grouped then runs other kernels, and their result is held to fp64."""
    from supervised_gan_amd import _lib
    G = T.Guards()
    P = Pass(ops, row, G)
    before = [t.clone() for t in P.dins + P.dws]
    assert _lib.lib().sgan_conv_head_bwd(ops._dgrad_array(P.djobs), ops._wgrad_array(P.wjobs), len(P.djobs), ops._stream()) == 1
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(before, P.dins + P.dws)), "a declined call must write nothing"
    ops.conv_bwd_grouped(P.djobs, P.wjobs)
    torch.cuda.synchronize()
    assert T.last_kernel() != HC.HB
    P.check("after a decline", head=False)
    assert not G.broken(), G.broken()


def test_grouped_jobs_must_share_the_activation(ops):
    from supervised_gan_amd import _lib
    G = T.Guards()
    row = next(r for r in HC.BWD if r.name == "hb_k4p2_c200_8x15_lrelu")
    a, b = Pass(ops, row, G), Pass(ops, row, G)
    relu = ops.norm_desc(None, None, None, 8 * 15, 1e-5, 1, 0.0)      # the same problem once more, read through a ReLU
    dj = [a.djobs[0], b.djobs[0][:5] + (relu,) + b.djobs[0][6:]]
    rc = _lib.lib().sgan_conv_head_bwd(ops._dgrad_array(dj), None, 2, ops._stream())
    assert rc < 0 and b"share the activation" in _lib.lib().sgan_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(a.dins[0]).all())

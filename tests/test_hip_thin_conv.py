"""Forward and backward-data of the layers with a 4-stored-channel side -- sg_conv_scatter4_kernel, sg_conv_c4_kernel (plain and full
epilogue, two and four row blocks per wave) and the three forms of sg_conv_small_n_kernel -- against the float64 reference of
tests/thin_conv_ref.py (pinned on the CPU by tests/test_thin_conv_ref_host.py), row by row of tests/thin_conv_cases.py.

Per row: the kernel's name through sgan_last_kernel() and its variant (NB / RB / epilogue / grid.y, NR and weight layout) through
sgan_last_variant(); every element of every output within the derived bound of thin_conv_ref
((L + 1) u M_a + 8 u M_A forward, (L + 4) u M backward-data, u = 2^-24; tanh 4 u |tanh| on top), reported over the whole output and
over the outermost two rows and columns; padded channels exactly zero; overwritten outputs start NaN-filled; every operand stands in
front of a NaN guard that must be intact afterwards; result statistics and the two norm-backward sums within the summed bounds;
an accumulating launch equals, bit for bit, the plain launch plus the previous content.

The old tests (tests/test_hip_ops.py) reached scatter4 at Ck 16 and 32 (16 x 16, 21 x 23, the pair's shapes), c4 plain at N 32 and
64 (NB 2 and 4, RB 2), the c4 epilogue at N 32 and 256 (RB 2), small_n <64> (k7, 64 -> 2) and <8>, all against fp32 torch in one norm
over the tensor.  Only the rows here reach NB 3, RB 4, accumulate in the c4 epilogue, small_n <16>, Ck 48 / 512 and the phase extents
1, 2, 6, 7, 30, 31, 61 of scatter4, and its multi-problem tile decode against a reference.

Measured on an MI355X (pytest -s prints every row), worst |kernel - fp64| / bound: scatter4 0.067, c4 plain 0.085 (RB 4: 0.072),
c4 epilogue 0.074 (its sums 0.005), small_n <8> 0.086, <16> 0.001, <64> under 0.0005 -- the a-priori bound grows with L, the kernels'
trees err like sqrt(L) or less.  No kernel needed a fix.  This file and tests/test_hip_thin_wgrad.py together: 48 tests in 3.2 s.
"""
import pytest
import torch

import thin_conv_cases as K
import thin_conv_gpu as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import _lib, ops
    _lib.lib()
    yield ops
    print("\nworst ratio to the bound, per kernel: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(T.WORST.items())))


@pytest.mark.parametrize("case", K.FWD, ids=K.IDS)
def test_forward(ops, case):
    G = T.Guards()
    jobs, check = T.build_fwd(ops, case, G)
    ops.conv_fwd_grouped(jobs, ops.ACT_TANH if case.tanh else ops.ACT_NONE)
    torch.cuda.synchronize()
    T.launched(case.kernel, case.variant)
    check()
    assert not G.broken(), G.broken()


@pytest.mark.parametrize("case", K.DGRAD, ids=K.IDS)
def test_backward_data(ops, case):
    G = T.Guards()
    jobs, check, outs = T.build_dgrad(ops, case, G)
    ops.conv_dgrad_grouped(jobs)
    torch.cuda.synchronize()
    T.launched(case.kernel, case.variant)
    check()
    if case.accum:      # accumulate is exact in its own term: the plain launch's value plus what was there, one fp32 addition
        jobs0, check0, outs0 = T.build_dgrad(ops, case, G, accum=False)
        ops.conv_dgrad_grouped(jobs0)
        torch.cuda.synchronize()
        # (without a forward tensor or sums, dropping accumulate leaves nothing for the full epilogue: the plain instantiation)
        T.launched(case.kernel, case.variant if (case.x or case.stats) else case.variant.split(" EPI")[0])
        check0()
        for (din, _), (din0, _), p in zip(outs, outs0, K.data(case)["probs"]):
            assert torch.equal(din, din0 + T.to_buf(p["prev"][None]))
    assert not G.broken(), G.broken()

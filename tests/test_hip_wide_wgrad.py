"""Backward-weight of the exact-fp32 MFMA kernel, sg_wgrad_kernel in its three shapes (<16,128,1,4> for Cout <= 16, <32,64,1,4> for
Cout <= 32, <64,64,2,2> beyond), with and without the normalise-on-load prologue, against the float64 reference of
tests/thin_conv_ref.py, row by row of tests/wide_conv_cases.py.

Per row: operands in NaN-guarded storage; one launch; the kernel's name and "PRO<0|1> per<chunks> nsplit a,b,.." through
sgan_last_variant() (the restated planner: tests/test_wide_conv_host.py); every element of dw within (L + 1) u M_a + 8 u M_A
(L = pixels summed over every problem, u = 2^-24) and of the bias gradient within (L + 3) u M; padded rows and columns of dw exactly
zero; guards intact.  The rows cover Cout 8, 12 (10 logical), 20 and 72 (a ragged second row tile), K = taps x Cin that is no
multiple of the column tile, pixel counts that are no multiple of the 32-pixel chunk, a ConvT (four phases), IN + LeakyReLU,
BN + ReLU and a bare LeakyReLU prologue, the bias gradient, a pre-filled dw / dbias, and three problems into one dw whose pixel ranges
are cut 13, 4 and 1 times.

The bound holds for any order of summation, so it covers the MFMA's internal order, the chunk loop, and the fp32 atomics that
combine splits, phases and problems in the gradient buffer (whose previous content is one more term, its magnitude in both sums).
The prologue is the forward kernel's (see tests/test_hip_wide_conv.py); the bias gradient sums each thread's rows, then the
workgroup's threads, then one atomic: L terms and the previous value, L additions, 2 for the second order.

Measured on an MI355X (profiles/r19_wide_conv_ratios.json -- records, not thresholds), worst |kernel - fp64| / bound: dw 0.063
(<16,128>), 0.059 (<32,64>), 0.041 (<64,64>), bias gradient 0.012.  No kernel needed a fix.
"""
import pytest
import torch

import thin_conv_gpu as T
import wide_conv_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import _lib, ops
    _lib.lib()
    yield ops
    print("\nworst ratio to the bound, per kernel: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(T.WORST.items())))


@pytest.mark.parametrize("case", W.WGRAD, ids=W.IDS)
def test_backward_weight(ops, case):
    G = T.Guards()
    jobs, check = T.build_wgrad(ops, case, G)
    with ops.math_scope(case.math):
        ops.conv_wgrad_grouped(jobs)
    torch.cuda.synchronize()
    T.launched(case.kernel, case.variant)
    check()
    assert not G.broken(), G.broken()

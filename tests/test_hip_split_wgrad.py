"""Backward-weight of the split 16-bit-plane mode -- sg_wgrad3_kernel<64,64,2,2> (Cout 64, 72) and <32,128,1,4> (Cout 32, 40, 56),
with and without the normalise-on-load prologue, on bf16 planes and (published max|dY|) fp16 planes, three planes and one, pixel
splits 13,4,2 in one launch, the bias gradient, a prefilled dw / dbias -- against the float64 plane model, row by row of
tests/split_conv_cases.WGRAD (whose docstring derives the bounds and says why no row of this size has a dw element with one owner).
Per row: guarded storage, one launch, kernel and "PRO<0|1> F16<0|1> per<c> nsplit a,b,.." asserted, every element of dw and dbias
within its bound, G3, guards intact."""
import pytest
import torch

import split_conv_cases as S
import split_conv_gpu as SG
import thin_conv_gpu as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import _lib, ops
    _lib.lib()
    prev = ops.get_math()
    yield ops
    ops.set_math(prev)
    SG.clear_knobs()
    print("\nworst ratio to the bound, per kernel: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(T.WORST.items())))


@pytest.mark.parametrize("case", S.WGRAD, ids=S.IDS)
def test_backward_weight(ops, case):
    G = T.Guards()
    jobs, check, _ = SG.build_wgrad(ops, case, G)
    with SG.knobs(case), ops.math_scope(case.math):
        ops.conv_wgrad_grouped(jobs)
    torch.cuda.synchronize()
    T.launched(case.kernel, case.variant)
    check(case.kernel)
    assert not G.broken(), G.broken()

"""Backward-weight of the layers with a 4-stored-channel side (the five instantiations of sg_wgrad_thin_kernel, with and without
prologue) and sg_bwd_thin_pair_kernel, against the float64 reference of tests/thin_conv_ref.py, row by row of
tests/thin_conv_cases.py.  The pair is compared with the REFERENCE, not with the two grouped calls that run the same bodies.

Per row: the kernel's name and, through sgan_last_variant(), the pixel split of every problem (for the pair: which backward-data
body, its RB, the split); every element of dw and of the bias gradient within (L + 1) u M_a + 8 u M_A (L = pixels summed,
u = 2^-24; bias gradient (L + 3) u M), padded rows and columns of dw exactly zero; two or three problems into one dw; a pre-filled dw / dbias (its
magnitude joins both sums); every operand in front of an intact NaN guard.  SGAN_THIN_MINPIX / SGAN_THIN_WANT (read per call) cut 399
pixels into three workgroups whose waves include an empty one and one that ends mid-step (thin_conv_cases.thin_ranges, pinned by the
host test); the default min_pix = 256 leaves every small shape in one workgroup.  For the pair conv_bwd_grouped must return True
and name sg_bwd_thin_pair_kernel; the documented refusals (Cout > 32 beside cin4, Cin > 32 beside cout4, job lists that do not
match) return False and the two grouped launches are held to the same bounds.

The old tests reached <1,cin4>, <2,cin4>, <4,cin4>, <2,cout4> and <4,cout4> once each at nsplit = 1 against fp32 torch in one norm
(test_conv_layer_fwd_bwd), and the pair only against the grouped calls.  Only the rows here reach nsplit > 1 with its wave seams, the
cout4 bias gradient past its first 512 pixels per element, three logical thin channels, and the pair against a reference.

Measured on an MI355X, worst |kernel - fp64| / bound: dw 0.042 (split rows 0.002), bias gradient 0.012; the pair 0.075 for dX
(RB 4), 0.015 for dW; the refusals' grouped launches 0.049 / 0.013.  No kernel needed a fix.
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


@pytest.mark.parametrize("case", K.WGRAD, ids=K.IDS)
def test_backward_weight(ops, case, monkeypatch):
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    G = T.Guards()
    jobs, check = T.build_wgrad(ops, case, G)
    ops.conv_wgrad_grouped(jobs)
    torch.cuda.synchronize()
    T.launched(case.kernel, case.variant)
    check()
    assert not G.broken(), G.broken()


@pytest.mark.parametrize("row", K.PAIRS, ids=lambda r: r[0])
def test_pair(ops, row):
    name, dcase, wcase, launched, kernel, variant = row
    G = T.Guards()
    dj, dcheck, _ = T.build_dgrad(ops, dcase, G)
    wj, wcheck = T.build_wgrad(ops, wcase, G)
    if not launched and len(dj) == len(wj):      # the C entry point itself answers 1: not such a pair
        from supervised_gan_amd import _lib
        assert _lib.lib().sgan_conv_bwd_thin_pair(ops._dgrad_array(dj), len(dj), ops._wgrad_array(wj), len(wj), ops._stream()) == 1
    assert ops.conv_bwd_grouped(dj, wj) is launched
    torch.cuda.synchronize()
    T.launched(kernel, variant)
    dcheck()
    wcheck()
    if not launched:      # the fallback launched backward-weight first: the same jobs on their own, to see where they go
        wj2, wcheck2 = T.build_wgrad(ops, wcase, G)
        ops.conv_wgrad_grouped(wj2)
        torch.cuda.synchronize()
        T.launched(wcase.kernel, wcase.variant)
        wcheck2()
    assert not G.broken(), G.broken()

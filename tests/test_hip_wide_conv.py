"""Forward and backward-data of the exact-fp32 MFMA conv kernels -- sg_igemm_kernel in its five tile shapes (<128,16>, <128,32>,
<128,32,false>, <64,32>, <64,64>; k-contiguous and n-contiguous weights, with and without the normalise-on-load prologue, one and two
wave groups, split-K) and sg_splitk_epilogue_kernel -- against the float64 reference of tests/thin_conv_ref.py, row by row of
tests/wide_conv_cases.py.  These kernels serve, in the default bf16x3 mode, every layer the 16-bit kernels decline (gathered channels
below 16 or no multiple of 8, results under 16 channels, maps under 256 pixels: the FALLBACK rows assert that), and they are the
"fp32 kernel" the bf16x3 tests compare with.

Per row: operands and outputs in NaN-guarded storage, outputs NaN-filled; one launch; the kernel's name through sgan_last_kernel()
and "ks<k> KW<1|2> PRO<0|1>" through sgan_last_variant() (tests/test_wide_conv_host.py holds the same strings to a restatement of the
planners); every element within its derived bound, reported over the whole output and over its outermost two rows / columns; padded
channels exactly zero; result statistics / the two norm-backward sums within the summed bounds; guards intact; an accumulating launch
equals, bit for bit, the plain launch plus the previous content; a planned split that finds no workspace runs unsplit, says so, and
is held to the same bounds.

The bound is thin_conv_ref's (L + c_a) u M_a + c_A u M_A, u = 2^-24, valid for ANY order of summation -- so it covers the MFMA's
internal order, the split-K slabs, the LDS hand-off of the second wave group and (backward-weight) the fp32 atomics alike.  Checked
against the code, the constants of the 4-channel-side kernels carry over unchanged:
  * sg_igemm_body's prologue is sc = gamma rstd, sh = beta - mean sc, y = x sc + sh, max(ok y, ok neg y) with ok in {0, 1} (exact):
    the fp32 expressions plane_model._prologue restates, contraction allowed for by c_A = 6 (+ 2 second order);
  * forward: L products and the bias are L + 1 terms of one sum: (L + 1) u M_a.  Unsplit the bias joins last, in
    sg_splitk_epilogue_kernel first (v = bias; v += (t0 + t1) + (t2 + t3); ...): another order of the same L + 1 terms, so c_a = 1
    either way, and the slabs add no term (an empty trailing split writes zeros, x + 0 is exact);
  * backward-data: v = acc (+ 0 bias, exact), v *= act'(y) (1 rounding), v += previous (accumulate: 1 rounding, |previous| joins M),
    second order 2: (L + 4) u M in the kernel's epilogue and in the split-K epilogue; xhat = (x - mean) rstd, y = gamma xhat + beta
    are thin_conv_ref.act_grad's expressions in both;
  * tanhf: 4 u |tanh| on top; statistics are fp64 sums of the fp32 values before tanh (bound_sum / bound_sumsq).

Measured on an MI355X (pytest -s prints every row; profiles/r19_wide_conv_ratios.json keeps them -- records, not thresholds), worst
|kernel - fp64| / bound: <128,16> 0.025, <128,32> 0.040 (n-contiguous weights 0.053), <64,32> 0.055, <64,64> 0.002, through the
split-K epilogue 0.016, every statistic and norm sum at most 0.001 -- the a-priori bound grows like L^2 u, the MFMA chains err like
sqrt(L) u or less, hence the small ratios of the deep rows.  No kernel needed a fix.  This file and tests/test_hip_wide_wgrad.py
together: 30 tests in 2.8 s.
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


def key(case, variant=None):
    """Worst ratios are filed per kernel, the launches that end in sg_splitk_epilogue_kernel on their own."""
    return case.kernel + (" + sg_splitk_epilogue_kernel" if not (variant or case.variant).startswith("ks1 ") else "")


@pytest.mark.parametrize("case", W.FWD + W.FALLBACK, ids=W.IDS)
def test_forward(ops, case):
    G = T.Guards()
    jobs, check = T.build_fwd(ops, case, G, key(case))
    with ops.math_scope(case.math):
        ops.conv_fwd_grouped(jobs, ops.ACT_TANH if case.tanh else ops.ACT_NONE)
    torch.cuda.synchronize()
    T.launched(case.kernel, case.variant)
    check()
    assert not G.broken(), G.broken()


@pytest.mark.parametrize("case", W.DGRAD, ids=W.IDS)
def test_backward_data(ops, case):
    G = T.Guards()
    jobs, check, outs = T.build_dgrad(ops, case, G, key=key(case))
    with ops.math_scope(case.math):
        ops.conv_dgrad_grouped(jobs)
    torch.cuda.synchronize()
    T.launched(case.kernel, case.variant)
    check()
    if case.accum:      # accumulate is exact in its own term: the plain launch's value plus what was there, one fp32 addition
        jobs0, check0, outs0 = T.build_dgrad(ops, case, G, accum=False, key=key(case))
        with ops.math_scope(case.math):
            ops.conv_dgrad_grouped(jobs0)
        torch.cuda.synchronize()
        T.launched(case.kernel, case.variant)
        check0()
        for (din, _), (din0, _), p in zip(outs, outs0, T.K.data(case)["probs"]):
            assert torch.equal(din, din0 + T.to_buf(p["prev"][None]))
    assert not G.broken(), G.broken()


NOSLAB = {"f_128x32_split8": "ks1 KW1 PRO0 noslab", "f_64x64_split16_kw1": "ks1 KW2 PRO1 noslab"}      # (64 k-tiles in one workgroup: two wave groups)


@pytest.mark.parametrize("case", [c for c in W.FWD if c.name in NOSLAB], ids=W.IDS)
def test_split_without_workspace_runs_unsplit(ops, case, monkeypatch):
    """sg_launch_igemm with a split planned and no slab to put it in: the same tile unsplit, " noslab" in the variant."""
    monkeypatch.setattr(ops, "_workspace", lambda kib, device: None)
    G = T.Guards()
    jobs, check = T.build_fwd(ops, case, G, key(case, NOSLAB[case.name]))
    with ops.math_scope(case.math):
        ops.conv_fwd_grouped(jobs, ops.ACT_TANH if case.tanh else ops.ACT_NONE)
    torch.cuda.synchronize()
    T.launched(case.kernel, NOSLAB[case.name])
    check()
    assert not G.broken(), G.broken()

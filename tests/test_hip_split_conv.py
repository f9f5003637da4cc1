"""Forward and backward-data of the split 16-bit-plane conv kernels -- sg_igemm3_kernel in its four tile shapes (<128,32,4,1>,
<64,64,2,2>, <128,64,2,2>, <128,128,2,4>; prologue or none, fp16 or bf16 planes, three planes or one, split-K into a workspace and
sg_splitk_epilogue_kernel behind it) and sg_igemm3p_kernel in its three patch forms (AIT 2 / 4 / 6, one or two wave groups) --
against the float64 plane model, row by row of tests/split_conv_cases.py (whose docstring derives the bounds).

Per row: operands and outputs in NaN-guarded storage, outputs NaN-filled; the row's two per-call knobs set for its one launch; the
kernel's name through sgan_last_kernel() and its variant through sgan_last_variant() (tests/test_split_conv_host.py holds the same
strings to a restatement of the planners); every element within its bound; G3 (the documented distance from fp64); padded channels
exactly zero; result statistics / the two norm-backward sums within the summed bounds; guards intact; an accumulating launch equals,
bit for bit, the plain launch plus the previous content; a planned split without a workspace runs unsplit and says " noslab".
pytest -s prints every ratio; profiles/r22_split_conv_ratios.json keeps one run's -- records, not thresholds."""
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


def key(case, variant=None):
    v = variant or case.variant
    return case.kernel + (" + sg_splitk_epilogue_kernel" if v.startswith("ks") and not v.startswith("ks1 ") else "")


@pytest.mark.parametrize("case", S.FWD, ids=S.IDS)
def test_forward(ops, case):
    G = T.Guards()
    jobs, check = SG.build_fwd(ops, case, G)
    with SG.knobs(case), ops.math_scope(case.math):
        ops.conv_fwd_grouped(jobs)
    torch.cuda.synchronize()
    T.launched(case.kernel, case.variant)
    check(key(case))
    assert not G.broken(), G.broken()


@pytest.mark.parametrize("case", S.DGRAD, ids=S.IDS)
def test_backward_data(ops, case):
    G = T.Guards()
    jobs, check, outs = SG.build_dgrad(ops, case, G)
    with SG.knobs(case), ops.math_scope(case.math):
        ops.conv_dgrad_grouped(jobs)
    torch.cuda.synchronize()
    T.launched(case.kernel, case.variant)
    check(key(case))
    if case.accum:      # accumulate is exact in its own term: the plain launch's value plus what was there, one fp32 addition
        jobs0, check0, outs0 = SG.build_dgrad(ops, case, G, accum=False)
        with SG.knobs(case), ops.math_scope(case.math):
            ops.conv_dgrad_grouped(jobs0)
        torch.cuda.synchronize()
        T.launched(case.kernel, case.variant)
        check0(key(case))
        for (din, _), (din0, _), p in zip(outs, outs0, T.K.data(case)["probs"]):
            assert torch.equal(din, din0 + T.to_buf(p["prev"][None]))
    assert not G.broken(), G.broken()


NOSLAB = {"f_64x64_split8": "ks1 PRO1 F161 noslab", "f_convT_k3_short_phases_split4": "ks1 PRO0 F161 noslab"}


@pytest.mark.parametrize("case", [c for c in S.FWD if c.name in NOSLAB], ids=S.IDS)
def test_split_without_workspace_runs_unsplit(ops, case, monkeypatch):
    """sg3_launch with a split planned and no slab to put it in: the same tile unsplit, " noslab" in the variant."""
    assert S.igemm3_plan(case, workspace=False) == (case.kernel, NOSLAB[case.name])
    monkeypatch.setattr(ops, "_workspace", lambda kib, device: None)
    G = T.Guards()
    jobs, check = SG.build_fwd(ops, case, G)
    with SG.knobs(case), ops.math_scope(case.math):
        ops.conv_fwd_grouped(jobs)
    torch.cuda.synchronize()
    T.launched(case.kernel, NOSLAB[case.name])
    check(key(case, NOSLAB[case.name]))
    assert not G.broken(), G.broken()

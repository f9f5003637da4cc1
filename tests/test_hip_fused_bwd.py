"""sg_bwd_fused_kernel -- one grid for a layer's backward-data and backward-weight -- against the float64 plane model of each half,
pair by pair of tests/split_conv_cases.PAIRS: all ten DV x WV bodies, DV 3 with its K split through the workspace (and the
SGAN_FUSE_KS_WGS cap moving it), DV 6 on fp16 planes, a published maximum on another plan (re-planned on bf16 planes: the result
meets the bf16-plane model and is farther than the bound from the fp16-plane model), the backward-weight prologue, one plane in both
halves and in the backward-weight half alone, and the refusals, which answer 1 and leave every output as it was.

The C entry sgan_conv_bwd_fused_ws is called directly (ops.conv_bwd_grouped would run the two grouped launches after a refusal).
Every fused row asserts sgan_last_kernel() and "DV<n> WV<n> ks<k> F16<0|1> WPRO<0|1> nsplit a,b,.." from sgan_last_variant(), holds
both halves to their per-element bounds and G3, and is then compared with the two grouped launches on fresh outputs at the gates of
tests/test_hip_bf16x3.py (backward-data equal or within 4e-6, sums 4e-6, dw / dbias 2e-6).  Where the fused launch was re-planned on
bf16 planes the grouped backward-data launch gets the gradient without its maximum, so that both form the same planes."""
import ctypes as C

import pytest
import torch

import split_conv_cases as S
import split_conv_gpu as SG
import thin_conv_gpu as T
from hip_utils import from_buf, rel

pytestmark = pytest.mark.gpu
SENTINEL = 7.5


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


def fused(ops, d, w, djobs, wjobs, workspace=True):
    """-> (return code, KiB of workspace the pair asked for)"""
    from supervised_gan_amd import _lib
    lib = _lib.lib()
    with SG.knobs(d), ops.math_scope(w.mode):
        da, wa, dm = ops._dgrad_array(djobs), ops._wgrad_array(wjobs), ops._MATH_NAMES[d.mode]
        kib = lib.sgan_conv_bwd_fused_ws(da, len(djobs), wa, len(wjobs), dm, None, -1, None)
        ws = torch.empty(kib * 256, dtype=torch.float32, device="cuda") if (kib > 0 and workspace) else None
        rc = lib.sgan_conv_bwd_fused_ws(da, len(djobs), wa, len(wjobs), dm, C.c_void_p(ws.data_ptr() if ws is not None else 0),
                                        ws.numel() * 4 if ws is not None else 0, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, kib


LAUNCHED = [p for p in S.PAIRS if p[3] is not None]
REFUSED = [p for p in S.PAIRS if p[3] is None]


@pytest.mark.parametrize("pair", LAUNCHED, ids=lambda p: p[0])
def test_fused_pair(ops, pair):
    name, d, w, variant, kernel, ws = pair
    f16 = " F161 " in variant                      # the planes the backward-data half was actually formed from
    G = T.Guards()
    djobs, dcheck, douts = SG.build_dgrad(ops, d, G)
    wjobs, wcheck, (dw, db) = SG.build_wgrad(ops, w, G)
    rc, kib = fused(ops, d, w, djobs, wjobs)
    assert rc == 0, rc
    T.launched(kernel, variant)
    assert (kib > 0) == (" ks1 " not in variant)
    limit = "row" if f16 == d.planes else (1e-3 if d.mode == "bf16x3" else None)
    dcheck(f"{kernel} DV{variant[2]}", f16=f16, limit=limit)
    wcheck(f"{kernel} WV{variant[6]}")
    if d.planes and not f16:      # the re-plan: what ran is NOT the fp16-plane product the published maximum asked for
        for (din, _), ref in zip(douts, S.reference(d, True)):
            far = ((from_buf(din, d.layer.cin)[0].double() - ref["own"]).abs() / ref["own_bound"]).max()
            print(f"{name}: {float(far):.1f} bounds from the fp16-plane model")
            assert float(far) > 1.0
    # ---- the two grouped launches, as today ----
    djobs0, _, douts0 = SG.build_dgrad(ops, d, G, planes=f16)
    wjobs0, _, (dw0, db0) = SG.build_wgrad(ops, w, G)
    with SG.knobs(w), ops.math_scope(w.mode):
        ops.conv_wgrad_grouped(wjobs0)
    with SG.knobs(d), ops.math_scope(d.mode):
        ops.conv_dgrad_grouped(djobs0)
    torch.cuda.synchronize()
    for (df, sf), (da, sa) in zip(douts, douts0):
        assert torch.equal(da, df) or rel(df, da) < 4e-6
        if sa is not None:
            assert rel(sf, sa) < (1e-12 if torch.equal(da, df) else 4e-6)
    assert rel(dw, dw0) < 2e-6 and rel(db, db0) < 2e-6
    assert not G.broken(), G.broken()


@pytest.mark.parametrize("pair", REFUSED, ids=lambda p: p[0])
def test_refusals_answer_1_and_write_nothing(ops, pair):
    name, d, w, variant, kernel, ws = pair
    assert S.fused_plan(d, w, ws) is None
    G = T.Guards()
    djobs, _, douts = SG.build_dgrad(ops, d, G, sentinel=SENTINEL)
    wjobs, _, (dw, db) = SG.build_wgrad(ops, w, G, sentinel=SENTINEL)
    outs = [t for pair_ in douts for t in pair_ if t is not None] + [dw, db]
    before = [t.clone() for t in outs]
    assert all(bool((t == SENTINEL).any()) for t in outs)
    rc, kib = fused(ops, d, w, djobs, wjobs, workspace=ws)
    assert rc == 1, rc
    assert ws or kib > 0      # the workspace refusal: the pair did ask for one
    assert all(torch.equal(t, b) for t, b in zip(outs, before)), "a refused pair must leave every output buffer as it was"
    assert not G.broken(), G.broken()

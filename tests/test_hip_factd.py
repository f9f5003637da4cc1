"""sgan_factd_loss_multi_fwd / _bwd against the composition they replace: sigmoid -> F.interpolate(bilinear, align_corners=False) ->
F.pad(reflect, (l, r, t, b)) -> product -> F.binary_cross_entropy / F.mse_loss -> backward(), in float64 on the CPU, fed the same fp32
logits.  Pass rule for each / total / dl1 / dl2 (the parity gate of test_oracle_golden.py): max|a - b| / (max|b| + 1e-12) <=
max(1e-3, 4 e_ref), e_ref the same statistic of the fp32 composition on the CPU against the fp64 one.  Both errors are printed."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from hip_utils import rel

pytestmark = pytest.mark.gpu

# (h1, w1, up, H2, W2)
SHAPES = [(3, 5, 2, 9, 13),        # odd difference on both axes: top 2 / bottom 1, left 1 / right 2
          (4, 4, 2, 15, 15),       # pads 3 / 4 on a size-8 map: one source row is hit by the interior and by both reflections
          (7, 7, 1, 7, 7),         # pure product
          (5, 6, 1, 8, 9),         # pad without upsampling
          (4, 6, 2, 8, 12),        # upsampling without pad
          (11, 11, 2, 35, 35),     # the golden's nested pairs
          (7, 7, 2, 19, 19),
          (19, 19, 2, 67, 67)]     # 512^2: 4-layer D1 on the 256^2 label, 3-layer D2
MODES = [(1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1)]      # (sig1, sig2, mse)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def logits(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 1, *shape, generator=g) * 1.5


def composition(l1s, l2s, ups, targets, weights, mode, dtype, upstream=1.0):
    """(each, total, [dl1], [dl2]) of the torch composition on the CPU in `dtype`."""
    from supervised_gan_amd.losses import factd_pad_split
    sig1, sig2, mse = mode
    a = [t.detach().to(dtype).requires_grad_(True) for t in l1s]
    b = [t.detach().to(dtype).requires_grad_(True) for t in l2s]
    each = []
    for x, y, up, tg in zip(a, b, ups, targets):
        p1 = torch.sigmoid(x) if sig1 else x
        p2 = torch.sigmoid(y) if sig2 else y
        if up == 2:
            p1 = F.interpolate(p1, scale_factor=2, mode="bilinear", align_corners=False)
        pads = factd_pad_split(p2.shape[2] - p1.shape[2], p2.shape[3] - p1.shape[3])
        pred = (F.pad(p1, pads, mode="reflect") if any(pads) else p1) * p2
        t = torch.full_like(pred, tg)
        each.append(F.mse_loss(pred, t) if mse else F.binary_cross_entropy(pred, t))
    total = sum(e * w for e, w in zip(each, weights))
    (total * upstream).backward()
    return torch.stack([e.detach() for e in each]), total.detach(), [x.grad for x in a], [y.grad for y in b]


def buf(t, ld, dev):
    """[1, 1, H, W] -> [H, W, ld] device buffer whose padding channels hold garbage the kernel must not read."""
    out = torch.full((t.shape[2], t.shape[3], ld), 7.0)
    out[..., 0] = t[0, 0]
    return out.to(dev)


def run_kernel(dev, l1s, l2s, ups, targets, weights, mode, ld=1, want=(True, True)):
    from supervised_gan_amd import ops
    b1, b2 = [buf(t, ld, dev) for t in l1s], [buf(t, ld, dev) for t in l2s]
    d1 = [torch.full_like(x, float("nan")) for x in b1] if want[0] else None
    d2 = [torch.full_like(x, float("nan")) for x in b2] if want[1] else None
    each = torch.full((len(l1s),), float("nan"), device=dev)
    total = torch.full((), float("nan"), device=dev)
    ok = ops.factd_loss_multi_fwd(b1, b2, ups, targets, weights, ops.factd_mode(*mode), each, total, d1, d2)
    assert ok
    torch.cuda.synchronize()
    return each.cpu(), total.cpu(), d1, d2


def check(name, got, ref64, ref32):
    e, e_ref = rel(got, ref64), rel(ref32, ref64)
    print(f"{name}: kernel vs fp64 {e:.3e}, fp32 composition vs fp64 {e_ref:.3e}")
    assert e <= max(1e-3, 4 * e_ref), (name, e, e_ref)


def check_all(got, l1s, l2s, ups, targets, weights, mode, upstream=1.0):
    r64 = composition(l1s, l2s, ups, targets, weights, mode, torch.float64, upstream)
    r32 = composition(l1s, l2s, ups, targets, weights, mode, torch.float32, upstream)
    check("each", got[0], r64[0], r32[0])
    check("total", got[1], r64[1], r32[1])
    for i in range(len(l1s)):
        if got[2] is not None:
            check(f"dl1[{i}]", got[2][i][..., 0], r64[2][i][0, 0], r32[2][i][0, 0])
        if got[3] is not None:
            check(f"dl2[{i}]", got[3][i][..., 0], r64[3][i][0, 0], r32[3][i][0, 0])


@pytest.mark.parametrize("mode", MODES, ids=["sig_sig_bce", "raw_raw_mse", "sig_raw_mse", "raw_sig_mse"])
@pytest.mark.parametrize("target", [0.0, 1.0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_up%d_%dx%d" % s)
def test_one_term(dev, shape, target, mode):
    h1, w1, up, H2, W2 = shape
    l1, l2 = [logits((h1, w1), 100 + h1 * w1)], [logits((H2, W2), 200 + H2 * W2)]
    got = run_kernel(dev, l1, l2, [up], [target], [0.7], mode)
    check_all(got, l1, l2, [up], [target], [0.7], mode)


def _eight():
    shapes = [SHAPES[i] for i in (0, 1, 2, 3, 4, 5, 6, 7)]
    l1s = [logits(s[:2], 300 + i) for i, s in enumerate(shapes)]
    l2s = [logits(s[3:], 400 + i) for i, s in enumerate(shapes)]
    return l1s, l2s, [s[2] for s in shapes], [0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.0], [0.25, 0.25, 0.25, 0.25, 0.5, 0.5, -0.6, -0.4]


def test_eight_mixed_terms_then_three_on_the_same_workspace(dev):
    """One launch of 8 mixed-shape terms with weights of both signs; a 3-term launch directly after it finds the counter at zero."""
    from supervised_gan_amd import ops
    l1s, l2s, ups, ts, ws = _eight()
    got = run_kernel(dev, l1s, l2s, ups, ts, ws, (1, 1, 0))
    check_all(got, l1s, l2s, ups, ts, ws, (1, 1, 0))
    got3 = run_kernel(dev, l1s[5:], l2s[5:], ups[5:], ts[5:], ws[5:], (1, 1, 0))
    check_all(got3, l1s[5:], l2s[5:], ups[5:], ts[5:], ws[5:], (1, 1, 0))
    ws_buf = ops._factd_loss_workspace(dev)
    assert int(ws_buf.view(torch.int32)[2 * 8 * 16].item()) == 0      # the ticket behind the 8 x 16 partials


@pytest.mark.parametrize("want", [(True, False), (False, True), (False, False)], ids=["no_dl2", "no_dl1", "no_grads"])
def test_null_gradient_buffers(dev, want):
    l1s, l2s, ups, ts, ws = _eight()
    got = run_kernel(dev, l1s[:3], l2s[:3], ups[:3], ts[:3], ws[:3], (1, 1, 0), want=want)
    check_all(got, l1s[:3], l2s[:3], ups[:3], ts[:3], ws[:3], (1, 1, 0))


def test_stored_layout_ld4_zeroes_the_padding_channels(dev):
    l1s, l2s, ups, ts, ws = _eight()
    got = run_kernel(dev, l1s[:2], l2s[:2], ups[:2], ts[:2], ws[:2], (1, 1, 0), ld=4)
    check_all(got, l1s[:2], l2s[:2], ups[:2], ts[:2], ws[:2], (1, 1, 0))
    for d in got[2] + got[3]:
        assert d.shape[2] == 4 and float(d[..., 1:].abs().max()) == 0.0


def _tagged(t, dev):
    x = t.to(dev).requires_grad_(True)
    y = x * 1.0          # a non-leaf, like a discriminator output
    y._sgan_pending_sigmoid = True
    return x, y


def test_autograd_node_with_a_non_unit_upstream_gradient(dev):
    """(2.5 * total).backward() through _FactdLossMultiFn: the second entry point rescales."""
    from supervised_gan_amd import networks
    l1s, l2s, ups, ts, ws = _eight()
    sel = [0, 4, 6]      # all up == 2
    a = [_tagged(l1s[i], dev) for i in sel]
    b = [_tagged(l2s[i], dev) for i in sel]
    total, each = networks.factored_gan_loss([y for _, y in a], [y for _, y in b], [ts[i] == 1.0 for i in sel], [ws[i] for i in sel], up=2)
    assert total.grad_fn is not None and type(total.grad_fn).__name__.startswith("_FactdLossMultiFn")
    (2.5 * total).backward()
    got = (each.cpu(), total.detach().cpu(), [x.grad[0].permute(1, 2, 0).cpu() for x, _ in a], [x.grad[0].permute(1, 2, 0).cpu() for x, _ in b])
    check_all(got, [l1s[i] for i in sel], [l2s[i] for i in sel], [2] * 3, [ts[i] for i in sel], [ws[i] for i in sel], (1, 1, 0), upstream=2.5)


def test_autograd_node_detached_d1_side_gets_no_gradient(dev):
    from supervised_gan_amd import networks
    l1, l2 = logits((7, 7), 1), logits((19, 19), 2)
    y1 = l1.to(dev)
    y1._sgan_pending_sigmoid = True
    x2, y2 = _tagged(l2, dev)
    total, _ = networks.factored_gan_loss([y1], [y2], [True], [1.0], up=2)
    total.backward()
    got = (None, None, None, [x2.grad[0].permute(1, 2, 0).cpu()])
    r64 = composition([l1], [l2], [2], [1.0], [1.0], (1, 1, 0), torch.float64)
    r32 = composition([l1], [l2], [2], [1.0], [1.0], (1, 1, 0), torch.float32)
    check("dl2", got[3][0][..., 0], r64[3][0][0, 0], r32[3][0][0, 0])


def test_saturated_logits_stay_finite_and_match_the_fp32_composition(dev):
    """Logits from {+-40, +-120} and |x| <= 8 only (between 12 and 25 fp32 sigmoid rounds to exactly 1, the clamp switches, and
    fp32 and fp64 legitimately disagree): everything finite, compared by the same rule against the fp32 CPU composition."""
    g = torch.Generator().manual_seed(9)

    def sat(shape):
        small = (torch.rand(1, 1, *shape, generator=g) * 16 - 8)
        big = torch.tensor([40.0, -40.0, 120.0, -120.0])[torch.randint(0, 4, (1, 1, *shape), generator=g)]
        return torch.where(torch.rand(1, 1, *shape, generator=g) < 0.5, small, big)
    for mode in MODES:
        for target in (0.0, 1.0):
            l1, l2 = [sat((7, 7))], [sat((19, 19))]
            each, total, d1, d2 = run_kernel(dev, l1, l2, [2], [target], [1.0], mode)
            r32 = composition(l1, l2, [2], [target], [1.0], mode, torch.float32)
            for name, a_, b_ in (("each", each, r32[0]), ("total", total, r32[1]), ("dl1", d1[0][..., 0], r32[2][0][0, 0]),
                                 ("dl2", d2[0][..., 0], r32[3][0][0, 0])):
                assert torch.isfinite(a_).all(), (name, mode, target)
                e = rel(a_, b_)
                print(f"saturated {mode} t={target} {name}: kernel vs fp32 composition {e:.3e}")
                assert e <= 1e-3, (name, mode, target, e)


def test_two_calls_give_the_same_bits(dev):
    l1s, l2s, ups, ts, ws = _eight()
    a = run_kernel(dev, l1s, l2s, ups, ts, ws, (1, 1, 0))
    b = run_kernel(dev, l1s, l2s, ups, ts, ws, (1, 1, 0))
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])
    for x, y in zip(a[2] + a[3], b[2] + b[3]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("h1,w1,up,H2,W2,mode", [(5, 5, 2, 9, 9, (1, 1, 0)),      # the upsampled map is the larger one
                                                 (2, 2, 1, 7, 7, (1, 1, 0)),      # a pad as large as the map
                                                 (7, 7, 2, 19, 19, (0, 1, 0))],   # BCE on a raw score times a probability
                         ids=["d1_larger", "pad_ge_size", "raw_sig_bce"])
def test_outside_the_envelope_is_status_1_and_writes_nothing(dev, h1, w1, up, H2, W2, mode):
    """The C entry points alone: status 1, outputs untouched (no fallback BCE on out-of-range values runs on the device)."""
    from supervised_gan_amd import _lib, ops
    a, b = buf(logits((h1, w1), 1), 1, dev), buf(logits((H2, W2), 2), 1, dev)
    d1, d2 = torch.full_like(a, 5.0), torch.full_like(b, 5.0)
    each, total = torch.full((1,), 5.0, device=dev), torch.full((), 5.0, device=dev)
    job = (_lib.FactdLossJob * 1)()
    job[0] = _lib.FactdLossJob(a.data_ptr(), 1, h1, w1, b.data_ptr(), 1, H2, W2, up, 1.0, 1.0, d1.data_ptr(), 1, d2.data_ptr(), 1)
    ws = ops._factd_loss_workspace(dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    m = ops.factd_mode(*mode)
    assert _lib.lib().sgan_factd_loss_multi_fwd(job, 1, m, each.data_ptr(), total.data_ptr(), ws.data_ptr(), ops.FACTD_LOSS_WS_BYTES, st) == 1
    assert _lib.lib().sgan_factd_loss_multi_bwd(job, 1, m, total.data_ptr(), st) == 1
    torch.cuda.synchronize()
    for t in (d1, d2, each, total):
        assert float((t - 5.0).abs().max()) == 0.0


def test_wrapper_raises_the_trainers_value_error_for_a_larger_d1_map(dev):
    from supervised_gan_amd import networks
    y1, y2 = logits((5, 5), 1).to(dev), logits((9, 9), 2).to(dev)
    y1._sgan_pending_sigmoid = y2._sgan_pending_sigmoid = True
    with pytest.raises(ValueError, match=r"the upsampled D1 map \(10, 10\) is larger than D2's \(9, 9\)"):
        networks.factored_gan_loss([y1], [y2], [True], [1.0], up=2)

"""sgan_seg_head_pw / sgan_pixel_weight_sum (the pixel-weighted softmax head of `--border_weight`) against a torch composition in
float64 on the CPU: F.cross_entropy(reduction='none') times w_p = class_w[y_p] + pixel_add[p], divided by sum_p w_p, autograd for
d loss / d logits.  Pass rule (tests/test_hip_seg_head.py): max|a - b| / (max|b| + 1e-12) <= max(1e-3, 4 e_ref), e_ref the same
statistic of the fp32 composition on the CPU.  Both errors are printed.

Shapes: 17 x 19 (323 pixels: one full block and a guarded tail) and 64 x 64 (16 blocks), C = 2 and 3 (4-channel storage)."""
import pytest
import torch
import torch.nn.functional as F

from hip_utils import rel

pytestmark = pytest.mark.gpu

SHAPES = [(17, 19, 2), (17, 19, 3), (64, 64, 2), (64, 64, 3)]
CW = [2.0, 5.0, 0.5]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def inputs(H, W, C_):
    """Logits, a label map with torch's ignore_index and a label past the last class in it, and a border-like map: zero on most
    pixels, up to 10 on the others."""
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + C_)
    z = torch.randn(1, C_, H, W, generator=g) * 1.5
    lab = torch.randint(0, C_, (1, H, W), generator=g)
    lab[0, 0, :3] = -100
    lab[0, 1, 2] = C_ + 1
    add = torch.rand(H, W, generator=g) * 10.0 * (torch.rand(H, W, generator=g) > 0.7)
    return z, lab, add


def reference(z, lab, cw, add, dtype, gscale=1.7, norm=None):
    """(p, loss, d loss * gscale / dz, sum_p w_p); labels outside [0, C) contribute nothing."""
    C_ = z.shape[1]
    z = z.detach().to(dtype).requires_grad_(True)
    ok = (lab >= 0) & (lab < C_)
    y = torch.where(ok, lab, torch.full_like(lab, -100))
    w = (torch.ones(C_, dtype=dtype) if cw is None else cw.to(dtype))[y.clamp(min=0)] + add.to(dtype)[None]
    w = torch.where(ok, w, torch.zeros_like(w))
    total = w.sum() if norm is None else norm
    loss = (F.cross_entropy(z, y, reduction='none') * w).sum() / total
    (loss * gscale).backward()
    return F.softmax(z.detach(), dim=1), loss.detach(), z.grad, w.sum().detach()


def check(name, got, ref64, ref32):
    e, e_ref = rel(got, ref64), rel(ref32, ref64)
    print(f"{name}: kernel vs fp64 {e:.3e}, fp32 composition vs fp64 {e_ref:.3e}")
    assert e <= max(1e-3, 4 * e_ref), (name, e, e_ref)


def run(dev, z, lab, cw, add, norm=None, gscale=1.7):
    from supervised_gan_amd import losses, ops
    zd = z.to(dev).requires_grad_(True)
    p, loss = losses.seg_head(zd, lab.to(dev), None if cw is None else cw.to(dev), norm, ops.SEGHEAD_SOFTMAX,
                              pixel_add=None if add is None else add.to(dev))
    assert type(loss.grad_fn).__name__.startswith("_SegHeadFn")
    pb = ops.buffer_of(p)
    (loss * gscale).backward()
    torch.cuda.synchronize()
    return p.detach().cpu(), loss.detach().cpu(), zd.grad.cpu(), pb, ops.buffer_of(zd.grad)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_pixel_weighted_head(dev, shape, weighted):
    from supervised_gan_amd import ops
    H, W, C_ = shape
    z, lab, add = inputs(H, W, C_)
    cw = torch.tensor(CW[:C_]) if weighted else None
    r64, r32 = reference(z, lab, cw, add, torch.float64), reference(z, lab, cw, add, torch.float32)
    norm = torch.full((), -1.0, dtype=torch.float32, device=dev)
    ops.pixel_weight_sum(lab.to(dev).reshape(-1), C_, None if cw is None else cw.to(dev), add.to(dev).reshape(-1), norm)
    check("norm", norm.cpu(), r64[3], r32[3])
    p, loss, dz, pb, db = run(dev, z, lab, cw, add, norm)
    for name, g_, a, b in (("p", p, r64[0], r32[0]), ("loss", loss, r64[1], r32[1]), ("dz", dz, r64[2], r32[2])):
        check(name, g_, a, b)
    assert pb is not None, "seg_head must hand out an NHWC-backed view"
    for buf in (pb, db):      # the padding channels are written as zeros
        if buf is not None:
            assert buf.shape[2] == 4 and float(buf[..., C_:].abs().max()) == 0.0
    assert float(dz[0, :, 0, :3].abs().max()) == 0.0 and float(dz[0, :, 1, 2].abs().max()) == 0.0      # labels outside [0, C)
    # norm None: seg_head takes the sum itself; and a second call on the same workspaces gives the same bits
    p2, loss2, dz2, _, _ = run(dev, z, lab, cw, add, None)
    assert torch.equal(loss, loss2) and torch.equal(dz, dz2) and torch.equal(p, p2)
    for which in ("head", "norm"):      # both workspaces are left zeroed
        assert float(ops._seghead_workspace(dev, which).abs().max()) == 0.0


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_a_zero_map_reproduces_seg_head_bit_for_bit(dev, shape, weighted):
    from supervised_gan_amd import ops
    H, W, C_ = shape
    z, lab, _ = inputs(H, W, C_)
    cw = torch.tensor(CW[:C_]) if weighted else None
    cwd = None if cw is None else cw.to(dev)
    n_plain = torch.full((), -1.0, dtype=torch.float32, device=dev)
    n_pw = torch.full((), -2.0, dtype=torch.float32, device=dev)
    ops.label_weight_sum(lab.to(dev).reshape(-1), C_, cwd, n_plain)
    ops.pixel_weight_sum(lab.to(dev).reshape(-1), C_, cwd, torch.zeros(H * W, device=dev), n_pw)
    assert torch.equal(n_plain, n_pw)
    plain = run(dev, z, lab, cw, None)
    pw = run(dev, z, lab, cw, torch.zeros(H, W))
    assert torch.equal(plain[0], pw[0]) and torch.equal(plain[1], pw[1]) and torch.equal(plain[2], pw[2])


def test_a_zero_norm_gives_loss_zero(dev):
    z, lab, add = inputs(17, 19, 3)
    p, loss, dz, _, _ = run(dev, z, lab, None, add, torch.zeros((), dtype=torch.float32, device=dev))
    assert float(loss) == 0.0 and float(dz.abs().max()) == 0.0
    check("p", p, F.softmax(z.double(), dim=1), F.softmax(z, dim=1))


def test_the_entries_report_not_covered_for_a_missing_operand(dev):
    import ctypes
    from hip_utils import to_buf
    from supervised_gan_amd import _lib, ops
    z, lab, add = inputs(17, 19, 3)
    zb, lt, ad = to_buf(z), lab.to(dev).reshape(-1), add.to(dev).reshape(-1)
    pb, db = torch.full_like(zb, 7.0), torch.full_like(zb, 7.0)
    loss, norm = torch.full((), 7.0, device=dev), torch.ones((), device=dev)
    ws = ops._seghead_workspace(dev, "head")
    P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
    l = _lib.lib()
    head = lambda a, n, C_=3: l.sgan_seg_head_pw(P(zb), 4, 17 * 19, C_, P(lt), None, 0, P(a), P(n), P(pb), 4, P(db), 4, P(loss), P(ws), None)  # noqa: E731
    assert head(None, norm) == 1 and head(ad, None) == 1 and head(ad, norm, 17) == 1
    assert l.sgan_pixel_weight_sum(P(lt), 17 * 19, 3, None, None, P(norm), P(ws), None) == 1
    assert l.sgan_pixel_weight_sum(P(lt), 17 * 19, 17, None, P(ad), P(norm), P(ws), None) == 1
    torch.cuda.synchronize()
    assert bool((pb == 7.0).all()) and bool((db == 7.0).all()) and float(loss) == 7.0 and float(norm) == 1.0
    assert head(ad, norm) == 0


def test_a_gradient_sent_into_p_raises(dev):
    from supervised_gan_amd import losses, ops
    z, lab, add = inputs(17, 19, 2)
    zd = z.to(dev).requires_grad_(True)
    p, loss = losses.seg_head(zd, lab.to(dev), None, None, ops.SEGHEAD_SOFTMAX, pixel_add=add.to(dev))
    with pytest.raises(AssertionError, match="one consumer"):
        (loss + (p * 0.01).sum()).backward()


def test_the_map_goes_with_the_softmax_head_only(dev):
    from supervised_gan_amd import losses, ops
    z, lab, add = inputs(17, 19, 2)
    t = F.one_hot(lab.clamp(0, 1), 2).permute(0, 3, 1, 2).float()
    with pytest.raises(AssertionError, match="softmax"):
        losses.seg_head(z.to(dev), t.to(dev), None, None, ops.SEGHEAD_SIGMOID, pixel_add=add.to(dev))

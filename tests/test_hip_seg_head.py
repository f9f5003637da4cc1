"""sgan_seg_head / sgan_label_weight_sum (`--which_model_netD None`) against torch in float64 on the CPU: F.softmax +
F.cross_entropy(weight=), and torch.sigmoid + the weight-map loop + F.binary_cross_entropy(weight=).  Pass rule (the parity gate of
test_oracle_golden.py): max|a - b| / (max|b| + 1e-12) <= max(1e-3, 4 e_ref), e_ref the same statistic of the fp32 composition on the
CPU.  Both errors are printed."""
import pytest
import torch
import torch.nn.functional as F

from hip_utils import rel

pytestmark = pytest.mark.gpu

# H, W, C: 4-, 8- and 12/16-channel storage, pixel counts that are no multiple of the block, a single partial block
SHAPES = [(5, 7, 3), (33, 31, 2), (257, 3, 3), (64, 64, 4), (9, 7, 12)]
CW = [2.0, 5.0, 0.5, 3.0]
GUARD = 4096      # elements of sentinel behind every guarded operand


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def class_w(n):
    return torch.tensor((CW * 4)[:n]) if n else None


def inputs(H, W, C_, soft=False):
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + C_)
    z = torch.randn(1, C_, H, W, generator=g) * 1.5
    lab = torch.randint(0, C_, (1, H, W), generator=g)
    t = torch.rand(1, C_, H, W, generator=g) if soft else F.one_hot(lab, C_).permute(0, 3, 1, 2).float()
    lab = lab.clone()
    lab[0, 0, :3] = -100      # torch's ignore_index at the start of a row
    return z, lab, t


def ref_softmax(z, lab, cw, dtype, gscale=1.7):
    z = z.detach().to(dtype).requires_grad_(True)
    w = None if cw is None else cw.to(dtype)
    p = F.softmax(z, dim=1)
    loss = F.cross_entropy(z, lab, weight=w)
    (loss * gscale).backward()
    return p.detach(), loss.detach(), z.grad


def ref_sigmoid(z, t, cw, dtype, gscale=1.7):
    z = z.detach().to(dtype).requires_grad_(True)
    t = t.to(dtype)
    p = torch.sigmoid(z)
    wm = None
    if cw is not None:
        wm = torch.ones_like(t[:, :1])
        for i in range(cw.numel()):
            wm = wm + t.narrow(1, i, 1) * (cw[i].to(dtype) - 1.0)
    loss = F.binary_cross_entropy(p, t, weight=wm)
    (loss * gscale).backward()
    return p.detach(), loss.detach(), z.grad


def check(name, got, ref64, ref32):
    e, e_ref = rel(got, ref64), rel(ref32, ref64)
    print(f"{name}: kernel vs fp64 {e:.3e}, fp32 composition vs fp64 {e_ref:.3e}")
    assert e <= max(1e-3, 4 * e_ref), (name, e, e_ref)


def run(dev, z, lt, cw, mode, norm=None, gscale=1.7):
    """(p, loss, dz, p's buffer, dz's buffer) of losses.seg_head on the device, the gradient through (loss * gscale).backward()."""
    from supervised_gan_amd import losses, ops
    zd = z.to(dev).requires_grad_(True)
    p, loss = losses.seg_head(zd, lt.to(dev), None if cw is None else cw.to(dev), norm, mode)
    assert type(loss.grad_fn).__name__.startswith("_SegHeadFn")
    pb = ops.buffer_of(p)
    assert pb is not None, "seg_head must hand out an NHWC-backed view"
    (loss * gscale).backward()
    torch.cuda.synchronize()
    return p.detach().cpu(), loss.detach().cpu(), zd.grad.cpu(), pb, ops.buffer_of(zd.grad)


def padding_is_zero(buf, C_):
    if buf is not None and buf.shape[2] > C_:
        assert float(buf[..., C_:].abs().max()) == 0.0


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_softmax_head(dev, shape, weighted):
    from supervised_gan_amd import ops
    H, W, C_ = shape
    z, lab, _ = inputs(H, W, C_)
    cw = class_w(C_) if weighted else None
    norm = torch.full((), -1.0, dtype=torch.float32, device=dev)
    ops.label_weight_sum(lab.to(dev).reshape(-1), C_, None if cw is None else cw.to(dev), norm)
    valid = lab[lab >= 0]
    norm64 = (cw.double()[valid].sum() if weighted else torch.tensor(float(valid.numel()), dtype=torch.float64))
    norm32 = (cw[valid].sum() if weighted else torch.tensor(float(valid.numel())))
    check("norm", norm.cpu(), norm64, norm32)
    p, loss, dz, pb, db = run(dev, z, lab, cw, ops.SEGHEAD_SOFTMAX, norm)
    r64, r32 = ref_softmax(z, lab, cw, torch.float64), ref_softmax(z, lab, cw, torch.float32)
    for name, g_, a, b in (("p", p, r64[0], r32[0]), ("loss", loss, r64[1], r32[1]), ("dz", dz, r64[2], r32[2])):
        check(name, g_, a, b)
    padding_is_zero(pb, C_)
    padding_is_zero(db, C_)
    # norm None: seg_head takes the sum itself
    _, loss2, _, _, _ = run(dev, z, lab, cw, ops.SEGHEAD_SOFTMAX, None)
    assert torch.equal(loss, loss2)


@pytest.mark.parametrize("nw", ["0", "2", "C"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_sigmoid_head(dev, shape, nw):
    from supervised_gan_amd import ops
    H, W, C_ = shape
    z, _, t = inputs(H, W, C_)
    cw = class_w({"0": 0, "2": min(2, C_), "C": C_}[nw])
    p, loss, dz, pb, db = run(dev, z, t, cw, ops.SEGHEAD_SIGMOID)
    r64, r32 = ref_sigmoid(z, t, cw, torch.float64), ref_sigmoid(z, t, cw, torch.float32)
    for name, g_, a, b in (("p", p, r64[0], r32[0]), ("loss", loss, r64[1], r32[1]), ("dz", dz, r64[2], r32[2])):
        check(name, g_, a, b)
    padding_is_zero(pb, C_)
    padding_is_zero(db, C_)


def test_sigmoid_head_soft_targets(dev):
    from supervised_gan_amd import ops
    z, _, t = inputs(33, 31, 2, soft=True)
    cw = class_w(2)
    p, loss, dz, _, _ = run(dev, z, t, cw, ops.SEGHEAD_SIGMOID)
    r64, r32 = ref_sigmoid(z, t, cw, torch.float64), ref_sigmoid(z, t, cw, torch.float32)
    check("loss", loss, r64[1], r32[1])
    check("dz", dz, r64[2], r32[2])


def test_unit_upstream_gradient_hands_out_the_forwards_gradient(dev):
    """The trainers' cached unit gradient (ops.register_unit_grad): no rescaling launch, dz is what the forward wrote."""
    from supervised_gan_amd import losses, ops
    z, lab, _ = inputs(33, 31, 2)
    zd = z.to(dev).requires_grad_(True)
    p, loss = losses.seg_head(zd, lab.to(dev), None, None, ops.SEGHEAD_SOFTMAX)
    one = torch.ones_like(loss)
    ops.register_unit_grad(one)
    loss.backward(one)
    torch.cuda.synchronize()
    r64, r32 = ref_softmax(z, lab, None, torch.float64, 1.0), ref_softmax(z, lab, None, torch.float32, 1.0)
    check("dz", zd.grad.cpu(), r64[2], r32[2])


def _guarded(t, fill=float("nan")):
    """A copy of `t` whose storage ends in GUARD sentinel elements (NaN: an over-READ that is used turns the result NaN; an
    over-WRITE changes the sentinel's bit pattern).  Returns (view shaped like t, the guard)."""
    flat = torch.full((t.numel() + GUARD,), fill, dtype=t.dtype, device="cuda")
    flat[: t.numel()] = t.reshape(-1).to("cuda")
    return flat[: t.numel()].view(t.shape), flat[t.numel():]


def _guard_intact(g, fill=None):
    return bool(torch.isnan(g).all()) if fill is None else bool((g == fill).all())


@pytest.mark.parametrize("shape", [(5, 7, 3), (33, 31, 2), (9, 7, 12)], ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("mode", ["softmax", "sigmoid"])
def test_operands_with_guarded_tails(dev, mode, shape):
    """Every operand of the launch ends in a sentinel: the results are finite and match, and every guard keeps its bits."""
    from hip_utils import from_buf, to_buf
    from supervised_gan_amd import ops
    H, W, C_ = shape
    z, lab, t = inputs(H, W, C_)
    cw = class_w(C_)
    softmax = mode == "softmax"
    zb, gz = _guarded(to_buf(z))
    pb, gp = _guarded(torch.full_like(zb, 7.0))
    db, gd = _guarded(torch.full_like(zb, 7.0))
    cwd, gc = _guarded(cw)
    loss, gl = _guarded(torch.zeros(1))
    guards = [gz, gp, gd, gc, gl]
    if softmax:
        lt, glab = _guarded(lab.reshape(-1), fill=1 << 40)
        norm, gn = _guarded(torch.zeros(1))
        ops.label_weight_sum(lt, C_, cwd, norm[0])
        guards.append(gn)
        assert ops.seg_head(zb, C_, ops.SEGHEAD_SOFTMAX, lt, cwd, C_, norm[0], pb, db, loss[0])
        r64, r32 = ref_softmax(z, lab, cw, torch.float64, 1.0), ref_softmax(z, lab, cw, torch.float32, 1.0)
    else:
        lt, gt = _guarded(to_buf(t))
        guards.append(gt)
        assert ops.seg_head(zb, C_, ops.SEGHEAD_SIGMOID, lt, cwd, C_, None, pb, db, loss[0])
        r64, r32 = ref_sigmoid(z, t, cw, torch.float64, 1.0), ref_sigmoid(z, t, cw, torch.float32, 1.0)
    torch.cuda.synchronize()
    got = (from_buf(pb, C_), loss[0].cpu(), from_buf(db, C_))
    for name, g_, a, b in zip(("p", "loss", "dz"), got, r64, r32):
        assert bool(torch.isfinite(g_).all()), name
        check(name, g_, a, b)
    padding_is_zero(pb, C_)
    padding_is_zero(db, C_)
    assert all(_guard_intact(g) for g in guards)
    if softmax:
        assert _guard_intact(glab, 1 << 40)
    for which in ("head", "norm"):      # both workspaces are left zeroed
        assert float(ops._seghead_workspace(dev, which).abs().max()) == 0.0


@pytest.mark.parametrize("mode", ["softmax", "sigmoid"])
def test_operands_of_unequal_row_length_take_the_scalar_form(dev, mode):
    """Logits that are the first channels of an 8-channel buffer beside 4-channel outputs: no 16-byte rows, same results."""
    from hip_utils import from_buf, to_buf
    from supervised_gan_amd import ops
    H, W, C_ = 33, 31, 3
    z, lab, t = inputs(H, W, C_)
    cw = class_w(C_).to(dev)
    wide = torch.full((H, W, 8), float("nan"), device=dev)
    wide[..., :C_] = to_buf(z)[..., :C_]
    pb, db = torch.full((H, W, 4), 7.0, device=dev), torch.full((H, W, 4), 7.0, device=dev)
    loss = torch.zeros((), device=dev)
    if mode == "softmax":
        norm = torch.zeros((), device=dev)
        ops.label_weight_sum(lab.to(dev).reshape(-1), C_, cw, norm)
        assert ops.seg_head(wide, C_, ops.SEGHEAD_SOFTMAX, lab.to(dev).reshape(-1), cw, C_, norm, pb, db, loss)
        r64, r32 = ref_softmax(z, lab, cw.cpu(), torch.float64, 1.0), ref_softmax(z, lab, cw.cpu(), torch.float32, 1.0)
    else:
        assert ops.seg_head(wide, C_, ops.SEGHEAD_SIGMOID, to_buf(t), cw, C_, None, pb, db, loss)
        r64, r32 = ref_sigmoid(z, t, cw.cpu(), torch.float64, 1.0), ref_sigmoid(z, t, cw.cpu(), torch.float32, 1.0)
    torch.cuda.synchronize()
    for name, g_, a, b in zip(("p", "loss", "dz"), (from_buf(pb, C_), loss.cpu(), from_buf(db, C_)), r64, r32):
        check(name, g_, a, b)
    padding_is_zero(pb, C_)
    padding_is_zero(db, C_)


@pytest.mark.parametrize("mode", ["softmax", "sigmoid"])
def test_no_grad_call_and_a_second_call_on_the_same_workspace(dev, mode):
    from supervised_gan_amd import losses, ops
    z, lab, t = inputs(64, 64, 4)
    cw = class_w(4)
    m = ops.SEGHEAD_SOFTMAX if mode == "softmax" else ops.SEGHEAD_SIGMOID
    lt = (lab if mode == "softmax" else t).to(dev)
    with torch.no_grad():
        p, loss = losses.seg_head(z.to(dev), lt, cw.to(dev), None, m)
    assert not loss.requires_grad and not p.requires_grad
    r64, r32 = (ref_softmax if mode == "softmax" else ref_sigmoid)(z, lab if mode == "softmax" else t, cw, torch.float64), \
        (ref_softmax if mode == "softmax" else ref_sigmoid)(z, lab if mode == "softmax" else t, cw, torch.float32)
    check("p", p.cpu(), r64[0], r32[0])
    check("loss", loss.cpu(), r64[1], r32[1])
    with torch.no_grad():
        p2, again = losses.seg_head(z.to(dev), lt, cw.to(dev), None, m)
    assert torch.equal(loss, again) and torch.equal(p, p2)


def test_a_gradient_sent_into_p_raises(dev):
    """The fusion is valid only while the loss is p's one consumer: a second consumer's gradient has no way into dlogits."""
    from supervised_gan_amd import losses, ops
    z, lab, _ = inputs(5, 7, 3)
    zd = z.to(dev).requires_grad_(True)
    p, loss = losses.seg_head(zd, lab.to(dev), None, None, ops.SEGHEAD_SOFTMAX)
    with pytest.raises(AssertionError, match="one consumer"):
        (loss + (p * 0.01).sum()).backward()


def test_label_must_be_int64_on_the_device(dev):
    from supervised_gan_amd import losses, ops
    z, lab, _ = inputs(5, 7, 3)
    with pytest.raises(AssertionError, match="int64"):
        losses.seg_head(z.to(dev), lab.to(dev).int(), None, None, ops.SEGHEAD_SOFTMAX)
    with pytest.raises(AssertionError, match="int64"):
        losses.seg_head(z.to(dev), lab, None, None, ops.SEGHEAD_SOFTMAX)

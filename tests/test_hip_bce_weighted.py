"""sgan_sigmoid_nhwc_* and sgan_bce_weighted_* (`--use_sigmoid_ss`) against torch.sigmoid + the weight-map loop +
F.binary_cross_entropy(weight=) in float64 on the CPU.  Pass rule (the parity gate of test_oracle_golden.py): max|a - b| /
(max|b| + 1e-12) <= max(1e-3, 4 e_ref), e_ref the same statistic of the fp32 composition on the CPU.  Both errors are printed."""
import pytest
import torch
import torch.nn.functional as F

from hip_utils import rel

pytestmark = pytest.mark.gpu

SHAPES = [(5, 7, 3), (33, 31, 2), (257, 3, 3), (64, 64, 4)]      # H, W, C (5x7x3 is stored with 4 channels)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    return torch.device("cuda", 0)


def inputs(H, W, C_, soft=False):
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + C_)
    z = torch.randn(1, C_, H, W, generator=g) * 1.5
    if soft:
        t = torch.rand(1, C_, H, W, generator=g)
    else:
        t = F.one_hot(torch.randint(0, C_, (1, H, W), generator=g), C_).permute(0, 3, 1, 2).float()
    gp = torch.randn(1, C_, H, W, generator=g) * 0.01      # the gradient a second consumer of p (cat_pair -> D) sends back
    return z, t, gp


def composition(z, t, cw, dtype, gp=None):
    """(p, loss, dz) of the trainer's former code on the CPU in `dtype`; dz also carries `gp` arriving at p."""
    z = z.detach().to(dtype).requires_grad_(True)
    t = t.to(dtype)
    p = torch.sigmoid(z)
    wm = None
    if cw is not None:
        wm = torch.ones_like(t[:, :1])
        for i in range(cw.numel()):
            wm = wm + t.narrow(1, i, 1) * (cw[i].to(dtype) - 1.0)
    loss = F.binary_cross_entropy(p, t, weight=wm)
    obj = loss if gp is None else loss + (p * gp.to(dtype)).sum()
    obj.backward()
    return p.detach(), loss.detach(), z.grad


def check(name, got, ref64, ref32):
    e, e_ref = rel(got, ref64), rel(ref32, ref64)
    print(f"{name}: kernel vs fp64 {e:.3e}, fp32 composition vs fp64 {e_ref:.3e}")
    assert e <= max(1e-3, 4 * e_ref), (name, e, e_ref)


def run(dev, z, t, cw, gp=None):
    from supervised_gan_amd import losses, ops
    zd = z.to(dev).requires_grad_(True)
    p = losses.sigmoid_channels(zd)
    assert type(p.grad_fn).__name__.startswith("_SigmoidChannelsFn")
    pb = ops.buffer_of(p)
    assert pb is not None, "sigmoid_channels must hand out an NHWC-backed view (cat_pair reads it without a layout copy)"
    loss = losses.weighted_bce(p, t.to(dev), None if cw is None else cw.to(dev))
    assert type(loss.grad_fn).__name__.startswith("_WeightedBceFn")
    obj = loss if gp is None else loss + (p * gp.to(dev)).sum()
    obj.backward()
    torch.cuda.synchronize()
    return p.detach().cpu(), loss.detach().cpu(), zd.grad.cpu(), pb


@pytest.mark.parametrize("nw", ["0", "2", "C"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_sigmoid_and_weighted_bce(dev, shape, nw):
    H, W, C_ = shape
    z, t, _ = inputs(H, W, C_)
    n = {"0": 0, "2": min(2, C_), "C": C_}[nw]
    cw = torch.tensor([2.0, 5.0, 0.5, 3.0][:n]) if n else None
    p, loss, dz, pb = run(dev, z, t, cw)
    r64, r32 = composition(z, t, cw, torch.float64), composition(z, t, cw, torch.float32)
    for name, g_, a, b in (("p", p, r64[0], r32[0]), ("loss", loss, r64[1], r32[1]), ("dz", dz, r64[2], r32[2])):
        check(name, g_, a, b)
    if pb.shape[2] > C_:
        assert float(pb[..., C_:].abs().max()) == 0.0      # padded channels of p


def test_soft_targets(dev):
    z, t, _ = inputs(33, 31, 2, soft=True)
    cw = torch.tensor([2.0, 5.0])
    p, loss, dz, _ = run(dev, z, t, cw)
    r64, r32 = composition(z, t, cw, torch.float64), composition(z, t, cw, torch.float32)
    check("loss", loss, r64[1], r32[1])
    check("dz", dz, r64[2], r32[2])


def test_second_consumer_of_p_adds_its_gradient(dev):
    """dz is the sum of the BCE path and of a gradient arriving at p from another consumer (the discriminators behind cat_pair)."""
    z, t, gp = inputs(5, 7, 3)
    cw = torch.tensor([2.0, 5.0])
    p, loss, dz, _ = run(dev, z, t, cw, gp)
    r64, r32 = composition(z, t, cw, torch.float64, gp), composition(z, t, cw, torch.float32, gp)
    check("loss", loss, r64[1], r32[1])
    check("dz", dz, r64[2], r32[2])


def test_no_grad_unweighted_call_of_validation(dev):
    from supervised_gan_amd import losses
    z, t, _ = inputs(64, 64, 4)
    with torch.no_grad():
        p = losses.sigmoid_channels(z.to(dev))
        loss = losses.weighted_bce(p, t.to(dev), None)
    assert not loss.requires_grad
    r64, r32 = composition(z, t, None, torch.float64), composition(z, t, None, torch.float32)
    check("loss", loss.cpu(), r64[1], r32[1])
    # a second call on the same workspace: the ticket was left at zero
    with torch.no_grad():
        again = losses.weighted_bce(p, t.to(dev), None)
    assert torch.equal(loss, again)

"""FusedAdam / AdamGroups / FusedSGD on real networks, fed the gradients of a real backward, against the fp64 reference of
tests/adam_ref.py -- and the host logic around the kernels: which launch runs (`_fused_plan`), when the derived weight copies count
as current (`_wt_key`, `_wt_epoch`), what `zero_grads_in_step` and `reset_state()` promise.

The reference is applied to the SNAPSHOTTED gradient arena of every step, so both sides see the same gradients and the parameters
can be compared (bound: adam_ref.assert_within_yardstick, as in tests/test_hip_adam_pack.py).  Derived copies, gradients and padded
positions are exact.  Only the derived-copy checks depend on the arithmetic mode; they run under bf16x3 and f32."""
import numpy as np
import pytest
import torch

import adam_ref as A

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = A.as_f32(2e-4, 0.5, 0.999, 1e-8)


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    from supervised_gan_amd import _lib, networks
    _lib.lib()
    return networks


@pytest.fixture(params=["bf16x3", "f32"])
def math_mode(request, N):
    from supervised_gan_amd import ops
    prev = ops.get_math()
    ops.set_math(request.param)
    yield request.param
    ops.set_math(prev)


class Net:
    """The small fcgan generator or the 3-layer PatchGAN of tests/test_hip_nets.py, with a fixed input and a fixed random
    cotangent: backward() is a real forward / backward of (out * R).sum() into the net's gradient arena."""

    def __init__(self, N, kind, seed):
        torch.manual_seed(seed)
        if kind == "G":
            self.net = N.define_G(2, 0, 8, "fcgan", "instance", False, n_layers_G=5, use_fcn=True, noise_nc=8, gpu_ids=[0])
            self.x = torch.randn(1, 8, 2, 2, device="cuda")
        else:
            self.net = N.define_D(2, 8, "n_layers", n_layers_D=3, norm="instance", use_sigmoid=True, scale_factor=1, gpu_ids=[0])
            self.x = torch.rand(1, 2, 64, 64, device="cuda")
        self.net.apply(N.weights_init)
        with torch.no_grad():
            self.R = torch.randn_like(self.net.forward(self.x))
        net = self.net
        self.padded = torch.zeros(net._nflat, dtype=torch.bool)          # stored positions that are no logical parameter
        for L in net.layers:
            w = self.padded[L.w_off: L.w_off + L.k * L.k * L.cout_s * L.cin_s].view(L.k * L.k, L.cout_s, L.cin_s)
            w[:, L.cout:, :] = True
            w[:, :, L.cin:] = True
            for off in ((L.b_off,) if L.bias else ()) + ((L.g_off, L.be_off) if L.norm == "bn" else ()):
                self.padded[off + L.cout: off + L.cout_s] = True
        self.padded = self.padded.numpy()
        assert self.padded.any() and not self.flat()[self.padded].any()

    def backward(self):
        (self.net.forward(self.x) * self.R).sum().backward()
        torch.cuda.synchronize()

    def flat(self):
        return self.net._flat.detach().cpu().numpy()

    def gflat(self):
        return self.net._gflat.detach().cpu().numpy()

    def assert_derived_fresh(self, what):
        """The four derived copies are bit-identical to a fresh ops.pack_weights of the master (into zeroed buffers, as the
        net's own were allocated: ranges no kernel writes compare equal too)."""
        from supervised_gan_amd import ops
        net = self.net
        fresh = [torch.zeros_like(net._flat) for _ in range(4)]
        ops.pack_weights(net._flat, fresh[0], fresh[1], fresh[2], net._conv_segments(), fresh[3])
        torch.cuda.synchronize()
        for name, b in zip(("_flat_t", "_pk_f", "_pk_b", "_pk_bh"), fresh):
            assert torch.equal(getattr(net, name).view(torch.int32), b.view(torch.int32)), f"{what}: {name} is not a pack of the current master"
        assert fresh[0].abs().max() > 0


class AdamRef:
    """fp64 Adam and its fp32 restatement over one flat arena, stepped with the gradients the GPU step consumed."""

    def __init__(self, p0, lr=LR):
        self.lr, self.t = lr, 0
        self.ref = (p0.astype(np.float64), np.zeros(p0.size), np.zeros(p0.size))
        self.f32 = (p0.copy(), np.zeros(p0.size, dtype=np.float32), np.zeros(p0.size, dtype=np.float32))

    def step(self, g):
        self.t += 1
        self.ref = A.adam_step(self.ref[0], g, self.ref[1], self.ref[2], self.t, self.lr, B1, B2, EPS)
        self.f32 = A.adam_step_f32(self.f32[0], g, self.f32[1], self.f32[2], self.t, self.lr, B1, B2, EPS)

    def check(self, T, opt, seg, what):
        got = (T.flat(), opt._m[seg].cpu().numpy(), opt._v[seg].cpu().numpy())
        A.assert_within_yardstick(got, self.f32, self.ref, what)
        assert float(np.abs(self.ref[0] - self.f32[0]).max()) < 0.1 * self.lr        # the bound is far below one step
        assert not got[0][T.padded].any(), f"{what}: a padded position left 0"
        assert opt.step_count == self.t


@pytest.mark.parametrize("zero_in_step", [False, True], ids=["keep_grads", "zero_in_step"])
@pytest.mark.parametrize("kind", ["G", "D"])
def test_fused_adam_three_steps(N, math_mode, kind, zero_in_step):
    """FusedAdam over one network = one sgan_adam_pack launch per step: parameters and moments against fp64 on the snapshotted
    gradients, padded positions, the derived copies, `_wt_key`, and what zero_grads_in_step promises."""
    from supervised_gan_amd.optim import FusedAdam
    T = Net(N, kind, 7)
    net = T.net
    opt = FusedAdam(list(net.parameters()), lr=2e-4, betas=(0.5, 0.999), zero_grads_in_step=zero_in_step)
    assert len(opt._segs) == 1 and opt._segs[0][2:] == (0, net._nflat)
    R = AdamRef(T.flat())
    for step in range(1, 4):
        opt.zero_grad()
        T.backward()
        g = T.gflat()
        assert np.abs(g).max() > 0 and not g[T.padded].any()
        assert opt._fused_plan() is not None             # the one-launch path, not sgan_adam_multi behind its back
        opt.step()
        torch.cuda.synchronize()
        R.step(g)
        R.check(T, opt, 0, f"FusedAdam {kind} step {step}")
        T.assert_derived_fresh(f"step {step}")
        assert net._wt_key == net._derived_key()
        if zero_in_step:
            assert not T.gflat().view(np.int32).any()            # exactly +0.0 everywhere
            net._gflat[:4] = 5.0
            opt.zero_grad()                                      # the step cleared already: a no-op, once
            assert net._gflat[:4].tolist() == [5.0] * 4
            net._gflat[:4] = 0.0
        else:
            assert np.array_equal(T.gflat().view(np.int32), g.view(np.int32))        # step() does not write the gradients
    opt.zero_grad()
    assert not T.gflat().any()


def test_reset_state_starts_again_at_t1(N):
    from supervised_gan_amd.optim import FusedAdam
    T = Net(N, "D", 8)
    opt = FusedAdam(list(T.net.parameters()), lr=2e-4, betas=(0.5, 0.999))
    for _ in range(2):
        opt.zero_grad()
        T.backward()
        opt.step()
    assert opt.step_count == 2
    opt.reset_state()
    assert opt.step_count == 0
    opt.zero_grad()
    T.backward()
    R = AdamRef(T.flat())                                # zero moments, t = 1, from the parameters as they are now
    g = T.gflat()
    opt.step()
    torch.cuda.synchronize()
    R.step(g)
    R.check(T, opt, 0, "the step after reset_state()")
    T.assert_derived_fresh("after reset_state()")


def _stale_then_refreshed(Ts, what):
    """After a step that did not write the derived copies itself: every net is flagged stale, and the next forward / backward
    re-makes the copies from the updated master."""
    for T in Ts:
        assert T.net._wt_key != T.net._derived_key(), f"{what}: the derived copies still count as current"
    for T in Ts:
        T.backward()
        T.assert_derived_fresh(f"{what}, after the next pass")
        assert T.net._wt_key == T.net._derived_key()


def test_adam_groups_joint_group_takes_adam_multi(N, math_mode):
    """One group over two networks with separate storage: two segments, so no fused plan -- sgan_adam_multi with both segments in
    one launch, `_wt_epoch` moved on, and the derived copies re-made lazily by the next pass."""
    from supervised_gan_amd.optim import AdamGroups
    Ts = [Net(N, "G", 9), Net(N, "D", 10)]
    opt = AdamGroups([{"name": "both", "params": [p for T in Ts for p in T.net.parameters()], "lr": 2e-4}], betas=(0.5, 0.999))
    o = opt.optimizers[0]
    assert len(o._segs) == 2 and o._fused_plan() is None
    order = [next(i for i, T in enumerate(Ts) if T.net._flat.data_ptr() == seg[0].data_ptr()) for seg in o._segs]
    Rs = [AdamRef(T.flat()) for T in Ts]
    for T in Ts:
        T.backward()                                     # the first pass makes the derived copies
    for step in range(1, 3):
        if step > 1:
            opt.zero_grad()
            for T in Ts:
                T.backward()
        gs = [T.gflat() for T in Ts]
        epochs = [getattr(T.net, "_wt_epoch", 0) for T in Ts]
        opt.step()
        torch.cuda.synchronize()
        for seg, i in enumerate(order):
            Rs[i].step(gs[i])
            Rs[i].check(Ts[i], o, seg, f"AdamGroups joint, net {i}, step {step}")
            assert np.array_equal(Ts[i].gflat().view(np.int32), gs[i].view(np.int32))
        assert all(getattr(T.net, "_wt_epoch", 0) > e for T, e in zip(Ts, epochs))
        opt.zero_grad()
        _stale_then_refreshed(Ts, f"AdamGroups joint step {step}")


def test_adam_groups_one_group_per_network(N):
    """As the two-stage trainers build it: one group (one FusedAdam, its own learning rate and step counter) per network -- each is
    a single arena and takes the one-launch path."""
    from supervised_gan_amd.optim import AdamGroups
    Ts = [Net(N, "G", 11), Net(N, "D", 12)]
    lrs = A.as_f32(2e-4, 5e-5)
    opt = AdamGroups([{"name": f"n{i}", "params": T.net.parameters(), "lr": lr} for i, (T, lr) in enumerate(zip(Ts, lrs))], lr=1e-3, betas=(0.5, 0.999))
    assert [g["lr"] for g in opt.param_groups] == list(lrs) and [g["name"] for g in opt.param_groups] == ["n0", "n1"]
    Rs = [AdamRef(T.flat(), lr) for T, lr in zip(Ts, lrs)]
    for step in range(1, 3):
        opt.zero_grad()
        for T in Ts:
            T.backward()
        gs = [T.gflat() for T in Ts]
        assert all(o._fused_plan() is not None for o in opt.optimizers)
        opt.step()
        torch.cuda.synchronize()
        for T, R, o, g in zip(Ts, Rs, opt.optimizers, gs):
            R.step(g)
            R.check(T, o, 0, f"AdamGroups per net step {step}")
            T.assert_derived_fresh(f"step {step}")
            assert T.net._wt_key == T.net._derived_key()
    assert opt.step_count == 2


def test_fused_sgd_momentum(N, math_mode):
    """FusedSGD (momentum 0.9) = sgan_sgd_multi: parameters and momentum buffer against sgd_step on the snapshotted gradients (the
    same 4 x rule against sgd_step_f32), padded positions, `_wt_epoch`, the lazy repack."""
    from supervised_gan_amd.optim import FusedSGD
    T = Net(N, "D", 13)
    lr, mu = A.as_f32(1e-3, 0.9)
    opt = FusedSGD(list(T.net.parameters()), lr=lr, momentum=mu)
    p0 = T.flat()
    ref, f32 = (p0.astype(np.float64), None), (p0.copy(), None)
    T.backward()
    for step in range(1, 4):
        if step > 1:
            opt.zero_grad()
            T.backward()
        g = T.gflat()
        epoch = getattr(T.net, "_wt_epoch", 0)
        opt.step()
        torch.cuda.synchronize()
        ref, f32 = A.sgd_step(ref[0], g, ref[1], lr, mu), A.sgd_step_f32(f32[0], g, f32[1], lr, mu)
        got = (T.flat(), opt._m[0].cpu().numpy())
        dev, yard = A.deviation(got, ref), A.deviation(f32, ref)
        print(f"FusedSGD step {step}: deviation from fp64 {dev} | fp32 yardstick {yard}")
        assert all(np.isfinite(d) and d <= A.YARDSTICK_FACTOR * y for d, y in zip(dev, yard)), (step, dev, yard)
        assert float(np.abs(ref[0] - p0).max()) > 100 * A.YARDSTICK_FACTOR * yard[0]      # a step is far above the bound
        assert not got[0][T.padded].any()
        assert np.array_equal(T.gflat().view(np.int32), g.view(np.int32))
        assert getattr(T.net, "_wt_epoch", 0) > epoch
        opt.zero_grad()
        _stale_then_refreshed([T], f"FusedSGD step {step}")

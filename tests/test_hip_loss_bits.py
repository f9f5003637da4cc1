"""The loss kernels bit for bit: every entry point that reduces through sgan_reduce.h (the workgroup sum, the slot / ticket hand-off,
the BCE arithmetic) on inputs from a fixed numpy seed, compared on the raw bits with tests/golden/loss_bits.npz.  The golden was
recorded on an MI355X with the library built from csrc/ of commit 81a09a0 ("State each trainer's step once; run and capture the same
program"), the last one whose kernels each carried their own copy of the reduction.  `python tests/test_hip_loss_bits.py OUT.npz`
records.

Every case runs twice in a row on the same workspace: the second run finds the ticket where the first left it and must give the
same bits.  After each call the words behind the slots (the ticket) are zero, as read back, never as written by the test; the
seg-head kernels zero their slots too, so there the whole workspace is.  The gan / factd / bce_weighted kernels leave their fp64
partials in the slots: those are compared with the golden like every other output (and cleared, the ticket left alone, so that a
call with fewer workgroups shows its own).

An output of up to 4096 bytes is stored as it is; a larger one as the SHA-256 of its bytes (a committed file stays under 1 MiB).
Either way the comparison is numpy.array_equal on bytes.  sg_ce_fwd_kernel adds its workgroups' fp64 sums with atomics, in any
order: with several workgroups its loss must be the golden's or an fp32 neighbour of it, and ce_bwd is compared after one-workgroup
forwards only.

That the file can fail, shown on the library of commit 81a09a0 with one change each:
  * every `(w0 + w1) + (w2 + w3)` written as `((w0 + w1) + w2) + w3`: 14 cases fail, among them
    bce_weighted_C1_ld1, factd_up2_mse_n1 and gan_multi_m1_n3_nograd (the fp64 partials in the slots, and losses through them)
  * every `fmaxf(log.., -100.f)` without its clamp: 30 cases fail, among them
    gan_multi_m0_n1_nograd, gan_single_m0_1x1, factd_up1_bce_n1, bce_weighted_C3_ld4, seg_head_sigmoid_ld5 and image_losses_10x10
"""
import hashlib
import os
import sys
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "loss_bits.npz")
EXTREMES = np.array([40, -40, 30, -30, 100, -100, 17, -17], dtype=np.float32)      # the -100 clamp of the logs, the 1e-12 clamp of p (1 - p)
SMALL, BIG = (15, 20), (363, 362)      # seg head: one workgroup and a half; 131 406 pixels, past the 512-workgroup cap


def pack(a):
    raw = np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).reshape(-1).view(np.uint8)
    return raw.copy() if raw.size <= 4096 else np.frombuffer(hashlib.sha256(raw.tobytes()).digest(), dtype=np.uint8).copy()


class Ctx:
    """What a case needs: its random stream, the device, tensors from arrays, and the workspaces it touched."""

    def __init__(self, name, dev):
        self.rng = np.random.RandomState(zlib.crc32(name.encode()))
        self.dev = dev
        self.touched = {}

    def T(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def normal(self, H, W, C, ld, scale=3.0, extremes=True):
        """[H, W, ld] fp32 buffer: normal * scale in the C logical channels (the first of them the EXTREMES), zeros behind"""
        a = np.zeros((H, W, ld), dtype=np.float32)
        a[..., :C] = self.rng.standard_normal((H, W, C)).astype(np.float32) * scale
        if extremes:
            flat = a.reshape(-1, ld)
            k = min(len(EXTREMES), flat.shape[0])
            flat[:k, 0] = EXTREMES[:k]
        return self.T(a)

    def sentinel(self, H, W, ld):
        return torch.full((H, W, ld), 7.0, dtype=torch.float32, device=self.dev)

    def scalar(self, v=7.0):
        return torch.full((), v, dtype=torch.float32, device=self.dev)

    def labels(self, H, W, C):
        """int64 label map with torch's ignore_index and an out-of-range class in it"""
        lab = self.rng.randint(0, C, size=(H, W)).astype(np.int64)
        lab[0, :3] = -100
        lab[-1, -2:] = C
        return self.T(lab.reshape(-1))

    def ws(self, key, nbytes, nslots, slots_zeroed):
        from supervised_gan_amd import ops
        w = ops._zeroed_workspace(key, self.dev, nbytes)
        self.touched[key] = (w, nslots, slots_zeroed)
        return w


def sync_and_check_workspaces(cx, out, tag):
    torch.cuda.synchronize()
    for key, (w, nslots, slots_zeroed) in cx.touched.items():
        bits = w.view(torch.int64).cpu().numpy()
        assert not bits[nslots:].any(), f"{key}: the ticket is not back at zero"
        if slots_zeroed:
            assert not bits.any(), f"{key}: the workspace is not left zeroed"
        out[f"{tag}ws_{key}"] = bits[:nslots]
        if not slots_zeroed:
            w[:nslots].zero_()      # the next call may use fewer slots than this one


# ------------------------------------------------------------------------------------------------
# cases: name -> function(cx) -> {output name: tensor or array}
# ------------------------------------------------------------------------------------------------
GAN_SIZES = [(1, 1), (67, 67), (130, 127), (5, 7), (35, 35), (19, 21), (2, 3), (9, 9)]      # 130 x 127 = 16 510: past one 16 * 256 * 4 sweep
GAN_TARGETS = [1.0, 0.0, 1.0, 0.0, 0.9, 0.1, 1.0, 0.0]
GAN_WEIGHTS = [0.5, 0.25, 2.0, -0.6, 1.0, 0.125, 3.0, 0.75]


def gan_multi(mode, n, grads):
    def run(cx):
        from supervised_gan_amd import ops
        ws = cx.ws("gan_loss", ops.GAN_LOSS_WS_BYTES, 8 * 16, False)
        ld = 4 if n == 3 else 1
        lg = [cx.normal(h, w, 1, ld) for h, w in GAN_SIZES[:n]]
        dld = {"nograd": 0, "dld1": 1, "dld4": 4}[grads]

        def once(out, tag):
            ds = [cx.sentinel(h, w, dld) for h, w in GAN_SIZES[:n]] if dld else None
            each, total = torch.full((n,), 7.0, device=cx.dev), cx.scalar()
            ops.gan_loss_multi_fwd(lg, GAN_TARGETS[:n], GAN_WEIGHTS[:n], mode, each, total, ds)
            sync_and_check_workspaces(cx, out, tag)
            out.update({f"{tag}each": each, f"{tag}total": total})
            for i, d in enumerate(ds or []):
                out[f"{tag}d{i}"] = d
            if n == 3 and dld == 1:      # the gradients again for an upstream gradient of 0.37
                ds2 = [cx.sentinel(h, w, 1) for h, w in GAN_SIZES[:n]]
                ops.gan_loss_multi_bwd(lg, GAN_TARGETS[:n], GAN_WEIGHTS[:n], mode, cx.scalar(0.37), ds2)
                for i, d in enumerate(ds2):
                    out[f"{tag}bwd{i}"] = d
        ws.zero_()
        return once
    return run


def gan_single(mode, shape, dld):
    def run(cx):
        from supervised_gan_amd import ops
        H, W = shape
        lg = cx.normal(H, W, 1, 1)

        def once(out, tag):
            loss, p, d = cx.scalar(), cx.sentinel(H, W, 1), cx.sentinel(H, W, dld)
            ops.gan_loss_fwd(lg, 0.9, mode, loss, p if mode == 0 else None)
            ops.gan_loss_bwd(lg, 0.9, mode, cx.scalar(0.37), d)
            out.update({f"{tag}loss": loss, f"{tag}p": p, f"{tag}d": d})
        return once
    return run


FACTD_SHAPES = [((5, 7), (13, 16)), ((35, 33), (70, 66))]      # reflection pad on every side; 4620 pixels, past one 16 * 256 sweep


def factd(up, mode, n):
    def run(cx):
        from supervised_gan_amd import ops
        ws = cx.ws("factd_loss", ops.FACTD_LOSS_WS_BYTES, 8 * 16, False)
        shapes = [FACTD_SHAPES[(i + 1) % 2] for i in range(n)]
        scale = 3.0 if mode == (1, 1, 0) else 1.0
        l1s = [cx.normal(a[0], a[1], 1, 1, scale) for a, _ in shapes]
        l2s = [cx.normal(b[0], b[1], 1, 4, scale) for _, b in shapes]
        m = ops.factd_mode(*mode)
        args = (l1s, l2s, [up] * n, GAN_TARGETS[:n], GAN_WEIGHTS[:n], m)

        def once(out, tag):
            each, total = torch.full((n,), 7.0, device=cx.dev), cx.scalar()
            d1 = [cx.sentinel(a[0], a[1], 1) for a, _ in shapes]
            d2 = [cx.sentinel(b[0], b[1], 4) for _, b in shapes]
            assert ops.factd_loss_multi_fwd(*args, each, total, d1, d2)
            sync_and_check_workspaces(cx, out, tag)
            out.update({f"{tag}each": each, f"{tag}total": total})
            e1 = [cx.sentinel(a[0], a[1], 1) for a, _ in shapes]
            e2 = [cx.sentinel(b[0], b[1], 4) for _, b in shapes]
            ops.factd_loss_multi_bwd(*args, cx.scalar(0.37), e1, e2)
            for i in range(n):
                out.update({f"{tag}dl1_{i}": d1[i], f"{tag}dl2_{i}": d2[i], f"{tag}bwd1_{i}": e1[i], f"{tag}bwd2_{i}": e2[i]})
        ws.zero_()
        return once
    return run


def probabilities(cx, H, W, C, ld):
    """[H, W, ld]: sigmoid(normal * 3) in the logical channels, an exact 0 and an exact 1 among them"""
    a = np.zeros((H, W, ld), dtype=np.float32)
    a[..., :C] = 1.0 / (1.0 + np.exp(-cx.rng.standard_normal((H, W, C)).astype(np.float32) * 3))
    a[0, 0, 0], a[0, 1, 0] = 0.0, 1.0
    return cx.T(a)


def targets01(cx, H, W, C, ld):
    a = np.zeros((H, W, ld), dtype=np.float32)
    a[..., :C] = (cx.rng.uniform(size=(H, W, C)) < 0.4).astype(np.float32)
    return cx.T(a)


def bce_weighted(C, ld):
    def run(cx):
        from supervised_gan_amd import ops
        ws = cx.ws("bce_weighted", ops.BCE_WEIGHTED_WS_BYTES, 64, False)
        cw = cx.T(cx.rng.uniform(0.5, 5.0, size=C).astype(np.float32))
        data = [(H, W, probabilities(cx, H, W, C, ld), targets01(cx, H, W, C, ld)) for H, W in ((10, 20), (130, 127))]   # one workgroup; past the 64-workgroup cap

        def once(out, tag):
            for H, W, p, t in data:
                for nw in (0, C):
                    loss, dp = cx.scalar(), cx.sentinel(H, W, ld)
                    ops.bce_weighted_fwd(p, t, C, cw if nw else None, nw, loss)
                    sync_and_check_workspaces(cx, out, f"{tag}{H}x{W}_nw{nw}_")
                    ops.bce_weighted_bwd(p, t, C, cw if nw else None, nw, cx.scalar(0.37), dp)
                    out.update({f"{tag}{H}x{W}_nw{nw}_loss": loss, f"{tag}{H}x{W}_nw{nw}_dp": dp})
        ws.zero_()
        return once
    return run


SEG_C = {4: 3, 8: 7, 12: 12, 16: 16, 5: 5}      # storage channels -> logical channels; 5: no 16-byte rows, the scalar form


def seg_head(mode, ld):
    def run(cx):
        from supervised_gan_amd import ops
        C = SEG_C[ld]
        softmax = mode == "softmax"
        wh = cx.ws("seghead_head", ops.SEGHEAD_WS_BYTES, 512, True)
        wn = cx.ws("seghead_norm", ops.SEGHEAD_WS_BYTES, 512, True)
        cw = cx.T(cx.rng.uniform(0.5, 5.0, size=C).astype(np.float32))
        data = []
        for H, W in (SMALL, BIG):
            z = cx.normal(H, W, C, ld, 1.5 if softmax else 3.0)
            data.append((H, W, z, cx.labels(H, W, C) if softmax else targets01(cx, H, W, C, ld)))

        def once(out, tag):
            for H, W, z, lt in data:
                for weighted in (False, True):
                    k = f"{tag}{H}x{W}_{'w' if weighted else 'u'}_"
                    norm = None
                    if softmax:
                        norm = cx.scalar()
                        ops.label_weight_sum(lt, C, cw if weighted else None, norm)
                        out[k + "norm"] = norm
                    for with_dz in (True, False):
                        p, dz, loss = cx.sentinel(H, W, ld), cx.sentinel(H, W, ld) if with_dz else None, cx.scalar()
                        assert ops.seg_head(z, C, ops.SEGHEAD_SOFTMAX if softmax else ops.SEGHEAD_SIGMOID, lt, cw if weighted else None,
                                            C if weighted else 0, norm, p, dz, loss)
                        sync_and_check_workspaces(cx, out, k + ("dz_" if with_dz else "nodz_"))
                        out.update({k + f"p{int(with_dz)}": p, k + f"loss{int(with_dz)}": loss})
                        if with_dz:
                            out[k + "dz"] = dz
        wh.zero_()
        wn.zero_()
        return once
    return run


def image_losses(shape):
    def run(cx):
        from supervised_gan_amd import ops
        H, W = shape
        C, ld = 2, 4
        x, y = torch.tanh(cx.normal(H, W, C, ld, 1.0, False)), torch.tanh(cx.normal(H, W, C, ld, 1.0, False))
        x[0, 0, 0], x[0, 1, 0], y[0, 2, 0], y[0, 3, 0] = 1.0, -1.0, 1.0, -1.0      # BCE on (x + 1) / 2: p = 1 and p = 0
        a = torch.tanh(cx.normal(H, W, 3, 4, 1.0, False))
        wts = cx.T(np.array([2.0, 5.0, 0.5], dtype=np.float32))
        wmap = cx.T(cx.rng.uniform(0.5, 3.0, size=(H, W, 1)).astype(np.float32))

        def once(out, tag):
            for name, aa, ww, nw in (("label3", a, wts, 3), ("map", wmap, None, 0), ("plain", None, None, 0)):
                loss, g = cx.scalar(), cx.sentinel(H, W, ld)
                ops.l1w_fwd(x, y, C, aa, ww, nw, 10.0, loss, g)
                out.update({f"{tag}l1w_{name}_loss": loss, f"{tag}l1w_{name}_g": g})
            loss, g = cx.scalar(), cx.sentinel(H, W, ld)
            ops.bce01_fwd(x, y, C, loss, g)
            out.update({f"{tag}bce01_loss": loss, f"{tag}bce01_g": g})
        return once
    return run


NEIGHBOUR = "ce_70x66"      # the case whose fp64 sums arrive in any order


def ce(shape):
    def run(cx):
        from supervised_gan_amd import ops
        H, W = shape
        C, ld = 5, 8
        z = cx.normal(H, W, C, ld, 1.5)
        lab = cx.labels(H, W, C)
        cw = cx.T(cx.rng.uniform(0.5, 5.0, size=C).astype(np.float32))
        one_workgroup = H * W <= 256

        def once(out, tag):
            for name, label, const, w in (("lab_w", lab, 0, cw), ("lab_u", lab, 0, None), ("const", None, 2, cw)):
                acc = torch.zeros(3, dtype=torch.float64, device=cx.dev)
                loss, d = cx.scalar(), cx.sentinel(H, W, ld)
                ops.ce_fwd(z, C, label, const, w, acc, loss)
                out[f"{tag}{name}_loss"] = loss
                torch.cuda.synchronize()
                assert int(acc.view(torch.int64)[2]) == 0, "the ticket is not back at zero"
                if one_workgroup:
                    ops.ce_bwd(z, C, label, const, w, acc, cx.scalar(0.37), d)
                    out.update({f"{tag}{name}_acc": acc[:2].clone(), f"{tag}{name}_d": d})
        return once
    return run


CASES = {}
for _mode in (0, 1):
    for _n in (1, 3, 8):
        for _g in ("nograd", "dld1", "dld4"):
            CASES[f"gan_multi_m{_mode}_n{_n}_{_g}"] = gan_multi(_mode, _n, _g)
    for _shape, _dld in (((1, 1), 1), ((33, 31), 4), ((67, 67), 1)):      # 1, 1023 and 4489 pixels
        CASES[f"gan_single_m{_mode}_{_shape[0]}x{_shape[1]}"] = gan_single(_mode, _shape, _dld)
for _up in (1, 2):
    for _mname, _m in (("bce", (1, 1, 0)), ("mse", (0, 0, 1))):
        for _n in (1, 8):
            CASES[f"factd_up{_up}_{_mname}_n{_n}"] = factd(_up, _m, _n)
for _C, _ld in ((1, 1), (1, 4), (1, 16), (3, 3), (3, 4), (3, 16), (16, 16)):
    CASES[f"bce_weighted_C{_C}_ld{_ld}"] = bce_weighted(_C, _ld)
for _mode in ("softmax", "sigmoid"):
    for _ld in (4, 8, 12, 16, 5):
        CASES[f"seg_head_{_mode}_ld{_ld}"] = seg_head(_mode, _ld)
for _shape in ((10, 10), (257, 256)):      # 100 pixels; past the 256-workgroup cap
    CASES[f"image_losses_{_shape[0]}x{_shape[1]}"] = image_losses(_shape)
CASES["ce_10x20"] = ce((10, 20))
CASES[NEIGHBOUR] = ce((70, 66))


def run_case(name, dev):
    """Both runs of a case, packed: ({key: bytes} of the first, of the second)."""
    from supervised_gan_amd import _lib
    _lib.lib()
    cx = Ctx(name, dev)
    once = CASES[name](cx)
    runs = []
    for _ in range(2):
        out = {}
        once(out, "")
        torch.cuda.synchronize()
        runs.append({k: pack(v) for k, v in out.items()})
    return runs


def same_or_fp32_neighbour(a, b):
    return a.size == 4 and b.size == 4 and abs(int(a.view(np.int32)[0]) - int(b.view(np.int32)[0])) <= 1


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("name", list(CASES))
def test_loss_bits(name, golden):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need an MI355X; no CUDA/HIP device is visible")
    first, second = run_case(name, torch.device("cuda", 0))
    want = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "/")}
    assert len(want) > 0 and sorted(want) == sorted(first) == sorted(second)
    bad = []
    for k in sorted(want):
        for run, got in (("first", first[k]), ("second", second[k])):
            ok = np.array_equal(got, want[k]) or (name == NEIGHBOUR and same_or_fp32_neighbour(got, want[k]))
            if not ok:
                bad.append(f"{k} ({run} run)")
    assert not bad, f"{len(bad)} outputs differ from the golden: " + ", ".join(bad[:12])


if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    dev = torch.device("cuda", 0)
    out = {}
    for name in CASES:
        first, second = run_case(name, dev)
        for k in first:
            assert np.array_equal(first[k], second[k]) or name == NEIGHBOUR, (name, k)
            out[f"{name}/{k}"] = first[k]
    np.savez_compressed(sys.argv[1], **out)
    print(len(CASES), "cases,", len(out), "outputs,", os.path.getsize(sys.argv[1]), "bytes")

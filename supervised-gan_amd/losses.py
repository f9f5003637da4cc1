"""Losses and small differentiable ops of the trainers on the MI355X path (models/networks.py:152-214 GANLoss / GANLossMultiClass /
WeightedL1Loss; the (label, image) pair concat, BCE on rescaled tanh outputs, bilinear x2 upsampling, the factored-discriminator loss,
the channel sigmoid and weighted BCE of `--use_sigmoid_ss`): one kernel forward, one backward."""
from __future__ import annotations

import math
import os
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._lib import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH, CONV, CONVT, SganError
from .ops import pad4


class _GanLossFn(torch.autograd.Function):
    """Sigmoid + BCELoss(mean) (or MSELoss) against a constant target, on the logits map."""

    @staticmethod
    def forward(ctx, logits, target, mode):
        lb = ops.as_nhwc(logits)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        ops.gan_loss_fwd(lb, target, mode, loss)
        ctx.lb, ctx.target, ctx.mode = lb, target, mode
        return loss

    @staticmethod
    def backward(ctx, gout):
        d = torch.empty_like(ctx.lb)
        ops.gan_loss_bwd(ctx.lb, ctx.target, ctx.mode, gout.contiguous(), d)
        return ops.logical_view(d, 1), None, None


class _CatPairFn(torch.autograd.Function):
    """torch.cat((a, b), 1) of two logical [1, C, H, W] tensors as ONE kernel that writes the padded NHWC buffer the discriminators
    read (no CatArrayBatchedCopy + layout pass), and one slice kernel per member that needs a gradient in backward."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.Ca, ctx.Cb = a.shape[1], b.shape[1]
        out = ops.concat_nhwc(ops.as_nhwc(a), ctx.Ca, ops.as_nhwc(b), ctx.Cb)
        # autograd hands the caller a detached alias of a differentiable view output; the buffer object must outlive this call
        # for that alias to map back to it without a copy (ops.as_nhwc looks the buffer up by address)
        ctx.out = out
        return ops.logical_view(out, ctx.Ca + ctx.Cb)

    @staticmethod
    def backward(ctx, g):
        gb = ops.as_nhwc(g)
        ga = ops.logical_view(ops.slice_nhwc(gb, 0, ctx.Ca), ctx.Ca) if ctx.needs_input_grad[0] else None
        gbb = ops.logical_view(ops.slice_nhwc(gb, ctx.Ca, ctx.Cb), ctx.Cb) if ctx.needs_input_grad[1] else None
        return ga, gbb


def cat_pair(a, b):
    """The conditional discriminators' input cat((label, image), 1) (models/cgan_model.py:162,172,187) on the HIP path; anything
    that is not a batch-1 fp32 device pair goes to torch.cat."""
    if a.is_cuda and b.is_cuda and a.dim() == 4 and a.shape[0] == 1 and a.shape[2:] == b.shape[2:] and a.dtype == b.dtype == torch.float32:
        return _CatPairFn.apply(a, b)
    return torch.cat((a, b), 1)


class _GanLossMultiFn(torch.autograd.Function):
    """total = sum_i w_i * GANLoss(pred_i, target_i) -- ONE kernel for all terms, their finish and (when a gradient will be asked
    for) d total / d pred_i for an upstream gradient of 1.  backward() hands those out as they are when the upstream gradient is
    the trainers' cached unit gradient (ops.register_unit_grad), and rescales them with one more kernel per term otherwise."""

    @staticmethod
    def forward(ctx, targets, weights, mode, *logits):
        lbs = [ops.as_nhwc(l) for l in logits]
        dev = logits[0].device
        each = torch.empty(len(lbs), dtype=torch.float32, device=dev)
        total = torch.empty((), dtype=torch.float32, device=dev)
        ds = [torch.empty_like(lb) for lb in lbs] if any(ctx.needs_input_grad[3:]) else None
        ops.gan_loss_multi_fwd(lbs, targets, weights, mode, each, total, ds)
        ctx.ds = ds
        ctx.mark_non_differentiable(each)
        ctx.set_materialize_grads(False)      # or autograd zero-fills a gradient for `each` on every backward (one more launch)
        return total, each

    @staticmethod
    def backward(ctx, gtotal, _geach):
        ds = ctx.ds
        if gtotal is None:
            return (None,) * (3 + len(ds))
        if not ops.is_unit_grad(gtotal):
            scaled = [torch.empty_like(d) for d in ds]
            g = gtotal.contiguous()
            for d, o in zip(ds, scaled):
                ops.scale(g, d, o)
            ds = scaled
        return (None, None, None) + tuple(ops.logical_view(d, 1) for d in ds)


def _logits_behind(out, use_lsgan, who):
    """The logits behind a discriminator output: the output itself for lsgan, the tagged logits otherwise."""
    if use_lsgan:
        return out
    logits = getattr(out, "_sgan_logits", None)
    if logits is None and getattr(out, "_sgan_pending_sigmoid", False):
        logits = out
    if logits is None:
        raise SganError(f"{who}(use_lsgan=False) needs the output of a supervised_gan_amd discriminator built with "
                        "use_sigmoid=True (it carries its logits); got a plain tensor")
    return logits


class GANLoss(nn.Module):
    """GANLoss (models/networks.py:152-185).  With `use_lsgan=False` the reference applies BCELoss to
    the discriminator's Sigmoid output; here the loss kernel consumes the logits behind that output
    (numerically the same function, torch's -100 log clamp included)."""

    def __init__(self, use_lsgan=True, target_real_label=1.0, target_fake_label=0.0, tensor=torch.FloatTensor):
        super().__init__()
        self.real_label = target_real_label
        self.fake_label = target_fake_label
        self.use_lsgan = use_lsgan
        self.Tensor = tensor

    def _logits_of(self, input):
        return _logits_behind(input, self.use_lsgan, "GANLoss")

    def __call__(self, input, target_is_real):
        t = self.real_label if target_is_real else self.fake_label
        return _GanLossFn.apply(self._logits_of(input), t, 1 if self.use_lsgan else 0)

    def weighted_sum(self, inputs, targets_are_real, weights):
        """sum_i weights[i] * self(inputs[i], targets_are_real[i]) as ONE autograd node (<= 8 terms): returns
        (total, each) where `each` holds the unweighted terms for logging."""
        ts = [self.real_label if r else self.fake_label for r in targets_are_real]
        return _GanLossMultiFn.apply(ts, [float(w) for w in weights], 1 if self.use_lsgan else 0,
                                     *[self._logits_of(i) for i in inputs])


# ------------------------------------------------------------------------------------------------
# factored discriminators (`--model twostage_factd`): D2_i's map times D1_i's, upsampled and reflection-padded (util.mul)
# ------------------------------------------------------------------------------------------------
def factd_pad_split(dH, dW):
    """(left, right, top, bottom) of util.mul (util/util.py:140-144) for a map that is dH rows and dW columns short: the left and
    the bottom take the floor of the half, the right and the top the remainder."""
    pl, pb = int(dW / 2), int(dH / 2)
    return pl, dW - pl, dH - pb, pb


def factored_product(in1, in2):
    """util.mul (util/util.py:131-145): in1 reflection-padded up to in2's size, times in2; the reference returns None when in1 is
    the larger one."""
    if in1.shape == in2.shape:
        return in1 * in2
    if not (in1.shape[2] <= in2.shape[2] and in1.shape[3] <= in2.shape[3]):
        raise ValueError("twostage_factd: the upsampled D1 map %s is larger than D2's %s (the reference's util.mul returns None here); "
                         "choose --n_layers_D1 / --n_layers_D2 so that it is not" % (tuple(in1.shape[2:]), tuple(in2.shape[2:])))
    return F.pad(in1, factd_pad_split(in2.shape[2] - in1.shape[2], in2.shape[3] - in1.shape[3]), mode='reflect') * in2


def factored_gan_loss_composed(l1s, l2s, targets, weights, up, sig1, sig2, mse):
    """The factored terms as a composition of torch calls -- what the trainer ran before sgan_factd_loss_multi_fwd and what
    factored_gan_loss still runs for a call the kernel does not cover: (total, each)."""
    each = []
    for l1, l2, t in zip(l1s, l2s, targets):
        a1 = torch.sigmoid(l1) if sig1 else l1
        a2 = torch.sigmoid(l2) if sig2 else l2
        if up == 2:
            a1 = F.interpolate(a1, scale_factor=2, mode='bilinear', align_corners=False)
        pred = factored_product(a1, a2)
        tgt = torch.full_like(pred, float(t))
        each.append(F.mse_loss(pred, tgt) if mse else F.binary_cross_entropy(pred, tgt))
    total = sum(e * float(w) for e, w in zip(each, weights))
    return total, torch.stack([e.detach() for e in each])


class _FactdNotCovered(Exception):
    pass


class _FactdLossMultiFn(torch.autograd.Function):
    """total = sum_i w_i * crit(mul(transform(act(l1_i)), act(l2_i)), target_i) -- ONE kernel for all terms (<= 8), their finish and,
    for every logits map that needs one, d total / d l for an upstream gradient of 1 (_GanLossMultiFn's contract).  backward()
    hands those out as they are under the trainers' cached unit gradient and has the kernel's second entry point write them again
    for any other upstream gradient.  `logits`: l1_0 .. l1_{n-1}, l2_0 .. l2_{n-1}."""

    @staticmethod
    def forward(ctx, targets, weights, mode, up, *logits):
        n = len(logits) // 2
        lbs = [ops.as_nhwc(l) for l in logits]
        dev = logits[0].device
        each = torch.empty(n, dtype=torch.float32, device=dev)
        total = torch.empty((), dtype=torch.float32, device=dev)
        ds = [torch.empty_like(lb) if need else None for lb, need in zip(lbs, ctx.needs_input_grad[4:])]
        ctx.args = (lbs[:n], lbs[n:], [up] * n, targets, weights, mode)
        if not ops.factd_loss_multi_fwd(*ctx.args, each, total, ds[:n], ds[n:]):
            raise _FactdNotCovered()
        ctx.ds = ds
        ctx.mark_non_differentiable(each)
        ctx.set_materialize_grads(False)      # or autograd zero-fills a gradient for `each` on every backward (one more launch)
        return total, each

    @staticmethod
    def backward(ctx, gtotal, _geach):
        ds = ctx.ds
        if gtotal is None:
            return (None,) * (4 + len(ds))
        if not ops.is_unit_grad(gtotal) and any(d is not None for d in ds):
            n = len(ds) // 2
            ds = [torch.empty_like(d) if d is not None else None for d in ds]
            ops.factd_loss_multi_bwd(*ctx.args, gtotal.contiguous().float(), ds[:n], ds[n:])
        return (None, None, None, None) + tuple(ops.logical_view(d, 1) if d is not None else None for d in ds)


def factored_gan_loss(d1_outs, d2_outs, targets_are_real, weights, up=2, use_lsgan1=False, use_lsgan2=False):
    """sum_i weights[i] * crit(util.mul(transform(D1 output i), D2 output i), target i) of the factored discriminators as ONE
    autograd node and one launch (<= 8 terms): returns (total, each), `each` the unweighted terms for logging.

    d1_outs / d2_outs: what the discriminators return under `fuse_sigmoid_into_loss` (tagged logits with use_sigmoid, raw scores
    without); no stand-alone sigmoid is launched.  up: 1 or 2, the `--transform_1to2` step.  crit is BCE without lsgan2, MSE with
    it.  A call the kernel does not cover (more than 8 terms, a pad as large as the map, BCE on anything but two probabilities,
    tensors that are not batch-1 fp32 on the device) runs as the composition of torch calls; an upsampled D1 map larger than D2's
    raises the ValueError of util.mul's None."""
    l1s = [_logits_behind(o, use_lsgan1, "factored_gan_loss") for o in d1_outs]
    l2s = [_logits_behind(o, use_lsgan2, "factored_gan_loss") for o in d2_outs]
    assert len(l1s) == len(l2s) == len(targets_are_real) == len(weights) and len(l1s) >= 1
    assert up in (1, 2), "--transform_1to2: None or bilinear_2"
    for a, b in zip(l1s, l2s):
        if a.shape[2] * up > b.shape[2] or a.shape[3] * up > b.shape[3]:
            factored_product(a.new_empty((1, 1, a.shape[2] * up, a.shape[3] * up), device="meta"), b)       # raises
    ts = [1.0 if r else 0.0 for r in targets_are_real]
    ws = [float(w) for w in weights]
    sig1, sig2, mse = not use_lsgan1, not use_lsgan2, bool(use_lsgan2)
    on_dev = all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.shape[0] == 1 and t.shape[1] == 1 for t in l1s + l2s)
    if on_dev:
        try:
            return _FactdLossMultiFn.apply(ts, ws, ops.factd_mode(sig1, sig2, mse), int(up), *l1s, *l2s)
        except _FactdNotCovered:
            pass
    return factored_gan_loss_composed(l1s, l2s, ts, ws, up, sig1, sig2, mse)


class _CEFn(torch.autograd.Function):
    """Class-weighted cross-entropy of a [1, C, H, W] logits map against an int64 label map [1, H, W] (or one class for every
    pixel): sgan_ce_fwd / sgan_ce_bwd.  The forward keeps nothing but the two fp64 sums; the backward recomputes the softmax."""

    @staticmethod
    def forward(ctx, logits, label, const_label, class_w):
        zb = ops.as_nhwc(logits)
        acc = ops.stat_arena(3, logits.device)      # [sum w nll, sum w, ticket]; zeroed
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        lab = label.reshape(-1).contiguous() if label is not None else None
        ops.ce_fwd(zb, logits.shape[1], lab, const_label, class_w, acc, loss)
        ctx.zb, ctx.lab, ctx.cl, ctx.cw, ctx.acc, ctx.C = zb, lab, const_label, class_w, acc, logits.shape[1]
        return loss

    @staticmethod
    def backward(ctx, gout):
        dz = torch.empty_like(ctx.zb)
        ops.ce_bwd(ctx.zb, ctx.C, ctx.lab, ctx.cl, ctx.cw, ctx.acc, gout.contiguous().float(), dz)
        return ops.logical_view(dz, ctx.C), None, None, None


def cross_entropy_logits(logits, label=None, const_label=0, class_weights=None):
    """nn.CrossEntropyLoss(weight=class_weights)(logits, label) for a [1, C, H, W] map on the HIP kernel (C <= 16, batch 1); `label`
    None: every pixel has class `const_label`.  The kernel reads an int64 map: a label map of any other integer type is converted,
    one on another device than the logits raises ValueError.  Anything outside the kernel's envelope (a batch, C > 16, not fp32 on
    the device) goes to F.cross_entropy, like sigmoid_channels.  On both paths a label outside [0, C) is skipped like torch's
    ignore_index -100 (the kernels skip it; in front of F.cross_entropy, which would raise, it is set to -100), and a map that
    is skipped entirely gives 0 with an all-zero gradient."""
    if label is not None:
        if label.device != logits.device:
            raise ValueError(f"cross_entropy_logits: the label map is on {label.device}, the logits are on {logits.device}")
        if label.dtype != torch.int64:
            label = label.long()
    if not _bce_envelope(logits):
        if label is None:
            label = torch.full((logits.shape[0],) + tuple(logits.shape[2:]), int(const_label), dtype=torch.int64, device=logits.device)
        label = torch.where((label < 0) | (label >= logits.shape[1]), torch.full_like(label, -100), label)
        if not bool((label >= 0).any()):      # every pixel skipped: 0 with an all-zero gradient, as the kernel has it (torch: nan)
            return logits.sum() * 0.0
        cw = class_weights.detach().to(logits.dtype) if class_weights is not None else None
        return F.cross_entropy(logits, label, weight=cw, ignore_index=-100)
    cw = class_weights.detach().float().contiguous() if class_weights is not None else None
    return _CEFn.apply(logits, label, int(const_label), cw)


class _SoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits):
        zb = ops.as_nhwc(logits)
        pb = torch.empty_like(zb)
        ops.softmax_fwd(zb, logits.shape[1], pb)
        ctx.pb, ctx.C = pb, logits.shape[1]
        return ops.logical_view(pb, logits.shape[1])

    @staticmethod
    def backward(ctx, g):
        dz = torch.empty_like(ctx.pb)
        ops.softmax_bwd(ops.as_nhwc(g), ctx.pb, ctx.C, dz)
        return ops.logical_view(dz, ctx.C)


def softmax_channels(logits):
    """F.softmax(logits, dim=1) of a [1, C, H, W] map on the HIP kernel (the result is NHWC-backed: the discriminators read it with
    no layout copy).  Anything else (a batch, C > 16, not fp32 on the device) goes to F.softmax, like sigmoid_channels."""
    if not _bce_envelope(logits):
        return F.softmax(logits, dim=1)
    return _SoftmaxFn.apply(logits)


class _SigmoidChannelsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits):
        zb = ops.as_nhwc(logits)
        pb = torch.empty_like(zb)
        ops.sigmoid_nhwc_fwd(zb, logits.shape[1], pb)
        ctx.pb, ctx.C = pb, logits.shape[1]
        return ops.logical_view(pb, logits.shape[1])

    @staticmethod
    def backward(ctx, g):
        dz = torch.empty_like(ctx.pb)
        ops.sigmoid_nhwc_bwd(ops.as_nhwc(g), ctx.pb, ctx.C, dz)
        return ops.logical_view(dz, ctx.C)


def _bce_envelope(t):
    return t.is_cuda and t.dim() == 4 and t.shape[0] == 1 and t.shape[1] <= 16 and t.dtype == torch.float32


def sigmoid_channels(logits):
    """torch.sigmoid(logits) of a [1, C, H, W] map on the HIP kernel (`--use_sigmoid_ss`; NHWC-backed like softmax_channels, so
    cat_pair reads it with no layout copy).  Anything else (a batch, C > 16, not fp32 on the device) goes to torch.sigmoid."""
    if not _bce_envelope(logits):
        return torch.sigmoid(logits)
    return _SigmoidChannelsFn.apply(logits)


class _WeightedBceFn(torch.autograd.Function):
    """mean(w * BCE(p, t)) with w = 1 + sum_{i < nw} t_i (cw_i - 1) built inside the kernel; gradient w.r.t. p only."""

    @staticmethod
    def forward(ctx, p, t, cw, nw):
        pb, tb = ops.as_nhwc(p), ops.as_nhwc(t)
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        ops.bce_weighted_fwd(pb, tb, p.shape[1], cw, nw, loss)
        ctx.pb, ctx.tb, ctx.cw, ctx.nw, ctx.C = pb, tb, cw, nw, p.shape[1]
        return loss

    @staticmethod
    def backward(ctx, gout):
        dp = torch.empty_like(ctx.pb)
        ops.bce_weighted_bwd(ctx.pb, ctx.tb, ctx.C, ctx.cw, ctx.nw, gout.contiguous().float(), dp)
        return ops.logical_view(dp, ctx.C), None, None, None


def weighted_bce(p, t, class_weights=None):
    """F.binary_cross_entropy(p, t, weight=wm) with the weight map wm = 1 + sum_i t[:, i] * (class_weights[i] - 1) of the
    segmentation trainers (models/segm_model.py:216-225) on the HIP kernel; class_weights None: unweighted.  `t` is a constant.
    Outside the kernel's envelope (a batch, C > 16, not fp32 on the device) the torch calls run.  class_weights on another device
    than p raise ValueError, as a label map does in cross_entropy_logits: the kernel would read a host pointer."""
    t = t.detach()
    nw = 0 if class_weights is None else int(class_weights.numel())
    if nw and class_weights.device != p.device:
        raise ValueError(f"weighted_bce: class_weights are on {class_weights.device}, p is on {p.device}")
    if not (_bce_envelope(p) and _bce_envelope(t) and p.shape == t.shape and nw <= p.shape[1]):
        wm = None
        if nw:
            wm = torch.ones_like(t[:, :1])
            for i in range(nw):
                wm = wm + t.narrow(1, i, 1) * (class_weights[i] - 1.0)
        return F.binary_cross_entropy(p, t, weight=wm)
    cw = class_weights.detach().float().contiguous() if nw else None
    return _WeightedBceFn.apply(p, t, cw, nw)


class _SegHeadNotCovered(Exception):
    pass


class _SegHeadFn(torch.autograd.Function):
    """(p, loss) of a segmentation step whose loss is the ONE consumer of the prediction: softmax (or sigmoid) over the channels, the
    class-weighted cross-entropy (or weighted BCE) and d loss / d logits in one launch (sgan_seg_head).  A gradient arriving at p
    has no way into the dlogits the forward wrote, so the backward refuses one."""

    @staticmethod
    def forward(ctx, logits, lt, cw, nw, norm, mode, pixel_add=None):
        zb = ops.as_nhwc(logits)
        C_ = logits.shape[1]
        if mode == ops.SEGHEAD_SOFTMAX:
            lt = lt.reshape(-1).contiguous()
        else:
            lt = ops.as_nhwc(lt)
        pb = torch.empty_like(zb)
        dz = torch.empty_like(zb) if ctx.needs_input_grad[0] else None
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        if not ops.seg_head(zb, C_, mode, lt, cw, nw, norm, pb, dz, loss, pixel_add=pixel_add):
            raise _SegHeadNotCovered()
        ctx.dz, ctx.C = dz, C_
        ctx.pb = pb      # the buffer object outlives this call: the detached alias autograd hands out maps back to it (as _CatPairFn)
        ctx.set_materialize_grads(False)      # no gradient for p is the rule: None, not a zero fill, is what backward sees then
        return ops.logical_view(pb, C_), loss

    @staticmethod
    def backward(ctx, gp, gout):
        assert gp is None, "seg_head: a gradient arrived at p -- the fused head is valid only while the loss is p's one consumer"
        if gout is None or ctx.dz is None:
            return None, None, None, None, None, None, None
        dz = ctx.dz
        if not ops.is_unit_grad(gout):
            dz = torch.empty_like(ctx.dz)
            ops.scale(gout.contiguous().float(), ctx.dz, dz)
        return ops.logical_view(dz, ctx.C), None, None, None, None, None, None


def seg_head(logits, label_or_target, class_weights=None, norm=None, mode=0, pixel_add=None):
    """The loss section of a segmentation step with no discriminator: returns (p, loss).

    mode ops.SEGHEAD_SOFTMAX: p = F.softmax(logits, 1), loss = sum_p w[y_p] nll_p / norm with `label_or_target` the int64 label map
    [1, H, W] on the logits' device and `norm` the device scalar sum_p w[y_p] (ops.label_weight_sum; None: computed here) -- that is
    F.cross_entropy(logits, label, weight=class_weights).  mode ops.SEGHEAD_SIGMOID: p = torch.sigmoid(logits), loss =
    F.binary_cross_entropy(p, target, weight=wm) with wm = 1 + sum_i target[:, i] (class_weights[i] - 1); `norm` is not read.
    pixel_add (softmax mode, on the device): a float32 [H, W] map added to the weight of every labelled pixel, w_p = w[y_p] +
    pixel_add[p] (ops.border_weight's map: the U-Net loss), `norm` then sum_p w_p (ops.pixel_weight_sum; None: computed here).  This
    form has no composition to fall back on: outside the kernel's envelope it raises.

    One launch (sgan_seg_head) writes p, the loss and d loss / d logits; the backward hands the last out times the upstream gradient.
    p comes back NHWC-backed, like softmax_channels': it must have no consumer that sends a gradient back (the backward asserts it;
    read it through .detach(), as the metrics and the visuals do).  Under torch.no_grad() no gradient is written.  Outside the kernel's envelope (a batch, more than 16 channels, not
    fp32 on the device) the existing functions are composed: softmax_channels + cross_entropy_logits on the device, torch calls off it."""
    softmax = mode == ops.SEGHEAD_SOFTMAX
    lt = label_or_target.detach()
    nw = 0 if class_weights is None else int(class_weights.numel())
    if softmax:
        assert lt.dtype == torch.int64 and lt.device == logits.device, "seg_head: the label map is torch.int64 on the logits' device"
    if _bce_envelope(logits) and (softmax or (_bce_envelope(lt) and lt.shape == logits.shape and nw <= logits.shape[1])):
        cw = class_weights.detach().float().contiguous() if nw else None
        if softmax:
            assert lt.numel() == logits.shape[2] * logits.shape[3] and (cw is None or nw == logits.shape[1])
            if pixel_add is not None:
                pixel_add = pixel_add.detach().reshape(-1).contiguous()
            if norm is None:
                norm = torch.empty((), dtype=torch.float32, device=logits.device)
                if pixel_add is not None:
                    ops.pixel_weight_sum(lt.reshape(-1).contiguous(), logits.shape[1], cw, pixel_add, norm)
                else:
                    ops.label_weight_sum(lt.reshape(-1).contiguous(), logits.shape[1], cw, norm)
        else:
            assert pixel_add is None, "seg_head: pixel_add goes with the softmax cross-entropy only"
        try:
            return _SegHeadFn.apply(logits, lt, cw, nw, norm, int(mode), pixel_add)
        except _SegHeadNotCovered:
            pass
    if pixel_add is not None:
        raise SganError("seg_head: the pixel-weighted head covers [1, C <= 16, H, W] fp32 logits on the device only")
    if softmax:
        if logits.is_cuda and logits.dim() == 4 and logits.shape[0] == 1 and logits.shape[1] <= 16 and logits.dtype == torch.float32:
            return softmax_channels(logits), cross_entropy_logits(logits, lt, 0, class_weights)
        return F.softmax(logits, dim=1), F.cross_entropy(logits, lt, weight=class_weights)
    p = sigmoid_channels(logits)
    return p, weighted_bce(p, lt, class_weights)


class ClDiceBuffers:
    """What a soft-clDice node keeps between calls for H x W planes and K = iters: the workspace with the I_j of the forward (read
    again by the backward), the skeleton of the prediction, the state with the sums and scalar derivatives, the loss scalar and the
    gradient plane the node hands out, so that a step allocates nothing.  One node at a time: the backward of a forward must run, and
    its gradient be consumed, before the next forward on the same buffers."""

    def __init__(self, H, W, iters, device):
        self.shape, self.iters = (H, W), int(iters)
        self.work = ops.new_cldice_workspace(H, W, iters, device, backward=True)
        self.sp = torch.empty((H, W), dtype=torch.float32, device=device)
        self.state = ops.new_cldice_state(device)
        self.loss = torch.empty((), dtype=torch.float32, device=device)
        self.dp = torch.empty((H, W), dtype=torch.float32, device=device)

    def fits(self, H, W, iters, device):
        return self.shape == (H, W) and self.iters == int(iters) and self.sp.device == device


class _SoftClDiceFn(torch.autograd.Function):
    """L = 1 - 2 Tprec Tsens / (Tprec + Tsens) of the soft skeletons (sgan_soft_skeleton, sgan_cldice_finish); the backward is
    sgan_cldice_backward, which takes the upstream gradient as a device scalar.  Gradient w.r.t. the probability plane only."""

    @staticmethod
    def forward(ctx, p, t, st, iters, bufs):
        ops.soft_skeleton(p, iters, out=bufs.sp, work=bufs.work)
        ops.cldice_finish(bufs.sp, t, st, p, bufs.state, bufs.loss)
        ctx.t, ctx.st, ctx.iters, ctx.bufs = t, st, iters, bufs
        return bufs.loss.detach()      # an alias of the persistent scalar: the node hangs on a tensor of its own, as _SegHeadFn's p

    @staticmethod
    def backward(ctx, gout):
        if gout is None:
            return None, None, None, None, None
        g = None if ops.is_unit_grad(gout) else gout.contiguous().float()
        dp = ops.cldice_backward(ctx.t, ctx.st, ctx.bufs.state, ctx.iters, ctx.bufs.work, dp=ctx.bufs.dp, gout=g)
        return dp.detach(), None, None, None, None


def soft_cldice(p_plane, t_plane, iters, t_skel=None, buffers=None):
    """The soft-clDice loss (Shit et al., CVPR 2021; util.soft_cldice_ref) of the probability plane p_plane [H, W] against the binary
    truth t_plane [H, W], both fp32 on the device, with K = iters: a float32 device scalar whose backward hands d L / d P times the
    upstream gradient to p_plane.  t_skel: ops.soft_skeleton(t_plane, iters) where the caller keeps it (None: computed here);
    buffers: a ClDiceBuffers the caller keeps between steps (None: made here).  The planes are read where they lie when their
    strides are positive (a channel of an NHWC buffer).  No fallback: off the device or outside 1 .. 16 iterations it raises."""
    ops.require_gpu(p_plane, "soft_cldice")
    assert p_plane.dim() == 2 and p_plane.shape == t_plane.shape and p_plane.dtype == t_plane.dtype == torch.float32, (p_plane.shape, t_plane.shape)
    if not 1 <= int(iters) <= ops.CLDICE_MAX_ITERS:
        raise SganError(f"soft_cldice: not covered ({iters} iterations: 1 .. {ops.CLDICE_MAX_ITERS})")
    H, W = p_plane.shape
    t_plane = t_plane.detach()
    if buffers is None:
        buffers = ClDiceBuffers(H, W, iters, p_plane.device)
    assert buffers.fits(H, W, iters, p_plane.device), (buffers.shape, buffers.iters, (H, W), iters)
    if t_skel is None:
        t_skel = ops.soft_skeleton(t_plane, iters)
    return _SoftClDiceFn.apply(p_plane, t_plane, t_skel.detach(), int(iters), buffers)


def class_probability_plane(logits, cls, use_sigmoid=False):
    """The probability plane [H, W] of class `cls` from the [1, C, H, W] logits, with a gradient path back into them: softmax over the
    channels, or the sigmoid of each under `--use_sigmoid_ss` (softmax_channels / sigmoid_channels, both with HIP backwards).  A
    view into the NHWC-backed prediction: nothing is copied."""
    assert logits.dim() == 4 and logits.shape[0] == 1 and 0 <= int(cls) < logits.shape[1], (logits.shape, cls)
    p = sigmoid_channels(logits) if use_sigmoid else softmax_channels(logits)
    return p[0, int(cls)]


class LovaszBuffers:
    """What a Lovasz-softmax node keeps between calls for a [1, C, H, W] prediction and n listed classes: the workspace with pi, g and
    the scales of the forward (read again by the backward), the loss scalar and the gradient of the whole prediction the node hands
    out, so that a step allocates nothing.  One node at a time, as ClDiceBuffers."""

    def __init__(self, C, H, W, n, device):
        self.shape, self.n = (C, H, W), int(n)
        self.work = ops.new_lovasz_workspace(H, W, n, device)
        self.loss = torch.empty((), dtype=torch.float32, device=device)
        self.dp = torch.empty((1, C, H, W), dtype=torch.float32, device=device)

    def fits(self, C, H, W, n, device):
        return self.shape == (C, H, W) and self.n == int(n) and self.dp.device == device


class _LovaszSoftmaxFn(torch.autograd.Function):
    """L = the mean Lovasz extension of the Jaccard loss over the present listed classes (sgan_lovasz_forward); the backward is
    sgan_lovasz_backward, which takes the upstream gradient as a device scalar and writes the gradient of the whole prediction."""

    @staticmethod
    def forward(ctx, p, label, classes, bufs):
        ops.lovasz_forward(p, label, classes, bufs.work, loss_out=bufs.loss)
        ctx.p, ctx.classes, ctx.bufs = p.detach(), classes, bufs
        return bufs.loss.detach()

    @staticmethod
    def backward(ctx, gout):
        if gout is None:
            return None, None, None, None
        g = None if ops.is_unit_grad(gout) else gout.contiguous().float()
        dp = ops.lovasz_backward(ctx.p, ctx.classes, ctx.bufs.work, dp=ctx.bufs.dp, gout=g)
        return dp.detach(), None, None, None


def lovasz_softmax(p, label, classes, buffers=None):
    """The Lovasz-softmax loss (Berman, Triki, Blaschko, CVPR 2018, classes = 'present'; util.lovasz_ref) of the prediction
    p [1, C, H, W] (fp32 probabilities on the device) against the index label [H, W] (int64) over the listed classes: a float32
    device scalar whose backward hands d L / d p times the upstream gradient to p, zeros in the unlisted channels.  p is read where it
    lies when its strides are positive (the NHWC-backed prediction of the trainer).  buffers: a LovaszBuffers the caller keeps
    between steps (None: made here).  No fallback: off the device, above 2^20 pixels or outside 1 .. 8 classes it raises."""
    ops.require_gpu(p, "lovasz_softmax")
    assert p.dim() == 4 and p.shape[0] == 1 and p.dtype == torch.float32, (p.shape, p.dtype)
    classes = tuple(int(c) for c in classes)
    _, C, H, W = p.shape
    if H * W > ops.LOVASZ_MAX_PIXELS or not 1 <= len(classes) <= ops.LOVASZ_MAX_CLASSES:
        raise SganError(f"lovasz_softmax: not covered ({H} x {W} pixels, {len(classes)} classes: H W <= 2^20, 1 .. {ops.LOVASZ_MAX_CLASSES})")
    if buffers is None:
        buffers = LovaszBuffers(C, H, W, len(classes), p.device)
    assert buffers.fits(C, H, W, len(classes), p.device), (buffers.shape, buffers.n, p.shape, classes)
    return _LovaszSoftmaxFn.apply(p, label.detach(), classes, buffers)


class SegTermsBuffers:
    """What a Tversky / focal node keeps between calls for [1, C, H, W] logits: the fp64 state the forward writes and the backward
    reads, the zeroed workspace of the forward's hand-off, the two loss scalars and the gradient buffer the node hands out, so that
    a step allocates nothing.  One node at a time, as ClDiceBuffers."""

    def __init__(self, C, H, W, device):
        self.shape = (C, H, W)
        self.state = ops.new_seg_terms_state(device)
        self.work = ops.new_seg_terms_workspace(device)
        self.loss_t = torch.zeros((), dtype=torch.float32, device=device)
        self.loss_f = torch.zeros((), dtype=torch.float32, device=device)
        self.dz = torch.empty((H, W, pad4(C)), dtype=torch.float32, device=device)

    def fits(self, C, H, W, device):
        return self.shape == (C, H, W) and self.dz.device == device


class _SegTermsFn(torch.autograd.Function):
    """(L_T, L_F) from the logits in one launch (sgan_seg_terms_forward); the backward is one launch too (sgan_seg_terms_backward): it
    takes the two upstream gradients as device scalars -- a term without one is not taken -- and writes the gradient of the logits."""

    @staticmethod
    def forward(ctx, logits, lt, mode, classes, alpha, beta, smooth, power, gamma, cw, bufs):
        zb = ops.as_nhwc(logits)
        C_ = logits.shape[1]
        lt = lt.reshape(-1).contiguous() if mode == ops.SEGHEAD_SOFTMAX else ops.as_nhwc(lt)
        ops.seg_terms_forward(zb, C_, mode, lt, classes, alpha, beta, smooth, power, gamma, cw, bufs.state, bufs.loss_t, bufs.loss_f, bufs.work)
        ctx.zb, ctx.lt, ctx.C, ctx.mode, ctx.classes, ctx.gamma, ctx.cw, ctx.bufs = zb, lt, C_, mode, classes, gamma, cw, bufs
        ctx.set_materialize_grads(False)      # a term nobody uses arrives as None: the kernel then leaves it out
        return bufs.loss_t.detach(), bufs.loss_f.detach()      # aliases of the persistent scalars, as _SoftClDiceFn's

    @staticmethod
    def backward(ctx, gt, gf):
        none = (None,) * 11
        if (gt is None and gf is None) or not ctx.needs_input_grad[0]:
            return none
        gt = None if gt is None or not ctx.classes else gt.contiguous().float()
        gf = None if gf is None or ctx.gamma is None else gf.contiguous().float()
        dz = ops.seg_terms_backward(ctx.zb, ctx.C, ctx.mode, ctx.lt, ctx.classes, ctx.gamma, ctx.cw, ctx.bufs.state, gt, gf, ctx.bufs.dz)
        return (ops.logical_view(dz, ctx.C),) + none[1:]


def seg_terms(logits, label_or_target, mode, classes=(), alpha=0.5, beta=0.5, smooth=1.0, power=1.0, focal_gamma=None, class_weights=None,
              buffers=None):
    """The Tversky term (soft Dice at alpha = beta = 0.5, focal-Tversky at power < 1) over the listed `classes` and the focal term
    of the [1, C, H, W] fp32 logits on the device, against the int64 label map (mode ops.SEGHEAD_SOFTMAX) or the [1, C, H, W] float
    target (ops.SEGHEAD_SIGMOID): (L_T, L_F), float32 device scalars; util.seg_terms_ref states the mathematics.  classes empty: the
    Tversky term is off and L_T = 0; focal_gamma None: the focal term is off and L_F = 0; one of them must be on.  class_weights: the
    focal term's (None: 1).  The gradient flows to the logits only, each term's times its own upstream gradient; the logit tensor is
    taken the way seg_head takes it (NHWC-backed, read where it lies).  buffers: a SegTermsBuffers the caller keeps between steps
    (None: made here).  One launch forward, one backward; no fallback: off the device, with a batch or above 16 channels it raises."""
    ops.require_gpu(logits, "seg_terms")
    if not _bce_envelope(logits):
        raise SganError(f"seg_terms: not covered ({tuple(logits.shape)} {logits.dtype}: [1, C <= 16, H, W] fp32 logits on the device)")
    softmax = mode == ops.SEGHEAD_SOFTMAX
    lt = label_or_target.detach()
    _, C_, H, W = logits.shape
    if softmax:
        assert lt.dtype == torch.int64 and lt.device == logits.device and lt.numel() == H * W, "seg_terms: an int64 label map on the logits' device"
    else:
        assert _bce_envelope(lt) and lt.shape == logits.shape, "seg_terms: a [1, C, H, W] fp32 target on the logits' device"
    classes = tuple(int(c) for c in classes)
    cw = None if class_weights is None or focal_gamma is None else class_weights.detach().float().contiguous()
    if buffers is None:
        buffers = SegTermsBuffers(C_, H, W, logits.device)
    assert buffers.fits(C_, H, W, logits.device), (buffers.shape, logits.shape)
    return _SegTermsFn.apply(logits, lt, int(mode), classes, float(alpha), float(beta), float(smooth), float(power),
                             None if focal_gamma is None else float(focal_gamma), cw, buffers)


class DistLossBuffers:
    """What a boundary / Hausdorff node keeps between calls for [1, C, H, W] logits: the fp64 state the forward writes, the zeroed
    workspace of the forward's hand-off, the two loss scalars and the gradient buffer the node hands out, so that a step allocates
    nothing.  One node at a time, as SegTermsBuffers."""

    def __init__(self, C, H, W, device):
        self.shape = (C, H, W)
        self.state = ops.new_dist_loss_state(device)
        self.work = ops.new_dist_loss_workspace(device)
        self.loss_b = torch.zeros((), dtype=torch.float32, device=device)
        self.loss_h = torch.zeros((), dtype=torch.float32, device=device)
        self.dz = torch.empty((H, W, pad4(C)), dtype=torch.float32, device=device)

    def fits(self, C, H, W, device):
        return self.shape == (C, H, W) and self.dz.device == device


class _DistTermsFn(torch.autograd.Function):
    """(L_B, L_H) from the logits in one launch (sgan_dist_loss_forward); the backward is one launch too (sgan_dist_loss_backward): it
    takes the two upstream gradients as device scalars -- a term without one is not taken -- and writes the gradient of the logits."""

    @staticmethod
    def forward(ctx, logits, lt, mode, cls, t_sdsq, p_sdsq, boundary, alpha, bufs):
        zb = ops.as_nhwc(logits)
        C_ = logits.shape[1]
        lt = lt.reshape(-1).contiguous() if mode == ops.SEGHEAD_SOFTMAX else ops.as_nhwc(lt)
        ops.dist_loss_forward(zb, C_, mode, lt, cls, t_sdsq, p_sdsq, boundary, alpha, bufs.state, bufs.loss_b, bufs.loss_h, bufs.work)
        ctx.zb, ctx.lt, ctx.C, ctx.mode, ctx.cls, ctx.maps, ctx.boundary, ctx.alpha, ctx.bufs = zb, lt, C_, mode, cls, (t_sdsq, p_sdsq), boundary, alpha, bufs
        ctx.set_materialize_grads(False)      # a term nobody uses arrives as None: the kernel then leaves it out
        return bufs.loss_b.detach(), bufs.loss_h.detach()      # aliases of the persistent scalars, as _SegTermsFn's

    @staticmethod
    def backward(ctx, gb, gh):
        none = (None,) * 9
        if (gb is None and gh is None) or not ctx.needs_input_grad[0]:
            return none
        gb = None if gb is None or not ctx.boundary else gb.contiguous().float()
        gh = None if gh is None or ctx.alpha is None else gh.contiguous().float()
        dz = ops.dist_loss_backward(ctx.zb, ctx.C, ctx.mode, ctx.lt, ctx.cls, ctx.maps[0], ctx.maps[1], ctx.boundary, ctx.alpha, gb, gh,
                                    ctx.bufs.dz)
        return (ops.logical_view(dz, ctx.C),) + none[1:]


def dist_terms(logits, label_or_target, mode, cls, t_sdsq, p_sdsq=None, boundary=True, hausdorff_alpha=None, buffers=None):
    """The boundary loss (Kervadec et al., MIDL 2019) and the distance-transform Hausdorff loss (Karimi & Salcudean, TMI 2019) of
    class `cls` of the [1, C, H, W] fp32 logits on the device, against the int64 label map (mode ops.SEGHEAD_SOFTMAX) or the
    [1, C, H, W] float target (ops.SEGHEAD_SIGMOID): (L_B, L_H), float32 device scalars; util.dist_terms_ref states the mathematics.
    t_sdsq / p_sdsq: the signed squared distance maps (ops.signed_edt_sq, int32 [H, W]) of the truth plane and of the thresholded
    prediction, constants of the node.  boundary False: that term is off and L_B = 0; hausdorff_alpha None: the Hausdorff term is off,
    L_H = 0 and p_sdsq is not read; one of them must be on.  The gradient flows to the logits only, each term's times its own
    upstream gradient.  buffers: a DistLossBuffers the caller keeps between steps (None: made here).  One launch forward, one
    backward; no fallback: off the device, with a batch or above 16 channels it raises."""
    ops.require_gpu(logits, "dist_terms")
    if not _bce_envelope(logits):
        raise SganError(f"dist_terms: not covered ({tuple(logits.shape)} {logits.dtype}: [1, C <= 16, H, W] fp32 logits on the device)")
    lt = label_or_target.detach()
    _, C_, H, W = logits.shape
    if mode == ops.SEGHEAD_SOFTMAX:
        assert lt.dtype == torch.int64 and lt.device == logits.device and lt.numel() == H * W, "dist_terms: an int64 label map on the logits' device"
    else:
        assert _bce_envelope(lt) and lt.shape == logits.shape, "dist_terms: a [1, C, H, W] fp32 target on the logits' device"
    if buffers is None:
        buffers = DistLossBuffers(C_, H, W, logits.device)
    assert buffers.fits(C_, H, W, logits.device), (buffers.shape, logits.shape)
    return _DistTermsFn.apply(logits, lt, int(mode), int(cls), t_sdsq, None if hausdorff_alpha is None else p_sdsq, bool(boundary),
                              None if hausdorff_alpha is None else float(hausdorff_alpha), buffers)


class GANLossMultiClass(nn.Module):
    """GANLossMultiClass (models/networks.py:188-202): CrossEntropyLoss over the class channel of every pixel of a
    discriminator map against one class: one forward and one backward launch (sgan_ce_fwd / sgan_ce_bwd)."""

    def __init__(self, use_lsgan=False, num_classes=3, use_gpu=False):
        super().__init__()
        assert use_lsgan is False
        self.num_classes = num_classes

    def __call__(self, input, target_label):
        assert input.shape[1] == self.num_classes
        return cross_entropy_logits(input, None, int(target_label))


def _scale_saved_grad(ctx, gout):
    """d loss / d x of _L1Fn / _Bce01Fn: the forward kernel's unit-gradient result ctx.g times the upstream scalar."""
    dx = torch.empty_like(ctx.g)
    ops.scale(gout.contiguous(), ctx.g, dx)
    return ops.logical_view(dx, ctx.C)


class _L1Fn(torch.autograd.Function):
    """lambda * mean(|x - y| * w) with w = 1 + sum_i (A_i + 1) / 2 * (weights_i - 1), or w a per-pixel map, or 1."""

    @staticmethod
    def forward(ctx, x, y, a, wts, nw, lam):
        xb = ops.as_nhwc(x)
        yb = ops.as_nhwc(y)
        ab = None
        if a is not None:
            ab = ops.as_nhwc(a)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        g = torch.empty_like(xb)
        ops.l1w_fwd(xb, yb, x.shape[1], ab, wts, nw, lam, loss, g)
        ctx.g, ctx.C = g, x.shape[1]
        return loss

    @staticmethod
    def backward(ctx, gout):
        return _scale_saved_grad(ctx, gout), None, None, None, None, None


class _Bce01Fn(torch.autograd.Function):
    """BCELoss((x + 1) / 2, (t + 1) / 2), gradient w.r.t. x only."""

    @staticmethod
    def forward(ctx, x, t):
        xb, tb = ops.as_nhwc(x), ops.as_nhwc(t)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        g = torch.empty_like(xb)
        ops.bce01_fwd(xb, tb, x.shape[1], loss, g)
        ctx.g, ctx.C = g, x.shape[1]
        return loss

    @staticmethod
    def backward(ctx, gout):
        return _scale_saved_grad(ctx, gout), None


def bce_on_rescaled(x, t):
    """torch.nn.BCELoss()((x + 1) / 2, (t + 1) / 2) of the two-stage trainers (twostage_cycle_model.py:398-403) as one
    forward and one backward kernel; `t` is treated as a constant."""
    return _Bce01Fn.apply(x, t.detach())


class _Bilinear2xFn(torch.autograd.Function):
    """nn.Upsample(scale_factor=2, mode='bilinear') on a logical [1, C, H, W] tensor (`--transform_1to2 bilinear_2`)."""

    @staticmethod
    def forward(ctx, x):
        xb = ops.as_nhwc(x)
        H, W, Cs = xb.shape
        out = torch.empty((2 * H, 2 * W, Cs), dtype=torch.float32, device=x.device)
        ops.bilinear_up2_fwd(xb, out, None)
        ctx.shape, ctx.C = (H, W, Cs), x.shape[1]
        return ops.logical_view(out, x.shape[1])

    @staticmethod
    def backward(ctx, g):
        din = torch.empty(ctx.shape, dtype=torch.float32, device=g.device)
        ops.bilinear_up2_bwd(ops.as_nhwc(g), din)
        return ops.logical_view(din, ctx.C)


def bilinear_upsample2x(x):
    return _Bilinear2xFn.apply(x)


class WeightedL1Loss(nn.Module):
    """WeightedL1Loss (models/networks.py:205-214): mean(|x - y| * w).  One forward kernel (which also writes the
    gradient for a unit upstream) and one scaling kernel in backward."""

    def __call__(self, x, y, w=None):
        return _L1Fn.apply(x, y, w, None, 0, 1.0)

    def from_labels(self, x, y, real_A, weights, lam=1.0):
        """lam * self(x, y, w) with the weight map of CGANModel.backward_G (models/cgan_model.py:198-207),
        w = 1 + sum_i (real_A[:, i] + 1) / 2 * (weights[i] - 1), evaluated inside the kernel."""
        if weights is None:
            return _L1Fn.apply(x, y, None, None, 0, float(lam))
        wts = getattr(self, "_wts", None)
        if wts is None or wts.device != x.device or wts.numel() != len(weights):
            wts = self._wts = torch.tensor([float(v) for v in weights], dtype=torch.float32, device=x.device)
        return _L1Fn.apply(x, y, real_A, wts, len(weights), float(lam))

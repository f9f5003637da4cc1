"""SegmentationModel (models/segm_model.py:15-341): the conditional-GAN step with the generator emitting class logits -- image
real_A -> U-Net -> logits -> softmax (or `--use_sigmoid_ss` sigmoid) = the "fake" one-hot label the PatchGAN discriminators see on
cat(real_A, .); generator loss = sum_i lambda_i GAN(D_i(fake), 1) + (class-weighted) cross-entropy against the label.

`--which_model_netD None` is the supervised baseline (segm_model.py:76,91,103,115,203,239,255,267,274): no discriminators, the
generator trained on the (class-weighted) cross-entropy alone.  With no second consumer of the prediction the loss section of the
step -- softmax / sigmoid, the loss, d loss / d logits -- is one launch (losses.seg_head, sgan_seg_head).

Built on CGANModel: the step with or without its discriminator stage, pooling, optimizers, checkpoints and the LR schedule are
inherited; the generator runs
with the caller's `activation=` (identity) so the conv chain ends raw; softmax / cross-entropy (models/loss.py:6-12 is
NLLLoss2d(log_softmax)) and the sigmoid / weighted BCE of `--use_sigmoid_ss` are kernels of losses.py on the num_classes x H x W maps.
The accuracy half (segm_model.py:265-341) is SegMetricsMixin over self.seg_metrics (seg_metrics.py)."""
from collections import OrderedDict

import torch

from . import networks, ops, util
from .cgan_model import CGANModel
from .losses import (ClDiceBuffers, DistLossBuffers, LovaszBuffers, SegTermsBuffers, class_probability_plane, cross_entropy_logits, dist_terms,
                     lovasz_softmax, seg_head, seg_terms, sigmoid_channels, soft_cldice, softmax_channels, weighted_bce)
from .options import check_tile_options
from .seg_metrics import SegMetrics, SegMetricsMixin


def _identity(x):
    return x


class SegmentationModel(SegMetricsMixin, CGANModel):
    def name(self):
        return 'SegmentationModel'

    def initialize(self, opt):
        idx = {'r': 0, 'g': 1, 'b': 2}
        picks = [[idx[c] for c in part] for part in opt.which_channel.split('_')]
        assert len(picks) == 2
        self.label_nc = len(picks[1])
        self.num_classes = self.label_nc + 1 if opt.add_background_onehot else self.label_nc          # segm_model.py:45
        CGANModel.initialize(self, opt)
        self.class_weights = None if opt.weights is None else torch.tensor(opt.weights, dtype=torch.float32, device=self.device)
        self.use_sigmoid_ss = opt.use_sigmoid_ss
        self.no_netD = self.isTrain and not self.has_netD
        if self.no_netD:
            assert opt.weights is None or self.use_sigmoid_ss or len(opt.weights) == self.num_classes, \
                "--weights: one per class (%d) for the softmax cross-entropy" % self.num_classes
            self.loss_G_GAN = 0
            self.norm = None      # sum_p w[label_p], a persistent device scalar refreshed with the label (softmax mode)
        self.border = getattr(opt, 'border_weight', None)      # (w0, sigma) of the U-Net border term, or None
        self.bmap = None                                       # its map of the current crop, persistent like the label
        if self.border is not None:
            assert self.no_netD and not self.use_sigmoid_ss, \
                "--border_weight: softmax training with --which_model_netD None only (options.check_border_options)"
            assert opt.border_class < self.num_classes, "--border_class %d: there are %d classes" % (opt.border_class, self.num_classes)
            assert opt.batchSize == 1 and self.device.type == 'cuda', "--border_weight: batch 1 on the device, like every kernel of this path"
        self.cldice = None      # (lambda, K, class) of the soft-clDice term, or None: then nothing of it runs
        if self.isTrain and getattr(opt, 'cldice_weight', 0.0) > 0.0:
            assert opt.cldice_class < self.num_classes, "--cldice_class %d: there are %d classes" % (opt.cldice_class, self.num_classes)
            assert opt.batchSize == 1 and self.device.type == 'cuda', "--cldice_weight: batch 1 on the device, like every kernel of this path"
            self.cldice = (float(opt.cldice_weight), int(opt.cldice_iters), int(opt.cldice_class))
            self._cld_truth = self._cld_tskel = self._cld_bufs = None      # persistent: the truth plane, its skeleton, the node's buffers
            self.loss_G_clDice = 0
        self.lovasz = None      # (lambda, classes) of the Lovasz-softmax term, or None: then nothing of it runs
        if self.isTrain and getattr(opt, 'lovasz_weight', 0.0) > 0.0:
            classes = tuple(int(c) for c in opt.lovasz_classes)
            assert all(c < self.num_classes for c in classes), "--lovasz_classes %s: there are %d classes" % (list(classes), self.num_classes)
            assert opt.batchSize == 1 and self.device.type == 'cuda', "--lovasz_weight: batch 1 on the device, like every kernel of this path"
            self.lovasz = (float(opt.lovasz_weight), classes)
            self._lov_bufs = None      # persistent: the node's buffers
            self.loss_G_Lovasz = 0
        self.segterms = None      # (lambda_dice, classes, a, b, s, E, lambda_focal, gamma) of the Tversky / focal terms, or None: nothing runs
        if self.isTrain and (getattr(opt, 'dice_weight', 0.0) > 0.0 or getattr(opt, 'focal_weight', 0.0) > 0.0):
            lam_d, lam_f = float(getattr(opt, 'dice_weight', 0.0)), float(getattr(opt, 'focal_weight', 0.0))
            classes = tuple(int(c) for c in opt.dice_classes) if lam_d > 0.0 else ()
            assert all(c < self.num_classes for c in classes), "--dice_classes %s: there are %d classes" % (list(classes), self.num_classes)
            assert opt.batchSize == 1 and self.device.type == 'cuda', "--dice_weight / --focal_weight: batch 1 on the device, like every kernel of this path"
            assert lam_f == 0.0 or opt.weights is None or self.use_sigmoid_ss or len(opt.weights) == self.num_classes, \
                "--focal_weight with --weights: one per class (%d) for the softmax head" % self.num_classes
            self.segterms = (lam_d, classes, float(opt.tversky[0]), float(opt.tversky[1]), float(opt.dice_smooth), float(opt.tversky_power),
                             lam_f, float(opt.focal_gamma) if lam_f > 0.0 else None)
            self._st_bufs = None      # persistent: the node's buffers
            self.loss_G_Dice = self.loss_G_Focal = 0
        self.distterms = None      # (lambda_boundary, lambda_hausdorff, alpha, class) of the distance-map terms, or None: nothing runs
        if self.isTrain and (getattr(opt, 'boundary_loss_weight', 0.0) > 0.0 or getattr(opt, 'hausdorff_weight', 0.0) > 0.0):
            assert opt.dist_class < self.num_classes, "--dist_class %d: there are %d classes" % (opt.dist_class, self.num_classes)
            assert opt.batchSize == 1 and self.device.type == 'cuda', \
                "--boundary_loss_weight / --hausdorff_weight: batch 1 on the device, like every kernel of this path"
            self.distterms = (float(opt.boundary_loss_weight), float(opt.hausdorff_weight), float(opt.hausdorff_alpha), int(opt.dist_class))
            self._dl_truth = self._dl_tsdsq = self._dl_psdsq = self._dl_bufs = None      # persistent: the truth plane, both maps, the node's buffers
            self.loss_G_Boundary = self.loss_G_Hausdorff = 0
        self.seg_metrics = SegMetrics(opt, self.device, self.num_classes)
        self.reset_accs()
        self._tiling = not self.isTrain and getattr(opt, 'tiling', False)      # test(): whole-image inference (check_tile_options)
        self._tile_src = self._tile_st = None                                  # the uint8 image of set_input(); plan and buffers
        if self._tiling:
            assert self.num_classes <= 4 and opt.batchSize == 1 and self.device.type == 'cuda', \
                "--whole_image / --tta d4: at most 4 classes, batch 1, on the device"

    def _builds_netD(self, opt):
        return getattr(opt, 'which_model_netD', 'None') != 'None'

    def _output_channels(self, opt):
        return self.num_classes          # generator output and discriminator input are sized by the class count (:69,83-86)

    # ---- data ---------------------------------------------------------------------------------
    def set_input(self, input):
        """segm_model.py:120-143: label channels rescaled to [0, 1], optional background class, index label = argmax."""
        CGANModel.set_input(self, input)
        self._one_hot_label()
        self._tile_src = input.get('A_u8') if self._tiling else None

    def _one_hot_label(self):
        b = (self.input_B[:, :self.label_nc] + 1) / 2.0
        if self.opt.add_background_onehot:
            b = torch.cat([b, 1.0 - torch.clamp(b.sum(dim=1, keepdim=True), 0, 1)], dim=1)
        self.input_B.resize_(b.size()).copy_(b)
        lab = b.max(dim=1)[1]
        if getattr(self, 'label', None) is None or self.label.shape != lab.shape:
            self.label = torch.empty_like(lab)        # persistent: a captured hipGraph keeps reading this buffer (label_, :61,138-139)
        self.label.copy_(lab)
        if getattr(self, 'no_netD', False) and not self.use_sigmoid_ss and self.device.type == 'cuda':
            if self.norm is None:
                self.norm = torch.zeros((), dtype=torch.float32, device=self.device)
            if self.border is not None:
                self._border_weight_map()
                ops.pixel_weight_sum(self.label.reshape(-1), self.num_classes, self.class_weights, self.bmap.reshape(-1), self.norm)
            else:
                ops.label_weight_sum(self.label.reshape(-1), self.num_classes, self.class_weights, self.norm)
        if getattr(self, 'cldice', None) is not None:
            self._cldice_truth()
        if getattr(self, 'distterms', None) is not None:
            self._dist_truth()

    def _cldice_truth(self):
        """The truth plane of --cldice_class (1.0 where the label is that class) and its soft skeleton into persistent buffers, once per
        set_input like the border map: a captured step keeps reading them.  Enqueues only."""
        _, K, cls = self.cldice
        hw = tuple(self.label.shape[1:])
        if self._cld_truth is None or tuple(self._cld_truth.shape) != hw:
            self._cld_is = torch.empty(hw, dtype=torch.bool, device=self.device)
            self._cld_truth = torch.empty(hw, dtype=torch.float32, device=self.device)
            self._cld_tskel = torch.empty(hw, dtype=torch.float32, device=self.device)
            self._cld_bufs = ClDiceBuffers(hw[0], hw[1], K, self.device)
        torch.eq(self.label[0], cls, out=self._cld_is)
        self._cld_truth.copy_(self._cld_is)
        ops.soft_skeleton(self._cld_truth, K, out=self._cld_tskel)

    def _dist_truth(self):
        """The truth plane of --dist_class (1.0 where the label is that class) and its signed squared distance map into persistent
        buffers, once per set_input like the soft-clDice truth: a captured step keeps reading them.  Enqueues only."""
        cls = self.distterms[3]
        hw = tuple(self.label.shape[1:])
        if self._dl_truth is None or tuple(self._dl_truth.shape) != hw:
            self._dl_is = torch.empty(hw, dtype=torch.bool, device=self.device)
            self._dl_truth = torch.empty(hw, dtype=torch.float32, device=self.device)
            self._dl_tsdsq = torch.empty(hw, dtype=torch.int32, device=self.device)
            self._dl_psdsq = torch.empty(hw, dtype=torch.int32, device=self.device) if self.distterms[1] > 0.0 else None
        torch.eq(self.label[0], cls, out=self._dl_is)
        self._dl_truth.copy_(self._dl_is)
        ops.signed_edt_sq(self._dl_truth, out=self._dl_tsdsq)

    def _with_dist_terms(self, loss):
        """loss + lambda_boundary * boundary loss + lambda_hausdorff * Hausdorff loss of the --dist_class channel; the loss unchanged
        with both options off.  The node reads the logits of the last forward() whether discriminators exist or not and hands the
        gradient of the logits back.  The truth's map is the one set_input left; with the Hausdorff term on, the map of the
        prediction is taken here, inside the step, from the detached --dist_class plane of fake_B thresholded at > 0.5 like every
        metric: a graph replay computes it again.  A term whose weight is 0 is switched off in the call and takes no gradient."""
        if self.distterms is None:
            return loss
        lam_b, lam_h, alpha, cls = self.distterms
        shape = tuple(self.logit.shape[1:])
        if self._dl_bufs is None or not self._dl_bufs.fits(*shape, self.logit.device):
            self._dl_bufs = DistLossBuffers(*shape, self.logit.device)
        if lam_h > 0.0:
            ops.signed_edt_sq(self.fake_B.detach()[0, cls], out=self._dl_psdsq)
        if self.use_sigmoid_ss:
            mode, lt = ops.SEGHEAD_SIGMOID, self.real_B
        else:
            mode, lt = ops.SEGHEAD_SOFTMAX, self.label
        self.loss_G_Boundary, self.loss_G_Hausdorff = dist_terms(self.logit, lt, mode, cls, self._dl_tsdsq, self._dl_psdsq, lam_b > 0.0,
                                                                 alpha if lam_h > 0.0 else None, buffers=self._dl_bufs)
        if lam_b > 0.0:
            loss = loss + lam_b * self.loss_G_Boundary
        if lam_h > 0.0:
            loss = loss + lam_h * self.loss_G_Hausdorff
        return loss

    def _with_cldice(self, loss):
        """loss + lambda * soft-clDice of the class plane; the loss unchanged with the option off.  With discriminators fake_B is the
        softmax / sigmoid of the logits with a gradient path and the term reads its plane; the fused head's p takes no gradient, so
        without them the term computes its own from the logits of the last forward()."""
        if self.cldice is None:
            return loss
        lam, K, cls = self.cldice
        p = class_probability_plane(self.logit, cls, self.use_sigmoid_ss) if self.no_netD else self.fake_B[0, cls]
        self.loss_G_clDice = soft_cldice(p, self._cld_truth, K, t_skel=self._cld_tskel, buffers=self._cld_bufs)
        return loss + lam * self.loss_G_clDice

    def _with_lovasz(self, loss):
        """loss + lambda * Lovasz-softmax over the listed classes; the loss unchanged with the option off.  With discriminators the
        term reads fake_B; without them its own softmax / sigmoid of the logits of the last forward(), as the soft-clDice term: the
        fused head's p takes no gradient.  The prediction is read where it lies and the node returns the gradient of all of it."""
        if self.lovasz is None:
            return loss
        lam, classes = self.lovasz
        if self.no_netD:
            p = sigmoid_channels(self.logit) if self.use_sigmoid_ss else softmax_channels(self.logit)
        else:
            p = self.fake_B
        shape = tuple(p.shape[1:])
        if self._lov_bufs is None or not self._lov_bufs.fits(*shape, len(classes), p.device):
            self._lov_bufs = LovaszBuffers(*shape, len(classes), p.device)
        self.loss_G_Lovasz = lovasz_softmax(p, self.label[0], classes, buffers=self._lov_bufs)
        return loss + lam * self.loss_G_Lovasz

    def _with_seg_terms(self, loss):
        """loss + lambda_dice * Tversky + lambda_focal * focal; the loss unchanged with both options off.  The node reads the logits
        of the last forward() whether discriminators exist or not and hands the gradient of the logits back: it needs no prediction
        and no softmax of its own.  A term whose weight is 0 is switched off in the call and takes no gradient."""
        if self.segterms is None:
            return loss
        lam_d, classes, a, b, s, E, lam_f, gamma = self.segterms
        shape = tuple(self.logit.shape[1:])
        if self._st_bufs is None or not self._st_bufs.fits(*shape, self.logit.device):
            self._st_bufs = SegTermsBuffers(*shape, self.logit.device)
        if self.use_sigmoid_ss:
            mode, lt = ops.SEGHEAD_SIGMOID, self.real_B
        else:
            mode, lt = ops.SEGHEAD_SOFTMAX, self.label
        self.loss_G_Dice, self.loss_G_Focal = seg_terms(self.logit, lt, mode, classes, a, b, s, E, gamma, self.class_weights,
                                                        buffers=self._st_bufs)
        if lam_d > 0.0:
            loss = loss + lam_d * self.loss_G_Dice
        if lam_f > 0.0:
            loss = loss + lam_f * self.loss_G_Focal
        return loss

    def _border_weight_map(self):
        """The U-Net border term of the current label into self.bmap: the pixels of --border_class are the wall, its complement is
        labelled into cells (ops.ccl_label), and every wall pixel gets w0 exp(-(d1 + d2)^2 / (2 sigma^2)) from its two nearest cells
        (ops.border_weight).  Enqueues into persistent buffers; nothing is read back and nothing is allocated after the first call.
        Runs on every set_input, a validation image's included: forward() of this trainer always goes through the pixel-weighted
        head, which reads the map of the image it is given (the validation LOSS, compute_cross_entropy_loss, does not read it)."""
        hw = tuple(self.label.shape[1:])
        if self.bmap is None or tuple(self.bmap.shape) != hw:
            self._border_is_wall = torch.empty(hw, dtype=torch.bool, device=self.device)
            self._border_wall = torch.empty(hw, dtype=torch.float32, device=self.device)
            self._border_cells = torch.empty(hw, dtype=torch.int32, device=self.device)
            self.bmap = torch.empty(hw, dtype=torch.float32, device=self.device)
        w0, sigma = self.border
        torch.eq(self.label[0], self.opt.border_class, out=self._border_is_wall)
        self._border_wall.copy_(self._border_is_wall)      # 1.0 = wall, as ccl_label reads a plane
        ops.ccl_label(self._border_wall, self._border_cells)
        ops.border_weight(self._border_cells, self.opt.border_radius, w0, sigma, bmap=self.bmap)

    def forward(self, val_mode=False, netG=None):
        """val_mode: the validation pass of train_ss.py draws its latent at --noiseSizeVal (segm_model.py:145-155) and, under
        --ema_eval, runs the averaged generator (so --best_metric scores the average); netG: the generator to run, None = that rule."""
        if netG is None:
            netG = self._eval_netG() if val_mode else self.netG
        self.real_A = self.input_A
        self.real_B = self.input_B
        self.noise = self._draw_noise_val() if val_mode else self._draw_noise()
        self.logit = netG.forward(self.real_A, self.noise, activation=_identity)                 # :155
        if getattr(self, 'no_netD', False):      # the loss is fake_B's one consumer: prediction, loss and d loss / d logit in one launch
            if self.use_sigmoid_ss:
                self.fake_B, self._head_loss = seg_head(self.logit, self.real_B, self.class_weights, None, ops.SEGHEAD_SIGMOID)
            else:
                self.fake_B, self._head_loss = seg_head(self.logit, self.label, self.class_weights, self.norm, ops.SEGHEAD_SOFTMAX,
                                                        pixel_add=self.bmap)
            return      # backward_G names it loss_G_CE: the re-draw that ends an update (n_update_G > 1) must not replace the logged loss
        self.fake_B = sigmoid_channels(self.logit) if self.use_sigmoid_ss else softmax_channels(self.logit)

    sample_noise = forward

    def _draw_noise_val(self):
        o = self.opt
        if not hasattr(self.netG, 'noise_nc'):
            return None
        if getattr(self, 'noise_val_', None) is None:
            self.noise_val_ = self.Tensor(o.batchSize, o.noise_nc, o.noiseSizeVal, o.noiseSizeVal)
        ops.normal_fill(self.noise_val_, self._rng_seed + 977, self._rng_offset)
        return self.noise_val_

    def test(self):
        with torch.no_grad():
            if self._tiling:
                self._test_tiled()
            else:
                self.forward(netG=self._eval_netG())

    # ---- whole-image inference (--whole_image / --tta d4 of the test options; util.tile_plan) --------------------
    def _tile_state(self, H, W):
        """Plan and buffers of an H x W image; persistent, re-made when the size changes (like SegMetrics._plane)."""
        st = self._tile_st
        if st is None or st['hw'] != (H, W):
            o, dev = self.opt, self.device
            check_tile_options(o, size=(H, W))
            oy, ox, Wy, Wx = util.tile_plan(H, W, o.tile, o.tile_margin, o.tile_ramp, o.tile_stride)
            st = self._tile_st = {
                'hw': (H, W), 'passes': util.tile_passes(oy, ox, o.tta == 'd4'),
                'Wy': torch.tensor(Wy, dtype=torch.int32, device=dev), 'Wx': torch.tensor(Wx, dtype=torch.int32, device=dev),
                'canvas': torch.empty((H, W, 4), dtype=torch.float32, device=dev), 'prob': torch.empty((H, W, 4), dtype=torch.float32, device=dev),
                'logp': torch.empty((H, W, 4), dtype=torch.float32, device=dev),
                'rgb': torch.empty((o.tile, o.tile, 4), dtype=torch.float32, device=dev),
                'tile_A': torch.empty((o.tile, o.tile, ops.pad4(len(self.chnl_idx_input[0]))), dtype=torch.float32, device=dev)}
        return st

    def _test_tiled(self):
        """The prediction of the whole image set_input() was given: per pass (tile-row, tile-column, flip, rot) one image_prep_tile from
        the uint8 image, the channel pick of --which_channel, the generator with the latent forward() would draw, and one tile_blend
        into the canvas; then one tile_finish.  Leaves fake_B = P and logit = log P at full size beside real_A / real_B / label, so the
        cross-entropy (-log P[label]), the accuracies (argmax log P = argmax P) and the visuals read the whole image unchanged."""
        o, u8 = self.opt, self._tile_src
        assert u8 is not None, "--whole_image / --tta d4: the feeder did not hand over the uint8 image ('A_u8'; data.SingleFolderDataset does)"
        H, W = u8.shape[:2]
        assert tuple(self.input_A.shape[2:]) == (H, W), (self.input_A.shape, u8.shape)
        st = self._tile_state(H, W)
        self.real_A, self.real_B = self.input_A, self.input_B
        mode = ops.SEGHEAD_SIGMOID if self.use_sigmoid_ss else ops.SEGHEAD_SOFTMAX
        idx = self.chnl_idx_input[0]
        run = idx == list(range(idx[0], idx[0] + len(idx)))
        st['canvas'].zero_()
        for y0, x0, flip, rot in st['passes']:
            ops.image_prep_tile(u8, x0, y0, o.tile, o.tile, flip, rot, out=st['rgb'])
            if run:
                a = ops.logical_view(ops.slice_nhwc(st['rgb'], idx[0], len(idx), out=st['tile_A']), len(idx))
            else:
                a = ops.logical_view(st['rgb'], 3).index_select(1, self._chnl_dev[0])
            self.noise = self._draw_noise()
            z = self.netG.forward(a, self.noise, activation=_identity)
            assert z.shape == (1, self.num_classes, o.tile, o.tile), z.shape
            ops.tile_blend(ops.as_nhwc(z), self.num_classes, mode, x0, y0, o.tile_margin, o.tile_ramp, flip, rot, st['canvas'])
        ops.tile_finish(st['canvas'], self.num_classes, st['Wy'], st['Wx'], 8 if o.tta == 'd4' else 1, st['prob'], st['logp'])
        self.fake_B = ops.logical_view(st['prob'], self.num_classes)
        self.logit = ops.logical_view(st['logp'], self.num_classes)

    # ---- losses -------------------------------------------------------------------------------
    def compute_cross_entropy_loss(self, weighted=False):
        if self.use_sigmoid_ss:                                                                           # :216-225, :235-236
            self.loss_G_CE = weighted_bce(self.fake_B, self.real_B, self.class_weights if weighted else None)      # sgan_bce_weighted_*
        else:
            w = self.class_weights if (weighted or self.isTrain) else None
            self.loss_G_CE = cross_entropy_logits(self.logit, self.label, 0, w)      # models/loss.py:6-12 on the HIP kernel
        return self.loss_G_CE

    def backward_G(self):
        """loss_G = sum_i lambda_i * GAN(D_i(cat(A, fake_B)), 1) + CE   (segm_model.py:203-232)"""
        if self.no_netD:      # :202-203,227: loss_G_GAN = 0, the cross-entropy forward() left behind is the whole loss
            self.loss_G_GAN = 0
            self.loss_G_CE = self._head_loss
            self.loss_G = self._with_dist_terms(self._with_seg_terms(self._with_lovasz(self._with_cldice(self.loss_G_CE))))
            self._backward(self.loss_G)
            return
        skip = getattr(self.opt, 'skip_wasted_D_wgrad', False)
        for netD in self.netD:
            netD.compute_param_grads = not skip
        fake = self.fake_B if self.opt.no_cgan else networks.cat_pair(self.real_A, self.fake_B)
        fake, = self._augment([fake], 2)
        self.loss_G_GAN, self._each_G = self._d_losses([(d, fake, True) for d in self.netD], list(self.opt.lambda_D))
        for netD in self.netD:
            netD.compute_param_grads = True
        self.loss_G = self._with_dist_terms(self._with_seg_terms(self._with_lovasz(self._with_cldice(
            self.loss_G_GAN + self.compute_cross_entropy_loss(weighted=True)))))
        self._backward(self.loss_G)

    def get_current_errors(self):
        extra = [('G_clDice', float(self.loss_G_clDice.detach() if torch.is_tensor(self.loss_G_clDice) else 0.0))] if self.cldice is not None else []
        if self.lovasz is not None:
            extra = extra + [('G_Lovasz', float(self.loss_G_Lovasz.detach() if torch.is_tensor(self.loss_G_Lovasz) else 0.0))]
        if self.segterms is not None:
            if self.segterms[0] > 0.0:
                extra = extra + [('G_Dice', float(self.loss_G_Dice.detach() if torch.is_tensor(self.loss_G_Dice) else 0.0))]
            if self.segterms[6] > 0.0:
                extra = extra + [('G_Focal', float(self.loss_G_Focal.detach() if torch.is_tensor(self.loss_G_Focal) else 0.0))]
        if self.distterms is not None:
            if self.distterms[0] > 0.0:
                extra = extra + [('G_Boundary', float(self.loss_G_Boundary.detach() if torch.is_tensor(self.loss_G_Boundary) else 0.0))]
            if self.distterms[1] > 0.0:
                extra = extra + [('G_Hausdorff', float(self.loss_G_Hausdorff.detach() if torch.is_tensor(self.loss_G_Hausdorff) else 0.0))]
        if self.no_netD:                                     # :253-257
            return OrderedDict([('G_CE', float(self.loss_G_CE.detach()))] + extra)
        return OrderedDict([('G_CE', float(self.loss_G_CE.detach())), ('G_GAN', float(self.loss_G_GAN.detach())),
                            ('D_real', float(self.loss_D_real)), ('D_fake', float(self.loss_D_fake))] + extra)

    def get_current_visuals(self, save_as_single_image=False):
        three = lambda t: t if t.shape[1] in (1, 3) else torch.cat([t, torch.zeros_like(t[:, :1])], 1)[:, :3]      # noqa: E731
        return self.with_cleaned_visual(OrderedDict([('image', self.real_A.detach()), ('label', three(self.real_B.detach() * 2 - 1)),
                                                     ('prediction', three(self.fake_B.detach() * 2 - 1))]))

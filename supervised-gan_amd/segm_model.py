"""SegmentationModel (models/segm_model.py:15-341): the conditional-GAN step with the generator emitting class logits -- image
real_A -> U-Net -> logits -> softmax (or `--use_sigmoid_ss` sigmoid) = the "fake" one-hot label the PatchGAN discriminators see on
cat(real_A, .); generator loss = sum_i lambda_i GAN(D_i(fake), 1) + (class-weighted) cross-entropy against the label.

`--which_model_netD None` is the supervised baseline (segm_model.py:76,91,103,115,203,239,255,267,274): no discriminators, the
generator trained on the (class-weighted) cross-entropy alone.  With no second consumer of the prediction the loss section of the
step -- softmax / sigmoid, the loss, d loss / d logits -- is one launch (losses.seg_head, sgan_seg_head).

Built on CGANModel: the step with or without its discriminator stage, pooling, optimizers, checkpoints and the LR schedule are
inherited; the generator runs
with the caller's `activation=` (identity) so the conv chain ends raw; softmax / cross-entropy (models/loss.py:6-12 is
NLLLoss2d(log_softmax)) and the sigmoid / weighted BCE of `--use_sigmoid_ss` are kernels of losses.py on the num_classes x H x W maps."""
from collections import OrderedDict

import numpy as np
import torch

from . import networks, ops, util
from .cgan_model import CGANModel
from .losses import cross_entropy_logits, seg_head, sigmoid_channels, softmax_channels, weighted_bce


def _identity(x):
    return x


class SegmentationModel(CGANModel):
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
        self.reset_accs()

    def _builds_netD(self, opt):
        return getattr(opt, 'which_model_netD', 'None') != 'None'

    def _output_channels(self, opt):
        return self.num_classes          # generator output and discriminator input are sized by the class count (:69,83-86)

    # ---- data ---------------------------------------------------------------------------------
    def set_input(self, input):
        """segm_model.py:120-143: label channels rescaled to [0, 1], optional background class, index label = argmax."""
        CGANModel.set_input(self, input)
        self._one_hot_label()

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

    def forward(self, val_mode=False):
        """val_mode: the validation pass of train_ss.py draws its latent at --noiseSizeVal (segm_model.py:145-155)."""
        self.real_A = self.input_A
        self.real_B = self.input_B
        self.noise = self._draw_noise_val() if val_mode else self._draw_noise()
        self.logit = self.netG.forward(self.real_A, self.noise, activation=_identity)                 # :155
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
            self.forward()

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
            self.loss_G = self.loss_G_CE = self._head_loss
            self._backward(self.loss_G)
            return
        skip = getattr(self.opt, 'skip_wasted_D_wgrad', False)
        for netD in self.netD:
            netD.compute_param_grads = not skip
        fake = self.fake_B if self.opt.no_cgan else networks.cat_pair(self.real_A, self.fake_B)
        self.loss_G_GAN, self._each_G = self._d_losses([(d, fake, True) for d in self.netD], list(self.opt.lambda_D))
        for netD in self.netD:
            netD.compute_param_grads = True
        self.loss_G = self.loss_G_GAN + self.compute_cross_entropy_loss(weighted=True)
        self._backward(self.loss_G)

    def get_current_errors(self):
        if self.no_netD:                                     # :253-257
            return OrderedDict([('G_CE', float(self.loss_G_CE.detach()))])
        return OrderedDict([('G_CE', float(self.loss_G_CE.detach())), ('G_GAN', float(self.loss_G_GAN.detach())),
                            ('D_real', float(self.loss_D_real)), ('D_fake', float(self.loss_D_fake))])

    def get_current_visuals(self, save_as_single_image=False):
        three = lambda t: t if t.shape[1] in (1, 3) else torch.cat([t, torch.zeros_like(t[:, :1])], 1)[:, :3]      # noqa: E731
        return OrderedDict([('image', self.real_A.detach()), ('label', three(self.real_B.detach() * 2 - 1)),
                            ('prediction', three(self.fake_B.detach() * 2 - 1))])

    # ---- accuracy (segm_model.py:265-341) ---------------------------------------------------------------------------
    # The accumulators live on the device: accum_accs() only enqueues kernels (sgan_metrics.hip) behind the step, so a training loop
    # that accumulates after every step never waits for the GPU; get_current_accs() is the one place that synchronises and reads.
    def reset_accs(self):
        self.confusion, self.numAveragedPixels, self.numAveragedImages = 0, 0, 0
        self.pixelAcc = self.meanAcc = self.meanIU = self.RandScore = self.VInfo = self.RandScoreThin = self.VInfoThin = 0
        self.ObjF1 = self.ObjAP = self.SEG = self.PQ = 0
        self.BoundF = self.HausD = self.ASSD = 0
        for t in (getattr(self, '_acc_rand', None), getattr(self, '_acc_conf', None), getattr(self, '_acc_vinfo', None),
                  getattr(self, '_acc_thin', None), getattr(self, '_acc_obj_i', None), getattr(self, '_acc_obj_f', None),
                  getattr(self, '_acc_bnd_i', None), getattr(self, '_acc_bnd_f', None)):
            if t is not None:
                t.zero_()

    def _acc_buffers(self):
        if getattr(self, '_acc_rand', None) is None:
            k = self.num_classes + 1 if self.opt.add_background_onehot_acc else self.num_classes
            self._acc_rand = torch.zeros(2, dtype=torch.float64, device=self.device)          # sum of F, images
            self._acc_vinfo = torch.zeros(2, dtype=torch.float64, device=self.device)         # sum of VInfo, images
            self._acc_conf = torch.zeros((k, k), dtype=torch.int64, device=self.device)       # [label, prediction]
            self._acc_labels = None
        return self._acc_rand, self._acc_conf

    def accum_accs(self):
        if 'VInfo' in self.opt.which_metric:          # one labelling and one counting pass feed both scores
            self.compute_current_VInfo(with_rand='RandScore' in self.opt.which_metric)
        elif 'RandScore' in self.opt.which_metric:
            self.compute_current_Rand_score()
        labelled = 'VInfo' in self.opt.which_metric or 'RandScore' in self.opt.which_metric
        if any(k in self.opt.which_metric for k in util.OBJECT_METRICS):
            self.compute_current_object_matches(labelled=labelled)
            labelled = True
        if 'RandScoreThin' in self.opt.which_metric or 'VInfoThin' in self.opt.which_metric:
            self.compute_current_thinned_scores(truth_labelled=labelled)
        if 'meanIU' in self.opt.which_metric:
            self.compute_current_accuracy()
        if any(k in self.opt.which_metric for k in util.BOUNDARY_METRICS):
            self.compute_current_boundary(thinned='RandScoreThin' in self.opt.which_metric or 'VInfoThin' in self.opt.which_metric)

    def compute_current_Rand_score(self):
        """Adds the Rand F-score (util.compute_Rand_F_scores, do_thin=False) of the predicted against the true boundary map to the
        running sum on the device: two labellings, the contingency sums and the score itself are kernels on the current stream.

        The score is taken on CHANNEL 0 of fake_B and real_B: the first picked label channel, the boundary map (the background
        class of --add_background_onehot comes last).  The reference (segm_model.py:299-307) asserts num_classes == 2 and then hands
        the whole 2-channel maps to a function that squeezes a channel axis of size one, which cannot run; this is our reading of
        that call ("Segmentation metrics on the device").

        Batch 1, like every kernel of this path.  An image whose truth map has no free pixel scores NaN, and the NaN stays in the
        running sum until reset_accs(), as in the reference's running mean; nothing on the host sees it before get_current_accs()."""
        acc, _ = self._acc_buffers()
        t_labels, s_labels = self._label_boundary_maps()
        ops.rand_f_accumulate(t_labels, s_labels, acc)

    def _label_boundary_maps(self):
        """Labels the regions of channel 0 of real_B and fake_B (truth, prediction) into the trainer's own label buffer."""
        assert self.num_classes == 2      # binary segmentation only, as in the reference
        assert self.fake_B.shape[0] == 1, "the device metrics take batch 1, like every kernel of this path"
        self._acc_buffers()
        s, t = self.fake_B.detach()[0, 0], self.real_B.detach()[0, 0]
        if self._acc_labels is None or self._acc_labels.shape[1:] != t.shape:
            self._acc_labels = torch.empty((2,) + tuple(t.shape), dtype=torch.int32, device=self.device)
        ops.ccl_label(t, self._acc_labels[0])
        ops.ccl_label(s, self._acc_labels[1])
        return self._acc_labels[0], self._acc_labels[1]

    def compute_current_VInfo(self, with_rand=False):
        """Adds the information score (util.compute_VInfo_scores) of the same pair of maps, under the conventions of
        compute_current_Rand_score, to its running sum on the device.  with_rand: the Rand F-score of the pair goes to ITS running
        sum from the same call -- the counting pass is the expensive launch and both scores are functions of its counters, so asking
        for both costs one labelling and one count; the value added is rand_f_accumulate's, bit for bit."""
        t_labels, s_labels = self._label_boundary_maps()
        ops.vinfo_accumulate(t_labels, s_labels, self._acc_vinfo, acc_rand=self._acc_rand if with_rand else None)

    def compute_current_object_matches(self, labelled=False):
        """Adds the object-level match counts of the same pair of maps (ops.object_match_accumulate: which truth cell is found by
        which predicted cell at IoU > 0.5 .. 0.95, regions below --min_object_area left out) to pooled counters on the device;
        ObjF1, ObjAP, SEG and PQ are derived from them when the accuracies are read.  labelled: RandScore / VInfo were taken in this
        accum_accs, so both label maps are in place and nothing is labelled again."""
        if getattr(self, '_acc_obj_i', None) is None:
            self._acc_buffers()
            self._acc_obj_i = torch.zeros(len(ops.OBJECT_COUNTS), dtype=torch.int64, device=self.device)
            self._acc_obj_f = torch.zeros(len(ops.OBJECT_SUMS), dtype=torch.float64, device=self.device)
        if labelled and self._acc_labels is not None and self._acc_labels.shape[1:] == self.real_B.shape[2:]:
            t_labels, s_labels = self._acc_labels[0], self._acc_labels[1]
        else:
            t_labels, s_labels = self._label_boundary_maps()
        ops.object_match_accumulate(t_labels, s_labels, self._acc_obj_i, self._acc_obj_f, min_area=self.opt.min_object_area)

    def get_object_counts(self):
        """The pooled object-match numbers since reset_accs() as a dict: the 16 integers of ops.OBJECT_COUNTS (TP_0 .. TP_9 at
        IoU > 0.5 .. 0.95, N_t, N_s, images, SEGn) and the two sums of ops.OBJECT_SUMS.  Synchronises, like get_current_accs()."""
        counts, sums = [0] * len(ops.OBJECT_COUNTS), [0.0] * len(ops.OBJECT_SUMS)
        if getattr(self, '_acc_obj_i', None) is not None:
            ops.check_metric_err(self.device)
            counts, sums = self._acc_obj_i.cpu().tolist(), self._acc_obj_f.cpu().tolist()
        return OrderedDict(list(zip(ops.OBJECT_COUNTS, counts)) + list(zip(ops.OBJECT_SUMS, sums)))

    def compute_current_thinned_scores(self, truth_labelled=False):
        """Adds the scores after border thinning -- util.compute_thinned_scores, the reference's do_thin=True -- to running sums of
        their own: channel 0 of fake_B thinned to one-pixel lines (ops.thin) into a plane of the trainer's, that plane labelled into
        a third label buffer, then one counting pass for whichever of RandScoreThin / VInfoThin is asked for.  The truth is not
        thinned, and its labelling is the un-thinned scores' when they were taken in this accum_accs (truth_labelled)."""
        assert self.num_classes == 2 and self.fake_B.shape[0] == 1, "binary segmentation at batch 1, like every kernel of this path"
        self._acc_buffers()
        s, t = self.fake_B.detach()[0, 0], self.real_B.detach()[0, 0]
        if getattr(self, '_acc_thin', None) is None:
            self._acc_thin = torch.zeros((2, 2), dtype=torch.float64, device=self.device)      # [Rand, VInfo] x [sum, images]
            self._thin_plane = self._thin_labels = None
        if self._thin_plane is None or self._thin_plane.shape != t.shape:
            self._thin_plane = torch.empty(tuple(t.shape), dtype=torch.float32, device=self.device)
            self._thin_labels = torch.empty(tuple(t.shape), dtype=torch.int32, device=self.device)
        if self._acc_labels is None or self._acc_labels.shape[1:] != t.shape:
            self._acc_labels = torch.empty((2,) + tuple(t.shape), dtype=torch.int32, device=self.device)
            truth_labelled = False
        if not truth_labelled:
            ops.ccl_label(t, self._acc_labels[0])
        ops.thin(s, out=self._thin_plane)
        ops.ccl_label(self._thin_plane, self._thin_labels)
        with_rand = 'RandScoreThin' in self.opt.which_metric
        if 'VInfoThin' in self.opt.which_metric:
            ops.vinfo_accumulate(self._acc_labels[0], self._thin_labels, self._acc_thin[1], acc_rand=self._acc_thin[0] if with_rand else None)
        else:
            ops.rand_f_accumulate(self._acc_labels[0], self._thin_labels, self._acc_thin[0])

    def compute_current_boundary(self, thinned=False):
        """Adds the boundary counts of the same pair of maps (ops.boundary_accumulate: how far every predicted wall pixel lies from
        the true wall and every true wall pixel from the predicted one) to pooled counters on the device: two exact distance
        transforms (ops.edt_sq) of channel 0 of real_B and fake_B, one counting call.  BoundF, HausD and ASSD are derived from the
        counters when the accuracies are read.  With --boundary_thin the predicted wall is thinned to one-pixel lines first
        (ops.thin), the truth is not; thinned: RandScoreThin / VInfoThin were taken in this accum_accs, so the thinned plane is in
        place and is not thinned again."""
        assert self.num_classes == 2 and self.fake_B.shape[0] == 1, "binary segmentation at batch 1, like every kernel of this path"
        self._acc_buffers()
        s, t = self.fake_B.detach()[0, 0], self.real_B.detach()[0, 0]
        if getattr(self, '_acc_bnd_i', None) is None:
            self._acc_bnd_i = torch.zeros(len(ops.BOUNDARY_COUNTS), dtype=torch.int64, device=self.device)
            self._acc_bnd_f = torch.zeros(len(ops.BOUNDARY_SUMS), dtype=torch.float64, device=self.device)
            self._bnd_dsq = self._bnd_thin_plane = None
        if self._bnd_dsq is None or self._bnd_dsq.shape[1:] != t.shape:
            self._bnd_dsq = torch.empty((2,) + tuple(t.shape), dtype=torch.int32, device=self.device)
        if self.opt.boundary_thin:
            if thinned and getattr(self, '_thin_plane', None) is not None and self._thin_plane.shape == t.shape:
                s = self._thin_plane
            else:
                if self._bnd_thin_plane is None or self._bnd_thin_plane.shape != t.shape:
                    self._bnd_thin_plane = torch.empty(tuple(t.shape), dtype=torch.float32, device=self.device)
                s = ops.thin(s, out=self._bnd_thin_plane)
        ops.edt_sq(t, out=self._bnd_dsq[0])
        ops.edt_sq(s, out=self._bnd_dsq[1])
        ops.boundary_accumulate(self._bnd_dsq[0], self._bnd_dsq[1], self._acc_bnd_i, self._acc_bnd_f)

    def get_boundary_counts(self):
        """The pooled boundary numbers since reset_accs() as a dict: the 80 integers of ops.BOUNDARY_COUNTS (the two histograms by
        distance bin, N_s, N_t, images, ...) and the four sums of ops.BOUNDARY_SUMS.  Synchronises, like get_current_accs()."""
        counts, sums = [0] * len(ops.BOUNDARY_COUNTS), [0.0] * len(ops.BOUNDARY_SUMS)
        if getattr(self, '_acc_bnd_i', None) is not None:
            ops.check_metric_err(self.device)
            counts, sums = self._acc_bnd_i.cpu().tolist(), self._acc_bnd_f.cpu().tolist()
        return OrderedDict(list(zip(ops.BOUNDARY_COUNTS, counts)) + list(zip(ops.BOUNDARY_SUMS, sums)))

    def compute_current_accuracy(self):
        """conf[label, prediction] += 1 for every pixel, on the device (segm_model.py:309-331; the ratios are taken when the
        accuracies are read)."""
        _, conf = self._acc_buffers()
        assert self.logit.shape[0] == 1, "the device metrics take batch 1, like every kernel of this path"
        if self.opt.add_background_onehot_acc:
            ops.confusion_accumulate(ops.as_nhwc(self.fake_B.detach()), self.num_classes, conf, y=ops.as_nhwc(self.real_B.detach()),
                                     add_background=True)
        else:
            ops.confusion_accumulate(ops.as_nhwc(self.logit.detach()), self.num_classes, conf, label=self.label)

    def get_current_accs(self):
        """Reads the device accumulators (the only synchronisation of the metric path) and derives RandScore, VInfo, pixelAcc,
        meanAcc and meanIU from them, and RandScoreThin / VInfoThin, then ObjF1 / ObjAP / SEG / PQ (util.object_scores of the pooled
        counts), then BoundF / HausD / ASSD (util.boundary_scores of the pooled counts at --boundary_tolerance), after the existing
        keys when they were asked for.  A trainer built for evaluation (test_ss.py) also prints the pooled TP_k / N_t / N_s line when
        an object score was asked for, and the boundary precision / recall / F at the tolerances 0 .. 5 with the dataset's worst
        distance when a boundary score was."""
        if getattr(self, '_acc_rand', None) is not None:
            ops.check_metric_err(self.device)
            rand, conf = self._acc_rand.cpu().numpy(), self._acc_conf.cpu().numpy().astype(np.float64)
            vinfo = self._acc_vinfo.cpu().numpy()
            self.numAveragedImages = int(max(rand[1], vinfo[1]))
            if getattr(self, '_acc_thin', None) is not None:
                thin = self._acc_thin.cpu().numpy()
                self.numAveragedImages = int(max(self.numAveragedImages, thin[0, 1], thin[1, 1]))
                self.RandScoreThin = thin[0, 0] / thin[0, 1] if thin[0, 1] else 0
                self.VInfoThin = thin[1, 0] / thin[1, 1] if thin[1, 1] else 0
            if getattr(self, '_acc_obj_i', None) is not None:
                obj_i, obj_f = self._acc_obj_i.cpu().numpy(), self._acc_obj_f.cpu().numpy()
                self.numAveragedImages = int(max(self.numAveragedImages, obj_i[ops.OBJECT_COUNTS.index('images')]))
                for k, v in util.object_scores(obj_i, obj_f).items():
                    setattr(self, k, v)
                if not self.isTrain and any(k in self.opt.which_metric for k in util.OBJECT_METRICS):
                    # the evaluation drivers read the accuracies once, after the dataset: the per-threshold table goes beside them
                    print('objects: TP at IoU > 0.50 .. 0.95: %s, N_t %d, N_s %d (min area %d)'
                          % (' '.join(str(int(v)) for v in obj_i[:10]), obj_i[10], obj_i[11], self.opt.min_object_area))
            if getattr(self, '_acc_bnd_i', None) is not None:
                bnd_i, bnd_f = self._acc_bnd_i.cpu().numpy(), self._acc_bnd_f.cpu().numpy()
                self.numAveragedImages = int(max(self.numAveragedImages, bnd_i[ops.BOUNDARY_COUNTS.index('images')]))
                for k, v in util.boundary_scores(bnd_i, bnd_f, self.opt.boundary_tolerance).items():
                    setattr(self, k, v)
                if not self.isTrain and any(k in self.opt.which_metric for k in util.BOUNDARY_METRICS):
                    print('boundary: P/R/F at tolerance 0 .. 5: %s, worst distance %.3f (N_s %d, N_t %d%s)'
                          % (' '.join('%.4f/%.4f/%.4f' % util.boundary_pr(bnd_i, k) for k in range(6)),
                             float(np.sqrt(float(max(bnd_i[70], bnd_i[71])))), bnd_i[64], bnd_i[65],
                             ', prediction thinned' if self.opt.boundary_thin else ''))
            self.RandScore = rand[0] / rand[1] if rand[1] else 0
            self.VInfo = vinfo[0] / vinfo[1] if vinfo[1] else 0
            self.confusion, self.numAveragedPixels = conf, int(conf.sum())
            rel, sel, tp = conf.sum(axis=1), conf.sum(axis=0), np.diag(conf)
            self.pixelAcc = tp.sum() / max(1, self.numAveragedPixels)
            self.meanAcc = float(np.mean(tp / np.maximum(1, rel)))
            self.meanIU = float(np.mean(tp / np.maximum(1, rel + sel - tp)))
        return OrderedDict(([('RandScore', self.RandScore)] if 'RandScore' in self.opt.which_metric else [])
                           + ([('VInfo', self.VInfo)] if 'VInfo' in self.opt.which_metric else [])
                           + ([('meanIU', self.meanIU)] if 'meanIU' in self.opt.which_metric else [])
                           + ([('RandScoreThin', self.RandScoreThin)] if 'RandScoreThin' in self.opt.which_metric else [])
                           + ([('VInfoThin', self.VInfoThin)] if 'VInfoThin' in self.opt.which_metric else [])
                           + [(k, getattr(self, k)) for k in util.OBJECT_METRICS if k in self.opt.which_metric]
                           + [(k, getattr(self, k)) for k in util.BOUNDARY_METRICS if k in self.opt.which_metric])

"""SegmentationCycleModel (models/segm_cycle_model.py:15-394): G1 image -> class logits (softmax / `--use_sigmoid_ss` sigmoid gives
fake_B), G2 one-hot label -> image, run on the real label (fake_A, judged by the discriminators D2 on cat(label, image)) and on G1's
prediction (recon_A, the cycle); generator loss = lambda_A CE(fake_B) + GAN(D2(fake_A)) + lambda_B L1(fake_B, real_B) +
lambda_A_cycle L1(recon_A, real_A) with G1 stepped at lr1, G2 and D2 at lr2.

Built on CGANCycleModel's plumbing (channel picking, latents, AdamGroups, checkpoints); the segmentation-specific pieces come from
SegmentationModel's restatement (one-hot label, cross-entropy) and the accuracies from the same SegMetricsMixin."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from . import networks, ops
from .base_model import BaseModel
from .cgan_cycle_model import CGANCycleModel
from .image_pool import ImagePool
from .optim import AdamGroups, FusedAdam
from .losses import sigmoid_channels, softmax_channels
from .seg_metrics import SegMetrics, SegMetricsMixin
from .segm_model import SegmentationModel, _identity


class SegmentationCycleModel(SegMetricsMixin, CGANCycleModel):
    def name(self):
        return 'SegmentationCycleModel'

    def initialize(self, opt):
        BaseModel.initialize(self, opt)
        self.isTrain = opt.isTrain
        idx = {'r': 0, 'g': 1, 'b': 2}
        self.chnl_idx_input = [[idx[c] for c in part] for part in opt.which_channel.split('_')]
        assert len(self.chnl_idx_input) == 2
        opt.input_nc, self.label_nc = len(self.chnl_idx_input[0]), len(self.chnl_idx_input[1])
        self.num_classes = opt.output_nc = self.label_nc + 1 if opt.add_background_onehot else self.label_nc      # :41-42
        self._chnl_dev = [torch.tensor(ix, dtype=torch.long, device=self.device) for ix in self.chnl_idx_input]
        self.class_weights = None if opt.weights is None else torch.tensor(opt.weights, dtype=torch.float32, device=self.device)
        self.use_sigmoid_ss = opt.use_sigmoid_ss
        self.input_A = self.Tensor(opt.batchSize, opt.input_nc, opt.fineSize, opt.fineSize)
        self.input_B = self.Tensor(opt.batchSize, self.num_classes, opt.fineSize, opt.fineSize)
        self.noise1_ = self.Tensor(opt.batchSize, opt.noise_nc1, opt.noiseSize1, opt.noiseSize1)
        self.noise2_ = self.Tensor(opt.batchSize, opt.noise_nc2, opt.noiseSize2, opt.noiseSize2)
        self.noise1 = self.noise2 = self.label = None
        self._rng_seed = 0 if opt.manualSeed is None else int(opt.manualSeed)
        self._rng_offset = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.noise_source = None

        def G(cin, cout, k):
            g = lambda name: getattr(opt, name + k)      # noqa: E731
            return networks.define_G(cin, cout, g('ngf'), g('which_model_netG'), opt.norm, not g('no_dropout'), n_layers_G=g('n_layers_G'),
                                     use_residual=False, use_fcn=g('noiseSize') != 1, noise_nc=g('noise_nc'),
                                     add_gaussian_noise=opt.add_gaussian_noise, gaussian_sigma=opt.gaussian_sigma,
                                     upsample_mode=g('upsample_mode'), n_layers_CRN_block=g('n_layers_CRN_block'),
                                     share_label_weights=not g('no_share_label_block_weights'),
                                     n_layers_G_skip=getattr(opt, 'n_layers_G%s_skip' % k), gpu_ids=self.gpu_ids)
        self.netG1 = G(opt.input_nc, self.num_classes, '1')             # :63-69
        self.netG2 = G(self.num_classes, opt.input_nc, '2')             # :70-76
        self._own_rng_streams(self.netG1, self.netG2)
        if self.isTrain:
            assert (len(opt.scale_factor2) == len(opt.lambda_D2) == len(opt.n_layers_D2))
            self.n_netD2 = len(opt.scale_factor2)
            d_nc = opt.input_nc if opt.no_cgan else opt.input_nc + self.num_classes
            self.netD2 = []
            for scale, n_layers in zip(opt.scale_factor2, opt.n_layers_D2):
                d = networks.define_D(d_nc, opt.ndf2, opt.which_model_netD2, n_layers_D=n_layers, norm=opt.norm, use_sigmoid=opt.no_lsgan2,
                                      scale_factor=scale, gpu_ids=self.gpu_ids)
                d.fuse_sigmoid_into_loss = True
                self.netD2.append(d)
            if self.gpu_ids:
                networks.pack_flat(self.netD2)
        if self.isTrain and opt.sequential_train and not opt.continue_train:
            self.load(opt.which_epoch_sequential, only=opt.which_model_to_load, model_dir=opt.pretrained_model_dir)
        if not self.isTrain or opt.continue_train:
            self.load(opt.which_epoch)
        if self.isTrain:
            self.fake_pool2 = ImagePool(opt.pool_size)
            self.old_lr, self.old_lr1, self.old_lr2 = opt.lr, opt.lr1, opt.lr2
            self.criterionGAN1 = self.criterionGAN2 = networks.GANLoss(use_lsgan=not opt.no_lsgan2)      # _gan() reads criterionGAN1
            self.criterionL1 = networks.WeightedL1Loss()
            self.optimizer_G = AdamGroups([{'name': 'G1', 'params': self.netG1.parameters(), 'lr': opt.lr1},
                                           {'name': 'G2', 'params': self.netG2.parameters(), 'lr': opt.lr2}],
                                          lr=opt.lr, betas=(opt.beta1, 0.999))
            self.optimizer_D2 = FusedAdam([p for d in self.netD2 for p in d.model.parameters()], lr=opt.lr2, betas=(opt.beta1, 0.999))
            self.optimizer_D2.param_groups[0]['name'] = 'D2'      # decay_three_rates: follows lr2
        self.seg_metrics = SegMetrics(opt, self.device, self.num_classes)
        self.reset_accs()

    # ---- the step (:261-278): D2, then G1 and G2 together; G1 follows lr1, G2 and D2 follow lr2 (:313-332) ------------------------
    def step_stages(self):
        o = self.opt
        return [(self.optimizer_D2, self.backward_D2, o.n_update_D2), (self.optimizer_G, self.backward_G, o.n_update_G)]

    def step_pools(self):
        return [(self.fake_pool2, self._d_fake_source)]

    def checkpoint_nets(self):
        return [('G1', self.netG1), ('G2', self.netG2)] + [('D2_%d' % n, d) for n, d in enumerate(self.netD2 if self.isTrain else [])]

    # ---- data / forward ---------------------------------------------------------------------------
    def set_input(self, input):
        CGANCycleModel.set_input(self, input)
        SegmentationModel._one_hot_label(self)

    def forward(self, val_mode=False):
        """(:159-174); val_mode: G1's latent at --noiseSizeVal, as train_ss.py's validation pass asks for."""
        self.real_A, self.real_B = self.input_A, self.input_B
        self.noise1, self.noise2 = (self._draw_val() if val_mode else self._draw(1).clone()), self._draw(2).clone()
        self.logit = self.netG1.forward(self.real_A, self.noise1, activation=_identity)
        self.fake_B = sigmoid_channels(self.logit) if self.use_sigmoid_ss else softmax_channels(self.logit)
        self.fake_A = self.netG2.forward(self.real_B, self.noise2)
        self.recon_A = self.netG2.forward(self.fake_B, self.noise2)

    sample_noise = forward          # (:176-185) regenerates everything, fake_A included

    def _draw_val(self):
        o = self.opt
        z = torch.empty((o.batchSize, o.noise_nc1, o.noiseSizeVal, o.noiseSizeVal), dtype=torch.float32, device=self.device)
        ops.normal_fill(z, self._rng_seed + 977, self._rng_offset)
        return z

    def test(self):
        with torch.no_grad():
            self.real_A, self.real_B = self.input_A, self.input_B
            self.noise1 = self._draw(1).clone()
            self.logit = self.netG1.forward(self.real_A, self.noise1, activation=_identity)
            self.fake_B = sigmoid_channels(self.logit) if self.use_sigmoid_ss else softmax_channels(self.logit)

    # ---- losses -----------------------------------------------------------------------------------
    def _d_fake_source(self):
        return self.fake_A if self.opt.no_cgan else networks.cat_pair(self.real_B, self.fake_A)

    def backward_D2(self):
        """(:201-222)"""
        fake = self._pooled(0).detach()
        real = self.real_A if self.opt.no_cgan else networks.cat_pair(self.real_B, self.real_A)
        n = self.n_netD2
        self.loss_D2, each = self._gan([(d, fake, False) for d in self.netD2] + [(d, real, True) for d in self.netD2], [0.5] * (2 * n))
        self.loss_D2_fake, self.loss_D2_real = each[:n].sum(), each[n:].sum()
        self._backward(self.loss_D2)

    def backward_G(self):
        """(:224-259)"""
        o = self.opt
        for netD in self.netD2:
            netD.compute_param_grads = not getattr(o, 'skip_wasted_D_wgrad', False)
        self.loss_G2_GAN, _ = self._gan([(d, self._d_fake_source(), True) for d in self.netD2], list(o.lambda_D2))
        for netD in self.netD2:
            netD.compute_param_grads = True
        self.loss_G1_CE = SegmentationModel.compute_cross_entropy_loss(self, weighted=True)
        self.loss_G_L1 = self.criterionL1(self.fake_B, self.real_B)
        self.loss_G_cycle = self.criterionL1(self.recon_A, self.real_A)
        self.loss_G = self.loss_G1_CE * o.lambda_A + self.loss_G2_GAN + self.loss_G_L1 * o.lambda_B + self.loss_G_cycle * o.lambda_A_cycle
        self._backward(self.loss_G)

    def get_current_errors(self):
        return OrderedDict([('G_CE', float(self.loss_G1_CE.detach())), ('G_GAN', float(self.loss_G2_GAN.detach())),
                            ('G_L1', float(self.loss_G_L1.detach())), ('G_cycle', float(self.loss_G_cycle.detach())),
                            ('D_real', float(self.loss_D2_real)), ('D_fake', float(self.loss_D2_fake))])

    def get_current_visuals(self, save_as_single_image=False):
        three = lambda t: t if t.shape[1] in (1, 3) else torch.cat([t, torch.zeros_like(t[:, :1])], 1)[:, :3]      # noqa: E731
        return self.with_cleaned_visual(OrderedDict([('image', self.real_A.detach()), ('label', three(self.real_B.detach() * 2 - 1)),
                                                     ('prediction', three(self.fake_B.detach() * 2 - 1))]))

    compute_cross_entropy_loss = SegmentationModel.compute_cross_entropy_loss      # test_ss.py: sets loss_G_CE

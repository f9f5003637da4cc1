"""FCGANModel (models/fcgan_model.py:26-236): the unconditional GAN trainer -- noise -> G -> fake,
multi-scale discriminator list, D step / G step, Adam, checkpoint save/load, linear LR decay --
driving the MI355X kernels.  Method names, loss definitions and update order follow the reference
line by line in *behaviour*; data stays device resident and every network call is one autograd node.

Deviations, all observable-behaviour preserving:
  * sigmoid+BCE is evaluated by one kernel on the discriminator logits (GANLoss);
  * `--skip_wasted_D_wgrad`: the reference computes discriminator weight gradients during the G step
    and zeroes them before they are ever used (fcgan_model.py:176,182); with the flag they are not
    computed;
  * latent noise comes from a counter-based Philox kernel (`normal_fill`), not torch's RNG stream."""
from collections import OrderedDict

import torch

from . import networks, ops
from ._lib import SganError
from .base_model import BaseModel
from .image_pool import ImagePool
from .optim import FusedAdam


class FCGANModel(BaseModel):
    supports_diffaug = True

    def name(self):
        return 'FCGANModel'

    def initialize(self, opt):
        BaseModel.initialize(self, opt)
        self.isTrain = opt.isTrain
        # parse which_channel (fcgan_model.py:47-58)
        idx_dict = {'r': 0, 'g': 1, 'b': 2}
        self.chnl_idx_input, self.chnl_idx_visual = [], []
        for s in opt.which_channel.split('_'):
            self.chnl_idx_visual.append([idx_dict[c] for c in s])
            self.chnl_idx_input += [idx_dict[c] for c in s]
        opt.input_nc = len(self.chnl_idx_input)
        self._chnl_dev = torch.tensor(self.chnl_idx_input, dtype=torch.long, device=self.device)

        zshape = (opt.batchSize, opt.noise_nc, opt.noiseSize, opt.noiseSize)
        self.input = self.Tensor(opt.batchSize, opt.input_nc, opt.fineSize, opt.fineSize)
        self.noise = None
        if self.device.type == 'cuda' and opt.batchSize == 1:
            # the latent lives in the padded NHWC buffer the generator reads; `noise_` is its logical [1, C, H, W] view
            self._noise_buf = torch.zeros((opt.noiseSize, opt.noiseSize, ops.pad4(opt.noise_nc)), dtype=torch.float32, device=self.device)
            self.noise_ = ops.logical_view(self._noise_buf, opt.noise_nc)
        else:
            self._noise_buf = None
            self.noise_ = self.Tensor(*zshape)
        self._rng_seed = 0 if opt.manualSeed is None else int(opt.manualSeed)
        self._rng_offset = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.noise_source = None    # optional callable() -> z tensor (tests inject latents)
        if self.device.type == 'cuda':
            self.fixed_noiseA = self._draw_noise().clone()
            self.fixed_noiseB = self._draw_noise().clone()
        else:   # a CPU-resident model can be built (checkpoint surgery, tests) but never runs a network
            self.fixed_noiseA = torch.randn(zshape)
            self.fixed_noiseB = torch.randn(zshape)

        def build_G():
            return networks.define_G(opt.input_nc, 0, opt.ngf, opt.which_model_netG, opt.norm, not opt.no_dropout,
                                     n_layers_G=opt.n_layers_G, use_residual=opt.use_residual,
                                     use_fcn=opt.noiseSize != 1, noise_nc=opt.noise_nc,
                                     add_gaussian_noise=opt.add_gaussian_noise, gaussian_sigma=opt.gaussian_sigma,
                                     upsample_mode=opt.upsample_mode, n_layers_CRN_block=opt.n_layers_CRN_block,
                                     share_label_weights=not opt.no_share_label_block_weights, gpu_ids=self.gpu_ids)
        self.netG = build_G()
        if self.isTrain:
            use_sigmoid = opt.no_lsgan
            assert (len(opt.scale_factor) == len(opt.lambda_D) == len(opt.n_layers_D))
            self.n_netD = len(opt.scale_factor)
            self.netD = []
            for scale, n_layers in zip(opt.scale_factor, opt.n_layers_D):
                d = networks.define_D(opt.input_nc, opt.ndf, opt.which_model_netD, n_layers_D=n_layers, norm=opt.norm,
                                      use_sigmoid=use_sigmoid, scale_factor=scale, gpu_ids=self.gpu_ids)
                d.fuse_sigmoid_into_loss = True
                self.netD.append(d)
            if self.gpu_ids:
                networks.pack_flat(self.netD)   # one arena: single Adam segment, single gradient all-reduce
        self._init_ema(build_G)
        self._init_diffaug()
        if not self.isTrain or opt.continue_train:
            self.load(opt.which_epoch)

        if self.isTrain:
            self.fake_pool = ImagePool(opt.pool_size)
            self.old_lr = opt.lr
            self.criterionGAN = networks.GANLoss(use_lsgan=not opt.no_lsgan)
            self.optimizer_G = FusedAdam(self.netG.parameters(), lr=opt.lr, betas=(opt.beta1, 0.999), zero_grads_in_step=True)
            params = []
            for netD in self.netD:
                params += list(netD.model.parameters())   # "all learnable parameters should be in netD.model"
            self.optimizer_D = FusedAdam(params, lr=opt.lr, betas=(opt.beta1, 0.999))
            self._group = bool(self.gpu_ids) and not getattr(opt, 'no_group', False)
            n_streams = 2 * self.n_netD if (self.gpu_ids and not getattr(opt, 'no_d_streams', False)) else 0
            self._streams = [torch.cuda.Stream(device=self.device) for _ in range(n_streams)]

    # ---- data ---------------------------------------------------------------------------------
    def _draw_noise(self, alt=False):
        """alt: into the second latent buffer (sample_noise_and_prefetch: two latents alive at once)."""
        if alt and getattr(self, '_noise_buf_alt', None) is None:
            self._noise_buf_alt = torch.zeros_like(self._noise_buf)
            self._noise_alt = ops.logical_view(self._noise_buf_alt, self.opt.noise_nc)
        buf, view = (self._noise_buf_alt, self._noise_alt) if alt else (self._noise_buf, self.noise_)
        if self.noise_source is not None:
            z = self.noise_source()
            view.copy_(z)
        elif buf is not None:
            ops.normal_fill_nhwc(buf, self.opt.noise_nc, self._rng_seed, self._rng_offset)
        else:
            ops.normal_fill(view, self._rng_seed, self._rng_offset)
        return view

    def set_input(self, input):
        AorB = self.opt.which_direction == 'A'
        data = input['A' if AorB else 'B']
        idx = self.chnl_idx_input
        run = idx == list(range(idx[0], idx[0] + len(idx)))       # a contiguous channel range ('rg', 'gb', 'r', ...)
        if (self.device.type == 'cuda' and run and data.dim() == 4 and data.shape[0] == 1 and data.dtype == torch.float32
                and data.stride(3) == 1 and (data.is_cuda or data.is_pinned())):
            # one gather kernel reads the batch where it lies (pinned host memory is device-mapped: the kernel IS the H2D copy,
            # queued with the step's kernels), picks the channels and writes the padded NHWC buffer the discriminators read
            _, _, H, W = data.shape
            if getattr(self, '_input_buf', None) is None or self._input_buf.shape[:2] != (H, W):
                self._input_buf = torch.zeros((H, W, 4), dtype=torch.float32, device=self.device)
                self.input = ops.logical_view(self._input_buf, len(idx))
            ops.host_batch_to_nhwc(data[:, idx[0]: idx[0] + len(idx)], self._input_buf)
        else:
            data = data.to(self.device, non_blocking=True).index_select(1, self._chnl_dev)
            self._input_buf = None
            self.input = self.input if self.input.is_contiguous() else torch.empty(0, device=self.device)
            self.input.resize_(data.size()).copy_(data)
        self.image_paths = input.get('A_paths' if AorB else 'B_paths')

    def forward(self):
        self.refuse_eager_step('forward')
        self.real = self.input
        self.noise = self._draw_noise()
        self.netG._keep_next = getattr(self, '_prefetch', False)      # graphed step: forward_pair() refills THIS call's buffers
        self.fake = self.netG.forward(self.noise)

    def sample_noise(self):
        self.real = self.input
        self.noise = self._draw_noise()
        self.fake = self.netG.forward(self.noise)

    # ---- the step's last re-draw and the next step's forward() as one pass over the generator (graph_step.GraphedStep) -----------
    def prefetch_supported(self):
        """The re-draw after the last G update (fcgan_model.py:192-193) and the forward() that opens the next step (:179) see the same
        generator weights and independent latents: GraphedStep runs them as ONE two-problem pass (chain.forward_pair) when the
        generator is a plain chain without dropout state and the latents are drawn on the device."""
        from .chain import ChainNet
        o = self.opt
        return (self.isTrain and o.n_update_G > 1 and o.n_update_D == 1 and self.noise_source is None and self._noise_buf is not None
                and isinstance(self.netG, ChainNet) and hasattr(self.netG, '_wrap_output') and type(self.netG).__name__ == 'FCGANGenerator'
                and not any(L.drop > 0 for L in self.netG.layers))

    def sample_noise_and_prefetch(self):
        """sample_noise() of this step, then forward() of the next one: the same two latents in the same order, one launch per layer.
        `fake` is the re-drawn sample (what the reference leaves behind after a step); adopt_prefetched() installs the other one."""
        from .chain import forward_pair
        if getattr(self, '_noise_buf_alt', None) is None:
            self._noise_buf_alt = torch.zeros_like(self._noise_buf)
            self._noise_alt = ops.logical_view(self._noise_buf_alt, self.opt.noise_nc)
        za, zb = self._noise_alt, self.noise_
        full = getattr(self.netG, '_kept_full', None)
        fused = full is not None and full.numel() * 8 <= (1 << 22) and za.numel() <= 65536
        if fused:      # both latents and the cleared statistics arena of the pass in one launch
            ops.normal_fill_nhwc_pair(self._noise_buf_alt, self._noise_buf, self.opt.noise_nc, self._rng_seed, self._rng_offset, full)
        else:
            self._draw_noise(alt=True)
            self._draw_noise()
        self.noise = za
        self.fake, self._fake_next = forward_pair(self.netG, za, zb, arena_zeroed=fused)

    def adopt_prefetched(self):
        """What forward() would have done: `noise`, `fake` of the step that starts now (already computed by sample_noise_and_prefetch)."""
        self.real = self.input
        self.noise = self.noise_
        self.fake = self._fake_next

    def _draw_test_noise(self):
        """test()'s latent, next in the trainer's stream.  Under the graphed step's prefetch `_noise_buf` is the input of the kept
        forward -- the next step's first-layer backward-weight reads it -- so the draw goes into a buffer of its own."""
        if not getattr(self, '_prefetch', False):
            return self._draw_noise()
        if getattr(self, '_noise_buf_test', None) is None:
            self._noise_buf_test = torch.zeros_like(self._noise_buf)
        ops.normal_fill_nhwc(self._noise_buf_test, self.opt.noise_nc, self._rng_seed, self._rng_offset)
        return ops.logical_view(self._noise_buf_test, self.opt.noise_nc)

    def test(self):
        with torch.no_grad():
            self.noise = self._draw_test_noise()
            self.fake = self._eval_netG().forward(self.noise)

    def get_image_paths(self):
        return self.image_paths

    # ---- losses ---------------------------------------------------------------------------------
    def _d_losses(self, jobs, weights):
        """[(netD, input, target_is_real)], weights -> (total, each): total = sum_i w_i * GANLoss(D_i(x_i), t_i).

        The discriminator chains are independent and individually too small for 256 CUs (a 17x17 layer is 24
        workgroups).  Same-architecture chains run as GROUPED kernels -- one launch per layer for all of them --
        and every loss term plus the scalar arithmetic around it is one forward and one backward kernel.
        Fallback (--no_group or heterogeneous discriminators): one HIP stream per chain, forked from and
        joined back into the current stream."""
        if self._group and networks.can_group([d for d, _, _ in jobs]) and len(jobs) <= 8:
            preds = networks.multi_forward([(d, x) for d, x, _ in jobs])      # one launch per layer for all chains
            return self.criterionGAN.weighted_sum(preds, [r for _, _, r in jobs], weights)
        streams = self._streams[:len(jobs)] if self._streams else None
        losses = []
        if not streams:
            for netD, x, is_real in jobs:
                losses.append(self.criterionGAN(netD.forward(x), is_real))
        else:
            cur = torch.cuda.current_stream()
            # The same net may run on two side streams (fake and real batch): make its derived weight copies (one launch, keyed on the
            # host) on the CURRENT stream before the fork, so that no chain reads a copy another stream is still writing.
            for netD in {id(d): d for d, _, _ in jobs}.values():
                if hasattr(netD, "_refresh_derived"):
                    netD._refresh_derived()
            for st, (netD, x, is_real) in zip(streams, jobs):
                st.wait_stream(cur)
                with torch.cuda.stream(st):
                    l = self.criterionGAN(netD.forward(x), is_real)
                l.record_stream(cur)
                losses.append(l)
            for st in streams:
                cur.wait_stream(st)
        total = 0
        for l, w in zip(losses, weights):
            total = total + l * w
        return total, torch.stack([l.detach() for l in losses])

    def _join_streams(self):
        """The chains' backward kernels (weight-gradient atomics included) ran on the side streams: the
        optimizer step that follows on the current stream must wait for them."""
        cur = torch.cuda.current_stream()
        for st in self._streams:
            cur.wait_stream(st)

    def backward_D(self):
        """loss_D = 0.5 * (sum_i BCE(D_i(fake), 0) + sum_i BCE(D_i(real), 1))   (fcgan_model.py:146-163)"""
        fake = self._pooled(0).detach()
        fake, real = self._augment([fake, self.real], 0)
        n = self.n_netD
        self.loss_D, self._each_D = self._d_losses([(d, fake, False) for d in self.netD] + [(d, real, True) for d in self.netD],
                                                   [0.5] * (2 * n))
        self._backward(self.loss_D)
        self._join_streams()

    def backward_G(self):
        """loss_G = sum_i lambda_i * BCE(D_i(fake), 1)  (log-D trick) or -sum_i lambda_i * BCE(D_i(fake), 0)
        (fcgan_model.py:165-176)"""
        skip = getattr(self.opt, 'skip_wasted_D_wgrad', False)
        for netD in self.netD:
            netD.compute_param_grads = not skip
        trick = not self.opt.no_logD_trick
        fake, = self._augment([self.fake], 2)
        self.loss_G, self._each_G = self._d_losses([(d, fake, trick) for d in self.netD],
                                                   [l if trick else -l for l in self.opt.lambda_D])
        for netD in self.netD:
            netD.compute_param_grads = True
        self._backward(self.loss_G)
        self._join_streams()

    @property
    def loss_D_fake(self):
        return self._each_D[:self.n_netD].sum()

    @property
    def loss_D_real(self):
        return self._each_D[self.n_netD:].sum()

    # ---- the step (fcgan_model.py:178-193), as BaseModel.optimize_parameters and graph_step.GraphedStep run it --------------------
    def step_stages(self):
        o = self.opt
        return [(self.optimizer_D, self.backward_D, o.n_update_D), (self.optimizer_G, self.backward_G, o.n_update_G)]

    def step_zeroing(self):
        return self.optimizer_D.take_zeroing()      # the step's one zeroing launch clears D's gradients too

    def step_pools(self):
        return [(self.fake_pool, lambda: self.fake)]

    def check_graphable(self):
        assert self.opt.n_update_D == 1, "graphed step supports n_update_D == 1 (every README recipe)"

    def get_current_errors(self):
        return OrderedDict([('G_GAN', float(self.loss_G.detach())), ('D_real', float(self.loss_D_real)),
                            ('D_fake', float(self.loss_D_fake))])

    def get_current_visuals(self, save_real=False, save_as_single_image=True):
        out = OrderedDict()
        if self.isTrain or save_real:
            out['real'] = self.real.detach()
        out['fake'] = self.fake.detach()
        return out

    # ---- latent reconstruction (fcgan_model.py:238-319) ---------------------------------------------------------------------------
    def _draw_latent_buffer(self):
        """The next latent in the model's stream (or from `noise_source`), as a copy of the padded NHWC buffer the generator reads."""
        self._draw_noise()
        return self._noise_buf.clone()

    def _reconstructor(self, real, z0, n_steps, lr, graph, lbfgs_kw):
        """One reconstructor -- and so one captured program -- per (image buffer and shape, trial count, settings, arithmetic mode):
        the next image of the same shape only loads its latents and resets the optimizer state."""
        from .reconstruct import LatentReconstructor
        if self._noise_buf is None:
            raise SganError("reconstruction runs on the GPU path with batchSize 1")
        key = (tuple(z0.shape), real.data_ptr(), tuple(real.shape), tuple(real.stride()), int(n_steps), float(lr), bool(graph),
               tuple(sorted(lbfgs_kw.items())), ops.get_math(), self.netG._flat.data_ptr())
        cache = self.__dict__.setdefault('_recon_cache', OrderedDict())
        rec = cache.get(key)
        if rec is None:
            rec = LatentReconstructor(self.netG, real, z0, self.opt.noise_nc, n_steps=n_steps, lr=lr, graph=graph, **lbfgs_kw)
            cache[key] = rec
            while len(cache) > 2:
                cache.popitem(last=False)
        else:
            cache.move_to_end(key)
            rec.reset(z0, real)
        return rec

    def reconstruction(self, num_trials=3, n_steps=50, lr=0.1, graph=True, **lbfgs_kw):
        """Fit latents to `input` by L-BFGS (the reference: 3 trials x 50 step() calls of LBFGS(lr=0.1) with torch's defaults), all
        trials at once.  Returns (rec_error_best, ll_noise_best, ll_noise_init_best): the BCE of the best trial's reconstruction and
        -log N(z; 0, I) of its final and initial latent; sets `fake`, `fake_init` and `noise`.  The best trial is the first with the
        strictly smallest error.  The generator's parameters and buffers are left exactly as they were."""
        from .lbfgs import neg_log_likelihood
        self.real = self.input
        nc = self.opt.noise_nc
        z0 = torch.stack([self._draw_latent_buffer() for _ in range(num_trials)])
        rec = self._reconstructor(self.real, z0, n_steps, lr, graph, lbfgs_kw)
        rec.run()
        imgs_init = rec.images(z0)
        imgs = rec.images(rec.Z)
        errs = rec.errors(imgs)
        ll = [neg_log_likelihood(ops.logical_view(rec.Z[j], nc)) for j in range(num_trials)]
        ll_init = [neg_log_likelihood(ops.logical_view(z0[j], nc)) for j in range(num_trials)]
        best, err_best, ll_best, ll_init_best = None, float('inf'), float('inf'), float('inf')
        for j in range(num_trials):
            if errs[j] < err_best:
                best, err_best, ll_best, ll_init_best = j, errs[j], ll[j], ll_init[j]
        if best is None:        # every error NaN: the reference leaves zero images behind
            self.fake, self.fake_init = torch.zeros_like(self.real), torch.zeros_like(self.real)
        else:
            self.fake, self.fake_init = imgs[best].clone(), imgs_init[best].clone()
            self.noise = ops.logical_view(rec.Z[best].clone(), nc)
        self.recon_trials = dict(errors=errs, ll=ll, ll_init=ll_init, best=best, closures=rec.closures,
                                 latents=[ops.logical_view(rec.Z[j].clone(), nc) for j in range(num_trials)],
                                 latents_init=[ops.logical_view(z0[j], nc) for j in range(num_trials)], counters=rec.opt.counters())
        return err_best, ll_best, ll_init_best

    def reconstruct_cells(self, img, netG, opt, n_bfgs_iter=100, lbfgs_lr=0.1, graph=True, **lbfgs_kw):
        """One trial (fcgan_model.py:278-302): a fresh latent, `n_bfgs_iter` L-BFGS step() calls against `img`.
        Returns (noise_init, noise), logical [1, noise_nc, h, w] tensors."""
        assert netG is self.netG and opt.noise_nc == self.opt.noise_nc
        z0 = self._draw_latent_buffer().unsqueeze(0)
        rec = self._reconstructor(img, z0, n_bfgs_iter, lbfgs_lr, graph, lbfgs_kw)
        rec.run()
        return ops.logical_view(z0[0], opt.noise_nc), ops.logical_view(rec.Z[0].clone(), opt.noise_nc)

    def interpolate(self, alpha):
        """fake = G(alpha * fixed_noiseB + (1 - alpha) * fixed_noiseA)  (fcgan_model.py:304-308)."""
        noise = alpha * self.fixed_noiseB + (1 - alpha) * self.fixed_noiseA
        with torch.no_grad():
            self.fake = self.netG.forward(noise.contiguous())
        self.real = self.input

    def set_fixed_noise(self, which_one):
        """The latent of the last reconstruction becomes fixed_noiseA ('A') or fixed_noiseB (anything else)  (fcgan_model.py:310-314)."""
        if which_one == 'A':
            self.fixed_noiseA = self.noise
        else:
            self.fixed_noiseB = self.noise

    def checkpoint_nets(self):
        return [('G', self.netG)] + self._ema_nets() + [('D_%d' % n, netD) for n, netD in enumerate(self.netD if self.isTrain else [])]

    update_learning_rate = BaseModel.decay_single_rate

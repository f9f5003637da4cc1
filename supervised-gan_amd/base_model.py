"""BaseModel (models/base_model.py:5-64): trainer protocol, the training step and checkpoint I/O.

A trainer states its step once -- step_stages(), and where they apply step_zeroing(), step_pools(), check_graphable() -- and
optimize_parameters() here and graph_step.GraphedStep both run the program built from that statement.

Checkpoint layout is the reference's: one file per network, `<epoch>_net_<label>.pth`, holding the
bare CPU state_dict with the reference's key names and logical shapes.  Loading tolerates old-torch
checkpoints (InstanceNorm running stats present, BatchNorm num_batches_tracked absent)."""
import os
from collections import OrderedDict

import torch

from . import ops
from ._lib import SganError


class BaseModel:
    supports_ema = True       # --ema_decay / --use_ema: the models with ONE generator `netG` (fcgan, cgan, cgan2, segmentation, test); the
                              # cycle and two-stage trainers, which hold several, set it False

    supports_diffaug = False  # --diffaug: the trainers whose backward_D / backward_G carry the hook (fcgan, cgan and what derives from it)

    def name(self):
        return 'BaseModel'

    def initialize(self, opt):
        self.opt = opt
        self.gpu_ids = opt.gpu_ids
        self.isTrain = opt.isTrain
        self.device = torch.device('cuda', self.gpu_ids[0]) if self.gpu_ids else torch.device('cpu')
        self.save_dir = os.path.join(opt.checkpoints_dir, opt.name)
        self.model_dir = getattr(opt, 'pretrained_model_dir', '')
        self.grad_sync = None            # data-parallel hook: callable(optimizer) run between backward and step
        self._pool_overrides = None      # graphed step: one static buffer per step_pools() entry, read instead of querying the pool
        self.ema = None                  # optim.WeightEMA over (netG, netG_ema) under --ema_decay (_init_ema)
        if (getattr(opt, 'ema_decay', None) is not None or getattr(opt, 'use_ema', False)) and not self.supports_ema:
            raise NotImplementedError("--ema_decay / --use_ema average the one generator of fcgan, cgan, cgan2 and segmentation; "
                                      "--model %s is not among them" % getattr(opt, 'model', self.name()))

        self.diffaug = None              # diffaug.DiffAugment under --diffaug (_init_diffaug)
        if getattr(opt, 'diffaug', None) is not None and not self.supports_diffaug:
            from .diffaug import SUPPORTED_MODELS
            raise NotImplementedError("--diffaug augments the discriminator inputs of --model %s; --model %s is not among them"
                                      % (', '.join(SUPPORTED_MODELS), getattr(opt, 'model', self.name())))

    def Tensor(self, *size):
        return torch.empty(*size, dtype=torch.float32, device=self.device)

    def _own_rng_streams(self, *nets):
        """Every network of a trainer with more than one generator draws from Philox keys of its own: the trainer's seed in the
        low word, the net's position (1, 2, ...) in the high word.  The nets add small integers (level, block, stage) to their
        key and each counts its own offset from 0, so without this two generators of equal shape would draw the same dropout
        masks and noise on every step; the trainer's own latent keys (seed + small integer, high word 0) stay clear of all of them."""
        for i, net in enumerate(nets, 1):
            if net is not None:
                net._rng_seed = ops.net_stream_seed(self._rng_seed, i)

    def _backward(self, loss):
        """loss.backward() with a cached unit gradient (autograd would launch a fill kernel for it on every call)."""
        one = getattr(self, '_grad_one', None)
        if one is None or one.device != loss.device or one.shape != loss.shape:
            one = self._grad_one = torch.ones_like(loss)
            ops.register_unit_grad(one)      # fused loss nodes skip the rescaling of their gradients for this tensor
        loss.backward(one)

    def set_input(self, input):
        self.input = input

    def get_current_visuals(self):
        return self.input

    def get_current_errors(self):
        return {}

    # ---- exponential moving average of the generator's weights (--ema_decay; optim.WeightEMA) ------------------------
    def _init_ema(self, build_G):
        """Under --ema_decay (training only): netG_ema, a second generator from the same define_G call `build_G` (a deepcopy would
        lose the arenas and the .grad views), loaded from netG, with netG's Philox key, in no optimizer; self.ema averages netG into
        it.  Call it once netG and the discriminators exist (the discriminators' initial weights then do not depend on the option)
        and before load()."""
        from .optim import WeightEMA
        decay = getattr(self.opt, 'ema_decay', None)
        if not self.isTrain or decay is None:
            return
        self.netG_ema = build_G()
        self.netG_ema.load_state_dict(self.netG.state_dict())
        if hasattr(self.netG, '_rng_seed'):
            self.netG_ema._rng_seed = self.netG._rng_seed
        self.ema = WeightEMA(self.netG, self.netG_ema, decay, getattr(self.opt, 'ema_warmup', False))

    def averaged_generator(self):
        """Under --ema_eval: netG_ema, made ready for evaluation (WeightEMA.prepare_eval(): the live buffers, and derived weight copies
        that a replayed step cannot have kept current); None otherwise.  The preparation holds until the next training step: a pass
        of many forwards (train_ss.validate) asks once and hands the network to each of them."""
        if self.ema is not None and getattr(self.opt, 'ema_eval', False):
            self.ema.prepare_eval()
            return self.netG_ema
        return None

    def _eval_netG(self):
        """The generator one test() or one validation forward runs: the average under --ema_eval, prepared for this call, else netG."""
        return self.averaged_generator() or self.netG

    def _ema_nets(self):
        """checkpoint_nets() entry of the averaged generator: [('G_ema', netG_ema)] under --ema_decay, else nothing."""
        return [('G_ema', self.netG_ema)] if self.ema is not None else []

    # ---- differentiable augmentation of the discriminator inputs (--diffaug; diffaug.DiffAugment) ---------------------
    def _init_diffaug(self, has_netD=True):
        """Under --diffaug (training only): self.diffaug, keyed by the trainer's seed.  Call it once _rng_seed is set."""
        if not self.isTrain or getattr(self.opt, 'diffaug', None) is None:
            return
        from .diffaug import DiffAugment, check_options
        if not has_netD:
            raise ValueError("--diffaug with --which_model_netD None: there is no discriminator input to augment")
        if getattr(self.opt, 'diffaug_policy', None) is None:      # an options object that did not go through parse()
            check_options(self.opt)
        self.diffaug = DiffAugment.from_options(self.opt, self._rng_seed, self.device)

    def _augment(self, tensors, slot):
        """The tensors a discriminator call is about to see, each through a transform drawn now (slots: DiffAugment.SLOTS); as they
        are without --diffaug.  Sits between building fake / real and _d_losses, after the ImagePool query: the pool keeps plain images."""
        if self.diffaug is None:
            return tensors
        return self.diffaug.augment(tensors, slot)

    def _file_label(self, net_label):
        """--use_ema (test side): netG is read from `<epoch>_net_G_ema.pth`."""
        return 'G_ema' if net_label == 'G' and not self.isTrain and getattr(self.opt, 'use_ema', False) else net_label

    # ---- the training step -------------------------------------------------------------------------
    def step_stages(self):
        """[(optimizer, backward method, updates per step), ...] in the order the step runs them."""
        raise NotImplementedError

    def step_zeroing(self):
        """Gradient buffers the step's first launch (ops.begin_step) clears together with the statistics arenas."""
        return ()

    def step_pools(self):
        """[(ImagePool, callable -> what the step hands to its query()), ...] in the reference's query order."""
        return []

    def check_graphable(self):
        """Asserts what graph_step.GraphedStep needs of this trainer's options before it captures the step."""

    def step_program(self):
        """The step after forward(): lists of calls, with a ("sync", optimizer) item where the data-parallel gradient exchange goes."""
        program = []
        for optimizer, backward, n_updates in self.step_stages():
            for _ in range(n_updates):
                program += [[optimizer.zero_grad, backward], ("sync", optimizer), [optimizer.step]]
                if self.ema is not None and optimizer is self.optimizer_G:
                    program[-1].append(self.ema.update)      # with data parallelism every rank averages its identical weights
                if n_updates > 1:
                    program[-1].append(self.sample_noise)
        if self.ema is not None and hasattr(self, 'prefetch_supported') and self.prefetch_supported():
            # graph_step.GraphedStep replaces this slot with the prefetching re-draw
            assert program[-1][-1] == self.sample_noise, "the step's last call must be the re-draw when prefetch is supported"
        return program

    def run_program(self, program):
        for item in program:
            if isinstance(item, list):
                for call in item:
                    call()
            elif self.grad_sync is not None:
                self.grad_sync(item[1])

    def refuse_eager_step(self, what):
        """A trainer whose step graph_step.GraphedStep captured with prefetch keeps one generator forward alive between two steps, in
        buffers the graphs point into (netG._kept, its statistics arena): an eager forward() or optimize_parameters() would allocate
        that forward anew and zero the arena under them.  Raises before anything is launched unless GraphedStep itself is calling."""
        if getattr(self, '_prefetch', False) and not getattr(self, '_graphed_call', False):
            raise SganError("%s() on a trainer whose step was captured with prefetch: the captured graphs read the generator forward "
                            "this call would replace; run GraphedStep.step() (test() is safe between two steps)" % what)

    def optimize_parameters(self):
        self.refuse_eager_step('optimize_parameters')
        ops.begin_step(self.step_zeroing())      # one launch zeroes every statistics arena of the step
        self.forward()
        self.run_program(self.step_program())

    def _pooled(self, i):
        """Fake number `i` of the discriminator step: the answer of its ImagePool, or the buffer the graphed step filled with it."""
        if self._pool_overrides is not None:
            return self._pool_overrides[i]
        pool, source = self.step_pools()[i]
        return pool.query(source())

    # ---- learning-rate schedules: `update_learning_rate` of a trainer is one of these -----------------
    def decay_single_rate(self):
        """fcgan / cgan / segmentation (fcgan_model.py:224-236): every group at old_lr - lr / niter_decay, not clamped."""
        lr = self.old_lr - self.opt.lr / self.opt.niter_decay
        for optimizer, _, _ in self.step_stages():
            for group in optimizer.param_groups:
                group['lr'] = lr
            optimizer.sync_lr()
        print('update learning rate: %f -> %f' % (self.old_lr, lr))
        self.old_lr = lr

    def decay_three_rates(self):
        """The cycle and two-stage trainers (twostage_cycle_model.py:477-500): lr, lr1, lr2 each fall by their own base / niter_decay
        down to 0; the groups named G1 / D1 follow lr1, G2 / F2 / D2 follow lr2, any other lr."""
        new = {k: max(0, getattr(self, 'old_' + k) - getattr(self.opt, k) / self.opt.niter_decay) for k in ('lr', 'lr1', 'lr2')}
        follows = {'G1': 'lr1', 'D1': 'lr1', 'G2': 'lr2', 'F2': 'lr2', 'D2': 'lr2'}
        for optimizer, _, _ in self.step_stages():
            for group in optimizer.param_groups:
                group['lr'] = new[follows.get(group.get('name'), 'lr')]
            optimizer.sync_lr()
        print('update learning rate: %f -> %f, %f -> %f' % (self.old_lr1, new['lr1'], self.old_lr2, new['lr2']))
        self.old_lr, self.old_lr1, self.old_lr2 = new['lr'], new['lr1'], new['lr2']

    # ---- checkpoints -----------------------------------------------------------------------------
    def checkpoint_nets(self):
        """[(label, network)]: every network this trainer holds, under the label of its checkpoint file."""
        return []

    def save(self, label):
        if self.ema is not None:
            self.ema.prepare_eval()      # the averaged generator is saved with the live buffers (BatchNorm statistics are not averaged)
        for net_label, net in self.checkpoint_nets():
            self.save_network(net, net_label, label, gpu_ids=self.gpu_ids)

    def load(self, epoch_label, only=None, model_dir=''):
        """Reads every network's file; `only`: the networks whose label (a discriminator's without its `_<n>`) it names."""
        for net_label, net in self.checkpoint_nets():
            if only is None or net_label.split('_')[0] in only:      # 'G_ema' goes with 'G'
                if net is getattr(self, 'netG_ema', None):
                    self._load_ema(epoch_label, model_dir)
                else:
                    self.load_network(net, net_label, epoch_label, model_dir=model_dir)

    def _load_ema(self, epoch_label, model_dir=''):
        """--continue_train under --ema_decay: the saved average goes on at d_t = decay (the counter is not in the checkpoint); a
        run saved without one starts its average from the weights just loaded."""
        path = self._checkpoint_path('G_ema', epoch_label, model_dir)
        if os.path.exists(path):
            self.load_network(self.netG_ema, 'G_ema', epoch_label, model_dir=model_dir)
            self.ema.skip_warmup()
        else:
            print('%s not found: the average restarts from the loaded generator' % path)
            self.ema.reset_from_live()

    def _checkpoint_path(self, network_label, epoch_label, model_dir):
        """`<epoch>_net_<label>.pth` under the run's directory, or under --pretrained_model_dir when the caller asks for the
        pretrained copy (any true `model_dir`: the reference ignores its value and reads opt.pretrained_model_dir, :46-49,56-59)."""
        return os.path.join(self.model_dir if model_dir else self.save_dir, '%s_net_%s.pth' % (epoch_label, network_label))

    def save_network(self, network, network_label, epoch_label, gpu_ids=[], model_dir=''):
        path = self._checkpoint_path(network_label, epoch_label, model_dir)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        # same file content as torch.save(network.cpu().state_dict(), path), without moving the live module off the GPU
        torch.save(OrderedDict((k, v.detach().to('cpu').contiguous()) for k, v in network.state_dict().items()), path)

    def load_network(self, network, network_label, epoch_label, model_dir=''):
        network_label = self._file_label(network_label)      # --use_ema: 'G' is read from the averaged generator's file
        path = self._checkpoint_path(network_label, epoch_label, model_dir)
        if network_label == 'G_ema' and not os.path.exists(path):
            raise FileNotFoundError("%s not found: --use_ema reads the averaged generator a run with --ema_decay saves" % path)
        load_state_dict_compat(network, torch.load(path, map_location='cpu'))


def _not_overridden(self, *args, **kwargs):
    return None


# the rest of the trainer protocol: hooks a subclass overrides, no-ops here (models/base_model.py:21-39,63-64)
for _hook in ('forward', 'test', 'get_image_paths', 'update_learning_rate'):
    setattr(BaseModel, _hook, _not_overridden)


def load_state_dict_compat(network, sd):
    """load_state_dict that accepts checkpoints written by torch <= 0.3 (the reference's authoring
    era): those carry `running_mean/var` for InstanceNorm2d(affine=False) layers (dropped here: the
    layers never used them) and lack BatchNorm `num_batches_tracked`."""
    own = network.state_dict()
    clean = OrderedDict()
    for k, v in sd.items():
        if k in own:
            clean[k] = v
        elif k.endswith('running_mean') or k.endswith('running_var'):
            continue   # stale InstanceNorm buffers
        else:
            raise KeyError('unexpected key %s in checkpoint' % k)
    missing = [k for k in own if k not in clean and not k.endswith('num_batches_tracked')]
    if missing:
        raise KeyError('missing keys in checkpoint: %s' % missing)
    network.load_state_dict(clean, strict=False)

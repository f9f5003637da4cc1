"""Latent reconstruction of fcgan (models/fcgan_model.py:238-302): fit latents z to a real image by L-BFGS on
BCELoss((G(z) + 1) / 2, (real + 1) / 2), several trials at once.

Grouped path (a plain FCGANGenerator chain without dropout): the J trial latents go through the generator as ONE grouped pass --
one launch per layer for all trials -- then one BCE kernel per trial (loss and gradient), the tanh backward and the backward-data
chain into the latent-gradient buffers, then ONE sgan_lbfgs_advance launch for all trials.  No weight gradients, no BatchNorm
running-statistics updates: the generator comes out bit-identical.  That program is captured once into a hipGraph and replayed; the
`done` flags of the trials are read every `check_every` replays.  The graph owns what it points into: its statistics arenas are
allocated (and zero-filled) inside the capture from a private arena pool (ops.arena_scope), never from the pool of a training step.
Every eager pass of a reconstruction (closures, the final images) takes its arenas from a second private pool, so a reconstruction
never touches the arenas a training step -- eager or captured -- holds.  One reconstructor serves every image of the same shape and
trial count (reset() loads the next latents and fresh optimizer state; the captured program is reused).

Eager path: the same program without the graph (graph=False), and the fallback for generators that are not a plain chain
(fcgan_star) or that draw dropout masks (a mask per closure evaluation, as in the reference); there every trial's closure is one
autograd call of netG.forward and the BatchNorm running statistics are restored afterwards."""
import torch

from . import ops
from .chain import ChainNet, _grouped_backward, _grouped_forward
from .lbfgs import DeviceLBFGS
from .losses import bce_on_rescaled


def grouped_supported(netG):
    return (isinstance(netG, ChainNet) and type(netG).__name__ == "FCGANGenerator" and not any(L.drop > 0 for L in netG.layers))


class LatentReconstructor:
    """J trials of `n_steps` torch LBFGS step() calls each against one real image.

    z0: [J, h, w, Cs] initial latents (padded NHWC, the generator's input layout; padding channels zero).  real: logical [1, C, H, W]
    image on the GPU.  Latents that stay in padding channels stay zero: their gradient is exactly zero."""

    def __init__(self, netG, real, z0, noise_nc, n_steps=50, lr=0.1, graph=True, check_every=20, **lbfgs_kw):
        self.netG, self.J, self.nc = netG, int(z0.shape[0]), int(noise_nc)
        self.dev = z0.device
        self.real = real
        self.C = int(real.shape[1])
        self.grouped = grouped_supported(netG)
        self.graph = bool(graph) and self.grouped
        self.check_every = int(check_every)
        self.Z = z0.detach().clone().contiguous()
        self.G = torch.zeros_like(self.Z)
        self.loss = torch.zeros(self.J, dtype=torch.float32, device=self.dev)
        self.n = self.Z[0].numel()
        self.opt = DeviceLBFGS(self.n, self.J, lr=lr, n_steps=n_steps, device=self.dev, **lbfgs_kw)
        self.closures = 0
        self._graph = None
        self._arenas = ops.ArenaPool()         # the captured program's arenas (allocated inside the capture)
        self._eager_arenas = ops.ArenaPool()   # every eager pass of this reconstructor

    def reset(self, z0, real=None):
        """Next image: new initial latents (and image), fresh optimizer state; a captured program stays valid as long as the image
        buffer it reads is the same."""
        self.Z.copy_(z0)
        if real is not None:
            self.real = real
        self.opt.reset()
        self.closures = 0

    # ---- one closure evaluation of every trial: loss[j], G[j] = d loss_j / d Z[j] ---------------------------------------------
    def _closure_grouped(self):
        nets = [self.netG] * self.J
        xs = [self.Z[j] for j in range(self.J)]
        real_buf = ops.as_nhwc(self.real)
        outs, stats = _grouped_forward(nets, xs, update_running=False)
        gs = []
        for j in range(self.J):
            g = torch.empty_like(outs[j][-1])
            ops.bce01_fwd(outs[j][-1], real_buf, self.C, self.loss[j], g)
            gs.append(g)
        _grouped_backward(nets, xs, outs, stats, gs, [True] * self.J, [False] * self.J, dx_out=[self.G[j] for j in range(self.J)])

    def _closure_eager(self):
        nc = self.nc
        wg, self.netG.compute_param_grads = getattr(self.netG, "compute_param_grads", True), False     # latent gradient only
        try:
            for j in range(self.J):
                z = ops.logical_view(self.Z[j], nc).detach().clone().requires_grad_(True)
                loss = bce_on_rescaled(self.netG.forward(z), self.real)
                (gz,) = torch.autograd.grad(loss, z)
                self.loss[j].copy_(loss.detach())
                self.G[j].zero_()
                self.G[j].permute(2, 0, 1)[:nc].copy_(gz[0])
        finally:
            self.netG.compute_param_grads = wg

    def _program(self):
        if self.grouped:
            self._closure_grouped()
        else:
            self._closure_eager()
        self.opt.advance(self.loss, self.G.view(self.J, self.n), self.Z.view(self.J, self.n))

    def _capture(self):
        stream = torch.cuda.Stream(device=self.dev)
        stream.wait_stream(torch.cuda.current_stream())
        self.netG._refresh_derived()
        with torch.cuda.stream(stream), ops.arena_scope(self._eager_arenas):
            self._closure_grouped()             # warm-up closure (no advance): lazy state exists before the capture
        stream.synchronize()
        self._graph = torch.cuda.CUDAGraph()
        with ops.arena_scope(self._arenas, begin=False):
            with ops.graph_capture(self._graph, stream=stream):
                self._program()
        torch.cuda.current_stream().wait_stream(stream)

    def run(self, max_calls=None):
        """Replay closure + advance until every trial is done.  Returns the number of closure evaluations issued per trial."""
        h = self.opt.hyper
        limit = max_calls if max_calls is not None else h["n_steps"] * (h["max_eval"] + 1) + 1
        snapshot = None
        if not self.grouped:
            snapshot = [b.detach().clone() for b in self.netG.buffers()]
        try:
            if self.graph:
                if self._graph is None:
                    self._capture()
                self.netG._refresh_derived()    # weights changed since the capture (a training step): the copies the graph reads
            while self.closures < limit:
                k = min(self.check_every, limit - self.closures)
                for _ in range(k):
                    if self.graph:
                        self._graph.replay()
                    else:
                        with ops.arena_scope(self._eager_arenas):
                            self._program()
                self.closures += k
                if all(self.opt.done()):
                    break
        finally:
            if snapshot is not None:
                with torch.no_grad():
                    for b, v in zip(self.netG.buffers(), snapshot):
                        b.copy_(v)
        return self.closures

    def images(self, Z):
        """G(Z[j]) for every row of Z ([K, h, w, Cs], K <= 8): logical [1, C, H, W] tensors, no running-statistics update."""
        with torch.no_grad(), ops.arena_scope(self._eager_arenas):
            if self.grouped:
                outs, _ = _grouped_forward([self.netG] * Z.shape[0], [Z[k] for k in range(Z.shape[0])], update_running=False)
                return [ops.logical_view(o[-1], self.C) for o in outs]
            snapshot = [b.detach().clone() for b in self.netG.buffers()]
            nc = self.nc
            ys = [self.netG.forward(ops.logical_view(Z[k].contiguous(), nc)).clone() for k in range(Z.shape[0])]
            for b, v in zip(self.netG.buffers(), snapshot):
                b.copy_(v)
            return ys

    def errors(self, images):
        """BCELoss((y + 1) / 2, (real + 1) / 2) of each image, on the host (one read-back)."""
        real_buf = ops.as_nhwc(self.real)
        out = torch.zeros(len(images), dtype=torch.float32, device=self.dev)
        for k, y in enumerate(images):
            yb = ops.as_nhwc(y)
            ops.bce01_fwd(yb, real_buf, self.C, out[k], torch.empty_like(yb))
        return [float(v) for v in out.cpu()]

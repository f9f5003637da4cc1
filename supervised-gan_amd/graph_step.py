"""hipGraph capture of a trainer's optimize_parameters (models/fcgan_model.py:178-193, models/cgan_model.py:212-226, ...).  Every
trainer states its step once (BaseModel.step_stages); BaseModel.optimize_parameters runs the program built from it launch by
launch, GraphedStep captures the very same program.

A bs=1 step is a few hundred short kernels; launched eagerly from Python the host is the bottleneck.
The step is therefore captured once into hipGraphs and replayed:

    graph A : forward()                      latent fill + G forward -> static `fake` (cgan: cat(real_A, fake_B))
    host    : ImagePool.query(fake)          the reference's python-random history policy, one D2D copy
    graph B : BaseModel.step_program()       D step(s), then the G step(s): zero_grad / backward / Adam, loss scalars left on device

Everything that changes from step to step lives in device memory the kernels read and advance
themselves (Adam step counter and LR, Philox offset, BatchNorm num_batches_tracked), so replays are
faithful.  With data parallelism the gradient all-reduce is not captured: graph B is cut at the
program's ("sync", optimizer) items -- one per update -- and RCCL runs between the pieces on the same stream.

Prefetch (fcgan with n_update_G > 1): the re-draw that ends a step and the forward() that opens the next one are two generator
passes over the same weights, each a chain of launches too small to fill the card (~100 us for 4 GFLOP).  The graphed step runs
them as ONE two-problem pass at the end of graph B (FCGANModel.sample_noise_and_prefetch -> chain.forward_pair) which writes the
second problem into the buffers of the forward the captured backward was built on; graph A disappears.  Same latents in the same
order, same BatchNorm running-statistics updates in the same order.  SGAN_NO_G_PREFETCH=1 switches it off.

Between two steps a prefetching GraphedStep is therefore ONE generator forward ahead of the eager trainer, and so is a checkpoint
saved there: every generator BatchNorm's num_batches_tracked is the eager count + 1, running_mean / running_var carry that
forward's update, and the trainer's Philox offset is the eager offset plus the draws of one forward().  After the eager trainer's
next set_input(); forward() the two agree again (tests/test_graph_step_snapshot.py holds the integer identities)."""
import contextlib
import os

import torch

from . import ops


class GraphedStep:
    """Captures the step a trainer declares (base_model.BaseModel): `step_program()` is what graph B runs, `step_zeroing()` what the
    first launch clears, `step_pools()` the ImagePools the host queries between the graphs, `_pool_overrides` the static buffers
    the discriminator step reads in their place, `check_graphable()` the trainer's own preconditions.

    With prefetch the state between two steps is one generator forward ahead of the eager trainer's (module docstring): BatchNorm
    num_batches_tracked + 1 with the matching running statistics, the Philox offset advanced by one forward()'s draws.  A trainer
    whose step was captured with prefetch refuses an eager forward() / optimize_parameters() of its own (they would re-allocate
    the kept forward the graphs point into); test() is safe between two replays."""

    def __init__(self, model, warmup_steps=2):
        self.m = model
        model.check_graphable()
        assert model.opt.batchSize == 1
        self._captured = False
        self._warmup_steps = warmup_steps
        self._arenas = ops.ArenaPool()      # a captured program owns the pool its arenas came from: the graphs point into its slots
        self._prefetch = (hasattr(model, "prefetch_supported") and model.prefetch_supported()
                          and os.environ.get("SGAN_NO_G_PREFETCH", "0") in ("", "0"))
        self._launched = False      # the last step ran launch by launch (step(replay=False)): reinstall() before the next replay

    def _begin(self):
        """Start of a step: the arenas' zeroing launch, which also clears the gradient buffers the trainer folds into it."""
        ops.begin_step(self.m.step_zeroing())

    def capture(self, example_input):
        """Warm-up steps, the eager run of the graph's own program and every capture draw their arenas from this step's own pool;
        replays do not touch a pool on the host."""
        with ops.arena_scope(self._arenas), self._own_calls():
            self._capture_all(example_input)

    @contextlib.contextmanager
    def _own_calls(self):
        """Inside the block the trainer's forward() / optimize_parameters() are this object's calls: a trainer captured with
        prefetch refuses them from anybody else (BaseModel.refuse_eager_step)."""
        m = self.m
        saved, m._graphed_call = getattr(m, "_graphed_call", False), True
        try:
            yield
        finally:
            m._graphed_call = saved

    def _capture_all(self, example_input):
        m = self.m
        assert getattr(m, "noise_source", None) is None, "graphed step draws its latents on the device"
        program, pools = m.step_program(), m.step_pools()
        if self._prefetch:
            program[-1][-1] = m.sample_noise_and_prefetch      # the step's last re-draw also runs the next step's forward()
        sources = lambda: [source() for _, source in pools]      # noqa: E731
        for _ in range(self._warmup_steps - (1 if self._prefetch else 0)):   # lazy state (optimizer moments, caches) must exist before capture
            m.set_input(example_input)
            m.optimize_parameters()
        if self._prefetch:
            # the last warm-up step runs the graph's own program eagerly: the arena pool then holds the sequence of arenas the
            # capture is going to ask for, and the step ends with the first two-problem pass (the next forward() is in place)
            # ON the stream the capture will use: autograd runs a node's backward on the stream its forward ran on, and the capture's
            # first backward walks the node this pass leaves behind (a backward hopping to the default stream mid-capture crashed
            # hipStreamEndCapture)
            m._prefetch = True
            m.set_input(example_input)
            self._cap_stream = torch.cuda.Stream(device=m.device)
            self._cap_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self._cap_stream):
                self._begin()
                m.forward()
                m.run_program(program)
            torch.cuda.current_stream().wait_stream(self._cap_stream)
        for optimizer, _, _ in m.step_stages():
            optimizer.sync_lr()
        torch.cuda.synchronize()
        if self._prefetch:
            m.adopt_prefetched()
        self.pools = [pool for pool, _ in pools]
        shapes = [tuple(t.shape) for t in sources()]
        self.fake_for_D = [torch.zeros((h, w, ops.pad4(nc)), dtype=torch.float32, device=m.device) for (_, nc, h, w) in shapes]
        m._pool_overrides = [ops.logical_view(buf, sh[1]) for buf, sh in zip(self.fake_for_D, shapes)]
        # with a process group alive its watchdog thread polls CUDA events: only the capturing thread is held to the
        # capture rules then (PyTorch's recipe for graphs next to NCCL)
        dist_on = torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1
        self._mode = "thread_local" if dist_on else "global"
        if dist_on:
            torch.distributed.barrier()
            torch.cuda.synchronize()
        if self._prefetch:
            self.gA = None
            self._fakeA = sources()      # the kept forward's output: every replay's two-problem pass rewrites it in place
            pool = None
            merged = [self._begin]
        else:
            self.gA = torch.cuda.CUDAGraph()
            self.fnsA = [self._begin, m.forward]      # _begin: the statistics arenas of the whole step (graph A and every piece of graph B), one launch
            with ops.graph_capture(self.gA, capture_error_mode=self._mode):
                for f in self.fnsA:
                    f()
                self._fakeA = sources()
            pool = self.gA.pool()
            merged = []
        self.segs, self.seg_fns = [], []      # seg_fns[i]: the calls segs[i]'s graph was captured from (None beside a sync item)
        for item in program:
            if isinstance(item, list):
                merged += item
            elif m.grad_sync is not None:        # ("sync", optimizer): data-parallel hand-off point, graph B is cut here
                self.segs.append(("graph", self._capture(merged, pool, self._mode)))
                self.segs.append(item)
                self.seg_fns += [merged, None]
                merged = []
        if merged:
            self.segs.append(("graph", self._capture(merged, pool, self._mode)))
            self.seg_fns.append(merged)
        self._captured = True
        torch.cuda.synchronize()
        if self._prefetch:
            self._fake_last = m.fake      # the re-drawn sample of the step just finished: what `fake` is between steps
        self._step_tensors = {k: v for k, v in vars(m).items() if torch.is_tensor(v)}

    @property
    def captured(self):
        return self._captured

    def reinstall(self):
        """Point the trainer's tensor attributes at the captured step's tensors again.  An eager forward() between two replays (a
        validation pass) leaves fake_B, logit, ... naming its own results, and a replay only writes the captured ones: call this
        before the next step() so that whatever reads the attributes after it sees the step's results."""
        vars(self.m).update(self._step_tensors)

    def _capture(self, fns, pool, mode="global"):
        g = torch.cuda.CUDAGraph()
        if pool is None:
            pool = getattr(self, "_pool", None)
        with ops.graph_capture(g, pool=pool, stream=getattr(self, "_cap_stream", None), capture_error_mode=mode):
            for f in fns:
                f()
        self._pool = g.pool()
        return g

    def step(self, data=None, replay=True):
        """One training step == model.optimize_parameters() (set_input first when data is given).

        replay=False (a test seam): the same host sequence with every graph replay replaced by the calls the graph was captured
        from, launch by launch on a side stream (the capture's own where there is one) inside this step's arena pool -- the
        reference a replay is compared with from one device state (tests/test_graph_step_snapshot.py).  The trainer's attributes
        then name that step's own results (losses, outputs) until the next replay=True step, which starts with reinstall()."""
        m = self.m
        if not replay:
            return self._step_launches(data)
        if self._launched:
            self.reinstall()
            self._launched = False
        if data is not None:
            m.set_input(data)
        if self._prefetch:
            m.adopt_prefetched()      # host attributes only: the forward itself ran at the end of the previous step
        else:
            self.gA.replay()
        self._query_pools(self._fakeA)
        for kind, obj in self.segs:
            if kind == "graph":
                obj.replay()
            else:
                m.grad_sync(obj)
        if self._prefetch:
            m.fake, m.noise = self._fake_last, m._noise_alt

    def _query_pools(self, sources):
        for pool, src, buf in zip(self.pools, sources, self.fake_for_D):      # the reference's query order
            # a copy KERNEL on the step's stream: Tensor.copy_ of a contiguous tensor is hipMemcpyAsync, which on this stack starts
            # ~100 us after the work queued before it (measured: profiles/r02 timeline), a bubble in every step
            q = ops.as_nhwc(pool.query(src))
            ops.slice_nhwc(q, 0, q.shape[2], out=buf)

    def _step_launches(self, data):
        """step(replay=False).  Same arenas, same static buffers (fake_for_D, the kept forward under prefetch), same device-side
        counters as the replays; activations and losses are this call's own tensors."""
        m = self.m
        if data is not None:
            m.set_input(data)
        stream = getattr(self, "_cap_stream", None) or getattr(self, "_launch_stream", None)
        if stream is None:
            stream = self._launch_stream = torch.cuda.Stream(device=m.device)
        caller = torch.cuda.current_stream()
        stream.wait_stream(caller)
        with ops.arena_scope(self._arenas, begin=False), self._own_calls(), torch.cuda.stream(stream):
            if self._prefetch:
                m.adopt_prefetched()
                sources = self._fakeA
            else:
                for f in self.fnsA:
                    f()
                sources = [source() for _, source in m.step_pools()]
            self._query_pools(sources)
            for (kind, obj), fns in zip(self.segs, self.seg_fns):
                if kind == "graph":
                    for f in fns:
                        f()
                else:
                    m.grad_sync(obj)
        caller.wait_stream(stream)
        if self._prefetch:
            # `fake` / `noise` already name the re-drawn sample; the node the two-problem pass left on the kept forward is the one
            # the next launch-by-launch step walks (an autograd node is walked once), over the memory the graphs read
            self._step_tensors["_fake_next"] = m._fake_next
        self._launched = True

GraphedFCGANStep = GraphedStep

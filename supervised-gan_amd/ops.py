"""Thin torch-tensor -> pointer wrappers over the C ABI (include/sgan_hip.h).

Activation tensors are `[H, W, Cs]` fp32 CUDA tensors (NHWC, batch 1, Cs = stored channels, a
multiple of 4; `tensor.stride(1)` is the pixel stride so channel slices of wider buffers work).
Everything here launches on torch's current stream and never synchronises."""
import contextlib
import ctypes as C
import gc
import weakref

import torch

from . import _lib as L
from ._lib import ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH, CONV, CONVT  # noqa: F401


def pad4(c: int) -> int:
    return (c + 3) // 4 * 4


# Arithmetic of the MFMA conv kernels (sgan_conv_desc.math): "bf16x3" = split-bf16 (fp32-equivalent, ~2^-16 per product,
# 16/3 of the fp32 matrix rate; the default), "f32" = exact fp32 MFMA (the parity mode), "bf16x1" (alias "bf16") = one 16-bit
# plane, hi(a) * hi(b), the speed mode (~2^-9 per bf16 operand; storage, accumulation, norms, losses and Adam stay fp32).
# SGAN_MATH selects at start-up, set_math() at run time (every conv call stamps the current mode into its descriptor).
_MATH_NAMES = {"f32": L.MATH_F32, "fp32": L.MATH_F32, "bf16x3": L.MATH_BF16X3, "bf16x1": L.MATH_BF16X1, "bf16": L.MATH_BF16X1}
_MATH_LABEL = {L.MATH_F32: "f32", L.MATH_BF16X3: "bf16x3", L.MATH_BF16X1: "bf16x1"}
_math = _MATH_NAMES[__import__("os").environ.get("SGAN_MATH", "bf16x3").lower()]


_DGRAD_MATH = _MATH_NAMES.get(__import__("os").environ.get("SGAN_DGRAD_MATH", "").lower())      # diagnostics: backward-data only


def set_math(name: str):
    global _math
    _math = _MATH_NAMES[name.lower()]


def get_math() -> str:
    return _MATH_LABEL[_math]


def uses_16bit() -> bool:
    """Does the current mode run the 16-bit MFMA kernels (bf16x3 or bf16x1)?  They read the packed weight copies and the published
    gradient maxima; the f32 mode reads neither."""
    return _math != L.MATH_F32


class math_scope:
    """`with ops.math_scope("f32"):` -- the conv calls inside run in that arithmetic mode (None: leave the current one)."""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        global _math
        self.prev = _math
        if self.name is not None:
            _math = _MATH_NAMES[self.name.lower()]

    def __exit__(self, *exc):
        global _math
        _math = self.prev
        return False


def with_packed(w: torch.Tensor, packed, packed_f16=None) -> torch.Tensor:
    """Tag a weight slice with the matching slice of the split 16-bit copy (sgan_pack_weights) for the job builders; packed_f16:
    the fp16-plane twin of the backward copy (backward-data with a known gradient maximum reads it)."""
    w._sgan_pk = packed
    w._sgan_pk16 = packed_f16
    return w


def _amax(t):
    """Device scalar max|t| when the producer published one (norm_bwd_apply*), else None."""
    a = getattr(t, "_sgan_amax", None)
    return a.data_ptr() if (a is not None and uses_16bit()) else None


def _pk16(w):
    pk = getattr(w, "_sgan_pk16", None)
    return pk.data_ptr() if (pk is not None and uses_16bit()) else None


def _pk(w):
    pk = getattr(w, "_sgan_pk", None)
    return pk.data_ptr() if (pk is not None and uses_16bit()) else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def require_gpu(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise L.SganError(f"{what}: supervised_gan_amd kernels run on an MI355X (gfx950) only; got a {t.device} tensor. "
                          "There is no CPU fallback -- move the module and its inputs to cuda.")


def _act(t):
    assert t.dim() == 3 and t.stride(2) == 1 and t.dtype == torch.float32, (t.shape, t.stride(), t.dtype)
    return t


def _avail(t):
    """fp32 elements between a tensor's first element and the end of its storage."""
    return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()


def _fits(t, H, W, Cs, what):
    """The C ABI takes raw pointers: it cannot see how much memory stands behind them, so the one place that can -- this wrapper --
    checks every conv operand against its descriptor BEFORE anything is launched: an [H][W][Cs] NHWC tensor with pixel stride
    stride(1) must lie inside its storage.  (Round 2's memory access fault was exactly this: a descriptor that had become legal
    described a larger layer than the tensors handed in with it)"""
    _act(t)
    if t.shape[0] * t.shape[1] != H * W or t.shape[2] < Cs or (H * W - 1) * t.stride(1) + Cs > _avail(t):
        raise L.SganError(f"{what}: tensor {tuple(t.shape)} (pixel stride {t.stride(1)}, {_avail(t)} elements of storage) does not "
                          f"match the descriptor's {H}x{W}x{Cs}; nothing was launched")
    return t


def _check_fwd_jobs(jobs):
    for job in jobs:
        desc, x, _, w, _, out = job[:6]
        _fits(x, desc.Hin, desc.Win, desc.Cin, "conv_fwd x")
        _fits(out, desc.Hout, desc.Wout, desc.Cout, "conv_fwd out")
        _fits_w(w, desc, "conv_fwd w")


def _check_dgrad_jobs(jobs):
    for job in jobs:
        desc, dout, w, din, x = job[:5]
        _fits(dout, desc.Hout, desc.Wout, desc.Cout, "conv_dgrad dout")
        _fits(din, desc.Hin, desc.Win, desc.Cin, "conv_dgrad din")
        _fits_w(w, desc, "conv_dgrad w")
        if x is not None:
            _fits(x, desc.Hin, desc.Win, desc.Cin, "conv_dgrad x")


def _check_wgrad_jobs(jobs):
    for desc, x, _, dout, dw, _ in jobs:
        _fits(x, desc.Hin, desc.Win, desc.Cin, "conv_wgrad x")
        _fits(dout, desc.Hout, desc.Wout, desc.Cout, "conv_wgrad dout")
        _fits_w(dw, desc, "conv_wgrad dw")


def _fits_w(w, desc, what):
    need = desc.k * desc.k * desc.Cin * desc.Cout
    if w is None or _avail(w) < need:
        raise L.SganError(f"{what}: weight tensor holds {0 if w is None else _avail(w)} elements, the descriptor's k{desc.k} "
                          f"{desc.Cin}->{desc.Cout} layer needs {need}; nothing was launched")
    return w


def conv_desc(kind, k, stride, pad, Hin, Win, Cin_s, Hout, Wout, Cout_s, Cin=0, Cout=0):
    """Cin / Cout: logical channel counts (0 = unknown), a hint that lets kernels skip the zero padding channels."""
    return L.ConvDesc(kind, k, stride, pad, Hin, Win, Cin_s, Hout, Wout, Cout_s, Cin, Cout, _math)


def stat_replicas():
    """SGAN_STAT_REPLICAS of the loaded library."""
    return L.lib().sgan_stat_replicas()



_STAT_REPLICATED = __import__("os").environ.get("SGAN_NO_STAT_REPLICAS", "0") in ("", "0")      # diagnostics switch


class ArenaPool:
    """The statistics arenas of a training step, zeroed by ONE launch at its start (round 2: one aten fill per network call, 6-9 per
    step).  A step asks for the same sequence of arenas every time, so the pool is a list walked by a cursor: begin_step() zeroes
    every slot handed out since the last call (sgan_zero_multi) and rewinds; stat_arena() takes the next slot when it is clean and
    of the right size, anything else (first step, a changed sequence, no begin_step at all) falls back to torch.zeros.  Each slot is
    its own allocation (a pool carved from one buffer measured +35 us per step in round 2: the arenas' atomics then share memory
    channels).  Slots stay alive as long as the pool; an autograd graph must not outlive the step it was built in.  A captured program
    keeps raw pointers into the slots it was handed, and take() replaces a slot in place when a caller asks for another sequence: so
    a captured program owns the pool its arenas came from (arena_scope) and holds it for as long as it can be replayed."""
    MAX_SLOTS = 128

    def __init__(self):
        self.slots, self.clean, self.cur = [], [], 0

    def begin_step(self, also_zero=()):
        dirty = [i for i, c in enumerate(self.clean) if not c]
        extra = []
        for t in also_zero:      # e.g. the discriminators' gradient arena: cleared by the same launch instead of a fill of its own
            if t.is_contiguous() and t.data_ptr() % 16 == 0 and (t.numel() * t.element_size()) % 16 == 0:
                extra.append(t)
            else:
                t.zero_()
        if dirty or extra:
            zero_multi([self.slots[i] for i in dirty] + extra)
            for i in dirty:
                self.clean[i] = True
        self.cur = 0

    def take(self, total, device):
        if _NO_ARENA_POOL:
            return torch.zeros(total, dtype=torch.float64, device=device)
        i = self.cur
        if i < len(self.slots) and self.clean[i] and self.slots[i].numel() == total and self.slots[i].device == torch.device(device):
            self.clean[i] = False
            self.cur += 1
            return self.slots[i]
        t = torch.zeros(total, dtype=torch.float64, device=device)
        if i < self.MAX_SLOTS:
            if i < len(self.slots):
                self.slots[i], self.clean[i] = t, False
            else:
                self.slots.append(t)
                self.clean.append(False)
            self.cur += 1
        return t


_NO_ARENA_POOL = __import__("os").environ.get("SGAN_NO_ARENA_POOL", "0") not in ("", "0")      # diagnostics: one aten fill per arena
_ARENAS = ArenaPool()      # the process-wide pool of the eager training step; arena_scope() puts another in its place


def arenas():
    """The ArenaPool that stat_arena() and begin_step() reach right now."""
    return _ARENAS


@contextlib.contextmanager
def arena_scope(pool, begin=True):
    """Inside the block stat_arena() and begin_step() use `pool` (begin: entered with pool.begin_step(), which zeroes what the
    pool's previous user left dirty); the pool in use before comes back on exit, also when the block raises."""
    global _ARENAS
    saved, _ARENAS = _ARENAS, pool
    try:
        if begin:
            pool.begin_step()
        yield pool
    finally:
        _ARENAS = saved


@contextlib.contextmanager
def graph_capture(graph, **kw):
    """torch.cuda.graph(graph, **kw) with the cycle collector out of the way: dead cycles are collected BEFORE the capture begins and
    the collector stays off until it ends.  torch no longer collects on entry, and a trainer, a GraphedStep or a reconstructor that
    has gone out of use is a reference cycle: it lives until some later allocation happens to start a collection.  If that is an
    allocation made while a stream is capturing, the dead object's graphs and their memory pool are destroyed in the middle of the
    capture, which a capture in the (default) global error mode refuses; the destructor cannot raise, so the process aborts."""
    gc.collect()
    was_on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, **kw):
            yield
    finally:
        if was_on:
            gc.enable()


def begin_step(also_zero=()):
    """Call at the start of a training step (the trainers' optimize_parameters and the captured graph do): one launch zeroes every
    statistics arena the step is going to use -- and the tensors in `also_zero` (FusedAdam.take_zeroing(): the gradient buffers an
    optimizer would otherwise clear with a fill of its own in zero_grad())."""
    _ARENAS.begin_step(also_zero)


def stat_arena(n, device):
    """Zeroed fp64 statistics arena of `n` doubles kept in STAT_REPLICAS copies `n` apart (returns the first copy; pass
    rep_stride = stat_rep(arena) wherever a slice of it is written or read): the conv epilogues spread their same-address atomics
    over the copies."""
    n = max(n, 1)
    return _ARENAS.take((stat_replicas() if _STAT_REPLICATED else 1) * n, device)[:n]


def stat_rep(arena):
    """Replica stride of a stat_arena (0 when replication is switched off: one copy)."""
    return arena.numel() if _STAT_REPLICATED else 0


def norm_desc(stats=None, gamma=None, beta=None, count=1, eps=1e-5, act=ACT_NONE, slope=0.0, sq_stride=0, rep_stride=0, table=None):
    """None when the read is a plain one (no norm, no activation).  `sq_stride`: distance from a channel's sum to its
    sum of squares inside `stats` (0 = the channel count of the tensor being read; wider when `stats` is a slice);
    `rep_stride`: `stats` is a slice of a stat_arena of that length (0: a plain array).  `table`: the finalised (mean, rstd) pairs
    of `stats` (norm_tables_register), for a backward reader."""
    if stats is None and act == ACT_NONE:
        return None
    if stats is None:
        table = None
    d = L.NormDesc(_ptr(stats).value, _ptr(gamma).value, _ptr(beta).value, int(count), float(eps), int(act), float(slope),
                   int(sq_stride), int(rep_stride) if stats is not None else 0, _ptr(table).value)
    d._keep = (stats, gamma, beta, table)
    return d


# ---- finalised normalisation statistics (sgan_norm_desc.mean_rstd) ------------------------------------------------------------
# A forward walk registers the normalised tensors it produced; the next GAN-loss forward launch on the same stream -- which every
# trainer issues between a pass's last forward launch and its first backward launch -- carries them as finalise jobs and hands each
# owner its table.  The backward walk passes the table to its kernels when its forward has one; whoever never meets such a launch
# (inference, the L-BFGS reconstructor, a stand-alone conv call) has none and runs on the fp64 sums as before.
NORM_FIN_MAX = L.DEFINES["SGAN_NORM_FIN_MAX"]
NO_NORM_TABLE = __import__("os").environ.get("SGAN_NO_NORM_TABLE", "0") not in ("", "0")      # switch: no tables anywhere
_fin_pending = []      # weakrefs to owners, oldest first
# tensors finalised; tensors that found no room in a launch (they stay on the fp64 path); the most one launch carried; normalised
# tensors the backward walk handed to its kernels with / without a table
NORM_TABLE_LOG = {"finalised": 0, "dropped": 0, "max_jobs": 0, "with_table": 0, "without_table": 0}


def norm_tables_register(owner, jobs, buf=None):
    """owner: any object (the walk's _BwdArena) that lives as long as the forward's statistics; jobs: [(stats, C, count, eps,
    sq_stride, rep_stride)] of the normalised tensors of that forward, complete in stream order at this point.  After the next loss
    launch on this stream owner.norm_tables maps stats.data_ptr() -> float[2 C] table (until then, and for ever under
    SGAN_NO_NORM_TABLE=1: None).  buf: float storage for the tables (a forward whose buffers are refilled in place brings its own, so
    that the refilled statistics land in the same table); None: allocated when the jobs run."""
    owner.norm_tables = None
    if NO_NORM_TABLE or not jobs:
        return
    owner._fin = (list(jobs), torch.cuda.current_stream().cuda_stream, buf)
    _fin_pending[:] = [r for r in _fin_pending if r() is not None and r() is not owner]
    _fin_pending.append(weakref.ref(owner))


def _take_finalise_jobs(device):
    """The pending finalise jobs of this stream and device for the launch being built: (ctypes array or None, n, commit).  Newest
    owners first, an owner's jobs all or none, at most NORM_FIN_MAX: what does not fit stays without a table.  commit() after the
    launch hands the tables out."""
    here, cur, taken, n = [], torch.cuda.current_stream().cuda_stream, [], 0
    for r in reversed(_fin_pending):
        o = r()
        if o is None or getattr(o, "_fin", None) is None:
            continue
        jobs, stream, buf = o._fin
        if stream != cur or jobs[0][0].device != device:
            here.append(r)      # another stream's: left for a loss launch there
        elif n + len(jobs) <= NORM_FIN_MAX:
            taken.append(o)
            n += len(jobs)
        else:
            o._fin = None       # no room: this forward stays on the fp64 path
            NORM_TABLE_LOG["dropped"] += len(jobs)
    _fin_pending[:] = list(reversed(here))
    if not n:
        return None, 0, lambda: None
    arr, i, tables = (L.NormFinaliseJob * n)(), 0, []
    for o in taken:
        jobs, _, buf = o._fin
        need = sum(2 * j[1] for j in jobs)
        if buf is None or buf.numel() < need:
            buf = torch.empty(need, dtype=torch.float32, device=device)
        tab, off = {}, 0
        for st, Cs, count, eps, sq, rep in jobs:
            t = buf[off: off + 2 * Cs]
            off += 2 * Cs
            arr[i] = L.NormFinaliseJob(_ptr(st).value, int(Cs), int(count), float(eps), int(sq), int(rep), _ptr(t).value)
            tab[st.data_ptr()] = t
            i += 1
        tables.append((o, tab))

    def commit():
        for o, tab in tables:
            o.norm_tables, o._fin = tab, None
        NORM_TABLE_LOG["finalised"] += n
        NORM_TABLE_LOG["max_jobs"] = max(NORM_TABLE_LOG["max_jobs"], n)
    return arr, n, commit


def _nd(d):
    return C.byref(d) if d is not None else None


def _workspace(kib, device):
    """Split-K scratch for one call (torch's caching allocator; static inside a captured graph)."""
    if kib < 0:
        raise L.SganError(f"workspace query failed ({kib}): {L.lib().sgan_last_error().decode()}")
    return torch.empty(kib * 256, dtype=torch.float32, device=device) if kib > 0 else None


def conv_fwd(desc, x, in_norm, w, bias, out, out_act=ACT_NONE, out_stats=None, stats_sq=0, stats_rep=0):
    return conv_fwd_grouped([(desc, x, in_norm, w, bias, out, out_stats, stats_sq, stats_rep)], out_act)


def conv_dgrad(desc, dout, w, din, x=None, x_norm=None, bwd_sums=None, sums_sq=0, accumulate=False, w_transposed=False, sums_rep=0):
    """accumulate: din += result (a tensor with two consumers); sums_sq: see norm_desc; w_transposed: `w` is the
    [tap][Cin][Cout] copy made by pack_weights."""
    return conv_dgrad_grouped([(desc, dout, w, din, x, x_norm, bwd_sums, sums_sq, accumulate, w_transposed, sums_rep)])


def conv_wgrad(desc, x, in_norm, dout, dw, dbias):
    return conv_wgrad_grouped([(desc, x, in_norm, dout, dw, dbias)])


def _pn(d):
    return C.pointer(d) if d is not None else None


def conv_fwd_grouped(jobs, out_act=ACT_NONE):
    """jobs: list of (desc, x, in_norm, w, bias, out, out_stats[, stats_sq, stats_rep]) of the same layer type -> one launch."""
    arr = (L.ConvFwdJob * len(jobs))()
    for i, job in enumerate(jobs):
        desc, x, in_norm, w, bias, out, st = job[:7]
        desc.math = _math
        arr[i] = L.ConvFwdJob(C.pointer(desc), _ptr(_act(x)).value, x.stride(1), _pn(in_norm), _ptr(w).value, _ptr(bias).value,
                              _ptr(_act(out)).value, out.stride(1), _ptr(st).value, int(job[7]) if len(job) > 7 else 0, _pk(w),
                              int(job[8]) if (len(job) > 8 and st is not None) else 0)
    ws = _workspace(L.lib().sgan_conv_fwd_grouped(arr, len(jobs), out_act, None, -1, None), jobs[0][1].device)
    _check_fwd_jobs(jobs)      # after the size query: a descriptor the library rejects is reported in the library's words
    L.check(L.lib().sgan_conv_fwd_grouped(arr, len(jobs), out_act, _ptr(ws), ws.numel() * 4 if ws is not None else 0, _stream()),
            "sgan_conv_fwd_grouped")


def _dgrad_array(jobs):
    arr = (L.ConvDgradJob * len(jobs))()
    for i, job in enumerate(jobs):
        desc, dout, w, din, x, x_norm, sums = job[:7]
        desc.math = _DGRAD_MATH if _DGRAD_MATH is not None else _math
        arr[i] = L.ConvDgradJob(C.pointer(desc), _ptr(_act(dout)).value, dout.stride(1), _ptr(w).value, _ptr(_act(din)).value,
                                din.stride(1), _ptr(x).value, x.stride(1) if x is not None else 0, _pn(x_norm), _ptr(sums).value,
                                int(job[7]) if len(job) > 7 else 0, int(bool(job[8])) if len(job) > 8 else 0,
                                int(bool(job[9])) if len(job) > 9 else 0, _pk(w),
                                int(job[10]) if (len(job) > 10 and sums is not None) else 0, _amax(dout), _pk16(w))
    return arr


def _wgrad_array(jobs):
    arr = (L.ConvWgradJob * len(jobs))()
    for i, (desc, x, in_norm, dout, dw, dbias) in enumerate(jobs):
        desc.math = _math
        arr[i] = L.ConvWgradJob(C.pointer(desc), _ptr(_act(x)).value, x.stride(1), _pn(in_norm), _ptr(_act(dout)).value,
                                dout.stride(1), _ptr(dw).value, _ptr(dbias).value, _amax(dout))
    return arr


def conv_dgrad_grouped(jobs):
    """jobs: list of (desc, dout, w, din, x, x_norm, bwd_sums[, sums_sq, accumulate, w_transposed, sums_rep])."""
    arr = _dgrad_array(jobs)
    ws = _workspace(L.lib().sgan_conv_dgrad_grouped(arr, len(jobs), None, -1, None), jobs[0][1].device)
    _check_dgrad_jobs(jobs)
    L.check(L.lib().sgan_conv_dgrad_grouped(arr, len(jobs), _ptr(ws), ws.numel() * 4 if ws is not None else 0, _stream()),
            "sgan_conv_dgrad_grouped")


def conv_wgrad_grouped(jobs):
    """jobs: list of (desc, x, in_norm, dout, dw, dbias)."""
    arr = _wgrad_array(jobs)
    _check_wgrad_jobs(jobs)
    d0 = jobs[0][0]
    ws = _workspace(L.lib().sgan_conv_wgrad_grouped(arr, len(jobs), None, -1, None), jobs[0][1].device) if min(d0.Cin, d0.Cout) <= 4 else None
    L.check(L.lib().sgan_conv_wgrad_grouped(arr, len(jobs), _ptr(ws), ws.numel() * 4 if ws is not None else 0, _stream()),
            "sgan_conv_wgrad_grouped")


def conv_bwd_grouped(djobs, wjobs, dgrad_math=None):
    """A layer's backward-weight and backward-data (job lists as for the two calls above): one fused launch where
    sgan_conv_bwd_fused covers the layer, the two grouped launches otherwise.  dgrad_math: arithmetic of the backward-data half
    ("f32" / "bf16x3" / "bf16x1"; None = the current mode)."""
    dm = _DGRAD_MATH if _DGRAD_MATH is not None else (_MATH_NAMES[dgrad_math] if dgrad_math else _math)
    d0 = djobs[0][0]
    if d0.Cout == 4 and d0.Cout_logical == 1 and d0.kind == L.CONV and d0.stride == 1 and len(djobs) == len(wjobs) and djobs[0][4] is not None:
        _check_dgrad_jobs(djobs)
        _check_wgrad_jobs(wjobs)
        rc = L.lib().sgan_conv_head_bwd(_dgrad_array(djobs), _wgrad_array(wjobs), len(djobs), _stream())      # the one-channel head: one launch
        if rc == 0:
            return True
        if rc < 0:
            L.check(rc, "sgan_conv_head_bwd")
    if uses_16bit():
        _check_dgrad_jobs(djobs)
        _check_wgrad_jobs(wjobs)
        da, wa = _dgrad_array(djobs), _wgrad_array(wjobs)
        ws = _workspace(L.lib().sgan_conv_bwd_fused_ws(da, len(djobs), wa, len(wjobs), dm, None, -1, None), djobs[0][1].device)
        rc = L.lib().sgan_conv_bwd_fused_ws(da, len(djobs), wa, len(wjobs), dm, _ptr(ws), ws.numel() * 4 if ws is not None else 0, _stream())
        if rc == 0:
            return True
        if rc < 0:
            L.check(rc, "sgan_conv_bwd_fused_ws")
    if min(d0.Cin, d0.Cout) == 4 and len(djobs) == len(wjobs):      # a layer with a 4-channel side: its two launches in one grid
        _check_dgrad_jobs(djobs)
        _check_wgrad_jobs(wjobs)
        with math_scope(dgrad_math):
            rc = L.lib().sgan_conv_bwd_thin_pair(_dgrad_array(djobs), len(djobs), _wgrad_array(wjobs), len(wjobs), _stream())
        if rc == 0:
            return True
        if rc < 0:
            L.check(rc, "sgan_conv_bwd_thin_pair")
    conv_wgrad_grouped(wjobs)
    with math_scope(dgrad_math):
        conv_dgrad_grouped(djobs)
    return False


def transpose_weights(flat, flat_t, segs):
    """segs: list of (off, taps, cout_s, cin_s) conv ranges of the flat parameter buffer."""
    for i0 in range(0, len(segs), 64):
        part = segs[i0:i0 + 64]
        arr = (L.WtSeg * len(part))(*[L.WtSeg(int(o), int(t), int(co), int(ci)) for o, t, co, ci in part])
        L.check(L.lib().sgan_transpose_weights(_ptr(flat), _ptr(flat_t), arr, len(part), _stream()), "sgan_transpose_weights")


def pack_weights(flat, flat_t, pk_fwd, pk_bwd, segs, pk_bwd16=None):
    """Every derived weight copy of the conv ranges `segs` = [(off, taps, cout_s, cin_s)] of a flat parameter buffer in one
    launch per 64 ranges: fp32 transposed copy + the split 16-bit copies (sgan_pack_weights)."""
    for i0 in range(0, len(segs), 64):
        part = segs[i0:i0 + 64]
        arr = (L.WtSeg * len(part))(*[L.WtSeg(int(o), int(t), int(co), int(ci)) for o, t, co, ci in part])
        L.check(L.lib().sgan_pack_weights(_ptr(flat), _ptr(flat_t), _ptr(pk_fwd), _ptr(pk_bwd), _ptr(pk_bwd16), arr, len(part), _stream()),
                "sgan_pack_weights")


def norm_bwd_apply(dy, x, x_norm, bwd_sums, dgamma=None, dbeta=None, sums_sq=0, sums_rep=0, publish_amax=False):
    if sums_rep or publish_amax:
        return norm_bwd_apply_multi([(dy, x, x_norm, bwd_sums, dgamma, dbeta, sums_sq, sums_rep)], publish_amax)
    H, W, Cs = dy.shape
    L.check(L.lib().sgan_norm_bwd_apply(_ptr(_act(dy)), dy.stride(1), _ptr(_act(x)), x.stride(1), H * W, Cs, _nd(x_norm),
                                        _ptr(bwd_sums), int(sums_sq), _ptr(dgamma), _ptr(dbeta), _stream()), "sgan_norm_bwd_apply")


def norm_bwd_apply_multi(jobs, publish_amax=False):
    """jobs: list of (dy, x, x_norm, bwd_sums, dgamma, dbeta[, sums_sq, sums_rep]) -> one launch (<= 8 per launch).
    publish_amax: the kernel also leaves max|dy| of every result in a device scalar and tags the tensor with it (`dy._sgan_amax`): the
    backward-data / backward-weight calls that read THIS tensor object next then run on fp16 planes scaled by it (an fp32-equivalent
    product) instead of bf16 planes.  Only for callers that do not write dy again before it is consumed."""
    for i0 in range(0, len(jobs), 8):
        part = jobs[i0:i0 + 8]
        arr = (L.NormBwdJob * len(part))()
        am = None
        if publish_amax and uses_16bit() and not _NO_F16_BWD:
            am = stat_arena(len(part), part[0][0].device).view(torch.float32)      # one zeroed 8-byte slot per job (low word = the maximum)
        for i, job in enumerate(part):
            dy, x, x_norm, sums, dg, db = job[:6]
            H, W, Cs = dy.shape
            slot = am[2 * i: 2 * i + 1] if am is not None else None
            arr[i] = L.NormBwdJob(_ptr(_act(dy)).value, dy.stride(1), _ptr(_act(x)).value, x.stride(1), H * W, Cs, C.pointer(x_norm),
                                  _ptr(sums).value, int(job[6]) if len(job) > 6 else 0, _ptr(dg).value, _ptr(db).value,
                                  int(job[7]) if len(job) > 7 else 0, _ptr(slot).value)
            dy._sgan_amax = slot
        L.check(L.lib().sgan_norm_bwd_apply_multi(arr, len(part), _stream()), "sgan_norm_bwd_apply_multi")


_NO_F16_BWD = __import__("os").environ.get("SGAN_NO_F16_BWD", "0") not in ("", "0")      # diagnostics: bf16 planes in the backward pass as in round 2


def has_amax(t) -> bool:
    return getattr(t, "_sgan_amax", None) is not None and uses_16bit()


def norm_apply_fwd(u, u_norm, t, mask=None, noise=None, sigma=0.0):
    """t = norm(u) * mask + sigma * noise  (U-Net up path: upnorm -> Dropout -> + Gaussian noise, into a concat slice)."""
    H, W, Cs = u.shape
    L.check(L.lib().sgan_norm_apply_fwd(_ptr(_act(u)), u.stride(1), _nd(u_norm), _ptr(mask), _ptr(noise), float(sigma),
                                        _ptr(_act(t)), t.stride(1), H * W, Cs, _stream()), "sgan_norm_apply_fwd")


def norm_apply_bwd_sums(dt, u, u_norm, bwd_sums, mask=None):
    """dt *= mask (in place), bwd_sums += (sum dt, sum dt * norm(u)) per channel."""
    H, W, Cs = dt.shape
    L.check(L.lib().sgan_norm_apply_bwd_sums(_ptr(_act(dt)), dt.stride(1), _ptr(mask), _ptr(_act(u)), u.stride(1), _nd(u_norm),
                                             _ptr(bwd_sums), H * W, Cs, _stream()), "sgan_norm_apply_bwd_sums")


def pad_reflect_fwd(x, x_norm, pad, out, mask=None):
    """out [H + 2 pad, W + 2 pad, C] = mask * act(norm(x)) at the reflected positions (nn.ReflectionPad2d after norm / act / dropout)."""
    H, W, Cs = x.shape
    assert out.shape == (H + 2 * pad, W + 2 * pad, Cs)
    L.check(L.lib().sgan_pad_reflect_fwd(_ptr(_act(x)), x.stride(1), H, W, Cs, _nd(x_norm), _ptr(mask), int(pad), _ptr(_act(out)),
                                         out.stride(1), _stream()), "sgan_pad_reflect_fwd")


def pad_reflect_bwd(dout, pad, din, x=None, x_norm=None, mask=None, bwd_sums=None, sums_sq=0):
    """din = act'(norm(x)) * mask * fold(dout); bwd_sums += (sum din, sum din * xhat)."""
    H, W, Cs = din.shape
    assert dout.shape == (H + 2 * pad, W + 2 * pad, Cs)
    L.check(L.lib().sgan_pad_reflect_bwd(_ptr(_act(dout)), dout.stride(1), H, W, Cs, int(pad), _ptr(x), x.stride(1) if x is not None else 0,
                                         _nd(x_norm), _ptr(mask), _ptr(_act(din)), din.stride(1), _ptr(bwd_sums), int(sums_sq), _stream()),
            "sgan_pad_reflect_bwd")


def _fits_exact(t, H, W, Cs, what):
    """_fits, and the two sides on their own: an [H][W][>= Cs] view (H * W alone would let a transposed map through)."""
    _act(t)
    if tuple(t.shape[:2]) != (H, W):
        raise L.SganError(f"{what}: tensor {tuple(t.shape)} is not the {H}x{W}x(>= {Cs}) map this call addresses; nothing was launched")
    return _fits(t, H, W, Cs, what)


def bilinear_up2_fwd(x, out, out_stats=None, stats_sq=0):
    """out [2H, 2W, >= Cs] = x2 bilinear interpolation (align_corners=False) of x [H, W, Cs]; out_stats += its (sum, sum of squares)."""
    H, W, Cs = x.shape
    _fits_exact(x, H, W, Cs, "bilinear_up2_fwd x")
    _fits_exact(out, 2 * H, 2 * W, Cs, "bilinear_up2_fwd out")
    L.check(L.lib().sgan_bilinear_up2_fwd(_ptr(x), x.stride(1), H, W, Cs, _ptr(out), out.stride(1), _ptr(out_stats),
                                          int(stats_sq), _stream()), "sgan_bilinear_up2_fwd")


def bilinear_up2_bwd(dout, din):
    """din [H, W, Cs] = the transpose of bilinear_up2_fwd applied to dout [2H, 2W, >= Cs]."""
    H, W, Cs = din.shape
    _fits_exact(din, H, W, Cs, "bilinear_up2_bwd din")
    _fits_exact(dout, 2 * H, 2 * W, Cs, "bilinear_up2_bwd dout")
    L.check(L.lib().sgan_bilinear_up2_bwd(_ptr(dout), dout.stride(1), H, W, Cs, _ptr(din), din.stride(1), _stream()),
            "sgan_bilinear_up2_bwd")


def _level_table(levels, H, W, what):
    """Pointers and pixel strides of the six levels; every level present is checked as [H >> (s+1), W >> (s+1), >= 4] inside its storage."""
    if len(levels) != 6:
        raise L.SganError(f"{what}: six levels expected, got {len(levels)}; nothing was launched")
    for s, t in enumerate(levels):
        if t is not None:
            if t.dim() != 3 or t.dtype != torch.float32 or t.stride(2) != 1:
                raise L.SganError(f"{what}: level {s} {tuple(t.shape)} ({t.dtype}, strides {t.stride()}) is not a float32 NHWC map with "
                                  "unit channel stride; nothing was launched")
            _fits_exact(t, H >> (s + 1), W >> (s + 1), 4, f"{what} level {s}")
    ptrs = (C.c_void_p * 6)(*[t.data_ptr() if t is not None else None for t in levels])
    lds = (C.c_int32 * 6)(*[t.stride(1) if t is not None else 4 for t in levels])
    return ptrs, lds


def avgpool_pyramid_fwd(label, levels):
    """levels[s]: [H >> (s+1), W >> (s+1), 4] buffers (or channel slices), s = 0..5."""
    H, W, _ = label.shape
    _fits_exact(label, H, W, 4, "avgpool_pyramid_fwd label")
    if any(t is None for t in levels):
        raise L.SganError("avgpool_pyramid_fwd: the forward writes all six levels; nothing was launched")
    ptrs, lds = _level_table(levels, H, W, "avgpool_pyramid_fwd")
    L.check(L.lib().sgan_avgpool_pyramid_fwd(_ptr(label), label.stride(1), H, W, ptrs, lds, _stream()), "sgan_avgpool_pyramid_fwd")


def avgpool_pyramid_bwd(dlevels, dlabel, accumulate=False):
    """dlabel [H, W, 4] (+)= sum over the levels present (None: absent) of dlevels[s][y >> (s+1), x >> (s+1)] / 4^(s+1)."""
    H, W, _ = dlabel.shape
    _fits_exact(dlabel, H, W, 4, "avgpool_pyramid_bwd dlabel")
    ptrs, lds = _level_table(dlevels, H, W, "avgpool_pyramid_bwd")
    L.check(L.lib().sgan_avgpool_pyramid_bwd(ptrs, lds, H, W, _ptr(dlabel), dlabel.stride(1), int(accumulate), _stream()),
            "sgan_avgpool_pyramid_bwd")


def dropout_mask(mask, p, seed, offset_dev=None, advance=True):
    L.check(L.lib().sgan_dropout_mask(_ptr(mask), mask.numel(), float(p), C.c_uint64(seed & (2 ** 64 - 1)), _ptr(offset_dev),
                                      int(bool(advance)), _stream()), "sgan_dropout_mask")


def net_stream_seed(seed, index):
    """Philox key of the index-th network of a trainer seeded `seed`: the index goes into the high key word (k1), which the
    `seed + small integer` keys of the trainer itself and of the tensors inside one network never reach."""
    return (int(seed) + (int(index) << 32)) & (2 ** 64 - 1)


def rng_advance(offset_dev, by):
    L.check(L.lib().sgan_rng_advance(_ptr(offset_dev), C.c_uint64(int(by)), _stream()), "sgan_rng_advance")


IMAGE_LOSS_WS_BYTES = L.DEFINES["SGAN_IMAGE_LOSS_WS_BYTES"]


def l1w_fwd(x, y, Creal, a, weights_dev, nweights, lam, loss_out, g):
    H, W, _ = x.shape
    ws = torch.empty(IMAGE_LOSS_WS_BYTES // 8, dtype=torch.float64, device=x.device)
    L.check(L.lib().sgan_l1w_fwd(_ptr(_act(x)), x.stride(1), _ptr(_act(y)), y.stride(1), H * W, Creal,
                                 _ptr(a), a.stride(1) if a is not None else 0, _ptr(weights_dev), nweights, float(lam),
                                 _ptr(loss_out), _ptr(_act(g)), g.stride(1), _ptr(ws), IMAGE_LOSS_WS_BYTES, _stream()), "sgan_l1w_fwd")


def ce_fwd(logits, Creal, label, const_label, class_w, acc, loss_out):
    """Class-weighted cross-entropy of an [H, W, Cs] logits buffer (sgan_ce_fwd).  acc: zeroed float64[2 + 1] scratch (sums | ticket)."""
    H, W, _ = logits.shape
    L.check(L.lib().sgan_ce_fwd(_ptr(_act(logits)), logits.stride(1), H * W, Creal, _ptr(label), int(const_label), _ptr(class_w),
                                _ptr(acc), C.c_void_p(acc.data_ptr() + 16), _ptr(loss_out), _stream()), "sgan_ce_fwd")


def ce_bwd(logits, Creal, label, const_label, class_w, acc, gout, dlogits):
    H, W, _ = logits.shape
    L.check(L.lib().sgan_ce_bwd(_ptr(_act(logits)), logits.stride(1), H * W, Creal, _ptr(label), int(const_label), _ptr(class_w),
                                _ptr(acc), _ptr(gout), _ptr(_act(dlogits)), dlogits.stride(1), _stream()), "sgan_ce_bwd")


def softmax_fwd(z, Creal, p):
    H, W, _ = z.shape
    L.check(L.lib().sgan_softmax_fwd(_ptr(_act(z)), z.stride(1), H * W, Creal, _ptr(_act(p)), p.stride(1), _stream()), "sgan_softmax_fwd")


def softmax_bwd(dp, p, Creal, dz):
    H, W, _ = p.shape
    L.check(L.lib().sgan_softmax_bwd(_ptr(_act(dp)), dp.stride(1), _ptr(_act(p)), p.stride(1), H * W, Creal, _ptr(_act(dz)), dz.stride(1),
                                     _stream()), "sgan_softmax_bwd")


def bce01_fwd(x, t, Creal, loss_out, g):
    H, W, _ = x.shape
    ws = torch.empty(IMAGE_LOSS_WS_BYTES // 8, dtype=torch.float64, device=x.device)
    L.check(L.lib().sgan_bce01_fwd(_ptr(_act(x)), x.stride(1), _ptr(_act(t)), t.stride(1), H * W, Creal, _ptr(loss_out),
                                   _ptr(_act(g)), g.stride(1), _ptr(ws), IMAGE_LOSS_WS_BYTES, _stream()), "sgan_bce01_fwd")


def scale(gout, g, dx):
    assert g.is_contiguous() and dx.is_contiguous()
    L.check(L.lib().sgan_scale(_ptr(gout), _ptr(g), _ptr(dx), g.numel(), _stream()), "sgan_scale")


def bn_running_update(layers, momentum=0.1):
    """layers: list of (stats, running_mean, running_var, num_batches_tracked, C, count[, sq_stride, rep_stride])."""
    arr = (L.BnRunningDesc * len(layers))()
    for i, job in enumerate(layers):
        st, rm, rv, nbt, c, cnt = job[:6]
        arr[i] = L.BnRunningDesc(st.data_ptr(), rm.data_ptr(), rv.data_ptr(), nbt.data_ptr() if nbt is not None else 0, c, cnt,
                                 int(job[6]) if len(job) > 6 else 0, int(job[7]) if len(job) > 7 else 0)
    L.check(L.lib().sgan_bn_running_update(arr, len(layers), momentum, _stream()), "sgan_bn_running_update")


def image_prep(img_u8, x0, y0, n, flip, rot, out=None):
    """img_u8: [H0, W0, 3] uint8 device tensor -> [n, n, 4] fp32 NHWC buffer in [-1, 1] (crop, flip, rot90, ToTensor, Normalize)."""
    require_gpu(img_u8, "image_prep")
    assert img_u8.dtype == torch.uint8 and img_u8.dim() == 3 and img_u8.shape[2] == 3 and img_u8.is_contiguous(), (img_u8.shape, img_u8.dtype)
    if out is None:
        out = torch.empty((n, n, 4), dtype=torch.float32, device=img_u8.device)
    L.check(L.lib().sgan_image_prep(_ptr(img_u8), img_u8.shape[0], img_u8.shape[1], int(x0), int(y0), int(n), int(bool(flip)), int(rot),
                                    _ptr(_act(out)), out.stride(1), out.shape[2], _stream()), "sgan_image_prep")
    return out


def image_prep_elastic(img_u8, x0, y0, n, flip, rot, ctrl, nearest_mask, out=None, field_out=None):
    """image_prep through an elastic deformation (sgan_image_prep_elastic; util.elastic_prep is the host yardstick).  ctrl: [G + 3,
    G + 3, 2] fp32 device tensor of control displacements (dx, dy) in source pixels, G in 1..13; nearest_mask: bit c set = channel c
    of RGB is sampled at the nearest pixel (labels), clear = bilinearly (image).  field_out: optional [n, n, 2] fp32 device tensor
    that receives the clamped per-pixel field, indexed (v, u) in crop coordinates before flip and rotation."""
    require_gpu(img_u8, "image_prep_elastic")
    require_gpu(ctrl, "image_prep_elastic")
    assert img_u8.dtype == torch.uint8 and img_u8.dim() == 3 and img_u8.shape[2] == 3 and img_u8.is_contiguous(), (img_u8.shape, img_u8.dtype)
    assert ctrl.dtype == torch.float32 and ctrl.dim() == 3 and ctrl.shape[0] == ctrl.shape[1] and ctrl.shape[2] == 2 and ctrl.is_contiguous(), \
        (ctrl.shape, ctrl.dtype)
    n = int(n)
    if out is None:
        out = torch.empty((n, n, 4), dtype=torch.float32, device=img_u8.device)
    assert out.shape[0] == n and out.shape[1] == n and out.stride(0) == n * out.stride(1), (out.shape, out.stride())
    if field_out is not None:
        require_gpu(field_out, "image_prep_elastic")
        assert field_out.dtype == torch.float32 and tuple(field_out.shape) == (n, n, 2) and field_out.is_contiguous(), (field_out.shape, field_out.dtype)
    L.check(L.lib().sgan_image_prep_elastic(_ptr(img_u8), img_u8.shape[0], img_u8.shape[1], int(x0), int(y0), n, int(bool(flip)), int(rot),
                                            _ptr(ctrl), ctrl.shape[0] - 3, int(nearest_mask), _ptr(_act(out)), out.stride(1), out.shape[2],
                                            _ptr(field_out), _stream()), "sgan_image_prep_elastic")
    return out


def photo_record(rec):
    """util.PhotoRec -> the sgan_photo_rec the C entry reads (the seed stays with the caller: the kernel draws nothing)."""
    r = L.STRUCTS["sgan_photo_rec"]()
    r.R = rec.R
    for k, v in enumerate(rec.w):
        r.w[k] = float(v)
    r.gamma, r.contrast, r.brightness, r.sigma_n, r.nbox = rec.gamma, rec.contrast, rec.brightness, rec.sigma_n, len(rec.boxes)
    if len(rec.boxes) > len(r.box_value):
        raise L.SganError("image_photo: %d boxes (0 .. %d)" % (len(rec.boxes), len(r.box_value)))
    for b, (y0, y1, x0, x1, value) in enumerate(rec.boxes):
        r.box_y0[b], r.box_y1[b], r.box_x0[b], r.box_x1[b], r.box_value[b] = y0, y1, x0, x1, value
    return r


def image_photo(src, rec, mask, noise=None, out=None):
    """Photometric augmentation of a prepared crop (sgan_image_photo; util.photo_ref / util.photo_bounds are the host yardsticks):
    src [H, W, Cs] fp32 NHWC in [-1, 1], as image_prep* leaves it -> out (a new [H, W, Cs] buffer unless given; never src).  rec: a
    util.PhotoRec; mask: bit c set = channel c is an image channel, every other channel is copied bit for bit; noise: a contiguous
    [popcount(mask), H, W] fp32 device tensor of N(0, 1) values (ops.normal_fill) for the noise stage, or None."""
    require_gpu(src, "image_photo")
    H, W, Cs = src.shape
    assert src.stride(0) == W * src.stride(1), (src.shape, src.stride())
    if out is None:
        out = torch.empty((H, W, Cs), dtype=torch.float32, device=src.device)
    require_gpu(out, "image_photo")
    assert tuple(out.shape) == (H, W, Cs) and out.stride(0) == W * out.stride(1), (out.shape, out.stride())
    if noise is not None:
        require_gpu(noise, "image_photo")
        assert noise.dtype == torch.float32 and noise.is_contiguous() and tuple(noise.shape) == (bin(int(mask)).count("1"), H, W), \
            (noise.shape, noise.dtype, mask)
    L.check(L.lib().sgan_image_photo(_ptr(_act(src)), src.stride(1), _ptr(_act(out)), out.stride(1), H, W, Cs, int(mask),
                                     C.byref(photo_record(rec)), _ptr(noise), _stream()), "sgan_image_photo")
    return out


def image_prep_tile(img_u8, x0, y0, h, w, flip, rot, out=None):
    """image_prep whose h x w window at (x0, y0) may reach outside the image (indices reflected without repeating the edge, like
    F.pad(mode='reflect')) and may be rectangular (rot 0 only): [H0, W0, 3] uint8 device tensor -> [h, w, 4] fp32 NHWC buffer
    (sgan_image_prep_tile; util.prep_tile_ref is the host yardstick).  The tiles of whole-image inference, and with the full window
    the whole image itself."""
    require_gpu(img_u8, "image_prep_tile")
    assert img_u8.dtype == torch.uint8 and img_u8.dim() == 3 and img_u8.shape[2] == 3 and img_u8.is_contiguous(), (img_u8.shape, img_u8.dtype)
    h, w = int(h), int(w)
    if out is None:
        out = torch.empty((h, w, 4), dtype=torch.float32, device=img_u8.device)
    assert out.shape[0] == h and out.shape[1] == w and out.stride(0) == w * out.stride(1), (out.shape, out.stride())
    L.check(L.lib().sgan_image_prep_tile(_ptr(img_u8), img_u8.shape[0], img_u8.shape[1], int(x0), int(y0), h, w, int(bool(flip)), int(rot),
                                         _ptr(_act(out)), out.stride(1), out.shape[2], _stream()), "sgan_image_prep_tile")
    return out


def tile_blend(logits, Creal, mode, x0, y0, M, R, flip, rot, canvas):
    """One pass of whole-image inference: canvas[Y, X, c] += w(Y - y0) w(X - x0) p_c, p the softmax (mode SEGHEAD_SOFTMAX) or sigmoid
    (SEGHEAD_SIGMOID) of the [T, T, Cs] NHWC `logits` the generator left for the tile at (x0, y0) under the D4 element (flip, rot),
    gathered through the element's inverse (sgan_tile_blend; util.blend_tiles_ref is the host yardstick).  canvas: [H, W, 4] fp32,
    zeroed by the caller before the first pass of an image."""
    require_gpu(logits, "tile_blend")
    require_gpu(canvas, "tile_blend")
    T = logits.shape[0]
    assert logits.shape[1] == T and logits.stride(0) == T * logits.stride(1), (logits.shape, logits.stride())
    H, W, _ = canvas.shape
    assert canvas.stride(0) == W * canvas.stride(1), (canvas.shape, canvas.stride())
    L.check(L.lib().sgan_tile_blend(_ptr(_act(logits)), logits.stride(1), int(Creal), int(mode), int(x0), int(y0), T, int(M), int(R),
                                    int(bool(flip)), int(rot), _ptr(_act(canvas)), canvas.stride(1), H, W, _stream()), "sgan_tile_blend")


def tile_finish(canvas, Creal, Wy, Wx, n_tta, prob, logp):
    """prob = canvas / (n_tta Wy[Y] Wx[X]), logp = log max(prob, FLT_MIN) (sgan_tile_finish); Wy [H], Wx [W]: device int32 vectors of
    util.tile_plan; prob, logp: [H, W, 4] fp32 buffers (ops.logical_view hands them out as [1, C, H, W])."""
    H, W, _ = canvas.shape
    for t in (prob, logp):
        require_gpu(t, "tile_finish")
        assert t.shape[:2] == (H, W) and t.stride(0) == W * t.stride(1), (t.shape, t.stride())
    assert canvas.stride(0) == W * canvas.stride(1), (canvas.shape, canvas.stride())
    assert Wy.dtype == Wx.dtype == torch.int32 and Wy.is_cuda and Wx.is_cuda and Wy.is_contiguous() and Wx.is_contiguous()
    assert Wy.numel() == H and Wx.numel() == W, (Wy.shape, Wx.shape, H, W)
    L.check(L.lib().sgan_tile_finish(_ptr(_act(canvas)), canvas.stride(1), H, W, int(Creal), _ptr(Wy), _ptr(Wx), int(n_tta), _ptr(_act(prob)),
                                     prob.stride(1), _ptr(_act(logp)), logp.stride(1), _stream()), "sgan_tile_finish")


RESAMPLE = {n: L.DEFINES["SGAN_RESAMPLE_" + n.upper()] for n in ("bilinear", "bicubic")}      # Pillow's Image.BILINEAR / Image.BICUBIC


def image_resize(img_u8, wo, ho, resample):
    """img_u8 [H, W, C] uint8 device tensor -> [ho, wo, C] uint8: Image.resize((wo, ho), resample) bit for bit, on the device."""
    require_gpu(img_u8, "image_resize")
    assert img_u8.dtype == torch.uint8 and img_u8.dim() == 3 and img_u8.is_contiguous(), (img_u8.shape, img_u8.dtype)
    H, W, Cc = img_u8.shape
    f = RESAMPLE[resample] if isinstance(resample, str) else int(resample)
    lib = L.lib()
    need = int(lib.sgan_image_resize_workspace(H, W, Cc, int(ho), int(wo), f))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=img_u8.device)
    out = torch.empty((int(ho), int(wo), Cc), dtype=torch.uint8, device=img_u8.device)
    L.check(lib.sgan_image_resize(_ptr(img_u8), H, W, Cc, _ptr(out), int(ho), int(wo), f, _ptr(ws), need, _stream()), "sgan_image_resize")
    return out


def gauss_down_fwd(x, Creal, g, g_chan_stride, k, pad, s, out):
    H, W, Cs = x.shape
    Ho, Wo, _ = out.shape
    L.check(L.lib().sgan_gauss_down_fwd(_ptr(_act(x)), x.stride(1), H, W, Cs, Creal, _ptr(g), g_chan_stride, k, pad, s,
                                        _ptr(_act(out)), out.stride(1), Ho, Wo, _stream()), "sgan_gauss_down_fwd")


def gauss_down_bwd(dout, Creal, g, g_chan_stride, k, pad, s, din, accumulate=False):
    Ho, Wo, Cs = dout.shape
    H, W, _ = din.shape
    L.check(L.lib().sgan_gauss_down_bwd(_ptr(_act(dout)), dout.stride(1), Ho, Wo, Cs, Creal, _ptr(g), g_chan_stride, k, pad, s,
                                        _ptr(_act(din)), din.stride(1), H, W, int(bool(accumulate)), _stream()), "sgan_gauss_down_bwd")


def _gauss_jobs(jobs):
    """jobs: [(image, down, g, g_chan_stride, k, pad, s)] NHWC buffers of one channel count."""
    arr = (L.GaussJob * len(jobs))()
    for i, (img, down, g, gcs, k, pad, s) in enumerate(jobs):
        H, W, _ = img.shape
        Ho, Wo, _ = down.shape
        arr[i] = L.GaussJob(_ptr(_act(img)).value, img.stride(1), H, W, _ptr(_act(down)).value, down.stride(1), Ho, Wo,
                            _ptr(g).value, int(gcs), int(k), int(pad), int(s))
    return arr


def gauss_down_multi_fwd(jobs, Creal):
    for i0 in range(0, len(jobs), 4):
        part = jobs[i0: i0 + 4]
        L.check(L.lib().sgan_gauss_down_multi_fwd(_gauss_jobs(part), len(part), part[0][0].shape[2], Creal, _stream()),
                "sgan_gauss_down_multi_fwd")


def gauss_down_multi_bwd(jobs, Creal, accumulate=False):
    """All jobs share jobs[i][0], the image gradient, which receives the sum of their contributions."""
    for i0 in range(0, len(jobs), 4):
        part = jobs[i0: i0 + 4]
        L.check(L.lib().sgan_gauss_down_multi_bwd(_gauss_jobs(part), len(part), part[0][0].shape[2], Creal,
                                                  int(bool(accumulate or i0 > 0)), _stream()), "sgan_gauss_down_multi_bwd")


def gan_loss_fwd(logits, target, mode, loss_out, p_out=None):
    """p_out (optional, mode 0): sigmoid(logits) in channel 0 of a map that shares the logits' shape and pixel stride -- the kernel
    addresses it with the logits' leading dimension."""
    H, W, _ = logits.shape
    assert p_out is None or (p_out.dtype == torch.float32 and p_out.shape == logits.shape and p_out.stride(1) == logits.stride(1)), \
        (None if p_out is None else (p_out.dtype, tuple(p_out.shape), p_out.stride()), tuple(logits.shape), logits.stride())
    L.check(L.lib().sgan_gan_loss_fwd(_ptr(_act(logits)), logits.stride(1), H * W, float(target), mode, _ptr(loss_out),
                                      _ptr(p_out), _stream()), "sgan_gan_loss_fwd")


def gan_loss_bwd(logits, target, mode, gout, dlogits):
    H, W, _ = logits.shape
    L.check(L.lib().sgan_gan_loss_bwd(_ptr(_act(logits)), logits.stride(1), H * W, float(target), mode, _ptr(gout),
                                      _ptr(_act(dlogits)), dlogits.stride(1), _stream()), "sgan_gan_loss_bwd")


GAN_LOSS_WS_BYTES = L.DEFINES["SGAN_GAN_LOSS_WS_BYTES"]
_zeroed_ws = {}
_unit_grads = []           # weak references to gradient tensors known to hold 1.0 (BaseModel._backward's cached root gradient)


def register_unit_grad(t):
    """`t` holds 1.0 and is never written: a fused loss node that receives this very tensor object as its upstream gradient hands
    out its precomputed unit-gradient result without a rescaling kernel."""
    _unit_grads[:] = [r for r in _unit_grads if r() is not None]
    _unit_grads.append(weakref.ref(t))


def is_unit_grad(t) -> bool:
    return any(r() is t for r in _unit_grads)


def _zeroed_workspace(key, device, nbytes):
    """The float64 scratch of the loss entry point `key` on `device`: zeroed once, and every kernel that uses it leaves its ticket
    counter (the seg-head kernels: their slots too) at zero for the next call.  One buffer per entry point and device, so these
    losses run on the trainer's main stream only (side-stream chains use the per-term loss)."""
    ws = _zeroed_ws.get((key, device.index))
    if ws is None:
        ws = _zeroed_ws[(key, device.index)] = torch.zeros(nbytes // 8, dtype=torch.float64, device=device)
    return ws


def _gan_loss_workspace(device):
    return _zeroed_workspace("gan_loss", device, GAN_LOSS_WS_BYTES)


def gan_loss_multi_fwd(logits, targets, weights, mode, each_out, total_out, dlogits=None):
    """dlogits (optional list of NHWC buffers): also receives d total / d logits_i for an upstream gradient of 1."""
    arr = (L.GanLossJob * len(logits))()
    for i, (lb, t, w) in enumerate(zip(logits, targets, weights)):
        d = dlogits[i] if dlogits is not None else None
        arr[i] = L.GanLossJob(_ptr(_act(lb)).value, lb.stride(1), lb.shape[0] * lb.shape[1], float(t), float(w),
                              _ptr(_act(d)).value if d is not None else None, d.stride(1) if d is not None else 0)
    ws = _gan_loss_workspace(each_out.device)
    fin, nfin, commit = _take_finalise_jobs(each_out.device)      # the normalised tensors of the forwards this loss closes
    L.check(L.lib().sgan_gan_loss_multi_fwd_fin(arr, len(logits), mode, _ptr(each_out), _ptr(total_out), _ptr(ws), GAN_LOSS_WS_BYTES,
                                                fin, nfin, _stream()), "sgan_gan_loss_multi_fwd_fin")
    commit()


def gan_loss_multi_bwd(logits, targets, weights, mode, gout, dlogits):
    arr = (L.GanLossJob * len(logits))()
    for i, (lb, t, w, d) in enumerate(zip(logits, targets, weights, dlogits)):
        arr[i] = L.GanLossJob(_ptr(_act(lb)).value, lb.stride(1), lb.shape[0] * lb.shape[1], float(t), float(w),
                              _ptr(_act(d)).value, d.stride(1))
    L.check(L.lib().sgan_gan_loss_multi_bwd(arr, len(logits), mode, _ptr(gout), _stream()), "sgan_gan_loss_multi_bwd")


FACTD_LOSS_WS_BYTES = L.DEFINES["SGAN_FACTD_LOSS_WS_BYTES"]


def _factd_loss_workspace(device):
    return _zeroed_workspace("factd_loss", device, FACTD_LOSS_WS_BYTES)


def factd_mode(sig1, sig2, mse):
    return (L.FACTD_SIG1 if sig1 else 0) | (L.FACTD_SIG2 if sig2 else 0) | (L.FACTD_MSE if mse else 0)


def _factd_jobs(l1s, l2s, ups, targets, weights, dl1s, dl2s):
    """The C ABI sees raw pointers: every map is checked against its storage here, before anything is launched."""
    n = len(l1s)
    arr = (L.FactdLossJob * n)()
    for i in range(n):
        a, b = l1s[i], l2s[i]
        d1 = dl1s[i] if dl1s is not None else None
        d2 = dl2s[i] if dl2s is not None else None
        _fits(a, a.shape[0], a.shape[1], 1, "factd_loss l1")
        _fits(b, b.shape[0], b.shape[1], 1, "factd_loss l2")
        if d1 is not None:
            _fits(d1, a.shape[0], a.shape[1], d1.shape[2], "factd_loss dl1")
            assert d1.shape[:2] == a.shape[:2] and d1.is_contiguous()
        if d2 is not None:
            _fits(d2, b.shape[0], b.shape[1], d2.shape[2], "factd_loss dl2")
            assert d2.shape[:2] == b.shape[:2] and d2.is_contiguous()
        arr[i] = L.FactdLossJob(_ptr(a).value, a.stride(1), a.shape[0], a.shape[1], _ptr(b).value, b.stride(1), b.shape[0], b.shape[1],
                                int(ups[i]), float(targets[i]), float(weights[i]),
                                _ptr(d1).value if d1 is not None else None, d1.stride(1) if d1 is not None else 0,
                                _ptr(d2).value if d2 is not None else None, d2.stride(1) if d2 is not None else 0)
    return arr


def factd_loss_multi_fwd(l1s, l2s, ups, targets, weights, mode, each_out, total_out, dl1s=None, dl2s=None):
    """sgan_factd_loss_multi_fwd on lists of NHWC logits buffers [h, w, Cs] (channel 0 is read).  dl1s / dl2s: optional lists whose
    entries (buffers or None) receive d total / d l for an upstream gradient of 1.  Returns False, having launched nothing, when
    the library reports the call as not covered."""
    arr = _factd_jobs(l1s, l2s, ups, targets, weights, dl1s, dl2s)
    ws = _factd_loss_workspace(each_out.device)
    rc = L.lib().sgan_factd_loss_multi_fwd(arr, len(l1s), int(mode), _ptr(each_out), _ptr(total_out), _ptr(ws), FACTD_LOSS_WS_BYTES, _stream())
    if rc == 1:
        return False
    L.check(rc, "sgan_factd_loss_multi_fwd")
    return True


def factd_loss_multi_bwd(l1s, l2s, ups, targets, weights, mode, gout, dl1s, dl2s):
    arr = _factd_jobs(l1s, l2s, ups, targets, weights, dl1s, dl2s)
    L.check(L.lib().sgan_factd_loss_multi_bwd(arr, len(l1s), int(mode), _ptr(gout), _stream()), "sgan_factd_loss_multi_bwd")


def _rows_fit(name, npix, Creal, t, what, written):
    """The check of seg_head's rows_fit for the `--use_sigmoid_ss` kernels, which move scalars: an operand holds `npix` pixels of at
    least Creal channels, and its last row -- the Creal channels a kernel reads, the whole stored row (pixel stride) where it
    writes, padding channels included -- ends inside the storage.  Raised before anything is launched."""
    _act(t)
    require_gpu(t, name)
    row = t.stride(1) if written else Creal
    if t.shape[0] * t.shape[1] != npix or t.shape[2] < Creal or t.stride(1) < Creal or (npix - 1) * t.stride(1) + row > _avail(t):
        raise L.SganError(f"{name} {what}: tensor {tuple(t.shape)} (pixel stride {t.stride(1)}, {_avail(t)} elements of storage) does "
                          f"not hold {npix} rows of {row}; nothing was launched")


def _class_w_fits(name, class_w, nw, device):
    """0 <= nw <= 16 weights are read from a contiguous fp32 vector on the operands' device."""
    if not 0 <= int(nw) <= 16 or (nw and (class_w is None or class_w.dtype != torch.float32 or not class_w.is_contiguous()
                                         or class_w.device != device or class_w.numel() < nw)):
        raise L.SganError(f"{name} class_w: {nw} weights need a contiguous float32 vector of at least as many entries on {device}; got "
                          f"{None if class_w is None else (class_w.dtype, tuple(class_w.shape), class_w.stride(), class_w.device)}; "
                          "nothing was launched")


def sigmoid_nhwc_fwd(z, Creal, p):
    H, W, _ = z.shape
    _rows_fit("sigmoid_nhwc_fwd", H * W, Creal, z, "logits", False)
    _rows_fit("sigmoid_nhwc_fwd", H * W, Creal, p, "p", True)
    L.check(L.lib().sgan_sigmoid_nhwc_fwd(_ptr(_act(z)), z.stride(1), H * W, Creal, _ptr(_act(p)), p.stride(1), _stream()), "sgan_sigmoid_nhwc_fwd")


def sigmoid_nhwc_bwd(dp, p, Creal, dz):
    H, W, _ = p.shape
    _rows_fit("sigmoid_nhwc_bwd", H * W, Creal, p, "p", False)
    _rows_fit("sigmoid_nhwc_bwd", H * W, Creal, dp, "dp", False)
    _rows_fit("sigmoid_nhwc_bwd", H * W, Creal, dz, "dz", True)
    L.check(L.lib().sgan_sigmoid_nhwc_bwd(_ptr(_act(dp)), dp.stride(1), _ptr(_act(p)), p.stride(1), H * W, Creal, _ptr(_act(dz)),
                                          dz.stride(1), _stream()), "sgan_sigmoid_nhwc_bwd")


BCE_WEIGHTED_WS_BYTES = L.DEFINES["SGAN_BCE_WEIGHTED_WS_BYTES"]


def bce_weighted_fwd(p, t, Creal, class_w, nw, loss_out):
    """Weighted BCE of two [H, W, Cs] buffers (sgan_bce_weighted_fwd); class_w: contiguous float32 vector of >= nw entries on p's
    device, or None.  Every operand is checked against its storage here, before anything is launched."""
    H, W, _ = p.shape
    _rows_fit("bce_weighted_fwd", H * W, Creal, p, "p", False)
    _rows_fit("bce_weighted_fwd", H * W, max(Creal, nw), t, "t", False)
    _class_w_fits("bce_weighted_fwd", class_w, nw, p.device)
    assert loss_out.dtype == torch.float32 and loss_out.numel() == 1 and loss_out.device == p.device
    ws = _zeroed_workspace("bce_weighted", p.device, BCE_WEIGHTED_WS_BYTES)
    L.check(L.lib().sgan_bce_weighted_fwd(_ptr(_act(p)), p.stride(1), _ptr(_act(t)), t.stride(1), H * W, Creal, _ptr(class_w), int(nw),
                                          _ptr(loss_out), _ptr(ws), BCE_WEIGHTED_WS_BYTES, _stream()), "sgan_bce_weighted_fwd")


def bce_weighted_bwd(p, t, Creal, class_w, nw, gout, dp):
    H, W, _ = p.shape
    _rows_fit("bce_weighted_bwd", H * W, Creal, p, "p", False)
    _rows_fit("bce_weighted_bwd", H * W, max(Creal, nw), t, "t", False)
    _rows_fit("bce_weighted_bwd", H * W, Creal, dp, "dp", True)
    _class_w_fits("bce_weighted_bwd", class_w, nw, p.device)
    assert gout.dtype == torch.float32 and gout.numel() == 1 and gout.device == p.device
    L.check(L.lib().sgan_bce_weighted_bwd(_ptr(_act(p)), p.stride(1), _ptr(_act(t)), t.stride(1), H * W, Creal, _ptr(class_w), int(nw),
                                          _ptr(gout), _ptr(_act(dp)), dp.stride(1), _stream()), "sgan_bce_weighted_bwd")


SEGHEAD_WS_BYTES = L.DEFINES["SGAN_SEGHEAD_WS_BYTES"]
SEGHEAD_SOFTMAX, SEGHEAD_SIGMOID = L.SEGHEAD_SOFTMAX, L.SEGHEAD_SIGMOID


def _seghead_workspace(device, which):
    """which: "head" (sgan_seg_head) or "norm" (sgan_label_weight_sum) -- the two may be in flight behind one another"""
    return _zeroed_workspace("seghead_" + which, device, SEGHEAD_WS_BYTES)


def label_weight_sum(label, Creal, class_w, out):
    """out[0] = sum over the pixels of class_w[label] (class_w None: the count of labels in [0, Creal)): sgan_label_weight_sum on an
    int64 device label map; `out` a float32 device scalar."""
    require_gpu(label, "label_weight_sum")
    assert label.dtype == torch.int64 and label.is_contiguous() and out.dtype == torch.float32 and out.numel() == 1 and out.device == label.device
    assert class_w is None or (class_w.dtype == torch.float32 and class_w.is_contiguous() and class_w.numel() >= Creal and class_w.device == label.device)
    rc = L.lib().sgan_label_weight_sum(_ptr(label), label.numel(), int(Creal), _ptr(class_w), _ptr(out),
                                       _ptr(_seghead_workspace(label.device, "norm")), _stream())
    if rc == 1:
        raise L.SganError("sgan_label_weight_sum: not covered (more than 16 classes)")
    L.check(rc, "sgan_label_weight_sum")


def pixel_weight_sum(label, Creal, class_w, pixel_add, out):
    """out[0] = sum over the pixels with a label in [0, Creal) of class_w[label] + pixel_add (class_w None: 1 + pixel_add):
    sgan_pixel_weight_sum, the norm of seg_head_pw.  `pixel_add`: a dense float32 map of label.numel() entries (border_weight's bmap)."""
    require_gpu(label, "pixel_weight_sum")
    assert label.dtype == torch.int64 and label.is_contiguous() and out.dtype == torch.float32 and out.numel() == 1 and out.device == label.device
    assert class_w is None or (class_w.dtype == torch.float32 and class_w.is_contiguous() and class_w.numel() >= Creal and class_w.device == label.device)
    assert (pixel_add.dtype == torch.float32 and pixel_add.is_contiguous() and pixel_add.numel() == label.numel()
            and pixel_add.device == label.device), (pixel_add.shape, pixel_add.dtype)
    rc = L.lib().sgan_pixel_weight_sum(_ptr(label), label.numel(), int(Creal), _ptr(class_w), _ptr(pixel_add), _ptr(out),
                                       _ptr(_seghead_workspace(label.device, "norm")), _stream())
    if rc == 1:
        raise L.SganError("sgan_pixel_weight_sum: not covered (more than 16 classes)")
    L.check(rc, "sgan_pixel_weight_sum")


def seg_head(z, Creal, mode, label_or_target, class_w, nw, norm, p, dz, loss_out, pixel_add=None):
    """sgan_seg_head on an [H, W, Cs] logits buffer: p (and dz unless None) are [H, W, Cs'] buffers, `label_or_target` the int64 label
    map of H * W entries (softmax) or the [H, W, Cs''] target buffer (sigmoid), `norm` the float32 device scalar of label_weight_sum
    (softmax).  pixel_add (softmax only): the dense float32 map of H * W per-pixel weight terms of sgan_seg_head_pw, `norm` then the
    scalar of pixel_weight_sum.  Every operand is checked against its storage here, before anything is launched.  Returns False, having
    launched nothing, when the library reports the call as not covered."""
    H, W, _ = z.shape

    def rows_fit(t, what, written):
        # the kernel moves whole stored rows (16-byte accesses) where the pixel stride is 4, 8, 12 or 16, and writes the padding channels
        _act(t)
        row = t.stride(1) if (written or t.stride(1) in (4, 8, 12, 16)) else Creal
        if t.shape[0] * t.shape[1] != H * W or t.shape[2] < Creal or t.stride(1) < Creal or (H * W - 1) * t.stride(1) + row > _avail(t):
            raise L.SganError(f"seg_head {what}: tensor {tuple(t.shape)} (pixel stride {t.stride(1)}, {_avail(t)} elements of storage) does "
                              f"not hold {H}x{W} rows of {row}; nothing was launched")

    rows_fit(z, "logits", False)
    rows_fit(p, "p", True)
    assert loss_out.dtype == torch.float32 and loss_out.numel() == 1 and loss_out.is_cuda
    if dz is not None:
        rows_fit(dz, "dlogits", True)
    tld = 0
    if mode == SEGHEAD_SOFTMAX:
        assert label_or_target.dtype == torch.int64 and label_or_target.is_cuda and label_or_target.is_contiguous() and label_or_target.numel() == H * W
        assert norm is not None and norm.dtype == torch.float32 and norm.is_cuda and norm.numel() == 1
        assert class_w is None or nw >= Creal
    else:
        rows_fit(label_or_target, "target", False)
        tld = label_or_target.stride(1)
        assert nw <= Creal
    assert class_w is None or (class_w.dtype == torch.float32 and class_w.is_cuda and class_w.is_contiguous() and class_w.numel() >= nw)
    if pixel_add is not None:
        assert mode == SEGHEAD_SOFTMAX, "seg_head: a per-pixel weight goes with the softmax cross-entropy only"
        assert pixel_add.dtype == torch.float32 and pixel_add.is_cuda and pixel_add.is_contiguous() and pixel_add.numel() == H * W
        rc = L.lib().sgan_seg_head_pw(_ptr(z), z.stride(1), H * W, int(Creal), _ptr(label_or_target), _ptr(class_w),
                                      int(nw) if class_w is not None else 0, _ptr(pixel_add), _ptr(norm), _ptr(p), p.stride(1), _ptr(dz),
                                      dz.stride(1) if dz is not None else 0, _ptr(loss_out), _ptr(_seghead_workspace(z.device, "head")),
                                      _stream())
        name = "sgan_seg_head_pw"
    else:
        rc = L.lib().sgan_seg_head(_ptr(z), z.stride(1), H * W, int(Creal), int(mode), _ptr(label_or_target), tld, _ptr(class_w),
                                   int(nw) if class_w is not None else 0, _ptr(norm), _ptr(p), p.stride(1), _ptr(dz),
                                   dz.stride(1) if dz is not None else 0, _ptr(loss_out), _ptr(_seghead_workspace(z.device, "head")), _stream())
        name = "sgan_seg_head"
    if rc == 1:
        return False
    L.check(rc, name)
    return True


def seg_head_pw(z, Creal, label, class_w, nw, pixel_add, norm, p, dz, loss_out):
    """sgan_seg_head_pw: seg_head in softmax mode with w_p = class_w[y_p] + pixel_add[p]."""
    return seg_head(z, Creal, SEGHEAD_SOFTMAX, label, class_w, nw, norm, p, dz, loss_out, pixel_add=pixel_add)


def sigmoid_fwd(x, p):
    H, W, _ = x.shape
    L.check(L.lib().sgan_sigmoid_fwd(_ptr(_act(x)), x.stride(1), H * W, _ptr(_act(p)), p.stride(1), _stream()), "sgan_sigmoid_fwd")


def sigmoid_bwd(dp, p, dx):
    H, W, _ = p.shape
    L.check(L.lib().sgan_sigmoid_bwd(_ptr(_act(dp)), dp.stride(1), _ptr(_act(p)), p.stride(1), H * W, _ptr(_act(dx)),
                                     dx.stride(1), _stream()), "sgan_sigmoid_bwd")


def tanh_bwd(dy, y, dx):
    assert dy.is_contiguous() and y.is_contiguous() and dx.is_contiguous()
    L.check(L.lib().sgan_tanh_bwd(_ptr(dy), _ptr(y), _ptr(dx), dy.numel(), _stream()), "sgan_tanh_bwd")


def add_act_fwd(a, b, out, act=ACT_TANH):
    """out = act(a + b) on contiguous padded NHWC buffers of one shape (the --use_residual tail of the generators)."""
    assert a.shape == b.shape == out.shape and a.is_contiguous() and b.is_contiguous() and out.is_contiguous()
    L.check(L.lib().sgan_add_act_fwd(_ptr(a), _ptr(b), _ptr(out), a.numel(), int(act), _stream()), "sgan_add_act_fwd")


def adam_multi(segs, lr_dev, beta1, beta2, eps, state_dev):
    """segs: list of (p, g, m, v, n) flat fp32 tensors (16-byte aligned)."""
    arr = (L.AdamSeg * len(segs))()
    for i, (p, g, m, v, n) in enumerate(segs):
        arr[i] = L.AdamSeg(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n)
    L.check(L.lib().sgan_adam_multi(arr, len(segs), _ptr(lr_dev), beta1, beta2, eps, _ptr(state_dev), _stream()), "sgan_adam_multi")


def adam_pack(p, g, m, v, lr_dev, beta1, beta2, eps, state_dev, flat_t, pk_f, pk_b, pk_b16, segs, zero_grads):
    """One launch: Adam over the flat segment (p, g, m, v) + the derived weight copies of its conv ranges
    `segs` = [(off, taps, cout_s, cin_s)] (offsets relative to p; sorted) + optional zeroing of the consumed gradients."""
    arr = (L.WtSeg * max(len(segs), 1))(*[L.WtSeg(int(o), int(t), int(co), int(ci)) for o, t, co, ci in segs])
    L.check(L.lib().sgan_adam_pack(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), _ptr(lr_dev), beta1, beta2, eps, _ptr(state_dev),
                                   _ptr(flat_t), _ptr(pk_f), _ptr(pk_b), _ptr(pk_b16), arr, len(segs), int(bool(zero_grads)), _stream()), "sgan_adam_pack")


def zero_multi(bufs):
    """Zero a list of contiguous device tensors (byte sizes multiples of 16) in one launch per 64."""
    for i0 in range(0, len(bufs), 64):
        part = bufs[i0:i0 + 64]
        ptrs = (C.c_void_p * len(part))(*[t.data_ptr() for t in part])
        nb = (C.c_int64 * len(part))(*[t.numel() * t.element_size() for t in part])
        L.check(L.lib().sgan_zero_multi(ptrs, nb, len(part), _stream()), "sgan_zero_multi")


def sgd_multi(segs, lr_dev, momentum):
    """segs: list of (p, g, buf or None, n) flat fp32 tensors."""
    arr = (L.AdamSeg * len(segs))()
    for i, (p, g, m, n) in enumerate(segs):
        arr[i] = L.AdamSeg(p.data_ptr(), g.data_ptr(), m.data_ptr() if m is not None else None, None, n)
    L.check(L.lib().sgan_sgd_multi(arr, len(segs), _ptr(lr_dev), float(momentum), _stream()), "sgan_sgd_multi")


def ema_multi(segs, decay, warmup, state):
    """One sgan_ema_multi launch: shadow += (1 - d_t) * (p - shadow) over segs = [(shadow, p)], pairs of contiguous flat fp32 device
    tensors of equal length (4-byte alignment is enough; `p` is only read).  `state`: the 4 int32 words of the average on the device,
    state[0] = updates made so far.  d_t = decay, or min(decay, (1 + t) / (10 + t)) with `warmup`.  Nothing is read back."""
    arr = (L.EmaSeg * max(len(segs), 1))()
    for i, (s, p) in enumerate(segs):
        if (s.dtype != torch.float32 or p.dtype != torch.float32 or not s.is_contiguous() or not p.is_contiguous() or s.dim() != 1
                or s.shape != p.shape or s.device != p.device):
            raise L.SganError(f"ema_multi: segment {i} must be a pair of contiguous flat fp32 tensors of equal length on one device, got "
                              f"{tuple(s.shape)} {s.dtype} / {tuple(p.shape)} {p.dtype}; nothing was launched")
        require_gpu(s, "ema_multi")
        arr[i] = L.EmaSeg(s.data_ptr(), p.data_ptr(), s.numel())
    assert state.dtype == torch.int32 and state.numel() >= 4 and state.is_contiguous()
    require_gpu(state, "ema_multi")
    L.check(L.lib().sgan_ema_multi(arr, len(segs), float(decay), int(bool(warmup)), _ptr(state), _stream()), "sgan_ema_multi")


# ------------------------------------------------------------------------------------------------
# Differentiable augmentation of discriminator inputs (sgan_diffaug.hip).  A record is 8 words of device memory,
# {b, a, ty, tx, cy0, cy1, cx0, cx1}: `records` below is an int32 [n, 8] tensor whose first two columns hold the bits of two floats.
# ------------------------------------------------------------------------------------------------
DIFFAUG_BITS = {n: L.DEFINES['SGAN_DIFFAUG_' + n.upper()] for n in ('translation', 'cutout', 'brightness', 'contrast')}
DIFFAUG_MAX_JOBS = L.DEFINES['SGAN_DIFFAUG_MAX_JOBS']


def _diffaug_records(records, n, what):
    if (records.dtype != torch.int32 or records.dim() != 2 or records.shape[1] != 8 or records.shape[0] < n or not records.is_contiguous()):
        raise L.SganError(f"{what}: records must be a contiguous int32 [>= {n}, 8] tensor, got {tuple(records.shape)} {records.dtype}")
    require_gpu(records, what)


def diffaug_workspace(njobs, device):
    """The fp64 slots sgan_diffaug_multi_fwd / _bwd need when a record may carry a contrast a != 1."""
    nbytes = L.lib().sgan_diffaug_workspace(int(njobs))
    if nbytes < 0:
        raise L.SganError(f"diffaug_workspace: {njobs} jobs, 1..{DIFFAUG_MAX_JOBS} supported")
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def diffaug_draw(records, shapes, policy_bits, rt, rc, seed, offset_dev=None, advance=True):
    """One sgan_diffaug_draw launch: record j of `records` for an image of shapes[j] = (H, W), from the Philox blocks at
    offset + 2 j and offset + 2 j + 1 of the stream `seed`; `offset_dev` (device int64 [1]) moves on by 2 len(shapes) with `advance`."""
    n = len(shapes)
    _diffaug_records(records, n, "diffaug_draw")
    arr = (C.c_int32 * (2 * max(n, 1)))(*[int(v) for hw in shapes for v in hw])
    L.check(L.lib().sgan_diffaug_draw(_ptr(records), arr, n, int(policy_bits), float(rt), float(rc), C.c_uint64(seed & (2 ** 64 - 1)),
                                      _ptr(offset_dev), int(bool(advance)), _stream()), "sgan_diffaug_draw")


def _diffaug_multi(fn, what, srcs, dsts, Cs_real, colour_mask, records, workspace):
    n = len(srcs)
    _diffaug_records(records, n, what)
    arr = (L.DiffaugJob * max(n, 1))()
    for j, (s, d, Cr) in enumerate(zip(srcs, dsts, Cs_real)):
        _act(s), _act(d)
        require_gpu(s, what)
        if not (s.is_contiguous() and d.is_contiguous() and s.shape == d.shape):
            raise L.SganError(f"{what}: job {j} needs two contiguous [H, W, Cs] buffers of one shape, got {tuple(s.shape)} / {tuple(d.shape)}; "
                              "nothing was launched")
        H, W, Cs = s.shape
        arr[j] = L.DiffaugJob(s.data_ptr(), d.data_ptr(), H, W, int(Cr), Cs, int(colour_mask))
    if workspace is not None:
        assert workspace.dtype == torch.float64 and workspace.is_contiguous() and workspace.numel() * 8 >= L.lib().sgan_diffaug_workspace(max(n, 1))
        require_gpu(workspace, what)
    L.check(fn(arr, n, _ptr(records), _ptr(workspace), _stream()), what)


def diffaug_multi_fwd(srcs, dsts, Cs_real, colour_mask, records, workspace=None):
    """One sgan_diffaug_multi_fwd call: dsts[j] = the transform of srcs[j] (padded NHWC buffers, Cs_real[j] logical channels) under
    record j.  workspace None: the one-launch form, which takes every record's contrast as 1."""
    _diffaug_multi(L.lib().sgan_diffaug_multi_fwd, "sgan_diffaug_multi_fwd", srcs, dsts, Cs_real, colour_mask, records, workspace)


def diffaug_multi_bwd(dys, dxs, Cs_real, colour_mask, records, workspace=None):
    """The adjoint of diffaug_multi_fwd under the same records: dxs[j] from dys[j]."""
    _diffaug_multi(L.lib().sgan_diffaug_multi_bwd, "sgan_diffaug_multi_bwd", dys, dxs, Cs_real, colour_mask, records, workspace)


class _DiffAugFn(torch.autograd.Function):
    """The transform of several logical [1, C, H, W] tensors under consecutive records, one call forward; backward transforms the
    gradients of the tensors that need one under the records the forward used (one call per run of consecutive such tensors)."""

    @staticmethod
    def forward(ctx, records, colour_mask, workspace, *xs):
        xbs = [as_nhwc(x) for x in xs]
        outs = [torch.empty_like(xb) for xb in xbs]
        ctx.Cr = [x.shape[1] for x in xs]
        diffaug_multi_fwd(xbs, outs, ctx.Cr, colour_mask, records, workspace)
        ctx.records, ctx.colour_mask, ctx.workspace = records, colour_mask, workspace
        ctx.outs = outs      # as _CatPairFn: the buffers outlive the call so that the views map back to them without a copy
        return tuple(logical_view(o, c) for o, c in zip(outs, ctx.Cr))

    @staticmethod
    def backward(ctx, *gs):
        n = len(gs)
        dxs = [None] * n
        j = 0
        while j < n:
            if not ctx.needs_input_grad[3 + j] or gs[j] is None:
                j += 1
                continue
            k = j
            while k < n and ctx.needs_input_grad[3 + k] and gs[k] is not None:
                k += 1
            gbs = [as_nhwc(g) for g in gs[j:k]]
            dbs = [torch.empty_like(gb) for gb in gbs]
            diffaug_multi_bwd(gbs, dbs, ctx.Cr[j:k], ctx.colour_mask, ctx.records[j:], ctx.workspace)
            for i, db in enumerate(dbs):
                dxs[j + i] = logical_view(db, ctx.Cr[j + i])
            j = k
        return (None, None, None) + tuple(dxs)


def diffaug(x, state, slot=0):
    """DiffAugment of a logical [1, C, H, W] tensor -- or of a list of them in one launch -- under the records state.records[slot],
    state.records[slot + 1], ... (written by diffaug_draw, or by the caller), with state.colour_mask and state.workspace (None: no
    record carries a contrast).  Differentiable: backward calls sgan_diffaug_multi_bwd with the same records; a tensor that needs no
    gradient records no backward.  The records must not be redrawn between this call and its backward."""
    xs = list(x) if isinstance(x, (list, tuple)) else [x]
    for t in xs:
        require_gpu(t, "diffaug")
    outs = _DiffAugFn.apply(state.records[slot: slot + len(xs)], int(state.colour_mask), state.workspace, *xs)
    return list(outs) if isinstance(x, (list, tuple)) else outs[0]


def lbfgs_advance(state, J, n, x, grad, loss, d, prev_grad, hist_s, hist_y, hist_rho):
    """One sgan_lbfgs_advance launch over J problems of n unknowns (supervised_gan_amd.lbfgs.DeviceLBFGS owns the buffers).
    x, grad: [J, >= n] fp32 with unit element stride; loss: [J] fp32."""
    from .lbfgs import LbfgsState
    m = hist_rho.shape[1]
    assert 1 <= J <= 8 and n >= 1 and state.dtype == torch.uint8 and tuple(state.shape) == (J, C.sizeof(LbfgsState))
    for t, what in ((x, "x"), (grad, "grad")):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != J or t.shape[1] < n or t.stride(1) != 1 or (J - 1) * t.stride(0) + n > _avail(t):
            raise L.SganError(f"lbfgs_advance: {what} must be a [J={J}, >= {n}] fp32 tensor with unit element stride, got "
                              f"{tuple(t.shape)} / {tuple(t.stride())} {t.dtype}; nothing was launched")
    for t, shape in ((loss, (J,)), (d, (J, n)), (prev_grad, (J, n)), (hist_s, (J, m, n)), (hist_y, (J, m, n)), (hist_rho, (J, m))):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shape, (tuple(t.shape), shape)
    for t in (state, x, grad, loss, d, prev_grad, hist_s, hist_y, hist_rho):
        require_gpu(t, "lbfgs_advance")
    L.check(L.lib().sgan_lbfgs_advance(_ptr(state), J, n, _ptr(x), x.stride(0), _ptr(grad), grad.stride(0), _ptr(loss), _ptr(d),
                                       _ptr(prev_grad), _ptr(hist_s), _ptr(hist_y), _ptr(hist_rho), m, _stream()), "sgan_lbfgs_advance")


def normal_fill(dst, seed, offset_dev=None, advance=True):
    assert dst.is_contiguous() and dst.dtype == torch.float32
    L.check(L.lib().sgan_normal_fill(_ptr(dst), dst.numel(), C.c_uint64(seed & (2 ** 64 - 1)), _ptr(offset_dev), int(bool(advance)),
                                     _stream()), "sgan_normal_fill")


def normal_fill_nhwc(buf, C_real, seed, offset_dev=None, advance=True):
    """N(0, 1) values of a logical [1, C_real, H, W] tensor (the same values normal_fill gives its contiguous form), written into
    the padded NHWC buffer `buf` [H, W, Cs] the networks read: no layout kernel between the draw and the generator."""
    H, W, Cs = buf.shape
    assert buf.is_contiguous() and buf.dtype == torch.float32
    L.check(L.lib().sgan_normal_fill_nhwc(_ptr(buf), int(C_real), H, W, Cs, C.c_uint64(seed & (2 ** 64 - 1)), _ptr(offset_dev),
                                          int(bool(advance)), _stream()), "sgan_normal_fill_nhwc")


def normal_fill_nhwc_pair(buf_a, buf_b, C_real, seed, offset_dev, zero=None):
    """normal_fill_nhwc(buf_a) then normal_fill_nhwc(buf_b) -- same values, same advance of the stream -- as ONE launch that also
    zeroes the contiguous tensor `zero` (the statistics arena of the pass that reads the two latents)."""
    H, W, Cs = buf_a.shape
    assert buf_a.shape == buf_b.shape and buf_a.is_contiguous() and buf_b.is_contiguous() and buf_a.dtype == buf_b.dtype == torch.float32
    assert zero is None or zero.is_contiguous()
    L.check(L.lib().sgan_normal_fill_nhwc_pair(_ptr(buf_a), _ptr(buf_b), int(C_real), H, W, Cs, C.c_uint64(seed & (2 ** 64 - 1)),
                                               _ptr(offset_dev), _ptr(zero), zero.numel() * zero.element_size() if zero is not None else 0,
                                               _stream()), "sgan_normal_fill_nhwc_pair")


# ------------------------------------------------------------------------------------------------
# NCHW <-> NHWC boundary.  Tensors handed to user code are logical [1, C, H, W] *views* of our
# padded NHWC buffers (zero copy); a weak registry lets us recognise such a view (or its .detach())
# when it comes back, otherwise one strided-gather kernel converts the layout.
# ------------------------------------------------------------------------------------------------
_VIEW_REGISTRY = {}


def logical_view(buf: torch.Tensor, C_real: int) -> torch.Tensor:
    """[H, W, Cs] buffer -> logical [1, C_real, H, W] view; registered for zero-copy round trips."""
    v = buf.permute(2, 0, 1)[:C_real].unsqueeze(0)
    _VIEW_REGISTRY[buf.data_ptr()] = (weakref.ref(buf), C_real, buf.untyped_storage()._cdata, tuple(buf.shape))
    if len(_VIEW_REGISTRY) > 4096:
        for k in [k for k, e in _VIEW_REGISTRY.items() if e[0]() is None]:
            del _VIEW_REGISTRY[k]
    return v


def buffer_of(t: torch.Tensor):
    """The padded NHWC buffer a logical_view() tensor was made from (same memory), or None."""
    ent = _VIEW_REGISTRY.get(t.data_ptr())
    if ent is None or t.dim() != 4:
        return None
    buf = ent[0]()
    _, Cr, H, W = t.shape
    if (buf is not None and ent[1] == Cr and buf.shape[:2] == (H, W) and buf.data_ptr() == t.data_ptr()
            and t.stride(1) == 1 and t.stride(2) == buf.stride(0) and t.stride(3) == buf.stride(1)):
        return buf
    return None


def host_batch_to_nhwc(t: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """Pinned-host (or device) logical [1, C <= 4, H, W] fp32 batch -> the padded NHWC device buffer `out` [H, W, 4], by ONE gather
    kernel that reads the source where it lies: for a pinned host tensor that kernel is the H2D copy, on the current stream."""
    assert t.dim() == 4 and t.shape[0] == 1 and t.dtype == torch.float32 and t.stride(3) == 1, (t.shape, t.stride(), t.dtype)
    assert t.is_cuda or t.is_pinned(), "host batches must be pinned (page-locked) to be read by the device"
    _, Cr, H, W = t.shape
    assert out.shape == (H, W, 4) and Cr <= 4
    L.check(L.lib().sgan_to_nhwc(_ptr(t), t.stride(1), t.stride(2), 1, H, W, Cr, _ptr(out), out.stride(1), 4, _stream()), "sgan_to_nhwc")
    return out


def concat_nhwc(a, Ca, b, Cb):
    """Padded NHWC buffers a [H, W, >= Ca], b [H, W, >= Cb] -> [H, W, pad4(Ca + Cb)]: torch.cat of the logical tensors, one pass."""
    H, W, _ = a.shape
    assert b.shape[:2] == (H, W)
    out = torch.empty((H, W, pad4(Ca + Cb)), dtype=torch.float32, device=a.device)
    L.check(L.lib().sgan_concat_nhwc(_ptr(_act(a)), a.stride(1), int(Ca), _ptr(_act(b)), b.stride(1), int(Cb), H * W, _ptr(out), out.stride(1),
                                     out.shape[2], _stream()), "sgan_concat_nhwc")
    return out


def slice_nhwc(src, c0, Cn, out=None):
    """Channels [c0, c0 + Cn) of a padded NHWC buffer as a padded NHWC buffer of their own (`out`: write into this one)."""
    H, W, _ = src.shape
    if out is None:
        out = torch.empty((H, W, pad4(Cn)), dtype=torch.float32, device=src.device)
    assert out.shape[:2] == (H, W) and out.shape[2] >= pad4(Cn)
    L.check(L.lib().sgan_slice_nhwc(_ptr(_act(src)), src.stride(1), int(c0), int(Cn), H * W, _ptr(out), out.stride(1), out.shape[2], _stream()),
            "sgan_slice_nhwc")
    return out


def as_nhwc(t: torch.Tensor) -> torch.Tensor:
    """Logical [1, C, H, W] tensor (any strides) -> padded NHWC buffer [H, W, pad4(C)]."""
    require_gpu(t, "as_nhwc")
    assert t.dim() == 4 and t.shape[0] == 1, f"batch 1 NCHW expected, got {tuple(t.shape)}"
    if t.dtype != torch.float32:
        raise L.SganError(f"fp32 expected, got {t.dtype}")
    _, Cr, H, W = t.shape
    Cs = pad4(Cr)
    ent = _VIEW_REGISTRY.get(t.data_ptr())
    if ent is not None:
        buf = ent[0]()
        if (buf is None and ent[3] == (H, W, Cs) and t.untyped_storage()._cdata == ent[2] and t.stride(1) == 1
                and t.stride(3) == Cs and t.stride(2) == W * Cs):
            # the buffer's Python object is gone (autograd hands out detached aliases of view outputs, ImagePool.query detaches)
            # but `t` still IS that buffer's storage at the registered address: the same memory under the buffer's shape
            buf = t.as_strided((H, W, Cs), (W * Cs, Cs, 1))
        if (buf is not None and ent[1] == Cr and buf.shape == (H, W, Cs) and buf.data_ptr() == t.data_ptr()
                and t.stride(1) == 1 and t.stride(2) == buf.stride(0) and t.stride(3) == buf.stride(1)):
            return buf
    out = torch.empty((H, W, Cs), device=t.device, dtype=torch.float32)
    L.check(L.lib().sgan_to_nhwc(_ptr(t), t.stride(1), t.stride(2), t.stride(3), H, W, Cr, _ptr(out), Cs, Cs, _stream()),
            "sgan_to_nhwc")
    return out


# ------------------------------------------------------------------------------------------------
# Segmentation metrics (sgan_metrics.hip): labelling, Rand F-score sums, VInfo, confusion matrix.  All
# of them only enqueue; `metric_err` is the one word the kernels raise when they had to give up on a pixel.
# ------------------------------------------------------------------------------------------------
_metric_err = {}
_metric_ws = {}       # (C symbol of the size query, H, W, device index) -> the int64 scratch of that size
REGION_COLS = L.DEFINES["SGAN_REGION_COLS"]      # int64 per row of a region table (include/sgan_hip.h, sgan_region_stats)
# acc_i / counts_out and acc_f / sums_out of object_match_accumulate (SGAN_OBJ_* of include/sgan_hip.h); TP_k: matches at IoU > (10 + k) / 20
OBJECT_COUNTS = tuple('TP_%d' % k for k in range(10)) + ('N_t', 'N_s', 'images', 'SEGn', 'zero14', 'zero15')
OBJECT_SUMS = ('SIoU', 'SSEG')
# acc_i / counts_out and acc_f / sums_out of boundary_accumulate (SGAN_BND_* of include/sgan_hip.h); bin k: (k - 1)^2 < distance^2 <= k^2,
# bin 31: farther than 30 pixels, or the other map has no wall
BOUNDARY_BINS = L.DEFINES["SGAN_BND_BINS"]
BOUNDARY_COUNTS = (tuple('hist_s_%d' % k for k in range(BOUNDARY_BINS)) + tuple('hist_t_%d' % k for k in range(BOUNDARY_BINS))
                   + ('N_s', 'N_t', 'images', 'haus_images', 'defined_s', 'defined_t', 'max_dsq_s', 'max_dsq_t')
                   + tuple('zero%d' % k for k in range(72, 80)))
BOUNDARY_SUMS = ('sum_d_s', 'sum_d_t', 'sum_haus', 'zero3')
CLEAN_COUNTS = ('closed_pixels', 'wall_components_removed', 'wall_pixels_removed', 'cells_filled', 'cell_pixels_filled', 'images')      # acc of clean_wall (SGAN_CLEAN_COUNTS)
SPLIT_COUNTS = ('core_components', 'cut_pixels', 'labelled_pixels', 'rounds', 'budget_hits', 'images')      # acc of split_cells (SGAN_SPLIT_COUNTS)
SPLIT_BUDGET_BIT = 64      # metric_err: split_cells' last round still labelled something; the map is complete for that budget, so no error
# acc_i / counts_out of topo_accumulate (SGAN_TOPO_COUNTS of include/sgan_hip.h): windows scored, the summed |difference| of the windows'
# Betti numbers, their plain sums per map (s: prediction, t: truth), the skeleton pixels of clDice, images
TOPO_COUNTS = ('windows', 'abs_d0', 'abs_d1', 'b0_s', 'b0_t', 'b1_s', 'b1_t', 'skel_s', 'skel_s_in_t', 'skel_t', 'skel_t_in_s', 'images')
VINFO_PARTS = ('SA', 'SB', 'SAB', 'aux', 'm', 'H_S', 'H_T', 'I', 'VInfo', 'split', 'merge')      # parts_out of vinfo_accumulate


def metric_err(device):
    """The zero-initialised int32 the metric kernels of `device` set nonzero on a bounded loop that ran out, a full pair table or a
    label out of range (read it with check_metric_err when the results are read)."""
    e = _metric_err.get(device.index)
    if e is None:
        e = _metric_err[device.index] = torch.zeros(1, dtype=torch.int32, device=device)
    return e


def check_metric_err(device):
    """Synchronises.  Raises if a metric kernel flagged its result as incomplete since the last check."""
    e = _metric_err.get(device.index)
    code = int(e.item()) if e is not None else 0
    if code:
        e.zero_()
    if code & ~SPLIT_BUDGET_BIT:      # a split budget that was hit is counted in SPLIT_COUNTS; its map is what the budget defines
        raise L.SganError(f"segmentation metric kernels gave up on part of their input (flags {code:#x}: 1 = union-find bound, "
                          "2 = pair table full, 4 / 8 = label out of range, 16 = thinning budget ran out, 32 = region table full, 128 = patch position outside its level, 256 = a topology window's labelling did not converge); the accumulated values are incomplete")


def _metric_workspace(symbol, H, W, device):
    """The scratch whose byte count the C function `symbol` reports for H x W maps, made once per (symbol, H, W, device)."""
    key = (symbol, H, W, device.index)
    ws = _metric_ws.get(key)
    if ws is None:
        nbytes = getattr(L.lib(), symbol)(H, W)
        if nbytes < 0:
            raise L.SganError(f"{symbol}({H}, {W}): {L.lib().sgan_last_error().decode()}")
        ws = _metric_ws[key] = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=device)
    return ws


def _label_pair(t_maps, s_maps, what):
    """The check every counting call makes of its two int32 [H, W] maps on one device; returns (H, W, device)."""
    H, W = t_maps.shape
    dev = t_maps.device
    require_gpu(t_maps, what)
    for t in (t_maps, s_maps):
        assert t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == (H, W) and t.device == dev, (t.shape, t.dtype)
    return H, W, dev


def _is_acc(a, dtype, n, dev):
    """An optional accumulator / output of a metric call: None, or n contiguous elements of dtype on dev."""
    return a is None or (a.dtype == dtype and a.is_contiguous() and a.numel() == n and a.device == dev)


def _plane(t, what):
    """A [H, W] fp32 view whose rows follow each other at the pixel stride (channel 0 of an NHWC buffer, or a contiguous map)."""
    require_gpu(t, what)
    assert t.dim() == 2 and t.dtype == torch.float32, (t.shape, t.dtype)
    H, W = t.shape
    if t.stride(1) < 1 or (H > 1 and t.stride(0) != W * t.stride(1)):
        t = t.contiguous()
    if (H * W - 1) * t.stride(1) + 1 > _avail(t):
        raise L.SganError(f"{what}: plane {tuple(t.shape)} / {tuple(t.stride())} does not lie inside its storage; nothing was launched")
    return t


def ccl_label(plane, labels=None):
    """8-connected components of the pixels of `plane` [H, W] that are NOT > 0.5 (sgan_ccl_label): int32 [H, W], 0 = wall, else
    1 + the smallest raster index of the component.  `plane` is read in place when its rows are W pixel strides apart."""
    plane = _plane(plane, "ccl_label")
    H, W = plane.shape
    if labels is None:
        labels = torch.empty((H, W), dtype=torch.int32, device=plane.device)
    assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.numel() == H * W and labels.device == plane.device
    L.check(L.lib().sgan_ccl_label(_ptr(plane), plane.stride(1), H, W, _ptr(labels), _ptr(metric_err(plane.device)), _stream()),
            "sgan_ccl_label")
    return labels


def border_weight(labels, radius, w0, sigma, bmap=None, d1sq=None, d2sq=None):
    """The border term of the U-Net loss on `labels` (int32 [H, W] in ccl_label's form: 0 = wall, else a cell id), sgan_border_weight:
    bmap [H, W] float32 = w0 exp(-(d1 + d2)^2 / (2 sigma^2)) on wall pixels with two distinct cells within `radius` (1..32), else 0.
    d1sq / d2sq (optional int32 [H, W]) receive the squared distances to the nearest and second-nearest cell, -1 where there is none
    (util.border_weight_map is the host yardstick).  Only enqueues -- the launch depends on the shape and the radius alone.  A label
    < 0 counts as wall and raises bit 4 of metric_err."""
    require_gpu(labels, "border_weight")
    assert labels.dim() == 2 and labels.dtype == torch.int32 and labels.is_contiguous(), (labels.shape, labels.dtype)
    H, W = labels.shape
    dev = labels.device
    if bmap is None:
        bmap = torch.empty((H, W), dtype=torch.float32, device=dev)
    assert bmap.dtype == torch.float32 and bmap.is_contiguous() and bmap.numel() == H * W and bmap.device == dev
    for d in (d1sq, d2sq):
        assert d is None or (d.dtype == torch.int32 and d.is_contiguous() and d.numel() == H * W and d.device == dev)
    rc = L.lib().sgan_border_weight(_ptr(labels), H, W, int(radius), float(w0), float(sigma), _ptr(bmap), _ptr(d1sq), _ptr(d2sq),
                                    _ptr(metric_err(dev)), _stream())
    if rc == 1:
        raise L.SganError(f"sgan_border_weight: refused ({H} x {W}, radius {radius} (1..32), sigma {sigma} (> 0)); nothing was launched")
    L.check(rc, "sgan_border_weight")
    return bmap


def thin_workspace(H, W, device):
    """The scratch of thin for H x W planes (change counters and two byte masks), cached per (H, W, device) like rand_f_workspace."""
    return _metric_workspace("sgan_thin_workspace", H, W, device)


def thin(plane, out=None, max_num_iter=None, iters_out=None, workspace=None):
    """Guo-Hall thinning of the pixels of `plane` [H, W] that are > 0.5 to one-pixel lines (sgan_thin; util.thin is the host
    yardstick): float32 [H, W] of 0.0 / 1.0, which ccl_label labels as it lies.  max_num_iter None: until nothing changes.  iters_out
    (int32[1] on the device) receives the number of iterations that deleted something.  Only enqueues -- the launch sequence depends
    on the shape and max_num_iter alone -- and reads `plane` in place when its rows are W pixel strides apart."""
    plane = _plane(plane, "thin")
    assert max_num_iter is None or max_num_iter >= 1, max_num_iter
    H, W = plane.shape
    dev = plane.device
    if out is None:
        out = torch.empty((H, W), dtype=torch.float32, device=dev)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == H * W and out.device == dev
    assert _is_acc(iters_out, torch.int32, 1, dev)
    ws = thin_workspace(H, W, dev) if workspace is None else workspace
    L.check(L.lib().sgan_thin(_ptr(plane), plane.stride(1), H, W, _ptr(out), 0 if max_num_iter is None else int(max_num_iter), _ptr(ws),
                              ws.numel() * ws.element_size(), _ptr(iters_out), _ptr(metric_err(dev)), _stream()), "sgan_thin")
    return out


def region_stats_workspace(H, W, device):
    """The scratch of region_stats for H x W maps (block counts, ranks and the staging rows), cached per (H, W, device)."""
    return _metric_workspace("sgan_region_stats_workspace", H, W, device)


def region_stats(labels, table, cursor, workspace=None):
    """Appends one row of REGION_COLS exact integers per region of `labels` (int32 [H, W] from ccl_label) to `table` (int64
    [capacity, 16] on the device) at row cursor[0], in scipy.ndimage.label's order (sgan_region_stats; util.region_table is the host
    yardstick and names the columns).  cursor: int32[2] on the device, {rows used, images done}, zeroed by the caller once and
    advanced by the call.  Regions beyond the capacity are dropped and raise bit 32 of metric_err.  Only enqueues -- the launch
    sequence depends on the shape alone -- so any number of images go into one table without a read-back."""
    require_gpu(labels, "region_stats")
    assert labels.dim() == 2 and labels.dtype == torch.int32 and labels.is_contiguous(), (labels.shape, labels.dtype)
    H, W = labels.shape
    dev = labels.device
    assert (table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == REGION_COLS and table.shape[0] >= 1
            and table.is_contiguous() and table.device == dev), (table.shape, table.dtype)
    assert cursor.dtype == torch.int32 and cursor.is_contiguous() and cursor.numel() == 2 and cursor.device == dev
    ws = region_stats_workspace(H, W, dev) if workspace is None else workspace
    L.check(L.lib().sgan_region_stats(_ptr(labels), H, W, _ptr(table), table.shape[0], _ptr(cursor), _ptr(ws),
                                      ws.numel() * ws.element_size(), _ptr(metric_err(dev)), _stream()), "sgan_region_stats")
    return table


# ------------------------------------------------------------------------------------------------
# Sliced Wasserstein distance over Laplacian-pyramid patches (sgan_swd.hip; swd.py).  All of them only enqueue.
# ------------------------------------------------------------------------------------------------
SWD_MAX_N = 16384                                  # descriptors per set (include/sgan_hip.h, sgan_swd_distances)
SWD_AUTO, SWD_SPLIT, SWD_FUSED = 0, 1, 2           # `variant` of swd_distances
_swd_ws = {}


def _planes(t, what):
    """A [C, H, W] fp32 tensor whose planes follow each other H row pitches apart; returns (tensor, row pitch in floats)."""
    require_gpu(t, what)
    assert t.dim() == 3 and t.dtype == torch.float32, (t.shape, t.dtype)
    C, H, W = t.shape
    if t.stride(2) != 1 or t.stride(1) < W or (C > 1 and t.stride(0) != H * t.stride(1)):
        t = t.contiguous()
    if (C * H - 1) * t.stride(1) + W > _avail(t):
        raise L.SganError(f"{what}: planes {tuple(t.shape)} / {tuple(t.stride())} do not lie inside their storage; nothing was launched")
    return t, t.stride(1)


def lap_down(x, out=None):
    """One Gaussian pyramid step of x [C, H, W] (H, W even, >= 4): the 5 x 5 binomial blur with a mirrored border, even sites kept
    (sgan_lap_pyramid, mode down; util.lap_down_ref is the host yardstick).  Returns [C, H / 2, W / 2]."""
    x, ld = _planes(x, "lap_down")
    C, H, W = x.shape
    if out is None:
        out = torch.empty((C, H // 2, W // 2), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (C, H // 2, W // 2) and out.device == x.device
    L.check(L.lib().sgan_lap_pyramid(0, _ptr(x), ld, None, 0, C, H, W, _ptr(out), W // 2, _stream()), "sgan_lap_pyramid")
    return out


def lap_up_sub(fine, coarse, out=None):
    """The Laplacian level fine - up(coarse): fine [C, H, W], coarse [C, H / 2, W / 2] (sgan_lap_pyramid, mode up-and-subtract;
    util.lap_up_ref is the host yardstick of up)."""
    fine, ld = _planes(fine, "lap_up_sub")
    coarse, cld = _planes(coarse, "lap_up_sub")
    C, H, W = fine.shape
    assert tuple(coarse.shape) == (C, H // 2, W // 2) and coarse.device == fine.device, (fine.shape, coarse.shape)
    if out is None:
        out = torch.empty((C, H, W), dtype=torch.float32, device=fine.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (C, H, W) and out.device == fine.device
    assert out.data_ptr() != fine.data_ptr()
    L.check(L.lib().sgan_lap_pyramid(1, _ptr(fine), ld, _ptr(coarse), cld, C, H, W, _ptr(out), W, _stream()), "sgan_lap_pyramid")
    return out


def lap_pyramid(img):
    """The Laplacian pyramid of img [C, H, W] on the device, finest first, with the levels of util.lap_pyramid_ref: a further level
    while both sides are even and half the smaller side is at least 16; the last level is the Gaussian one."""
    from .util import lap_level_sizes
    g, _ = _planes(img, "lap_pyramid")
    levels = []
    for _ in lap_level_sizes(*g.shape[1:])[1:]:
        nxt = lap_down(g)
        levels.append(lap_up_sub(g, nxt))
        g = nxt
    levels.append(g)
    return levels


def swd_gather(level, pos, desc, row0, acc):
    """Copies the 7 x 7 patches of `level` [C, H, W] at the top-left corners pos (int32 [P, 3] on the device: image, y, x) into rows
    [row0, row0 + P) of desc (float32 [N, C * 49], order [c][dy][dx]) and adds the per-channel sum and sum of squares to acc (float64
    [2 C], zeroed by the caller once per set): sgan_swd_gather.  A position outside the level zero-fills its row and raises bit 128
    of metric_err."""
    level, ld = _planes(level, "swd_gather")
    C, H, W = level.shape
    dev = level.device
    assert pos.dtype == torch.int32 and pos.dim() == 2 and pos.shape[1] == 3 and pos.is_contiguous() and pos.device == dev, (pos.shape, pos.dtype)
    assert desc.dtype == torch.float32 and desc.dim() == 2 and desc.shape[1] == C * 49 and desc.is_contiguous() and desc.device == dev, desc.shape
    assert _is_acc(acc, torch.float64, 2 * C, dev) and acc is not None
    L.check(L.lib().sgan_swd_gather(_ptr(level), ld, C, H, W, _ptr(pos), pos.shape[0], _ptr(desc), int(row0), desc.shape[0], _ptr(acc),
                                    _ptr(metric_err(dev)), _stream()), "sgan_swd_gather")
    return desc


def swd_workspace(N, K, J, device):
    """The scratch of swd_distances (the projections of up to 512 directions of both sets), cached per (N, K, J, device)."""
    key = (N, K, J, device.index)
    ws = _swd_ws.get(key)
    if ws is None:
        nbytes = L.lib().sgan_swd_workspace(N, K, J)
        if nbytes < 0:
            raise L.SganError(f"sgan_swd_workspace({N}, {K}, {J}): {L.lib().sgan_last_error().decode()}")
        ws = _swd_ws[key] = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=device)
    return ws


def swd_distances(descA, descB, statsA, statsB, dirs, out=None, workspace=None, variant=SWD_AUTO):
    """Per-direction sliced Wasserstein distances of two descriptor matrices (float32 [N, K], K in {49, 98, 147}, N <= 16384):
    each normalised by its own statistics (float64 [2 C] as swd_gather accumulates them), projected onto dirs (float32 [J, K]),
    sorted, compared: out float64 [J] = mean_i |sA_i - sB_i| (sgan_swd_distances; util.swd_ref is the host yardstick).  The same
    bits on every run."""
    require_gpu(descA, "swd_distances")
    dev = descA.device
    assert descA.dim() == 2 and descA.dtype == torch.float32 and descA.is_contiguous(), (descA.shape, descA.dtype)
    N, K = descA.shape
    assert descB.dtype == torch.float32 and descB.is_contiguous() and tuple(descB.shape) == (N, K) and descB.device == dev, descB.shape
    assert dirs.dtype == torch.float32 and dirs.dim() == 2 and dirs.shape[1] == K and dirs.is_contiguous() and dirs.device == dev, dirs.shape
    J = dirs.shape[0]
    if K % 49:
        raise L.SganError(f"swd_distances: K = {K} is not 49, 98 or 147; nothing was launched")
    for s in (statsA, statsB):
        assert _is_acc(s, torch.float64, 2 * (K // 49), dev) and s is not None
    if out is None:
        out = torch.empty(max(J, 1), dtype=torch.float64, device=dev)[:J]
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == J and out.device == dev
    ws = swd_workspace(N, K, J, dev) if workspace is None else workspace
    L.check(L.lib().sgan_swd_distances(_ptr(descA), _ptr(descB), _ptr(statsA), _ptr(statsB), _ptr(dirs), N, K, J, _ptr(out), _ptr(ws),
                                       ws.numel() * ws.element_size(), int(variant), _stream()), "sgan_swd_distances")
    return out


PRD_AUTO, PRD_DIRECT, PRD_GRAM = 0, 1, 2           # `variant` of knn_radii and prd_rows
_prd_ws = {}


def _prd_desc(t, what):
    assert t.dim() == 2 and t.dtype == torch.float32 and t.is_contiguous(), (what, t.shape, t.dtype)
    if t.shape[1] % 49:
        raise L.SganError(f"{what}: K = {t.shape[1]} is not 49, 98 or 147; nothing was launched")
    return t.shape


def _prd_out(t, dtype, n, dev):
    if t is None:
        return torch.empty(max(n, 1), dtype=dtype, device=dev)[:n]
    assert _is_acc(t, dtype, n, dev), (t.shape, t.dtype)
    return t


def prd_workspace(Nq, Nr, K, device):
    """The scratch of knn_radii (Nq = Nr = N) and prd_rows (the row norms of the Gram form), cached per (Nq, Nr, K, device)."""
    key = (Nq, Nr, K, device.index)
    ws = _prd_ws.get(key)
    if ws is None:
        nbytes = L.lib().sgan_prd_workspace(Nq, Nr, K)
        if nbytes < 0:
            raise L.SganError(f"sgan_prd_workspace({Nq}, {Nr}, {K}): {L.lib().sgan_last_error().decode()}")
        ws = _prd_ws[key] = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=device)
    return ws


def knn_radii(desc, stats, k, group=1, rad=None, nn1=None, workspace=None, variant=PRD_AUTO):
    """(rad, nn1) float32 [N] of a descriptor matrix (float32 [N, K], K in {49, 98, 147}, N <= 16384) normalised by stats (float64
    [2 C] as swd_gather accumulates them, over N rows): the squared distance of every row to its k-th (k <= 8) and to its first
    nearest neighbour among the rows of other groups of `group` consecutive rows (sgan_knn_radii; util.knn_radii_ref is the host
    yardstick).  The same bits on every run."""
    require_gpu(desc, "knn_radii")
    dev = desc.device
    N, K = _prd_desc(desc, "knn_radii")
    assert _is_acc(stats, torch.float64, 2 * (K // 49), dev) and stats is not None
    rad, nn1 = _prd_out(rad, torch.float32, N, dev), _prd_out(nn1, torch.float32, N, dev)
    ws = prd_workspace(N, N, K, dev) if workspace is None else workspace
    L.check(L.lib().sgan_knn_radii(_ptr(desc), _ptr(stats), N, K, int(k), int(group), _ptr(rad), _ptr(nn1), _ptr(ws),
                                   ws.numel() * ws.element_size(), int(variant), _stream()), "sgan_knn_radii")
    return rad, nn1


def prd_rows(descQ, descR, stats, radR, cnt=None, nn_d2=None, nn_idx=None, workspace=None, variant=PRD_AUTO):
    """Per row of descQ (float32 [Nq, K]) against descR (float32 [Nr, K]) and the radii of its rows (float32 [Nr]), both normalised
    by stats (float64 [2 C], over Nr rows): (cnt int32 [Nq] = how many balls of R hold the row, nn_d2 float32 [Nq] = the squared
    distance to the nearest row of R, nn_idx int32 [Nq] = the smallest index that attains it): sgan_prd_rows; util.prd_rows_ref is
    the host yardstick.  The same bits on every run."""
    require_gpu(descQ, "prd_rows")
    dev = descQ.device
    Nq, K = _prd_desc(descQ, "prd_rows")
    Nr, Kr = _prd_desc(descR, "prd_rows")
    assert Kr == K and descR.device == dev, (descQ.shape, descR.shape)
    assert _is_acc(stats, torch.float64, 2 * (K // 49), dev) and stats is not None
    assert _is_acc(radR, torch.float32, Nr, dev) and radR is not None
    cnt, nn_d2, nn_idx = _prd_out(cnt, torch.int32, Nq, dev), _prd_out(nn_d2, torch.float32, Nq, dev), _prd_out(nn_idx, torch.int32, Nq, dev)
    ws = prd_workspace(Nq, Nr, K, dev) if workspace is None else workspace
    L.check(L.lib().sgan_prd_rows(_ptr(descQ), _ptr(descR), _ptr(stats), _ptr(radR), Nq, Nr, K, _ptr(cnt), _ptr(nn_d2), _ptr(nn_idx),
                                  _ptr(ws), ws.numel() * ws.element_size(), int(variant), _stream()), "sgan_prd_rows")
    return cnt, nn_d2, nn_idx


def prd_finish(cntB, cntA, nn_d2_A, radA, out=None):
    """int64 [4] on the device: precision hits #{cntB > 0}, recall hits #{cntA > 0}, sum cntB, coverage hits #{nn_d2_A <= radA}
    (sgan_prd_finish; util.prd_from_counts divides)."""
    require_gpu(cntB, "prd_finish")
    dev = cntB.device
    N = cntB.numel()
    assert _is_acc(cntB, torch.int32, N, dev) and _is_acc(cntA, torch.int32, N, dev) and cntA is not None
    assert _is_acc(nn_d2_A, torch.float32, N, dev) and nn_d2_A is not None and _is_acc(radA, torch.float32, N, dev) and radA is not None
    out = _prd_out(out, torch.int64, 4, dev)
    L.check(L.lib().sgan_prd_finish(_ptr(cntB), _ptr(cntA), _ptr(nn_d2_A), _ptr(radA), N, _ptr(out), _stream()), "sgan_prd_finish")
    return out


def rand_f_workspace(H, W, device):
    """The scratch of rand_f_accumulate for H x W maps, cached per (H, W, device); the kernels zero it themselves."""
    return _metric_workspace("sgan_rand_f_workspace", H, W, device)


def rand_f_accumulate(t_labels, s_labels, acc, sums_out=None, f_out=None, workspace=None):
    """acc[0] += Rand F-score of the labelling s_labels (prediction) against t_labels (truth), acc[1] += 1 (sgan_rand_f_accumulate);
    acc: float64[2] on the device.  sums_out (int64[4]: A2, B2, AB2, aux) and f_out (float64[1]) receive this pair's values."""
    H, W, dev = _label_pair(t_labels, s_labels, "rand_f_accumulate")
    assert acc is not None and _is_acc(acc, torch.float64, 2, dev)
    assert _is_acc(sums_out, torch.int64, 4, dev) and _is_acc(f_out, torch.float64, 1, dev)
    ws = rand_f_workspace(H, W, dev) if workspace is None else workspace
    L.check(L.lib().sgan_rand_f_accumulate(_ptr(t_labels), _ptr(s_labels), H, W, _ptr(ws), ws.numel() * ws.element_size(), _ptr(acc),
                                           _ptr(sums_out), _ptr(f_out), _ptr(metric_err(dev)), _stream()), "sgan_rand_f_accumulate")


def vinfo_workspace(H, W, device):
    """The scratch of vinfo_accumulate for H x W maps (the Rand layout and the VInfo sums behind it), cached per (H, W, device)."""
    return _metric_workspace("sgan_vinfo_workspace", H, W, device)


def vinfo_accumulate(t_labels, s_labels, acc, acc_rand=None, parts_out=None, workspace=None):
    """acc[0] += VInfo (the ISBI information score, include/sgan_hip.h) of the labelling s_labels (prediction) against t_labels
    (truth), acc[1] += 1 (sgan_vinfo_accumulate); acc: float64[2] on the device.  acc_rand (float64[2]) receives what
    rand_f_accumulate would add for the same pair, from the same counting pass; parts_out (float64[11], VINFO_PARTS) this pair's
    values."""
    H, W, dev = _label_pair(t_labels, s_labels, "vinfo_accumulate")
    assert acc is not None and _is_acc(acc, torch.float64, 2, dev) and _is_acc(acc_rand, torch.float64, 2, dev)
    assert _is_acc(parts_out, torch.float64, len(VINFO_PARTS), dev)
    ws = vinfo_workspace(H, W, dev) if workspace is None else workspace
    L.check(L.lib().sgan_vinfo_accumulate(_ptr(t_labels), _ptr(s_labels), H, W, _ptr(ws), ws.numel() * ws.element_size(), _ptr(acc),
                                          _ptr(acc_rand), _ptr(parts_out), _ptr(metric_err(dev)), _stream()), "sgan_vinfo_accumulate")


def object_match_workspace(H, W, device):
    """The scratch of object_match_accumulate for H x W maps (a staging block, the pair table and the counters), cached per
    (H, W, device) like vinfo_workspace; the kernels zero it themselves."""
    return _metric_workspace("sgan_object_match_workspace", H, W, device)


def object_match_accumulate(t_labels, s_labels, acc_i, acc_f, min_area=1, counts_out=None, sums_out=None, workspace=None):
    """Adds the object-level match counts (include/sgan_hip.h, "object-level scores") of the labelling s_labels (prediction) against
    t_labels (truth) to acc_i (int64[16], OBJECT_COUNTS: TP at IoU > 0.5 .. 0.95, N_t, N_s, images, SEGn) and acc_f (float64[2],
    OBJECT_SUMS: SIoU, SSEG), both on the device and zeroed by the caller once (sgan_object_match_accumulate).  Regions smaller than
    min_area count as absent.  counts_out (int64[16]) and sums_out (float64[2]) receive this pair's contribution alone.  Only
    enqueues; util.object_match_counts is the host yardstick and util.object_scores derives ObjF1, ObjAP, SEG and PQ."""
    H, W, dev = _label_pair(t_labels, s_labels, "object_match_accumulate")
    assert acc_i is not None and acc_f is not None
    assert all(_is_acc(a, torch.int64, len(OBJECT_COUNTS), dev) for a in (acc_i, counts_out))
    assert all(_is_acc(a, torch.float64, len(OBJECT_SUMS), dev) for a in (acc_f, sums_out))
    ws = object_match_workspace(H, W, dev) if workspace is None else workspace
    L.check(L.lib().sgan_object_match_accumulate(_ptr(t_labels), _ptr(s_labels), H, W, int(min_area), _ptr(ws),
                                                 ws.numel() * ws.element_size(), _ptr(acc_i), _ptr(acc_f), _ptr(counts_out),
                                                 _ptr(sums_out), _ptr(metric_err(dev)), _stream()), "sgan_object_match_accumulate")


def edt_workspace(H, W, device):
    """The scratch of edt_sq for H x W planes (the wall counter, the column masks and the g^2 plane), cached per (H, W, device) like
    thin_workspace; the kernels initialise what they use."""
    return _metric_workspace("sgan_edt_workspace", H, W, device)


def edt_sq(plane, out=None, workspace=None):
    """The exact squared Euclidean distance transform of the pixels of `plane` [H, W] that are > 0.5 (sgan_edt_sq; util.edt_sq is the
    host yardstick): int32 [H, W], the smallest dy^2 + dx^2 to a wall pixel, 0 on the wall, -1 everywhere when there is no wall.
    Only enqueues -- the launch sequence depends on the shape alone -- and reads `plane` in place when its rows are W pixel strides
    apart."""
    plane = _plane(plane, "edt_sq")
    H, W = plane.shape
    dev = plane.device
    if out is None:
        out = torch.empty((H, W), dtype=torch.int32, device=dev)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.numel() == H * W and out.device == dev
    ws = edt_workspace(H, W, dev) if workspace is None else workspace
    L.check(L.lib().sgan_edt_sq(_ptr(plane), plane.stride(1), H, W, _ptr(out), _ptr(ws), ws.numel() * ws.element_size(),
                                _ptr(metric_err(dev)), _stream()), "sgan_edt_sq")
    return out


def boundary_workspace(H, W, device):
    """The scratch of boundary_accumulate for H x W maps (one slot of partial counts per workgroup), cached per (H, W, device)."""
    return _metric_workspace("sgan_boundary_workspace", H, W, device)


def boundary_accumulate(t_dsq, s_dsq, acc_i, acc_f, counts_out=None, sums_out=None, workspace=None):
    """Adds the boundary counts (include/sgan_hip.h, "boundary scores") of the prediction against the truth, given as their edt_sq
    planes s_dsq and t_dsq, to acc_i (int64[80], BOUNDARY_COUNTS: the two histograms of wall pixels by distance bin, N_s, N_t, images,
    images with both walls, pixels with a defined distance, the two largest distance^2) and acc_f (float64[4], BOUNDARY_SUMS), both
    on the device and zeroed by the caller once (sgan_boundary_accumulate).  counts_out (int64[80]) and sums_out (float64[4]) receive
    this pair's contribution alone.  Only enqueues; util.boundary_counts is the host yardstick and util.boundary_scores derives
    BoundF, HausD and ASSD."""
    H, W, dev = _label_pair(t_dsq, s_dsq, "boundary_accumulate")
    assert acc_i is not None and acc_f is not None
    assert all(_is_acc(a, torch.int64, len(BOUNDARY_COUNTS), dev) for a in (acc_i, counts_out))
    assert all(_is_acc(a, torch.float64, len(BOUNDARY_SUMS), dev) for a in (acc_f, sums_out))
    ws = boundary_workspace(H, W, dev) if workspace is None else workspace
    L.check(L.lib().sgan_boundary_accumulate(_ptr(t_dsq), _ptr(s_dsq), H, W, _ptr(ws), ws.numel() * ws.element_size(), _ptr(acc_i),
                                             _ptr(acc_f), _ptr(counts_out), _ptr(sums_out), _ptr(metric_err(dev)), _stream()),
            "sgan_boundary_accumulate")


_topo_ws = {}         # (H, W, window, stride, device index) -> the int64 scratch of topo_accumulate


def topo_workspace(H, W, window, stride, device):
    """The scratch of topo_accumulate for H x W maps (the two Betti numbers of every window of both maps), cached per
    (H, W, window, stride, device); the kernels initialise what they use."""
    key = (H, W, int(window), int(stride), device.index)
    ws = _topo_ws.get(key)
    if ws is None:
        nbytes = L.lib().sgan_topo_workspace_bytes(H, W, int(window), int(stride))
        if nbytes < 0:
            raise L.SganError(f"sgan_topo_workspace_bytes({H}, {W}, {window}, {stride}): {L.lib().sgan_last_error().decode()}")
        ws = _topo_ws[key] = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=device)
    return ws


def topo_accumulate(t, s, acc_i, t_thin=None, s_thin=None, window=64, stride=None, counts_out=None, workspace=None):
    """Adds the topology counts (include/sgan_hip.h, "topology scores") of the predicted plane s against the truth t, both [H, W]
    float32 with wall where > 0.5, to acc_i (int64[12], TOPO_COUNTS) on the device, zeroed by the caller once
    (sgan_topo_accumulate): over the windows of `window` pixels every `stride` (None: window) the numbers of 8-connected wall
    components and of enclosed 4-connected free components of either map and the absolute differences between the maps; with
    t_thin / s_thin (thin's outputs of t / s, dense) the skeleton pixels of clDice.  A side whose thinned plane is None leaves its
    two counters alone.  counts_out (int64[12]) receives this pair's contribution alone.  Only enqueues -- the launch sequence
    depends on (H, W, window, stride) and on which thinned planes are given alone -- and reads t and s in place when their rows
    are W pixel strides apart.  util.topo_counts is the host yardstick and util.topo_scores derives Betti0Err, Betti1Err and
    clDice.  A window outside 8 .. 64 or a stride outside 1 .. window is not covered."""
    t, s = _plane(t, "topo_accumulate"), _plane(s, "topo_accumulate")
    H, W = t.shape
    dev = t.device
    stride = window if stride is None else stride
    assert tuple(s.shape) == (H, W) and s.device == dev, (s.shape, t.shape)
    for thin_plane in (t_thin, s_thin):
        assert thin_plane is None or (thin_plane.dtype == torch.float32 and thin_plane.is_contiguous() and tuple(thin_plane.shape) == (H, W)
                                      and thin_plane.device == dev), (thin_plane.shape, thin_plane.dtype)
    assert acc_i is not None and all(_is_acc(a, torch.int64, len(TOPO_COUNTS), dev) for a in (acc_i, counts_out))
    if not (8 <= int(window) <= 64 and 1 <= int(stride) <= int(window)):
        raise L.SganError(f"sgan_topo_accumulate: not covered (window {window}: 8 .. 64, stride {stride}: 1 .. window); nothing was launched")
    ws = topo_workspace(H, W, window, stride, dev) if workspace is None else workspace
    rc = L.lib().sgan_topo_accumulate(_ptr(t), t.stride(1), _ptr(s), s.stride(1), _ptr(t_thin), _ptr(s_thin), H, W, int(window), int(stride),
                                      _ptr(ws), ws.numel() * ws.element_size(), _ptr(acc_i), _ptr(counts_out), _ptr(metric_err(dev)), _stream())
    if rc == 1:
        raise L.SganError(f"sgan_topo_accumulate: {L.lib().sgan_last_error().decode()}; nothing was launched")
    L.check(rc, "sgan_topo_accumulate")


# ---- soft-clDice (sgan_cldice.hip; include/sgan_hip.h, "soft-clDice"): the loss whose hard form topo_accumulate scores ---------------
CLDICE_MAX_ITERS = L.DEFINES["SGAN_CLDICE_MAX_ITERS"]
CLDICE_STATE_BYTES = L.DEFINES["SGAN_CLDICE_STATE_BYTES"]
CLDICE_STATE = ('A', 'B', 'C', 'D', 'L', 'gA', 'gB', 'gC')      # the first doubles of the state sgan_cldice_finish writes
_cldice_ws = {}                # (H, W, iters, backward, device index) -> the float32 scratch


def _strided_plane(t, what):
    """A [H, W] fp32 view with positive strides whose rows do not overlap (a channel of an NHWC buffer, a window of a wider map, a
    dense map), inside its storage: (tensor, row stride, pixel stride).  Anything else is made contiguous."""
    require_gpu(t, what)
    assert t.dim() == 2 and t.dtype == torch.float32, (t.shape, t.dtype)
    H, W = t.shape
    if t.stride(1) < 1 or (H > 1 and t.stride(0) < (W - 1) * t.stride(1) + 1):
        t = t.contiguous()
    if (H - 1) * t.stride(0) + (W - 1) * t.stride(1) + 1 > _avail(t):
        raise L.SganError(f"{what}: plane {tuple(t.shape)} / {tuple(t.stride())} does not lie inside its storage; nothing was launched")
    return t, (t.stride(0) if H > 1 else W * t.stride(1)), t.stride(1)


def _dense_plane(t, H, W, dev):
    return t.dtype == torch.float32 and t.is_contiguous() and t.numel() == H * W and t.device == dev


def _cldice_refused(what, iters):
    if not 1 <= int(iters) <= CLDICE_MAX_ITERS:
        raise L.SganError(f"{what}: not covered ({iters} iterations: 1 .. {CLDICE_MAX_ITERS}); nothing was launched")


def cldice_workspace(H, W, iters, device, backward=False):
    """The scratch of soft_skeleton for H x W planes and K = iters (the K + 2 planes I_j) and, with backward, of cldice_backward
    (K + 3 planes more), cached per (H, W, iters, backward, device); the kernels initialise what they use.  A caller that keeps
    the I_j for a backward owns a workspace of its own (losses.soft_cldice does)."""
    key = (H, W, int(iters), bool(backward), device.index)
    ws = _cldice_ws.get(key)
    if ws is None:
        ws = _cldice_ws[key] = new_cldice_workspace(H, W, iters, device, backward)
    return ws


def new_cldice_workspace(H, W, iters, device, backward=False):
    nbytes = L.lib().sgan_cldice_workspace_bytes(H, W, int(iters), int(bool(backward)))
    if nbytes < 0:
        raise L.SganError(f"sgan_cldice_workspace_bytes({H}, {W}, {iters}): {L.lib().sgan_last_error().decode()}")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


def new_cldice_state(device):
    """The zeroed state of cldice_finish (sums, loss, scalar derivatives, slots and ticket): one per loss node, so that a backward
    reads the scalars of its own forward."""
    return torch.zeros(CLDICE_STATE_BYTES // 8, dtype=torch.float64, device=device)


def soft_skeleton(x, iters, out=None, work=None):
    """The soft skeleton S_K of the plane x [H, W] float32 in [0, 1] with K = iters (sgan_soft_skeleton; util.soft_skeleton_ref is
    the host yardstick): iterated plus-shaped min and 3 x 3 max selections, float32 [H, W].  `work` (cldice_workspace) receives the
    K + 2 planes I_j, bits of x, which cldice_backward reads.  Only enqueues -- K + 2 launches whose grids depend on the shape
    alone -- and reads x in place where its strides are positive (a channel of an NHWC buffer, a window of a wider map)."""
    _cldice_refused("sgan_soft_skeleton", iters)
    x, rs, ps = _strided_plane(x, "soft_skeleton")
    H, W = x.shape
    dev = x.device
    if out is None:
        out = torch.empty((H, W), dtype=torch.float32, device=dev)
    assert _dense_plane(out, H, W, dev), (out.shape, out.dtype)
    ws = cldice_workspace(H, W, iters, dev) if work is None else work
    rc = L.lib().sgan_soft_skeleton(_ptr(x), rs, ps, H, W, int(iters), _ptr(out), _ptr(ws), ws.numel() * ws.element_size(), _stream())
    if rc == 1:
        raise L.SganError(f"sgan_soft_skeleton: {L.lib().sgan_last_error().decode()}; nothing was launched")
    L.check(rc, "sgan_soft_skeleton")
    return out


def cldice_finish(sp, t, st, p, state, loss_out):
    """The four sums, L and the scalar derivatives of soft-clDice from sp = S(P), st = S(T) (dense) and the planes t, p (strided)
    into `state` (new_cldice_state; CLDICE_STATE names its first doubles) and loss_out (a float32 device scalar):
    sgan_cldice_finish, one launch, nothing read back."""
    t, t_rs, t_ps = _strided_plane(t, "cldice_finish")
    p, p_rs, p_ps = _strided_plane(p, "cldice_finish")
    H, W = t.shape
    dev = t.device
    assert tuple(p.shape) == (H, W) and p.device == dev and _dense_plane(sp, H, W, dev) and _dense_plane(st, H, W, dev)
    assert state.dtype == torch.float64 and state.is_contiguous() and state.numel() * 8 >= CLDICE_STATE_BYTES and state.device == dev
    assert loss_out.dtype == torch.float32 and loss_out.numel() == 1 and loss_out.device == dev
    rc = L.lib().sgan_cldice_finish(_ptr(sp), _ptr(t), t_rs, t_ps, _ptr(st), _ptr(p), p_rs, p_ps, H, W, _ptr(state), _ptr(loss_out), _stream())
    if rc == 1:
        raise L.SganError(f"sgan_cldice_finish: {L.lib().sgan_last_error().decode()}; nothing was launched")
    L.check(rc, "sgan_cldice_finish")
    return loss_out


def cldice_backward(t, st, state, iters, work, dp=None, gout=None):
    """dp [H, W] = gout * d L / d P of soft-clDice (sgan_cldice_backward) from the planes I_j soft_skeleton(P, work=work) left in
    `work` (cldice_workspace(..., backward=True)), the truth t, its skeleton st and the state of cldice_finish; gout: a float32
    device scalar, None = 1.  K + 3 launches, gathers only: the same bits on every run."""
    _cldice_refused("sgan_cldice_backward", iters)
    t, t_rs, t_ps = _strided_plane(t, "cldice_backward")
    H, W = t.shape
    dev = t.device
    if dp is None:
        dp = torch.empty((H, W), dtype=torch.float32, device=dev)
    assert _dense_plane(dp, H, W, dev) and _dense_plane(st, H, W, dev)
    assert state.dtype == torch.float64 and state.numel() * 8 >= CLDICE_STATE_BYTES and state.device == dev
    assert gout is None or (gout.dtype == torch.float32 and gout.numel() == 1 and gout.device == dev)
    rc = L.lib().sgan_cldice_backward(_ptr(t), t_rs, t_ps, _ptr(st), _ptr(state), _ptr(gout), H, W, int(iters), _ptr(dp), _ptr(work),
                                      work.numel() * work.element_size(), _stream())
    if rc == 1:
        raise L.SganError(f"sgan_cldice_backward: {L.lib().sgan_last_error().decode()}; nothing was launched")
    L.check(rc, "sgan_cldice_backward")
    return dp


# ---- Lovasz-softmax (sgan_lovasz.hip; include/sgan_hip.h, "Lovasz-softmax") ------------------------------------------------------------
LOVASZ_MAX_CLASSES = L.DEFINES["SGAN_LOVASZ_MAX_CLASSES"]
LOVASZ_MAX_PIXELS = L.DEFINES["SGAN_LOVASZ_MAX_PIXELS"]
LOVASZ_STATE_BYTES = L.DEFINES["SGAN_LOVASZ_STATE_BYTES"]
LOVASZ_STATE = {'L': 0, 'm': 1, 'Lc': 2, 'scale': 10}      # doubles of the state; the int32 G of the listed classes at byte 192


def _lovasz_refused(what, H, W, n):
    if H < 1 or W < 1 or H * W > LOVASZ_MAX_PIXELS or not 1 <= n <= LOVASZ_MAX_CLASSES:
        raise L.SganError(f"{what}: not covered ({H} x {W} pixels, {n} classes: H, W >= 1, H W <= 2^20, 1 .. {LOVASZ_MAX_CLASSES} classes); "
                          "nothing was launched")


def lovasz_layout(H, W, n):
    """Byte offsets of the regions of the Lovasz workspace for H x W pixels and n classes, as the header states them:
    {'state', 'g', 'keys', 'slots', 'perm', 'bsum', 'bytes', 'P', 'nb'}."""
    _lovasz_refused("lovasz_layout", H, W, n)
    N = H * W
    P = 4096
    while P < N:
        P *= 2
    nb = (N + 1023) // 1024
    off, out = 0, {'P': P, 'nb': nb}
    for name, size in (('state', LOVASZ_STATE_BYTES), ('g', 8 * n * N), ('keys', 8 * n * P), ('slots', 8 * n * nb), ('perm', 4 * n * N),
                       ('bsum', 4 * n * nb)):
        out[name] = off
        off += size
    out['bytes'] = (off + 7) & ~7
    return out


def new_lovasz_workspace(H, W, n, device):
    """The scratch of lovasz_forward / lovasz_backward for H x W pixels and n listed classes, as float64 (8-byte aligned); it may
    hold anything: the kernels write what they read.  A node that keeps pi and g for its backward owns one."""
    _lovasz_refused("sgan_lovasz_workspace_bytes", H, W, int(n))
    nbytes = L.lib().sgan_lovasz_workspace_bytes(H, W, int(n))
    if nbytes < 0:
        raise L.SganError(f"sgan_lovasz_workspace_bytes({H}, {W}, {n}): {L.lib().sgan_last_error().decode()}")
    assert nbytes == lovasz_layout(H, W, int(n))['bytes'], (nbytes, lovasz_layout(H, W, int(n)))
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device)


def lovasz_views(work, H, W, n):
    """(pi int32 [n, N], g float64 [n, N], state float64 [32], G int32 [8]) as views of a Lovasz workspace."""
    lay, N = lovasz_layout(H, W, n), H * W
    perm = work.view(torch.int32)[lay['perm'] // 4:lay['perm'] // 4 + n * N].view(n, N)
    g = work[lay['g'] // 8:lay['g'] // 8 + n * N].view(n, N)
    state = work[:LOVASZ_STATE_BYTES // 8]
    return perm, g, state, state.view(torch.int32)[48:56]


def _lovasz_prediction(p, what):
    """[C, H, W] fp32 view of the prediction with positive strides and rows that do not overlap, inside its storage."""
    require_gpu(p, what)
    if p.dim() == 4:
        assert p.shape[0] == 1, p.shape
        p = p[0]
    assert p.dim() == 3 and p.dtype == torch.float32, (p.shape, p.dtype)
    nch, H, W = p.shape
    if min(p.stride()) < 1 or (H > 1 and p.stride(1) < (W - 1) * p.stride(2) + 1):
        p = p.contiguous()
    if (nch - 1) * p.stride(0) + (H - 1) * p.stride(1) + (W - 1) * p.stride(2) + 1 > _avail(p):
        raise L.SganError(f"{what}: prediction {tuple(p.shape)} / {tuple(p.stride())} does not lie inside its storage; nothing was launched")
    return p


def _lovasz_classes(classes, nch, what):
    classes = [int(c) for c in classes]
    if len(set(classes)) != len(classes) or any(not 0 <= c < nch for c in classes):
        raise L.SganError(f"{what}: classes {classes}: distinct indices below C = {nch} are needed; nothing was launched")
    return (C.c_int32 * max(len(classes), 1))(*classes)


def lovasz_forward(p, label, classes, work, loss_out=None):
    """The Lovasz-softmax loss of the prediction p [1, C, H, W] or [C, H, W] (fp32, read where it lies: NCHW, a window, the channels
    of an NHWC-backed tensor) against the index label [H, W] (int64) over the listed classes: a float32 device scalar
    (sgan_lovasz_forward; util.lovasz_ref is the host yardstick).  `work` (new_lovasz_workspace) keeps pi, g and the scales for
    lovasz_backward.  Only enqueues; the launches depend on (H, W, n) alone."""
    classes = list(classes)
    p = _lovasz_prediction(p, "lovasz_forward")
    nch, H, W = p.shape
    _lovasz_refused("sgan_lovasz_forward", H, W, len(classes))
    arr = _lovasz_classes(classes, nch, "sgan_lovasz_forward")
    dev = p.device
    require_gpu(label, "lovasz_forward")
    assert label.dtype == torch.int64 and label.numel() == H * W and label.device == dev, (label.shape, label.dtype)
    label = label.contiguous()
    if loss_out is None:
        loss_out = torch.empty((), dtype=torch.float32, device=dev)
    assert loss_out.dtype == torch.float32 and loss_out.numel() == 1 and loss_out.device == dev
    assert work.is_contiguous() and work.device == dev
    rc = L.lib().sgan_lovasz_forward(_ptr(p), p.stride(0), p.stride(1) if H > 1 else W * p.stride(2), p.stride(2), _ptr(label), arr, len(classes),
                                     nch, H, W, _ptr(loss_out), _ptr(work), work.numel() * work.element_size(), _stream())
    if rc == 1:
        raise L.SganError(f"sgan_lovasz_forward: {L.lib().sgan_last_error().decode()}; nothing was launched")
    L.check(rc, "sgan_lovasz_forward")
    return loss_out


def lovasz_backward(p, classes, work, dp=None, gout=None):
    """dp [1, C, H, W] (dense) = gout * d L / d p of Lovasz-softmax from the workspace lovasz_forward(p, ..., work) left and the same
    p: listed planes scattered through pi, every other plane zero (sgan_lovasz_backward, one launch); gout: a float32 device scalar,
    None = 1."""
    classes = list(classes)
    p = _lovasz_prediction(p, "lovasz_backward")
    nch, H, W = p.shape
    _lovasz_refused("sgan_lovasz_backward", H, W, len(classes))
    arr = _lovasz_classes(classes, nch, "sgan_lovasz_backward")
    dev = p.device
    if dp is None:
        dp = torch.empty((1, nch, H, W), dtype=torch.float32, device=dev)
    assert dp.dtype == torch.float32 and dp.is_contiguous() and dp.numel() == nch * H * W and dp.device == dev, (dp.shape, dp.dtype)
    assert gout is None or (gout.dtype == torch.float32 and gout.numel() == 1 and gout.device == dev)
    assert work.is_contiguous() and work.device == dev
    rc = L.lib().sgan_lovasz_backward(_ptr(p), p.stride(0), p.stride(1) if H > 1 else W * p.stride(2), p.stride(2), arr, len(classes), nch, H, W,
                                      _ptr(gout), _ptr(dp), _ptr(work), work.numel() * work.element_size(), _stream())
    if rc == 1:
        raise L.SganError(f"sgan_lovasz_backward: {L.lib().sgan_last_error().decode()}; nothing was launched")
    L.check(rc, "sgan_lovasz_backward")
    return dp


# ---- Tversky / focal loss terms on the logits (sgan_segterms.hip; include/sgan_hip.h, "Segmentation loss terms") --------------------------
SEGTERMS_MAX_CLASSES = L.DEFINES["SGAN_SEGTERMS_MAX_CLASSES"]
SEGTERMS_STATE_BYTES = L.DEFINES["SGAN_SEGTERMS_STATE_BYTES"]
SEGTERMS_WS_BYTES = L.DEFINES["SGAN_SEGTERMS_WS_BYTES"]
SEGTERMS_STATE = {'class': 0, 'focal_num': 64, 'focal_norm': 65, 'L_T': 66, 'L_F': 67}      # doubles; per class 8: TP FP FN D TI L_c G(0) G(1)


def new_seg_terms_state(device):
    """The fp64 state seg_terms_forward writes and seg_terms_backward reads (68 doubles, SEGTERMS_STATE)."""
    return torch.zeros(SEGTERMS_STATE_BYTES // 8, dtype=torch.float64, device=device)


def new_seg_terms_workspace(device):
    """The slots and ticket of seg_terms_forward: zero on first use, left zeroed by every call; one per node and stream."""
    return torch.zeros(SEGTERMS_WS_BYTES // 8, dtype=torch.float64, device=device)


def _seg_terms_args(what, z, Creal, mode, label_or_target, classes, focal_gamma, class_w, state):
    """The operand checks both calls share: every tensor against its storage, before anything is launched.  Returns
    (label_or_target, tld, classes array, n, focal, gamma, nw)."""
    require_gpu(z, what)
    H, W, _ = z.shape
    dev = z.device

    def rows_fit(t, name, written):
        _act(t)
        row = t.stride(1) if (written or t.stride(1) in (4, 8, 12, 16)) else Creal
        if (t.device != dev or t.shape[0] * t.shape[1] != H * W or t.shape[2] < Creal or t.stride(1) < Creal
                or (H * W - 1) * t.stride(1) + row > _avail(t)):
            raise L.SganError(f"{what} {name}: tensor {tuple(t.shape)} (pixel stride {t.stride(1)}, {_avail(t)} elements of storage) does "
                              f"not hold {H}x{W} rows of {row}; nothing was launched")

    rows_fit(z, "logits", False)
    tld = 0
    if mode == SEGHEAD_SOFTMAX:
        assert (label_or_target.dtype == torch.int64 and label_or_target.device == dev and label_or_target.is_contiguous()
                and label_or_target.numel() == H * W), (label_or_target.shape, label_or_target.dtype)
    else:
        rows_fit(label_or_target, "target", False)
        tld = label_or_target.stride(1)
    classes = [int(c) for c in classes]
    n = len(classes)
    focal = focal_gamma is not None
    nw = 0 if class_w is None else int(class_w.numel())
    assert class_w is None or (class_w.dtype == torch.float32 and class_w.device == dev and class_w.is_contiguous())
    if focal and class_w is not None and mode == SEGHEAD_SOFTMAX and nw < Creal:
        raise L.SganError(f"{what}: {nw} class weights for {Creal} classes; nothing was launched")
    assert state.dtype == torch.float64 and state.is_contiguous() and state.numel() >= SEGTERMS_STATE_BYTES // 8 and state.device == dev
    arr = (C.c_int32 * max(n, 1))(*classes)
    return rows_fit, tld, arr, n, int(focal), float(focal_gamma) if focal else 0.0, min(nw, Creal)


def seg_terms_forward(z, Creal, mode, label_or_target, classes, alpha, beta, smooth, power, focal_gamma, class_w, state, loss_t, loss_f,
                      work):
    """sgan_seg_terms_forward on an [H, W, Cs] logits buffer: the Tversky term over `classes` (empty: off) and the focal term
    (focal_gamma None: off) into `state` (new_seg_terms_state) and the float32 device scalars loss_t, loss_f; `label_or_target` as
    seg_head takes it; `work`: new_seg_terms_workspace.  One launch, only enqueued.  Not covered (SganError, nothing launched):
    more than 16 channels, more than 8 or repeated or out-of-range classes, both terms off, parameters out of range."""
    what = "seg_terms_forward"
    _, tld, arr, n, focal, gamma, nw = _seg_terms_args(what, z, Creal, mode, label_or_target, classes, focal_gamma, class_w, state)
    H, W, _ = z.shape
    for t in (loss_t, loss_f):
        assert t.dtype == torch.float32 and t.numel() == 1 and t.device == z.device
    assert work.dtype == torch.float64 and work.is_contiguous() and work.numel() * 8 >= SEGTERMS_WS_BYTES and work.device == z.device
    rc = L.lib().sgan_seg_terms_forward(_ptr(z), z.stride(1), H * W, int(Creal), int(mode), _ptr(label_or_target), tld, arr, n, float(alpha),
                                        float(beta), float(smooth), float(power), focal, gamma, _ptr(class_w), nw, _ptr(state), _ptr(loss_t),
                                        _ptr(loss_f), _ptr(work), _stream())
    if rc == 1:
        raise L.SganError(f"sgan_seg_terms_forward: {L.lib().sgan_last_error().decode()}; nothing was launched")
    L.check(rc, "sgan_seg_terms_forward")


def seg_terms_backward(z, Creal, mode, label_or_target, classes, focal_gamma, class_w, state, gout_t, gout_f, dz):
    """dz [H, W, Cs'] = gout_t * dL_T/dz + gout_f * dL_F/dz from the state seg_terms_forward left and the same logits and label
    (sgan_seg_terms_backward, one launch).  gout_t / gout_f: float32 device scalars, None = that term is not taken (its part of dz
    is exactly zero); the padding channels of dz are written as zeros."""
    what = "seg_terms_backward"
    rows_fit, tld, arr, n, focal, gamma, nw = _seg_terms_args(what, z, Creal, mode, label_or_target, classes, focal_gamma, class_w, state)
    H, W, _ = z.shape
    rows_fit(dz, "dlogits", True)
    for g in (gout_t, gout_f):
        assert g is None or (g.dtype == torch.float32 and g.numel() == 1 and g.device == z.device)
    rc = L.lib().sgan_seg_terms_backward(_ptr(z), z.stride(1), H * W, int(Creal), int(mode), _ptr(label_or_target), tld, arr, n, focal, gamma,
                                         _ptr(class_w), nw, _ptr(state), _ptr(gout_t), _ptr(gout_f), _ptr(dz), dz.stride(1), _stream())
    if rc == 1:
        raise L.SganError(f"sgan_seg_terms_backward: {L.lib().sgan_last_error().decode()}; nothing was launched")
    L.check(rc, "sgan_seg_terms_backward")
    return dz


# ---- distance-map loss terms on the logits (sgan_distloss.hip; include/sgan_hip.h, "Distance-map loss terms") ------------------------------
DISTLOSS_STATE_BYTES = L.DEFINES["SGAN_DISTLOSS_STATE_BYTES"]
DISTLOSS_WS_BYTES = L.DEFINES["SGAN_DISTLOSS_WS_BYTES"]
DISTLOSS_STATE = {'sum_B': 0, 'sum_H': 1, 'N': 2, 'L_B': 3, 'L_H': 4}      # doubles


def signed_edt_workspace(H, W, device):
    """The scratch of signed_edt_sq for H x W planes (edt_sq's workspace, the complement plane and the second transform), cached per
    (H, W, device) like edt_workspace; the kernels initialise what they use."""
    return _metric_workspace("sgan_signed_edt_workspace", H, W, device)


def signed_edt_sq(plane, out=None, workspace=None):
    """The signed squared Euclidean distance map of the pixels of `plane` [H, W] that are > 0.5 (sgan_signed_edt_sq;
    util.signed_edt_sq is the host yardstick): int32 [H, W], +(dy^2 + dx^2 to the nearest inside pixel) outside, -(dy^2 + dx^2 to the
    nearest outside pixel) inside, 0 everywhere when the plane is empty or full.  Only enqueues -- the launch sequence depends on the
    shape alone -- and reads `plane` in place when its rows are W pixel strides apart."""
    plane = _plane(plane, "signed_edt_sq")
    H, W = plane.shape
    dev = plane.device
    if out is None:
        out = torch.empty((H, W), dtype=torch.int32, device=dev)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.numel() == H * W and out.device == dev
    ws = signed_edt_workspace(H, W, dev) if workspace is None else workspace
    L.check(L.lib().sgan_signed_edt_sq(_ptr(plane), plane.stride(1), H, W, _ptr(out), _ptr(ws), ws.numel() * ws.element_size(),
                                       _ptr(metric_err(dev)), _stream()), "sgan_signed_edt_sq")
    return out


def new_dist_loss_state(device):
    """The fp64 state dist_loss_forward writes (8 doubles, DISTLOSS_STATE)."""
    return torch.zeros(DISTLOSS_STATE_BYTES // 8, dtype=torch.float64, device=device)


def new_dist_loss_workspace(device):
    """The slots and ticket of dist_loss_forward: zero on first use, left zeroed by every call; one per node and stream."""
    return torch.zeros(DISTLOSS_WS_BYTES // 8, dtype=torch.float64, device=device)


def _dist_loss_args(what, z, Creal, mode, label_or_target, t_sdsq, p_sdsq, hausdorff_alpha):
    """The operand checks both calls share: every tensor against its storage, before anything is launched.  Returns
    (rows_fit, tld, hausdorff, alpha)."""
    require_gpu(z, what)
    H, W, _ = z.shape
    dev = z.device

    def rows_fit(t, name, written):
        _act(t)
        row = t.stride(1) if (written or t.stride(1) in (4, 8, 12, 16)) else Creal
        if (t.device != dev or t.shape[0] * t.shape[1] != H * W or t.shape[2] < Creal or t.stride(1) < Creal
                or (H * W - 1) * t.stride(1) + row > _avail(t)):
            raise L.SganError(f"{what} {name}: tensor {tuple(t.shape)} (pixel stride {t.stride(1)}, {_avail(t)} elements of storage) does "
                              f"not hold {H}x{W} rows of {row}; nothing was launched")

    rows_fit(z, "logits", False)
    tld = 0
    if mode == SEGHEAD_SOFTMAX:
        assert (label_or_target.dtype == torch.int64 and label_or_target.device == dev and label_or_target.is_contiguous()
                and label_or_target.numel() == H * W), (label_or_target.shape, label_or_target.dtype)
    else:
        rows_fit(label_or_target, "target", False)
        tld = label_or_target.stride(1)
    hausdorff = hausdorff_alpha is not None
    for m, name in ((t_sdsq, "t_sdsq"), (p_sdsq, "p_sdsq")):
        if m is None and name == "p_sdsq" and not hausdorff:
            continue
        if m is None:
            raise L.SganError(f"{what}: {name} is required; nothing was launched")
        assert m.dtype == torch.int32 and m.is_contiguous() and m.numel() == H * W and m.device == dev, (name, m.shape, m.dtype)
    return rows_fit, tld, int(hausdorff), float(hausdorff_alpha) if hausdorff else 2.0


def dist_loss_forward(z, Creal, mode, label_or_target, cls, t_sdsq, p_sdsq, boundary, hausdorff_alpha, state, loss_b, loss_h, work):
    """sgan_dist_loss_forward on an [H, W, Cs] logits buffer: the boundary term (`boundary` False: off) and the Hausdorff term with
    exponent hausdorff_alpha (None: off) of class `cls` against the signed maps t_sdsq / p_sdsq (int32 [H, W], signed_edt_sq; p_sdsq
    None with the Hausdorff term off) into `state` (new_dist_loss_state) and the float32 device scalars loss_b, loss_h;
    `label_or_target` as seg_head takes it; `work`: new_dist_loss_workspace.  One launch, only enqueued.  Not covered (SganError,
    nothing launched): more than 16 channels, a class out of range, both terms off, alpha outside (0, 4]."""
    what = "dist_loss_forward"
    _, tld, hausdorff, alpha = _dist_loss_args(what, z, Creal, mode, label_or_target, t_sdsq, p_sdsq, hausdorff_alpha)
    H, W, _ = z.shape
    for t in (loss_b, loss_h):
        assert t.dtype == torch.float32 and t.numel() == 1 and t.device == z.device
    assert state.dtype == torch.float64 and state.is_contiguous() and state.numel() * 8 >= DISTLOSS_STATE_BYTES and state.device == z.device
    assert work.dtype == torch.float64 and work.is_contiguous() and work.numel() * 8 >= DISTLOSS_WS_BYTES and work.device == z.device
    rc = L.lib().sgan_dist_loss_forward(_ptr(z), z.stride(1), H * W, int(Creal), int(mode), _ptr(label_or_target), tld, int(cls), _ptr(t_sdsq),
                                        _ptr(p_sdsq) if hausdorff else _ptr(None), int(bool(boundary)), hausdorff, alpha, _ptr(state),
                                        _ptr(loss_b), _ptr(loss_h), _ptr(work), _stream())
    if rc == 1:
        raise L.SganError(f"sgan_dist_loss_forward: {L.lib().sgan_last_error().decode()}; nothing was launched")
    L.check(rc, "sgan_dist_loss_forward")


def dist_loss_backward(z, Creal, mode, label_or_target, cls, t_sdsq, p_sdsq, boundary, hausdorff_alpha, gout_b, gout_h, dz):
    """dz [H, W, Cs'] = gout_b * dL_B/dz + gout_h * dL_H/dz from the same logits, label and maps as dist_loss_forward
    (sgan_dist_loss_backward, one launch).  gout_b / gout_h: float32 device scalars, None = that term is not taken (its part of dz is
    exactly zero); the padding channels of dz are written as zeros."""
    what = "dist_loss_backward"
    rows_fit, tld, hausdorff, alpha = _dist_loss_args(what, z, Creal, mode, label_or_target, t_sdsq, p_sdsq, hausdorff_alpha)
    H, W, _ = z.shape
    rows_fit(dz, "dlogits", True)
    for g in (gout_b, gout_h):
        assert g is None or (g.dtype == torch.float32 and g.numel() == 1 and g.device == z.device)
    rc = L.lib().sgan_dist_loss_backward(_ptr(z), z.stride(1), H * W, int(Creal), int(mode), _ptr(label_or_target), tld, int(cls), _ptr(t_sdsq),
                                         _ptr(p_sdsq) if hausdorff else _ptr(None), int(bool(boundary)), hausdorff, alpha, _ptr(gout_b),
                                         _ptr(gout_h), _ptr(dz), dz.stride(1), _stream())
    if rc == 1:
        raise L.SganError(f"sgan_dist_loss_backward: {L.lib().sgan_last_error().decode()}; nothing was launched")
    L.check(rc, "sgan_dist_loss_backward")
    return dz


def clean_workspace(H, W, device):
    """The scratch of clean_wall for H x W planes (edt_sq's workspace, one int32 plane for dsq / labels, the area table and the
    complement plane), cached per (H, W, device) like edt_workspace; the kernels initialise what they use."""
    return _metric_workspace("sgan_clean_workspace", H, W, device)


def clean_wall(plane, close_rsq=0, min_wall=0, min_cell=0, out=None, acc=None, workspace=None):
    """The cleaned wall map of the pixels of `plane` [H, W] that are > 0.5 (sgan_clean_wall; util.clean_wall is the host yardstick):
    closed with the disk dy^2 + dx^2 <= close_rsq, wall components below min_wall pixels dropped, regions below min_cell pixels
    filled, each stage skipped at 0.  float32 [H, W] of 0.0 / 1.0, which ccl_label, thin and edt_sq read as it lies.  acc (int64[6]
    on the device, CLEAN_COUNTS) is added to.  Only enqueues -- the launch sequence depends on the shape and on which parameters are
    nonzero alone -- and reads `plane` in place when its rows are W pixel strides apart."""
    plane = _plane(plane, "clean_wall")
    H, W = plane.shape
    dev = plane.device
    if out is None:
        out = torch.empty((H, W), dtype=torch.float32, device=dev)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == H * W and out.device == dev
    assert _is_acc(acc, torch.int64, len(CLEAN_COUNTS), dev)
    ws = clean_workspace(H, W, dev) if workspace is None else workspace
    L.check(L.lib().sgan_clean_wall(_ptr(plane), plane.stride(1), H, W, int(close_rsq), int(min_wall), int(min_cell), _ptr(out), _ptr(acc),
                                    _ptr(ws), ws.numel() * ws.element_size(), _ptr(metric_err(dev)), _stream()), "sgan_clean_wall")
    return out


def split_workspace(H, W, device):
    """The scratch of split_cells for H x W planes (edt_sq's workspace, the dsq plane, the core plane, two label planes and the round
    counters), cached per (H, W, device) like clean_workspace; the kernels initialise what they use."""
    return _metric_workspace("sgan_split_workspace", H, W, device)


def split_cells(plane, split_rsq, max_rounds=64, out=None, acc=None, workspace=None):
    """The wall map of the pixels of `plane` [H, W] that are > 0.5 with merged cells cut apart (sgan_split_cells; util.split_cells is
    the host yardstick): the cores of the free space (distance^2 to the wall >= split_rsq) are labelled, flooded back through the
    free pixels for max_rounds synchronous rounds, and a wall pixel is set where two different labels meet.  float32 [H, W] of
    0.0 / 1.0, which ccl_label, thin, edt_sq and clean_wall read as it lies.  acc (int64[6] on the device, SPLIT_COUNTS) is added to.
    A budget that was hit raises SPLIT_BUDGET_BIT of metric_err and acc[4]; the map is then the one for that budget.  Only
    enqueues -- the launch sequence depends on the shape and max_rounds alone -- and reads `plane` in place when its rows are W
    pixel strides apart."""
    plane = _plane(plane, "split_cells")
    H, W = plane.shape
    dev = plane.device
    if out is None:
        out = torch.empty((H, W), dtype=torch.float32, device=dev)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == H * W and out.device == dev
    assert _is_acc(acc, torch.int64, len(SPLIT_COUNTS), dev)
    ws = split_workspace(H, W, dev) if workspace is None else workspace
    L.check(L.lib().sgan_split_cells(_ptr(plane), plane.stride(1), H, W, int(split_rsq), int(max_rounds), _ptr(out), _ptr(acc), _ptr(ws),
                                     ws.numel() * ws.element_size(), _ptr(metric_err(dev)), _stream()), "sgan_split_cells")
    return out


def confusion_accumulate(x, C, conf, label=None, y=None, add_background=False):
    """conf[truth, pred] += 1 per pixel (sgan_confusion_accumulate).  x, y: padded NHWC buffers [H, W, >= C]; pred = argmax of x's C
    channels, truth = `label` (int64 map) or the argmax of y; add_background appends 1 - min(1, sum) as class C to both.
    conf: int64 [k, k] on the device, k = C + add_background.
    Equal to torch.argmax of the same maps; with add_background the fp32 sum is taken in channel order, which is torch's own
    `sum(dim=1)` wherever that sum has one value (C <= 2, or sums that are exact) -- for C >= 3 and arbitrary floats torch's
    reduction order is its own, and a pixel whose background value ties another class to the last bit may then fall differently."""
    H, W, _ = _act(x).shape
    require_gpu(x, "confusion_accumulate")
    k = C + (1 if add_background else 0)
    assert 1 <= C <= 16 and x.shape[2] >= C and (label is None) != (y is None)
    assert conf.dtype == torch.int64 and conf.is_contiguous() and conf.numel() == k * k and conf.device == x.device
    if (H * W - 1) * x.stride(1) + C > _avail(x):
        raise L.SganError("confusion_accumulate: x does not lie inside its storage; nothing was launched")
    if label is not None:
        assert label.dtype == torch.int64 and label.is_contiguous() and label.numel() == H * W and label.device == x.device
    else:
        assert _act(y).shape[:2] == (H, W) and y.shape[2] >= C and y.device == x.device and (H * W - 1) * y.stride(1) + C <= _avail(y)
    L.check(L.lib().sgan_confusion_accumulate(_ptr(x), x.stride(1), C, _ptr(label), _ptr(y), y.stride(1) if y is not None else 0,
                                              int(bool(add_background)), H * W, _ptr(conf), _ptr(metric_err(x.device)), _stream()),
            "sgan_confusion_accumulate")

"""torch.autograd Functions over the C ABI of libsbl_hip.so.

torch is plumbing only here: it owns device memory (caching allocator), the
current HIP stream and the autograd tape; every FLOP of forward and backward runs
in a hand-written HIP kernel reached through sbl_for_multilingual_lip_reading_amd._lib.call().
Nothing in this file falls back to torch math on failure: a missing library or a
non-zero status raises.

All Functions are hipGraph-capturable: no host sync, no host read of device data;
dropout seeds and teacher-forcing coins live in device memory.
"""
import collections as _collections
import contextlib as _contextlib
import copy as _copy
import ctypes as _ct
import functools as _functools
import threading as _threading
import types as _types
import weakref as _weakref

import numpy as _np
import torch
import torch.distributed as _dist

try:
    from . import _lib
except ImportError:      # drop-in mode: this directory itself is on sys.path
    import _lib

call = _lib.call

_PRECISIONS = {"f32": 0, "bf16x6": 6, "bf16x3": 3, "bf16": 1}


def set_matmul_precision(mode):
    """Arithmetic of every dense GEMM / trunk convolution (include/sbl_hip.h, sbl_set_matmul_precision), process-wide:
    "f32" exact fp32 MFMA; "bf16x6" exact three-way bf16 split, six bf16 MFMA products, fp32 accumulation (fp32-grade
    results, the default of bench.py); "bf16x3" two planes / three products; "bf16" plain bf16 inputs (BASELINE config 5)."""
    if mode not in _PRECISIONS:
        raise ValueError("matmul precision %r (one of %s)" % (mode, ", ".join(_PRECISIONS)))
    call("sbl_set_matmul_precision", _PRECISIONS[mode])


def get_matmul_precision():
    v = _lib.load().sbl_get_matmul_precision()
    return [k for k, t in _PRECISIONS.items() if t == v][0]


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


# What this module keeps per GPU, one record per device index (nn.DataParallel drives one replica per device, each from its
# own thread): `dropout` (DropoutState), `side` / `main` (the second HIP stream and the one it forks from / joins to),
# `zero_buf` / `zero_off` (the zero pool), `collectors` / `collectors_pass` (what flush_deferred() issues), and as the
# key of _first_in_pass the pass whose end-of-backward side-stream join is queued (_arm_side_join).
_devices = {}


def _dev(of=None):
    """The record of a torch.device, of a stream's device, or (None, or a device without an index) of the current device."""
    idx = of.device_index if isinstance(of, torch.cuda.Stream) else getattr(of, "index", None)
    if idx is None:
        idx = torch.cuda.current_device()
    if idx not in _devices:
        _devices[idx] = _types.SimpleNamespace(dropout=None, side=None, main=None, zero_buf=None, zero_off=0,
                                               collectors=[], collectors_pass=-1)
    return _devices[idx]


def _first_in_pass(obj):
    """Is this the first time `obj` is met in the backward pass that is running?  Passes are told apart by the autograd
    engine's graph-task id (monotonic; -1 outside a backward, where the answer is always yes), kept on `obj`, so nothing
    has to be reset when a pass ends - or fails to end: the engine runs no end-of-backward callback of a pass that raised."""
    cur = torch._C._current_graph_task_id()
    if cur != -1 and getattr(obj, "_pass", None) == cur:
        return False
    obj._pass = cur
    return True


# One pooled memset per training step instead of one per convolution: the packed weight-gradient buffers (split-K float atomics
# start from zero) and the BatchNorm-backward sums that ride on input-gradient epilogues are carved from a per-device pool
# that StemFn.forward - the first node of a step - zeroes with a single launch.  A region is handed out at most once per
# reset, so it still holds zeros when its kernel runs; without a reset in this process, or when the pool is used up, the
# takers fall back to a buffer the C call zeroes itself.
ZERO_POOL_BYTES = 64 << 20        # ResNet-18 trunk weights: 44.7 MB of fp32, + 0.2 MB of fp64 sums


def zero_pool_reset(dev):
    d = _dev(dev)
    if d.zero_buf is None:
        d.zero_buf = torch.empty(ZERO_POOL_BYTES, dtype=torch.uint8, device=dev)
    d.zero_buf.zero_()
    d.zero_off = 0


def zero_pool_take(dev, shape, dtype):
    """A zero-filled tensor from the pool, or None (the caller then allocates and lets the C call zero its buffer)."""
    d = _dev(dev)
    n = 1
    for k in shape:
        n *= k
    nbytes = n * torch.empty((), dtype=dtype).element_size()
    if d.zero_buf is None or d.zero_off + nbytes > ZERO_POOL_BYTES:
        return None
    off = d.zero_off
    d.zero_off = (off + nbytes + 255) & ~255
    return d.zero_buf[off:off + nbytes].view(dtype).view(*shape)


def _zeros_or_empty(dev, shape, dtype):
    """(tensor, pooled): a zero-filled tensor from the pool, or an uninitialised one that the C call has to zero."""
    t = zero_pool_take(dev, shape, dtype)
    if t is not None:
        return t, True
    return torch.empty(shape, device=dev, dtype=dtype), False


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.SblHipError("sbl ops need CUDA/HIP tensors (got a %s tensor); there is no CPU path" % t.device)


def _rows(t):
    """(M, ld) of a 2-D fp32 tensor whose last dim is dense."""
    assert t.dim() == 2 and t.stride(1) == 1 and t.dtype == torch.float32, (t.shape, t.stride(), t.dtype)
    return t.size(0), (t.stride(0) if t.size(0) > 1 else max(t.stride(0), t.size(1)))


# --------------------------------------------------------------------------- #
# dropout state: one device-resident seed shared by every mask of a step
# --------------------------------------------------------------------------- #
class DropoutState:
    """Device seed + per-call-site offsets.  `next_offset()` hands out a distinct
    stream offset per dropout site per forward; `bump()` advances the seed on the
    device (one tiny kernel), so a captured graph draws new masks on every replay."""

    def __init__(self, device, seed=None):
        if seed is None:
            # data-parallel replicas draw independent masks (nn.DataParallel's replicas each use their device's
            # generator, SBL/train.py:115): fold the rank into the default seed
            seed = 0x5B1C0FFEE
            if _dist.is_available() and _dist.is_initialized():
                seed ^= (_dist.get_rank() * 0x9E3779B97F4A7C15) & 0x7FFFFFFFFFFFFFFF
        self.seed = torch.tensor([seed], dtype=torch.int64, device=device)
        self._offset = 0

    def next_offset(self):
        self._offset += 1
        return self._offset

    def begin_step(self):
        self._offset = 0
        call("sbl_seed_bump", _p(self.seed), _s())


def dropout_state(device):
    d = _dev(device)
    if d.dropout is None:
        d.dropout = DropoutState(device)
    return d.dropout


def side_stream(device):
    """The per-device second HIP stream used to overlap the two decoder directions."""
    d = _dev(device)
    if d.side is None:
        # (stream priorities were measured and dropped: a low-priority side stream changes nothing, a high-priority
        # main stream captured into the hipGraph runs the step at 79 ms instead of 45)
        d.side = torch.cuda.Stream(device=device)
    return d.side


def set_main_stream(stream):
    """Remember which stream the side stream forks from / joins to (per device)."""
    _dev(stream).main = stream


def _on_side_stream():
    """The current stream when it is this device's side stream, else None."""
    cur = torch.cuda.current_stream()
    side = _dev(cur).side
    return cur if side is not None and cur == side else None


def _xs_in(*ts):
    """A tape node running on the side stream reads tensors that the main stream allocated (incoming grads):
    tell the caching allocator, or the block could be handed to a main-stream kernel while we still read it.
    Forward needs none of this (fork/join fences on both sides of every layer); backward's engine-inserted
    syncs are one-directional."""
    cur = _on_side_stream()
    if cur is not None:
        for t in ts:
            if t is not None:
                t.record_stream(cur)


def _xs_out(*ts):
    """...and what it hands back (allocated on the side stream) is consumed on the main stream."""
    cur = _on_side_stream()
    main = _dev(cur).main if cur is not None else None
    if main is not None:
        for t in ts:
            if t is not None:
                t.record_stream(main)


def join_side_streams():
    """Make the current stream wait for everything enqueued on the side stream (end of a step)."""
    cur = torch.cuda.current_stream()
    side = _dev(cur).side
    if side is not None:
        cur.wait_stream(side)


def _arm_side_join():
    """Once per (device, backward pass): make the stream that finishes backward wait for the side stream."""
    if _first_in_pass(_dev()):
        torch.autograd.Variable._execution_engine.queue_callback(join_side_streams)


def _side_to_main():
    """Explicit fence when a side-stream tape node hands its result to the main stream (belt and braces next to the
    autograd engine's own producer/consumer event)."""
    cur = _on_side_stream()
    main = _dev(cur).main if cur is not None else None
    if main is not None:
        main.wait_stream(cur)


class WgradCollector:
    """Deferred weight gradients of the decoder.  Every decoder weight is used once per stage (up to 16 times per
    step); instead of one skinny dW GEMM per use inside backward's dependency chain, the (dY, X) operand pairs are
    collected and each weight gets ONE GEMM that contracts over all stages' rows (K ~ 4352) when backward has
    finished (autograd engine callback).  Needs persistent gradient buffers (dp.FlatModel)."""

    def __init__(self):
        self.entries = {}

    def add(self, C, ldc, colsum, A, lda, B, ldb, rows, M, N):
        if _first_in_pass(self):
            self.entries = {}      # anything still here is of a pass over this graph that never finished
            # flush_deferred() sees the collectors of the newest pass on this device only: arming under a newer pass
            # drops those of a pass that raised, with the tensors they pin.  A pass nested in a node (checkpoint,
            # autograd.grad) takes the list over too; the outer pass's collectors then lose the early flush only, the
            # end-of-pass callback below still issues them.
            d = _dev()
            if self._pass > d.collectors_pass:
                d.collectors, d.collectors_pass = [], self._pass
            if self._pass == d.collectors_pass:
                d.collectors.append(self)
            torch.autograd.Variable._execution_engine.queue_callback(self.finish)
        e = self.entries.get(C.data_ptr())
        if e is None:
            e = self.entries[C.data_ptr()] = {"C": C, "ldc": ldc, "colsum": colsum, "lda": lda, "ldb": ldb, "M": M,
                                              "N": N, "A": [], "B": [], "rows": []}
        e["A"].append(A)
        e["B"].append(B)
        e["rows"].append(rows)

    def flush(self):
        """Issue the collected GEMMs.  Called from a hook on the decoder's encoder_outputs gradient (every decoder
        tape node has run by then: they all outrank the hoisted K/V projections in the engine's ready queue), so
        the GEMMs go to the side stream and overlap the encoder / frontend backward on the main stream; called
        again from the engine's end-of-backward callback, which issues anything that arrived late and joins."""
        if not self.entries:
            return
        cur = torch.cuda.current_stream()
        side = _dev(cur).side
        run = cur
        if side is not None and cur != side:
            cur.wait_stream(side)              # operands produced by the other direction's stream
            side.wait_stream(cur)
            run = side
        # weights whose stages have the same row structure (all layer weights of both directions) form one group
        groups = {}
        for e in self.entries.values():
            groups.setdefault(tuple(e["rows"]), []).append(
                (e["C"], e["ldc"], e["colsum"], e["A"], e["lda"], e["B"], e["ldb"], e["M"], e["N"]))
        with torch.cuda.stream(run):
            for seg_rows, problems in groups.items():
                wgrad_group(problems, seg_rows, run, _wgrad_seg)
        self.entries = {}

    def finish(self):
        """Engine end-of-backward callback: late entries, then the main stream waits for the side stream."""
        self.flush()
        join_side_streams()


def flush_deferred():
    """Issue every deferred weight-gradient GEMM collected so far in the running pass (idempotent).  dp.GradientExchange
    calls this before it all-reduces the decoder segment; the decoder calls it from its encoder_outputs gradient hook."""
    d = _dev()
    if d.collectors_pass == torch._C._current_graph_task_id():
        for c in list(d.collectors):
            c.flush()


_tls = _threading.local()      # the collector of the forward pass running on THIS thread (nn.DataParallel: one per replica)


@_contextlib.contextmanager
def deferring():
    """Encoder / decoder forward: tape nodes created inside defer their weight gradients (if enabled) to one collector."""
    _tls.collector = WgradCollector()
    try:
        yield
    finally:
        _tls.collector = None


def wgrad_gemm(M, N, K, A, lda, B, ldb, C, ldc, acc, colsum, defer=None):
    """dW (+)= A^T B with the bias gradient riding on it.  With a collector and a persistent gradient buffer (acc=1)
    the product is deferred to one all-stages GEMM per weight; else it is issued now."""
    if defer is not None and acc:
        defer.add(C, ldc, colsum, A, lda, B, ldb, K, M, N)
        return
    gemm(1, 0, M, N, K, A, lda, B, ldb, C, ldc, accumulate=acc, colsum=colsum)


# split-K workspace: int[4096] tile counters (kept zero by the kernel) + fp32 partial slabs, one per stream so
# that GEMMs running concurrently on different streams never share slabs
WS_BYTES = 16 << 20
_workspaces = {}


def _workspace():
    st = torch.cuda.current_stream()
    key = (st.device_index, st.cuda_stream)
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = torch.zeros(WS_BYTES // 4, dtype=torch.float32, device=torch.device("cuda", st.device_index))
    return ws


def gemm(ta, tb, M, N, K, A, lda, B, ldb, C, ldc, bias=None, relu=0, mask=None, ldm=0, accumulate=0, colsum=None):
    ws = _workspace()
    call("sbl_gemm_f32", ta, tb, M, N, K, _p(A), lda, _p(B), ldb, _p(C), ldc, _p(bias), relu, _p(mask), ldm,
         accumulate, _p(colsum), ws.data_ptr(), WS_BYTES, _s())


def gemm2(M, N, K, A0, A1, lda, B0, B1, ldb, C0, C1, ldc, bias0=None, bias1=None, relu=0):
    """C_d = A_d @ B_d^T (+ bias_d) (ReLU) for two same-shape problems in one launch (the two decoder directions); launches
    with few rows run on 16x16 tiles, every other one as sbl_gemm2_f32 (include/sbl_hip.h)."""
    ws = _workspace()
    call("sbl_gemm2_rows_f32", M, N, K, _p(A0), _p(A1), lda, _p(B0), _p(B1), ldb, _p(C0), _p(C1), ldc, _p(bias0), _p(bias1), relu,
         ws.data_ptr(), WS_BYTES, _s())


_group_tables = {}      # (device, stream, row structure) -> descriptor table of sbl_wgrad_group_f32


def _wgrad_seg(C, ldc, colsum, A, lda, B, ldb, M, N, seg_rows):
    """One weight's C += sum_s A_s^T B_s, at most 16 segments per launch."""
    for i in range(0, len(seg_rows), 16):
        rows = seg_rows[i:i + 16]
        k = len(rows)
        call("sbl_wgrad_seg_f32", k, (_ct.c_void_p * k)(*[t.data_ptr() for t in A[i:i + 16]]), lda,
             (_ct.c_void_p * k)(*[t.data_ptr() for t in B[i:i + 16]]), ldb, (_ct.c_int * k)(*rows), M, N, _p(C), ldc, _p(colsum), _s())


def _wgrad_splitk(C, ldc, colsum, A, lda, B, ldb, M, N, seg_rows):
    """One weight's C += A^T B over a single segment as a split-K GEMM."""
    (A,), (B,), (rows,) = A, B, seg_rows
    gemm(1, 0, M, N, rows, A, lda, B, ldb, C, ldc, accumulate=1, colsum=colsum)


def wgrad_group(problems, seg_rows, run, per_weight):
    """C += sum_s A_s^T B_s (colsum += column sums of A) for every problem (C, ldc, colsum, A_list, lda, B_list, ldb, M, N);
    segment s of every problem has seg_rows[s] rows.  `run` is the current stream.  One sbl_wgrad_group_f32 launch for all
    of them - each 128x128 tile of each gradient is owned by one workgroup over the whole K = all segments' rows, no split-K,
    no atomics - when the kernel takes them (several problems, at most 16 segments of a multiple of 16 rows, M and N
    multiples of 4); else per_weight(*problem, seg_rows) for each."""
    n, k = len(problems), len(seg_rows)
    if n > 1 and k <= 16 and all(r % 16 == 0 for r in seg_rows) and all(p[7] % 4 == 0 and p[8] % 4 == 0 for p in problems):
        need = _lib.load().sbl_wgrad_group_table_bytes(n)
        # one table per row structure: two grouped launches in flight on one stream never share one
        key = (run.device_index, run.cuda_stream, tuple(seg_rows))
        tab = _group_tables.get(key)
        if tab is None or tab.numel() < need:
            if len(_group_tables) >= 64:      # (on the per-stage tape the row structure follows the coin pattern)
                _group_tables.clear()
            tab = _group_tables[key] = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=torch.device("cuda", run.device_index))
        col = lambda i, ct: (ct * n)(*[p[i] for p in problems])      # noqa: E731
        call("sbl_wgrad_group_f32", n, k, (_ct.c_int * k)(*seg_rows),
             (_ct.c_void_p * (n * k))(*[t.data_ptr() for p in problems for t in p[3]]), col(4, _ct.c_long),
             (_ct.c_void_p * (n * k))(*[t.data_ptr() for p in problems for t in p[5]]), col(6, _ct.c_long),
             col(7, _ct.c_int), col(8, _ct.c_int), (_ct.c_void_p * n)(*[p[0].data_ptr() for p in problems]), col(1, _ct.c_long),
             (_ct.c_void_p * n)(*[_p(p[2]) for p in problems]), tab.data_ptr(), tab.numel(), _s())
    else:
        for p in problems:
            per_weight(*p, seg_rows)
    for p in problems:
        for t in p[3] + p[5]:
            t.record_stream(run)


_seg_arrays = {}


def _segs(segL):
    """host int array of prefix lengths for the ragged ("segmented") kernels, cached per tuple"""
    segL = tuple(int(v) for v in segL)
    arr = _seg_arrays.get(segL)
    if arr is None:
        arr = _seg_arrays[segL] = (_ct.c_int * len(segL))(*segL)
    return arr, len(segL)


def _gbuf(p):
    """The persistent gradient buffer of a parameter, if the model was flattened (dp.FlatModel): backward then
    accumulates into it inside the kernels (GEMM epilogue '+=', atomics) and returns None to autograd, instead of
    allocating a gradient and having AccumulateGrad add it with a separate kernel (16x per decoder parameter).
    The buffer is the parameter's fixed slice of the flat gradient whatever `p.grad` currently says; a `.grad` the caller
    dropped or replaced (torch.optim's zero_grad(set_to_none=True) default, possibly BETWEEN forward and backward as in
    SBL/train.py:195-196) is repaired at the root of the next backward pass (_backward_enter), whether or not the
    previous pass ran to its end."""
    if p is None:
        return None
    return getattr(p, "_sbl_grad", None)


_flat_models = _weakref.WeakSet()


def register_flat_model(fm):
    _flat_models.add(fm)


def _backward_enter():
    """First thing every sbl tape node's backward does: the first node of a backward pass lets each flat model of this
    device repair / zero detached gradients BEFORE any kernel accumulates (dp.FlatModel.begin_backward)."""
    if not _flat_models:
        return
    dev = torch.cuda.current_device() if torch.cuda.is_available() else None
    for fm in list(_flat_models):
        if fm.device_index in (None, dev) and _first_in_pass(fm):
            fm.begin_backward()


def _bw(fn):
    @_functools.wraps(fn)
    def wrapped(ctx, *grads):
        _backward_enter()
        return fn(ctx, *grads)
    return wrapped


def _target(buf, shape, dev, zero=False):
    """(tensor to write, accumulate flag, value to hand back to autograd)"""
    if buf is not None:
        return buf, 1, None
    t = (torch.zeros if zero else torch.empty)(shape, device=dev, dtype=torch.float32)
    return t, 0, t


# --------------------------------------------------------------------------- #
# Linear
# --------------------------------------------------------------------------- #
class LinearFn(torch.autograd.Function):
    """y = x W^T + b (optional ReLU).  nn.Linear: attention.py:16-18,27; module.py:42-43; encoder.py:27;
    decoder.py:59-60."""

    @staticmethod
    def forward(ctx, x, w, b, relu):
        _need_cuda(x, w, b)
        M, ldx = _rows(x)
        N, K = w.shape
        y = torch.empty(M, N, device=x.device, dtype=torch.float32)
        gemm(0, 1, M, N, K, x, ldx, w, K, y, N, bias=b, relu=int(relu))
        ctx.save_for_backward(x, w, y if relu else None)
        ctx.has_bias = b is not None
        ctx.relu = relu
        ctx.gb = (_gbuf(w), _gbuf(b))
        return y

    @staticmethod
    @_bw
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dy = dy.contiguous()
        if ctx.relu:
            dy = dy * (y > 0).to(dy.dtype)
        M, ldx = _rows(x)
        N, K = w.shape
        dev = dy.device
        dx = dw_ret = db_ret = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(M, K, device=dev, dtype=torch.float32)
            gemm(0, 0, M, K, N, dy, N, w, K, dx, K)
        if ctx.needs_input_grad[1]:
            dw, acc, dw_ret = _target(ctx.gb[0], (N, K), dev)
            db = None
            if ctx.has_bias and ctx.needs_input_grad[2]:
                db, _, db_ret = _target(ctx.gb[1], (N,), dev, zero=True)
            gemm(1, 0, N, K, M, dy, N, x, ldx, dw, K, accumulate=acc, colsum=db)
        elif ctx.has_bias and ctx.needs_input_grad[2]:
            db, acc, db_ret = _target(ctx.gb[1], (N,), dev)
            call("sbl_colsum_f32", _p(dy), N, _p(db), M, N, acc, _s())
        return dx, dw_ret, db_ret, None


def linear(x, w, b=None, relu=False):
    shp = x.shape
    x2 = x if x.dim() == 2 else x.reshape(-1, shp[-1])
    y = LinearFn.apply(x2, w, b, relu)
    return y if x.dim() == 2 else y.view(*shp[:-1], w.size(0))


# --------------------------------------------------------------------------- #
# dropout / PE / LayerNorm
# --------------------------------------------------------------------------- #
class DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        _need_cuda(x)
        x = x.contiguous()
        st = dropout_state(x.device)
        ctx.off = st.next_offset()
        ctx.p = p
        ctx.seed = st.seed
        y = torch.empty_like(x)
        call("sbl_dropout", _p(x), _p(y), x.numel(), p, _p(st.seed), ctx.off, _s())
        return y

    @staticmethod
    @_bw
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        call("sbl_dropout", _p(dy), _p(dx), dy.numel(), ctx.p, _p(ctx.seed), ctx.off, _s())
        return dx, None


def dropout(x, p, training):
    if not training or p <= 0.0:
        return x
    return DropoutFn.apply(x, float(p))


class AddPEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, pe):
        _need_cuda(x, pe)
        B, L, D = x.shape
        x = x.contiguous()
        y = torch.empty_like(x)
        call("sbl_add_pe", _p(x), _p(pe), _p(y), B, L, D, _s())
        return y

    @staticmethod
    @_bw
    def backward(ctx, dy):
        return dy, None


class AddLayerNormFn(torch.autograd.Function):
    """y = LayerNorm(x + res); encoder.py:54 (res=None), attention.py:58, module.py:51."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, eps):
        _need_cuda(x, gamma, beta)
        D = x.size(-1)
        x2 = x.contiguous().view(-1, D)
        r2 = None if res is None else res.contiguous().view(-1, D)
        M = x2.size(0)
        y = torch.empty_like(x2)
        mean = torch.empty(M, device=x.device, dtype=torch.float32)
        rstd = torch.empty(M, device=x.device, dtype=torch.float32)
        call("sbl_add_layernorm_fwd", _p(x2), _p(r2), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), M, D, eps, 0.0, None,
             0, _s())
        ctx.save_for_backward(x2, r2, gamma, mean, rstd)
        ctx.shape = x.shape
        ctx.ln = (gamma, beta, _gbuf(gamma), _gbuf(beta), eps)
        return y.view(x.shape)

    @staticmethod
    @_bw
    def backward(ctx, dy):
        x2, r2, gamma, mean, rstd = ctx.saved_tensors
        ln, (dg_ret, db_ret) = _ln_targets(ctx.ln, dy.device)
        dz, _ = ln_bwd(dy.contiguous().view(x2.shape), x2, r2, ln, mean, rstd, 0.0, None, 0, False)
        dz = dz.view(ctx.shape)
        return dz, (dz if r2 is not None else None), dg_ret, db_ret, None


class RowScaleFn(torch.autograd.Function):
    """x * non_pad_mask (mask: (..., 1) float, one factor per row); encoder.py:86,89."""

    @staticmethod
    def forward(ctx, x, scale):
        _need_cuda(x, scale)
        x = x.contiguous()
        sc = scale.to(torch.float32).contiguous().view(-1)
        D = x.size(-1)
        assert sc.numel() == x.numel() // D
        y = torch.empty_like(x)
        call("sbl_rowscale", _p(x), _p(sc), _p(y), sc.numel(), D, _s())
        ctx.save_for_backward(sc)
        return y

    @staticmethod
    @_bw
    def backward(ctx, dy):
        (sc,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        call("sbl_rowscale", _p(dy), _p(sc), _p(dx), sc.numel(), dy.size(-1), _s())
        return dx, None


def add_layernorm(x, res, gamma, beta, eps=1e-5):
    return AddLayerNormFn.apply(x, res, gamma, beta, eps)


# --------------------------------------------------------------------------- #
# attention core (used by ScaledDotProductAttention directly)
# --------------------------------------------------------------------------- #
def _mask_args(mask, B, Lq, Lk):
    """mask: None | 'causal' | uint8/bool tensor (B,Lq,Lk) -> (kind, tensor-or-None)"""
    if mask is None:
        return 0, None
    if isinstance(mask, str):
        assert mask == "causal"
        return 1, None
    m = mask
    if m.dim() == 3 and m.size(0) != B:            # head-repeated (n_head*B, Lq, Lk): attention.py:50
        m = m[:B]
    m = m.expand(B, Lq, Lk).to(torch.uint8).contiguous()
    return 2, m


class SDPAFn(torch.autograd.Function):
    """softmax(Q K^T * scale, masked) [dropout] V over (B, L, H*64) views; attention.py:72-83."""

    @staticmethod
    def forward(ctx, q, k, v, H, scale, mask_kind, mask_t, drop_p):
        _need_cuda(q, k, v)
        B, Lq, _ = q.shape
        Lk = k.size(1)
        assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
        assert q.stride(0) == Lq * q.stride(1) and k.stride(0) == Lk * k.stride(1) and v.stride(0) == Lk * v.stride(1)
        o = torch.empty(B, Lq, H * 64, device=q.device, dtype=torch.float32)
        p = torch.empty(H * B, Lq, Lk, device=q.device, dtype=torch.float32)
        seed, off = None, 0
        if drop_p > 0:
            st = dropout_state(q.device)
            seed, off = st.seed, st.next_offset()
        call("sbl_attention_fwd", _p(q), q.stride(1), _p(k), k.stride(1), _p(v), v.stride(1), _p(o), H * 64, _p(p),
             mask_kind, _p(mask_t), B, H, Lq, Lk, scale, drop_p, _p(seed), off, _s())
        ctx.save_for_backward(q, k, v, p, seed)
        ctx.cfg = (H, scale, drop_p, off)
        ctx.mark_non_differentiable(p)
        ctx.set_materialize_grads(False)      # else autograd zero-fills a gradient for p before every backward
        return o, p

    @staticmethod
    @_bw
    def backward(ctx, do, _dp):
        if do is None:
            return (None,) * 8
        q, k, v, p, seed = ctx.saved_tensors
        H, scale, drop_p, off = ctx.cfg
        B, Lq, _ = q.shape
        Lk = k.size(1)
        do = do.contiguous()
        dq = torch.empty(B, Lq, H * 64, device=q.device, dtype=torch.float32)
        dk = torch.empty(B, Lk, H * 64, device=q.device, dtype=torch.float32)
        dv = torch.empty(B, Lk, H * 64, device=q.device, dtype=torch.float32)
        call("sbl_attention_bwd", _p(do), H * 64, _p(q), q.stride(1), _p(k), k.stride(1), _p(v), v.stride(1), _p(p),
             _p(dq), H * 64, _p(dk), H * 64, _p(dv), H * 64, B, H, Lq, Lk, scale, drop_p, _p(seed), off, _s())
        return dq, dk, dv, None, None, None, None, None


# --------------------------------------------------------------------------- #
# the post-norm transformer sub-layer: its launch sequences, stated once
# --------------------------------------------------------------------------- #
# y = LayerNorm(dropout(core(x W_in^T + b_in) W_out^T + b_out) + x), core = attention or ReLU, as plain functions over
# explicit tensors: no autograd, no streams; they write into the buffers they are given and allocate the others.  Callers:
# the tape nodes below, the stage-batched decoder backward (transformer/decoder_stages.py), the KV-cached greedy decode
# (transformer/seq2seq.py).  The attention core draws its dropout mask at offset `off_a`, the output dropout (fused into the
# LayerNorm kernels) at `off_o` / `off`; backward passes the forward's offsets and the kernels regenerate the masks.  Every
# weight gradient goes to the caller's `sink(lin, dY, X)` (dW += dY^T X, the bias gradient riding on it) BEFORE the input
# gradient is accumulated in place onto the residual gradient.
def _adjacent(*ts):
    """True if the tensors are contiguous and laid out back to back in memory (rows of one fused matrix)."""
    p = ts[0].data_ptr()
    for t in ts:
        if not t.is_contiguous() or t.data_ptr() != p:
            return False
        p += t.numel() * t.element_size()
    return True


def fuse_rows(ws, bs):
    """Move the parameters `ws` (and their biases `bs`) to adjacent row ranges of one new buffer each."""
    with torch.no_grad():
        fw = torch.cat([w.data for w in ws], 0).contiguous()
        fb = torch.cat([b.data for b in bs], 0).contiguous()
        if fw.is_cuda:      # one-time set-up: the old storages are released below, so the copies must have run
            torch.cuda.current_stream(fw.device).synchronize()
        r = 0
        for w, b in zip(ws, bs):
            n = w.size(0)
            w.data = fw[r:r + n]
            b.data = fb[r:r + n]
            r += n


class Lin:
    """Handle of y = x W^T + b with W (N, K) = the weights `ws` stacked, which must be adjacent rows of one matrix (fused
    q/k/v or k/v; a single weight is its own stack), `bs` likewise.  gw / gb: the persistent gradient buffers of the
    stacked W / b when every part has one and they are adjacent too, else both None (backward then hands fresh gradients
    to autograd)."""

    def __init__(self, ws, bs):
        assert _adjacent(*ws) and _adjacent(*bs)
        self.w, self.b = ws[0], bs[0]
        self.N, self.K = sum(w.size(0) for w in ws), ws[0].size(1)
        gw, gb = [_gbuf(t) for t in ws], [_gbuf(t) for t in bs]
        ok = all(g is not None for g in gw + gb) and _adjacent(*gw) and _adjacent(*gb)
        self.gw, self.gb = (gw[0], gb[0]) if ok else (None, None)


def _sublayer(inp, out, gamma, beta, eps, drop_p, H=0):
    """Parameter handle of one sub-layer.  inp: the Lin in front of the core, out: the one behind it, ln: (gamma, beta, where
    backward accumulates dgamma, dbeta - persistent buffers or None -, eps), H heads (attention)."""
    return _types.SimpleNamespace(inp=inp, out=out, ln=(gamma, beta, _gbuf(gamma), _gbuf(beta), eps), drop_p=drop_p, H=H)


def attn_handle(wq, bq, wk, bk, wv, bv, wfc, bfc, gamma, beta, H, drop_p, eps):
    """inp = the fused q/k/v projection, or with wk = None q alone (cross-attention: [K|V] come pre-projected); out = fc."""
    inp = Lin((wq,), (bq,)) if wk is None else Lin((wq, wk, wv), (bq, bk, bv))
    return _sublayer(inp, Lin((wfc,), (bfc,)), gamma, beta, eps, drop_p, H)


def ffn_handle(w1, b1, w2, b2, gamma, beta, drop_p, eps):
    return _sublayer(Lin((w1,), (b1,)), Lin((w2,), (b2,)), gamma, beta, eps, drop_p)


def kv_block(mods):
    """(weights, biases) of the cross-attention modules' K/V projections in the order of the block [K_0; V_0; K_1; ...]"""
    return [w for m in mods for w in (m.w_ks.weight, m.w_vs.weight)], [b for m in mods for b in (m.w_ks.bias, m.w_vs.bias)]


def _new(like, *shape):
    return torch.empty(shape, device=like.device, dtype=torch.float32)


def lin_fwd(lin, x, out=None, relu=0):
    """out (M, N) = x W^T + b (ReLU)."""
    M, ldx = _rows(x)
    if out is None:
        out = _new(x, M, lin.N)
    gemm(0, 1, M, lin.N, lin.K, x, ldx, lin.w, lin.K, out, lin.N, bias=lin.b, relu=relu)
    return out


def out_ln_fwd(h, a, res, seed, off, bufs=None):
    """The closing half of sub-layer h: o = a W_out^T + b, y = LayerNorm(dropout(o) + res), into bufs = (o, y, mean, rstd)
    when given.  Returns (o, y, mean, rstd)."""
    M = a.size(0)
    o, y, mean, rstd = bufs or (None, _new(a, M, h.out.N), _new(a, M), _new(a, M))
    o = lin_fwd(h.out, a, o)
    call("sbl_add_layernorm_fwd", _p(o), _p(res), _p(h.ln[0]), _p(h.ln[1]), _p(y), _p(mean), _p(rstd), M, h.out.N, h.ln[4],
         h.drop_p, _p(seed) if h.drop_p > 0 else None, off, _s())
    return o, y, mean, rstd


def _counts(t, n, what):
    """The pointer of a per-clip counts tensor (key counts, step counts): contiguous CUDA int32 (n,), never read on the host."""
    assert t.is_cuda and t.dtype == torch.int32 and t.shape == (n,) and t.is_contiguous(), \
        "%s: a contiguous CUDA int32 tensor of %d counts" % (what, n)
    return _p(t)


def attn_fwd(a, x, B, segL, kv, mask_kind, mask_t, seed, off_a, off_o, kv_group=None, kv_len=None):
    """Attention sub-layer on the rows x (B * sum(segL), D) of a ragged batch: segment s has B sequences of length segL[s].
    kv = None: self-attention inside each segment; else cross-attention to the rows kv (B * Lk, 2 * H * 64) = [K|V] (a
    column block of a wider buffer is fine).  Returns (y, (qkv, att, p, o, mean, rstd)): the second is what attn_bwd wants
    back; p = the segments' (H*B, L, Lk) probability blocks back to back.
    kv_group = W (inference only, no mask): kv holds B / W entries and sequence b attends to entry b // W
    (sbl_attention_seg_grouped_fwd); no probabilities are kept (p = None).
    kv_len (inference only, no mask; kv_group = None means 1): a device int32 tensor of key counts, one per kv entry (B /
    kv_group of them) or, with kv = None (one segment), one per sequence: only the keys j < kv_len[.] are attended to
    (sbl_attention_seg_len_fwd).  The counts are never read on the host; p = None."""
    HD = a.H * 64
    qkv = lin_fwd(a.inp, x)
    if kv_len is not None or kv_group is not None:      # inference: the grouped entry, or the `len` one with the counts behind G
        G = 1 if kv_group is None else int(kv_group)
        assert mask_kind == 0 and B % G == 0
        name, counts = "sbl_attention_seg_grouped_fwd", ()
        if kv_len is not None:
            assert not torch.is_grad_enabled()
            name, counts = "sbl_attention_seg_len_fwd", (_counts(kv_len, B // G, "kv_len"),)
        if kv is None:
            assert kv_len is not None and G == 1 and len(segL) == 1
            k, v, ldk, Lk = qkv[:, HD:], qkv[:, 2 * HD:], 3 * HD, 0
        else:
            assert kv.size(0) % (B // G) == 0
            k, v, ldk, Lk = kv, kv[:, HD:], _rows(kv)[1], kv.size(0) // (B // G)
        att = _new(x, x.size(0), HD)
        call(name, _p(qkv), a.inp.N, _p(k), ldk, _p(v), ldk, _p(att), HD, B, a.H, *_segs(segL), Lk, G, *counts, 1.0 / 8.0, a.drop_p,
             _p(seed) if a.drop_p > 0 else None, off_a, _s())
        o, y, mean, rstd = out_ln_fwd(a, att, x, seed, off_o)
        return y, (qkv, att, None, o, mean, rstd)
    if kv is None:
        k, v, ldk, Lk = qkv[:, HD:], qkv[:, 2 * HD:], 3 * HD, 0       # Lk = 0: keys = the segment's own rows
        psize = a.H * B * sum(l * l for l in segL)
    else:
        k, v, ldk, Lk = kv, kv[:, HD:], _rows(kv)[1], kv.size(0) // B
        psize = a.H * B * sum(segL) * Lk
    att = _new(x, x.size(0), HD)
    p = _new(x, psize)
    call("sbl_attention_seg_fwd", _p(qkv), a.inp.N, _p(k), ldk, _p(v), ldk, _p(att), HD, _p(p), mask_kind, _p(mask_t), B, a.H,
         *_segs(segL), Lk, 1.0 / 8.0, a.drop_p, _p(seed) if a.drop_p > 0 else None, off_a, _s())
    o, y, mean, rstd = out_ln_fwd(a, att, x, seed, off_o)
    return y, (qkv, att, p, o, mean, rstd)


def ffn_fwd(f, x, seed, off, h=None, bufs=None):
    """Feed-forward sub-layer on the rows x (M, D).  Returns (y, (h, o, mean, rstd)), the second for ffn_bwd."""
    h = lin_fwd(f.inp, x, h, relu=1)
    o, y, mean, rstd = out_ln_fwd(f, h, x, seed, off, bufs)
    return y, (h, o, mean, rstd)


def project_kv_block(x, mods):
    """[K_0 | V_0 | K_1 | ...] = x [Wk_0; Wv_0; Wk_1; ...]^T + b for the cross-attention modules `mods`, whose K/V projections
    are rows of one matrix in that order: ONE GEMM.  Returns (the block's Lin, the buffer, every module's column block of
    it: read in place, its row stride is the buffer's)."""
    lin = Lin(*kv_block(mods))
    kv = lin_fwd(lin, x)
    return lin, kv, kv.split(lin.N // len(mods), 1)


def ln_bwd(dy, o, res, ln, mean, rstd, drop_p, seed, off, separate_do, ends=None):
    """Adjoint of y = LayerNorm(dropout(o) + res) -> (dz, do): dz = gradient of the residual `res` (of the sum when res is
    None), do = gradient of the pre-dropout o; dgamma / dbeta accumulate into ln[2] / ln[3].  do is a buffer of its own with
    dropout, and whenever the caller says so (`separate_do`): callers go on to accumulate the sub-layer's input gradient
    into dz in place, so a weight-gradient GEMM that is issued later (a deferring sink) must not find do aliased to it.
    Otherwise do IS dz.  ends = (B, segL): the rows are the compact "ends" rows of that ragged batch (include/sbl_hip.h) and
    the masks those of its full layout."""
    M, D = dy.shape
    dz = _new(dy, M, D)
    do = _new(dy, M, D) if separate_do or drop_p > 0 else None
    if ends is None:
        call("sbl_add_layernorm_bwd", _p(dy), _p(o), _p(res), _p(ln[0]), _p(mean), _p(rstd), _p(dz), _p(do), _p(ln[2]), _p(ln[3]),
             M, D, drop_p, _p(seed) if drop_p > 0 else None, off, _s())
    else:
        call("sbl_add_layernorm_ends_bwd", _p(dy), _p(o), _p(res), _p(ln[0]), _p(mean), _p(rstd), _p(dz), _p(do), _p(ln[2]), _p(ln[3]),
             ends[0], *_segs(ends[1]), D, drop_p, _p(seed) if drop_p > 0 else None, off, _s())
    return dz, (dz if do is None else do)


def _out_ln_bwd(h, dy, a, o, res, mean, rstd, seed, off, separate_do, sink, relu_mask=None, ends=None):
    """Adjoint of out_ln_fwd -> (dz = gradient of res, da = gradient of a; `relu_mask` = a when a is a ReLU's output: its
    adjoint is fused into the GEMM epilogue)."""
    lin = h.out
    dz, do = ln_bwd(dy, o, res, h.ln, mean, rstd, h.drop_p, seed, off, separate_do, ends)
    sink(lin, do, a)
    M = dy.size(0)
    da = _new(dy, M, lin.K)
    gemm(0, 0, M, lin.K, lin.N, do, lin.N, lin.w, lin.K, da, lin.K, mask=relu_mask, ldm=0 if relu_mask is None else lin.K)
    return dz, da


def _lin_bwd(lin, dY, x, dx, sink):
    """Adjoint of lin_fwd: dx, which already holds the residual-branch gradient, += dY W."""
    sink(lin, dY, x)
    gemm(0, 0, x.size(0), lin.K, lin.N, dY, lin.N, lin.w, lin.K, dx, lin.K, accumulate=1)


def attn_core_bwd(a, dx, datt, x, qkv, p, B, segL, kv, seed, off_a, sink, dkv=None, ends=False):
    """The attention core and input projection half of attn_bwd: datt = gradient of the core's output, dx = the residual
    gradient of x, which the input projection's adjoint is accumulated into -> (dx, dkv).  ends: cross-attention of the compact
    "ends" queries of the ragged batch segL (include/sbl_hip.h)."""
    HD = a.H * 64
    dq = _new(datt, x.size(0), a.inp.N)                  # self-attention: [dQ | dK | dV]
    if kv is None:
        assert not ends
        k, v, ldk, dk, dv, ldd, Lk = qkv[:, HD:], qkv[:, 2 * HD:], 3 * HD, dq[:, HD:], dq[:, 2 * HD:], 3 * HD, 0
    else:
        dkv = _new(datt, kv.size(0), 2 * HD) if dkv is None else dkv
        k, v, ldk, dk, dv, ldd, Lk = kv, kv[:, HD:], _rows(kv)[1], dkv, dkv[:, HD:], _rows(dkv)[1], kv.size(0) // B
    call("sbl_attention_ends_bwd" if ends else "sbl_attention_seg_bwd", _p(datt), HD, _p(qkv), a.inp.N, _p(k), ldk, _p(v), ldk, _p(p),
         _p(dq), a.inp.N, _p(dk), ldd, _p(dv), ldd, B, a.H, *_segs(segL), Lk, 1.0 / 8.0, a.drop_p, _p(seed) if a.drop_p > 0 else None,
         off_a, _s())
    _lin_bwd(a.inp, dq, x, dx, sink)
    return dx, dkv


def attn_bwd(a, dy, x, acts, B, segL, kv, seed, off_a, off_o, separate_do, sink, dkv=None, ends=False):
    """Adjoint of attn_fwd (acts = what it returned) -> (dx, dkv).  Cross-attention: dkv (B * Lk, 2 * H * 64) is written,
    not accumulated (several segments share the keys / values: their dK / dV contributions are summed inside the call);
    allocated when not given, a column block of a wider buffer is fine.  ends: cross-attention whose rows (dy, x, acts) are
    the compact "ends" rows of the ragged batch segL."""
    qkv, att, p, o, mean, rstd = acts
    dx, datt = _out_ln_bwd(a, dy, att, o, x, mean, rstd, seed, off_o, separate_do, sink, ends=(B, segL) if ends else None)
    return attn_core_bwd(a, dx, datt, x, qkv, p, B, segL, kv, seed, off_a, sink, dkv, ends)


def ffn_bwd(f, dy, x, acts, seed, off, separate_do, sink, ends=None):
    """Adjoint of ffn_fwd (acts = what it returned) -> dx.  ends = (B, segL): compact "ends" rows (ln_bwd)."""
    h, o, mean, rstd = acts
    dx, dh = _out_ln_bwd(f, dy, h, o, x, mean, rstd, seed, off, separate_do, sink, relu_mask=h, ends=ends)
    _lin_bwd(f.inp, dh, x, dx, sink)
    return dx


# ---- the tape's side of it: gradients go to the persistent buffers, or to fresh ones that are handed back to autograd
def _ln_targets(ln, dev):
    """(ln with somewhere for dgamma / dbeta to go, (what to hand back to autograd for gamma, for beta))"""
    gamma, beta, gg, gb, eps = ln
    gg, _, gg_ret = _target(gg, gamma.shape, dev, zero=True)
    gb, _, gb_ret = _target(gb, beta.shape, dev, zero=True)
    return (gamma, beta, gg, gb, eps), (gg_ret, gb_ret)


def _tape_bwd(ctx, dev):
    """-> (handle with LayerNorm gradient targets, separate_do, sink, rets) for a tape node's *_bwd call.  The sink issues a
    weight gradient now or defers it (wgrad_gemm); rets[lin] = (dW, db) and rets["ln"] are autograd's, None if accumulated."""
    h = _copy.copy(ctx.h)
    h.ln, ln_ret = _ln_targets(h.ln, dev)
    rets = {"ln": ln_ret}

    def sink(lin, dY, X):
        dw, acc, dw_ret = _target(lin.gw, (lin.N, lin.K), dev)
        db, _, db_ret = _target(lin.gb, (lin.N,), dev, zero=True)
        wgrad_gemm(lin.N, lin.K, X.size(0), dY, lin.N, X, lin.K, dw, lin.K, acc, db, ctx.defer)
        rets[lin] = (dw_ret, db_ret)

    return h, ctx.defer is not None and h.out.gw is not None, sink, rets


def _param_grads(ret, parts):
    """(dW, db) of a Lin of `parts` stacked weights -> (dW_0, db_0, dW_1, ...) for autograd"""
    dw, db = ret
    if dw is None:
        return (None,) * (2 * parts)
    n = dw.size(0) // parts
    return tuple(t[i * n:(i + 1) * n] for i in range(parts) for t in (dw, db))


class KVProjectFn(torch.autograd.Function):
    """[K | V] = x [Wk; Wv]^T + [bk; bv] -> (B*Lk, 2*H*64).  For decoder cross-attention this is hoisted out
    of the 16-step loop (step-invariant: SURVEY 3.2 consequence ii).  Wk/Wv (and bk/bv) must be adjacent rows of
    one fused buffer (MultiHeadAttention keeps them that way)."""

    @staticmethod
    def forward(ctx, x2, wk, bk, wv, bv):
        _need_cuda(x2, wk, wv)
        ctx.lin = Lin((wk, wv), (bk, bv))
        ctx.save_for_backward(x2, wk, wv)
        return lin_fwd(ctx.lin, x2)

    @staticmethod
    @_bw
    def backward(ctx, dkv):
        x2 = ctx.saved_tensors[0]
        lin = ctx.lin
        dkv = dkv.contiguous()
        _xs_in(dkv, x2)
        M, ldx = _rows(x2)
        dev = dkv.device
        dx = torch.empty(M, lin.K, device=dev, dtype=torch.float32)
        _xs_out(dx)
        gemm(0, 0, M, lin.K, lin.N, dkv, lin.N, lin.w, lin.K, dx, lin.K)
        dw, acc, dw_ret = _target(lin.gw, (lin.N, lin.K), dev)
        db, _, db_ret = _target(lin.gb, (lin.N,), dev, zero=True)
        wgrad_gemm(lin.N, lin.K, M, dkv, lin.N, x2, ldx, dw, lin.K, acc, db)
        _xs_out(dw_ret, db_ret)
        _side_to_main()     # dx joins the other direction's dx in the encoder-output gradient on the main stream
        return (dx,) + _param_grads((dw_ret, db_ret), 2)


class MHAFn(torch.autograd.Function):
    """One whole MultiHeadAttention.forward (attention.py:32-60) as a single tape node over attn_fwd / attn_bwd:
    projections -> attention core -> fc -> dropout -> LayerNorm(out + residual).

    self-attention (kv = None): q, k, v all come from x through ONE fused (M x 3*H*64) GEMM.
    cross-attention (wk = bk = wv = bv = None): q from x, [K|V] given pre-projected (kv, shape (B*Lk, 2*H*64)).
    The output dropout is fused into the LayerNorm kernels, the bias gradients into the weight-gradient GEMMs.
    """

    @staticmethod
    def forward(ctx, x, kv, wq, bq, wk, bk, wv, bv, wfc, bfc, gamma, beta, H, mask_kind, mask_t, drop_p, eps, B, segL):
        """x: (R, D) rows of a ragged batch: segment s has B sequences of length segL[s] (one segment = the plain
        (B, L, D) case).  Returns (y (R, D), p = the segments' (H*B, L, Lk) probability blocks back to back)."""
        _need_cuda(x, wq, wfc)
        x2 = x.contiguous()
        assert x2.size(0) == B * sum(segL), (x2.shape, B, segL)
        assert (kv is None) == (wk is not None)
        a = attn_handle(wq, bq, wk, bk, wv, bv, wfc, bfc, gamma, beta, H, drop_p, eps)
        seed, off_a, off_o = None, 0, 0
        if drop_p > 0:
            st = dropout_state(x.device)
            seed, off_a, off_o = st.seed, st.next_offset(), st.next_offset()
        y, acts = attn_fwd(a, x2, B, segL, kv, mask_kind, mask_t, seed, off_a, off_o)
        # (the weights ride along for autograd's modified-in-place check; backward reads them through the handle)
        ctx.save_for_backward(x2, kv, seed, *acts, wq, wk, wv, wfc, gamma)
        ctx.h, ctx.cfg = a, (B, tuple(segL), off_a, off_o)
        ctx.defer = getattr(_tls, "collector", None)
        ctx.mark_non_differentiable(acts[2])
        ctx.set_materialize_grads(False)      # else autograd zero-fills a gradient for p before every backward
        return y, acts[2]

    @staticmethod
    @_bw
    def backward(ctx, dy, _dp):
        if dy is None:
            return (None,) * 19
        saved = ctx.saved_tensors
        (x2, kv, seed), acts = saved[:3], saved[3:9]
        B, segL, off_a, off_o = ctx.cfg
        _xs_in(dy)
        a, sep, sink, rets = _tape_bwd(ctx, dy.device)
        dx, dkv = attn_bwd(a, dy.contiguous().view(x2.shape), x2, acts, B, segL, kv, seed, off_a, off_o, sep, sink)
        _xs_out(dx, dkv)
        return (dx, dkv) + _param_grads(rets[a.inp], 3 if kv is None else 1) + (None,) * (0 if kv is None else 4) \
            + rets[a.out] + rets["ln"] + (None,) * 7


# tests only: callable(w1, h) handed every feed-forward's post-ReLU hidden activation (tests/test_hip_parity.py compares the
# ReLU masks of this path and of the CPU oracle, to tell a flipped mask bit from an arithmetic error)
_ffn_probe = None


class FFNFn(torch.autograd.Function):
    """PositionwiseFeedForward.forward (module.py:47-52) as one tape node over ffn_fwd / ffn_bwd:
    LayerNorm(dropout(relu(x W1^T + b1) W2^T + b2) + x); dropout fused into the LayerNorm kernels."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, gamma, beta, drop_p, eps):
        _need_cuda(x, w1, w2)
        shp = x.shape
        x2 = x.contiguous().view(-1, shp[-1])
        f = ffn_handle(w1, b1, w2, b2, gamma, beta, drop_p, eps)
        seed, off = None, 0
        if drop_p > 0:
            st = dropout_state(x.device)
            seed, off = st.seed, st.next_offset()
        y, acts = ffn_fwd(f, x2, seed, off)
        if _ffn_probe is not None:
            _ffn_probe(w1, acts[0])
        ctx.save_for_backward(x2, seed, *acts, w1, w2, gamma)      # (the weights: as in MHAFn.forward)
        ctx.h, ctx.cfg = f, (shp, off)
        ctx.defer = getattr(_tls, "collector", None)
        return y.view(shp)

    @staticmethod
    @_bw
    def backward(ctx, dy):
        saved = ctx.saved_tensors
        (x2, seed), acts = saved[:2], saved[2:6]
        shp, off = ctx.cfg
        _xs_in(dy)
        f, sep, sink, rets = _tape_bwd(ctx, dy.device)
        dx = ffn_bwd(f, dy.contiguous().view(x2.shape), x2, acts, seed, off, sep, sink)
        _xs_out(dx)
        return (dx.view(shp),) + rets[f.inp] + rets[f.out] + rets["ln"] + (None, None)


# --------------------------------------------------------------------------- #
# decoder pieces
# --------------------------------------------------------------------------- #
class EmbedPEFn(torch.autograd.Function):
    """emb[tok] + pe[:L] for every segment (decoder step) of a run; decoder.py:116-120 (x_logit_scale = 1).
    tok: (B, 17) device token buffer; segment s embeds its first segL[s] columns.  Returns (B*sum(segL), D)."""

    @staticmethod
    def forward(ctx, tok, B, segL, emb, pe):
        _need_cuda(tok, emb, pe)
        V, D = emb.shape
        seg_arr, nseg = _segs(segL)
        out = torch.empty(B * sum(segL), D, device=emb.device, dtype=torch.float32)
        call("sbl_embed_pe_seg_fwd", _p(tok), tok.stride(0), _p(emb), _p(pe), _p(out), B, seg_arr, nseg, D, V, _s())
        # tokens are written in place by later steps, but positions inside an already embedded prefix never change
        ctx.tok, ctx.B, ctx.segL, ctx.shape = tok, B, tuple(segL), (V, D)
        ctx.gb = _gbuf(emb)
        return out

    @staticmethod
    @_bw
    def backward(ctx, dy):
        V, D = ctx.shape
        dy = dy.contiguous()
        seg_arr, nseg = _segs(ctx.segL)
        demb, _, demb_ret = _target(ctx.gb, (V, D), dy.device, zero=True)
        call("sbl_embed_seg_bwd", _p(ctx.tok), ctx.tok.stride(0), _p(dy), _p(demb), ctx.B, seg_arr, nseg, D, V, _s())
        return None, None, None, demb_ret, None


class FusionFn(torch.autograd.Function):
    """A' = A + flip(B), B' = 2B + flip(A) along each sequence's own prefix; decoder.py:132-143,160-164
    (closed form).  a, b: (B*sum(segL), D) rows, or (B, L, D) with segL=None."""

    @staticmethod
    def forward(ctx, a, b, B=None, segL=None):
        _need_cuda(a, b)
        a, b = a.contiguous(), b.contiguous()
        if segL is None:
            B, segL = a.size(0), (a.size(1),)
        D = a.size(-1)
        seg_arr, nseg = _segs(segL)
        a2, b2 = torch.empty_like(a), torch.empty_like(b)
        call("sbl_fusion_seg_fwd", _p(a), _p(b), _p(a2), _p(b2), B, seg_arr, nseg, D, _s())
        ctx.cfg = (B, tuple(segL), D)
        return a2, b2

    @staticmethod
    @_bw
    def backward(ctx, da2, db2):
        B, segL, D = ctx.cfg
        da2, db2 = da2.contiguous(), db2.contiguous()
        seg_arr, nseg = _segs(segL)
        da, db = torch.empty_like(da2), torch.empty_like(db2)
        call("sbl_fusion_seg_bwd", _p(da2), _p(db2), _p(da), _p(db), B, seg_arr, nseg, D, _s())
        return da, db, None, None


class GatherLastFn(torch.autograd.Function):
    """The last position of every sequence of a ragged batch, (nseg*B, D): the rows the heads read, decoder.py:166-167."""

    @staticmethod
    def forward(ctx, x, B, segL):
        _need_cuda(x)
        x = x.contiguous()
        D = x.size(-1)
        seg_arr, nseg = _segs(segL)
        out = torch.empty(nseg * B, D, device=x.device, dtype=torch.float32)
        call("sbl_gather_last_fwd", _p(x), _p(out), B, seg_arr, nseg, D, _s())
        ctx.cfg = (B, tuple(segL), D, x.shape)
        return out

    @staticmethod
    @_bw
    def backward(ctx, dy):
        B, segL, D, shp = ctx.cfg
        dy = dy.contiguous()
        seg_arr, nseg = _segs(segL)
        dx = torch.empty(shp, device=dy.device, dtype=torch.float32)
        call("sbl_gather_last_bwd", _p(dy), _p(dx), B, seg_arr, nseg, D, _s())
        return dx, None, None


def argmax_select(pred, gold, ys, step, use_argmax, coins_dev=None):
    """ys[:, step+1] = argmax(pred) if coin else gold[:, step]; decoder.py:173-186, on the device."""
    if pred is None:                       # pure teacher token (no logits needed)
        assert not use_argmax and coins_dev is None and gold is not None
        B, V, ldp = ys.size(0), 1, 1
    else:
        (B, V), ldp = pred.shape, pred.stride(0)
    call("sbl_argmax_select", _p(pred), ldp, _p(gold), 0 if gold is None else gold.stride(0), _p(ys),
         ys.stride(0), step, int(use_argmax), _p(coins_dev), B, V, _s())


class SmoothedCEFn(torch.autograd.Function):
    """cal_loss (loss.py:27-52): returns (mean loss over gold != ignore, stats[3] = (sum, n_valid, n_correct))."""

    @staticmethod
    def forward(ctx, pred, gold, eps, ignore_id):
        _need_cuda(pred, gold)
        pred = pred.contiguous()
        gold = gold.contiguous()
        R, C = pred.shape
        out3 = torch.empty(3, device=pred.device, dtype=torch.float32)
        call("sbl_smoothed_ce_fwd", _p(pred), _p(gold), _p(out3), R, C, eps, ignore_id, _s())
        ctx.save_for_backward(pred, gold, out3)
        ctx.cfg = (eps, ignore_id)
        ctx.mark_non_differentiable(out3)
        ctx.set_materialize_grads(False)
        return out3[0] / out3[1], out3

    @staticmethod
    @_bw
    def backward(ctx, gloss, _g3):
        if gloss is None:
            return None, None, None, None
        pred, gold, out3 = ctx.saved_tensors
        eps, ignore_id = ctx.cfg
        R, C = pred.shape
        gs = gloss.reshape(1).to(torch.float32).contiguous()
        dpred = torch.empty_like(pred)
        call("sbl_smoothed_ce_bwd", _p(pred), _p(gold), _p(out3), _p(gs), _p(dpred), R, C, eps, ignore_id, _s())
        return dpred, None, None, None


# --------------------------------------------------------------------------- #
# stage-1 classification heads (CLS pre-training model)
# --------------------------------------------------------------------------- #
class ClsHeadFn(torch.autograd.Function):
    """fc_1500(mean over time) and fc_2(row lang_index) of the encoder output (N, T, 512): CLS/transformer/transformer.py:31-35
    as oracle.sbl_oracle.cls_forward restates it.  Returns (logits1 (N, C1), logits2 (N, C2)).  Parameter gradients go
    straight into the flat gradient buffers when the model is flattened (dp.FlatModel), like LinearFn's."""

    @staticmethod
    def forward(ctx, enc, w1, b1, w2, b2, lang_index):
        _need_cuda(enc, w1, b1, w2, b2)
        enc = enc.contiguous()
        N, T, D = enc.shape
        C1, C2 = w1.size(0), w2.size(0)
        dev = enc.device
        pooled = torch.empty(N, D, device=dev, dtype=torch.float32)
        pooled_t = torch.empty(D, N, device=dev, dtype=torch.float32)
        l1 = torch.empty(N, C1, device=dev, dtype=torch.float32)
        l2 = torch.empty(N, C2, device=dev, dtype=torch.float32)
        call("sbl_cls_head_fwd", _p(enc), _p(w1), _p(b1), _p(w2), _p(b2), _p(pooled), _p(pooled_t), _p(l1), _p(l2), N, T, D,
             C1, C2, int(lang_index), _s())
        ctx.save_for_backward(enc, pooled, w1, w2)
        ctx.li = int(lang_index)
        ctx.gb = (_gbuf(w1), _gbuf(b1), _gbuf(w2), _gbuf(b2))
        return l1, l2

    @staticmethod
    @_bw
    def backward(ctx, dl1, dl2):
        enc, pooled, w1, w2 = ctx.saved_tensors
        N, T, D = enc.shape
        C1, C2 = w1.size(0), w2.size(0)
        dev = enc.device
        dl1, dl2 = dl1.contiguous(), dl2.contiguous()
        need = ctx.needs_input_grad
        d_enc = torch.empty_like(enc) if need[0] else None
        # all four into the flat gradient (+=), or all four fresh (=) and handed to autograd
        acc = int(all(g is not None for g in ctx.gb))
        shapes = ((C1, D), (C1,), (C2, D), (C2,))
        outs, rets = [], []
        for k, shp in enumerate(shapes):
            if not need[1 + k]:
                outs.append(None)
                rets.append(None)
            elif acc:
                outs.append(ctx.gb[k])
                rets.append(None)
            else:
                t = torch.empty(shp, device=dev, dtype=torch.float32)
                outs.append(t)
                rets.append(t)
        call("sbl_cls_head_bwd", _p(enc), _p(pooled), _p(dl1), _p(dl2), _p(w1), _p(w2), _p(d_enc), *[_p(t) for t in outs], N, T,
             D, C1, C2, ctx.li, acc, _s())
        return (d_enc,) + tuple(rets) + (None,)


class ClsLossFn(torch.autograd.Function):
    """CE(logits1, tgt1) + lang_weight * CE(logits2, tgt2), CLS/train.py:127-130, with the per-step correct counts of
    :115-121.  Returns (loss, stats[6] = (loss sum, valid rows, correct) per head); only the loss is differentiable."""

    @staticmethod
    def forward(ctx, l1, l2, t1, t2, lang_weight, ignore_id):
        _need_cuda(l1, l2, t1, t2)
        l1, l2 = l1.contiguous(), l2.contiguous()
        t1, t2 = t1.to(torch.int64).contiguous(), t2.to(torch.int64).contiguous()
        (N, C1), C2 = l1.shape, l2.size(1)
        if l2.size(0) != N or t1.numel() != N or t2.numel() != N:
            raise _lib.SblHipError("cls loss: %d rows of logits1, %d of logits2, %d and %d targets" % (N, l2.size(0), t1.numel(), t2.numel()))
        loss = torch.empty((), device=l1.device, dtype=torch.float32)
        stats = torch.empty(6, device=l1.device, dtype=torch.float32)
        call("sbl_cls_loss_fwd", _p(l1), _p(l2), _p(t1), _p(t2), N, C1, C2, float(lang_weight), int(ignore_id), _p(loss),
             _p(stats), _s())
        ctx.save_for_backward(l1, l2, t1, t2, stats)
        ctx.cfg = (float(lang_weight), int(ignore_id))
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)
        return loss, stats

    @staticmethod
    @_bw
    def backward(ctx, gloss, _gs):
        if gloss is None:
            return (None,) * 6
        l1, l2, t1, t2, stats = ctx.saved_tensors
        lw, ignore_id = ctx.cfg
        (N, C1), C2 = l1.shape, l2.size(1)
        gs = gloss.reshape(1).to(torch.float32).contiguous()
        d1, d2 = torch.empty_like(l1), torch.empty_like(l2)
        call("sbl_cls_loss_bwd", _p(l1), _p(l2), _p(t1), _p(t2), _p(stats), _p(gs), _p(d1), _p(d2), N, C1, C2, lw, ignore_id, _s())
        return d1, d2, None, None, None, None


# --------------------------------------------------------------------------- #
# visual frontend
# --------------------------------------------------------------------------- #
# Packed convolution weights.  The state dict keeps OIHW; the kernels read OHWI (forward / weight gradient) and
# [Cin][kh][kw][Cout] (input gradient).  Weights change once per optimizer step, not once per forward, so the two packed
# images of each of the 19 trunk convolutions are kept and re-made only when the weight changed:
#   * torch in-place updates (torch.optim, load_state_dict, copy_) bump `w._version` - or the flat buffer's version when the
#     parameter is a view of a dp.FlatModel - and the next forward re-packs;
#   * writers that bypass torch (FusedAdam's raw kernel on the flat buffer) call refresh_packed_weights(), which re-packs
#     every cached image IN PLACE right away, so hipGraphs captured with the cached images stay valid across optimizer steps.
# A captured graph that is replayed between FOREIGN in-place updates must call refresh_packed_weights() itself.
PACK_CACHE = True
_packed = {}          # id(weight) -> entry
_pack_epoch = [0]


def _pack_key(w):
    fm = getattr(w, "_sbl_flat", None)
    return (w.data_ptr(), w._version, fm.flat_param._version if fm is not None else -1, _pack_epoch[0])


def _pack_entry_alive(e):
    return e["ref"]() is not None


def packed_conv_weight(w, need_dg, stats):
    """(w_ohwi, w_dg) for an OIHW convolution weight; `stats` (fp64, 2*Cout, or None) is zero-filled for the caller either
    by the pack launch (as before) or, on a cache hit, here."""
    Cout, Cin, KH, KW = w.shape
    dev = w.device
    e = _packed.get(id(w)) if PACK_CACHE else None
    if e is not None and (e["ref"]() is not w or e["shape"] != tuple(w.shape)):
        e = None
    if e is not None and e["key"] == _pack_key(w) and (e["dg"] is not None or not need_dg):
        if stats is not None:
            stats.zero_()
        return e["ohwi"], e["dg"]
    w_ohwi = e["ohwi"] if e is not None else torch.empty(Cout, KH, KW, Cin, device=dev, dtype=torch.float32)
    w_dg = e["dg"] if (e is not None and e["dg"] is not None) else (torch.empty(Cin, KH, KW, Cout, device=dev, dtype=torch.float32) if need_dg else None)
    call("sbl_conv_weight_pack", _p(w.detach().contiguous()), _p(w_ohwi), _p(w_dg), Cout, Cin, KH, KW, _p(stats),
         stats.numel() if stats is not None else 0, _s())
    if PACK_CACHE:
        _packed[id(w)] = {"ref": _weakref.ref(w), "shape": tuple(w.shape), "key": _pack_key(w), "ohwi": w_ohwi, "dg": w_dg}
        if len(_packed) > 256:
            for k in [k for k, v in _packed.items() if not _pack_entry_alive(v)]:
                del _packed[k]
    return w_ohwi, w_dg


def refresh_packed_weights():
    """Re-pack every cached image in place from the current weights (current stream).  FusedAdam.step calls it; callers
    that update parameters by other raw kernels, or replay captured graphs between foreign in-place updates, must too."""
    _pack_epoch[0] += 1
    for k, e in list(_packed.items()):
        w = e["ref"]()
        if w is None or not w.is_cuda:
            del _packed[k]
            continue
        Cout, Cin, KH, KW = w.shape
        call("sbl_conv_weight_pack", _p(w.detach().contiguous()), _p(e["ohwi"]), _p(e["dg"]), Cout, Cin, KH, KW, None, 0, _s())
        e["key"] = _pack_key(w)


class StemFn(torch.autograd.Function):
    """frontend3D (video_frontend.py:99-104) on (N,T,H,W) clips -> pooled NHWC (N*T, H/4, W/4, 64).  x: the fp32 clips, or a
    RawClips - the loader's uint8 frames go straight into the convolution's patch staging (sbl_stem_conv_fwd_u8 /
    sbl_stem_wgrad_u8), no fp32 clip is allocated and backward keeps the bytes instead."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, running_mean, running_var, training, momentum, eps, nbt=None):
        """nbt: the BatchNorm's num_batches_tracked (int64 scalar) or None; incremented by the finalize kernel."""
        raw = x if isinstance(x, RawClips) else None
        if raw is None:
            _need_cuda(x, w, gamma, beta)
            x = x.contiguous()
            src, dims = (x,), tuple(x.shape)
        else:
            _need_cuda(*raw.tensors(), w, gamma, beta)
            src, dims = raw.tensors(), raw.src_dims()
        N, T, H, W = dims[0], dims[-3], dims[-2], dims[-1]
        dev = src[0].device
        if training and any(ctx.needs_input_grad):
            zero_pool_reset(dev)          # the step starts here: one memset for every zero-initialised buffer of its backward
        Ho, Wo = H // 2, W // 2
        w2 = w.contiguous().view(64, 245)
        conv = torch.empty(N * T, Ho, Wo, 64, device=dev, dtype=torch.float32)
        stats = torch.empty(128, device=dev, dtype=torch.float64)
        call("sbl_stem_conv_fwd" if raw is None else "sbl_stem_conv_fwd_u8", *[_p(t) for t in src], _p(w2), _p(conv), _p(stats), *dims, _s())
        mean = torch.empty(64, device=dev, dtype=torch.float32)
        invstd = torch.empty(64, device=dev, dtype=torch.float32)
        if training:
            call("sbl_bn_finalize", _p(stats), N * T * Ho * Wo, _p(running_mean), _p(running_var), momentum, eps, _p(mean),
                 _p(invstd), 64, _p(nbt), _s())
        else:
            call("sbl_bn_eval_stats", _p(running_mean), _p(running_var), eps, _p(mean), _p(invstd), 64, _s())
        pooled = torch.empty(N * T, Ho // 2, Wo // 2, 64, device=dev, dtype=torch.float32)
        argmax = torch.empty(N * T, Ho // 2, Wo // 2, 64, device=dev, dtype=torch.uint8)
        call("sbl_stem_bn_relu_pool_fwd", _p(conv), _p(mean), _p(invstd), _p(gamma), _p(beta), _p(pooled), _p(argmax),
             N * T, Ho, Wo, _s())
        ctx.save_for_backward(conv, argmax, mean, invstd, gamma, beta, *src)
        ctx.training, ctx.raw, ctx.dims = training, raw is not None, dims
        return pooled

    @staticmethod
    @_bw
    def backward(ctx, dpooled):
        conv, argmax, mean, invstd, gamma, beta, *src = ctx.saved_tensors
        if not ctx.training:
            raise _lib.SblHipError("stem backward is implemented for training-mode BatchNorm (batch statistics) only")
        dims = ctx.dims
        N, T, H, W = dims[0], dims[-3], dims[-2], dims[-1]
        dev = conv.device
        dpooled = dpooled.contiguous()
        sums = torch.empty(128, device=dev, dtype=torch.float64)
        call("sbl_stem_bwd_reduce", _p(conv), _p(dpooled), _p(argmax), _p(mean), _p(invstd), _p(gamma), _p(beta),
             _p(sums), N * T, H // 2, W // 2, _s())
        dw = torch.empty(64, 245, device=dev, dtype=torch.float32)
        dgamma = torch.empty(64, device=dev, dtype=torch.float32)
        dbeta = torch.empty(64, device=dev, dtype=torch.float32)
        call("sbl_stem_wgrad_u8" if ctx.raw else "sbl_stem_wgrad", *[_p(t) for t in src], _p(conv), _p(dpooled), _p(argmax), _p(mean),
             _p(invstd), _p(gamma), _p(beta), _p(sums), _p(dw), _p(dgamma), _p(dbeta), *dims, _s())
        return None, dw.view(64, 1, 5, 7, 7), dgamma, dbeta, None, None, None, None, None, None


def _dgrad_weight(w, w_dg):
    """The [Cin][kh][kw][Cout] image of an OIHW weight that the input-gradient kernels read: the one forward kept, or packed
    now (forward ran without needing an input gradient)."""
    if w_dg is None:
        Cout, Cin, KH, KW = w.shape
        w_ohwi = torch.empty(Cout, KH, KW, Cin, device=w.device, dtype=torch.float32)
        w_dg = torch.empty(Cin, KH, KW, Cout, device=w.device, dtype=torch.float32)
        call("sbl_conv_weight_pack", _p(w.contiguous()), _p(w_ohwi), _p(w_dg), Cout, Cin, KH, KW, None, 0, _s())
    return w_dg


# --- the ResNet trunk: plain functions over explicit tensors, then one tape node per BasicBlock ---
# One conv -> BatchNorm2d pair of a block: its three differentiable tensors, then what the BN layer keeps and the settings.
ConvBN = _collections.namedtuple("ConvBN", "w gamma beta running_mean running_var nbt stride momentum eps")


def _conv_geom(x, w, stride):
    """The nine integers every trunk convolution entry point takes: NHWC x, OIHW weight, 3x3 pad 1 or 1x1 pad 0."""
    NIMG, H, W, Cin = x.shape
    Cout, _, KH, KW = w.shape
    return NIMG, H, W, Cin, Cout, KH, KW, stride, (1 if KH == 3 else 0)


def conv_bn_fwd(x, c, res, relu, training, need_dg):
    """conv (bias-free) -> BatchNorm2d -> [+ res] -> [ReLU] on NHWC activations; video_frontend.py:28-41,69-71.
    -> (pre-BN output, y, mean, invstd, the weight image the input gradient reads or None).  The BN batch statistics are
    reduced in the conv epilogue; BN side effects (running statistics, c.nbt += 1) like nn.BatchNorm2d."""
    g = _conv_geom(x, c.w, c.stride)
    NIMG, H, W, _, Cout, KH, KW, stride, pad = g
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    dev = x.device
    # packed weight images (OHWI; and [Cin][kh][kw][Cout] for the input gradient, kept for backward): cached across
    # steps, see packed_conv_weight.  The BN statistics the convolution's epilogue accumulates into come zero-filled from
    # the step's pooled memset (or are zeroed by the pack launch / a fill when the pool is not armed).
    # (Measured and not kept in round 2: all 19 packs on the side stream while the stem runs - same-box A/B 32.94 vs
    # 32.72 ms, the fork/join and the contention with the stem cost more than the 10 us per convolution they take off.)
    stats, pooled_stats = _zeros_or_empty(dev, (2 * Cout,), torch.float64) if training else (None, False)
    w_ohwi, w_dg = packed_conv_weight(c.w, training and need_dg, None if pooled_stats else stats)
    conv = torch.empty(NIMG, Ho, Wo, Cout, device=dev, dtype=torch.float32)
    mean = torch.empty(Cout, device=dev, dtype=torch.float32)
    invstd = torch.empty(Cout, device=dev, dtype=torch.float32)
    y = torch.empty_like(conv)
    call("sbl_conv2d_fwd", _p(x), _p(w_ohwi), _p(conv), _p(stats), int(training), *g, _workspace().data_ptr(), WS_BYTES, _s())
    if training:
        # the BatchNorm "finalize" (mean / invstd / running statistics / num_batches_tracked) rides on the apply launch
        call("sbl_bn_apply_fwd_stats", _p(conv), _p(res), _p(stats), NIMG * Ho * Wo, _p(c.running_mean), _p(c.running_var), c.momentum,
             c.eps, _p(c.gamma), _p(c.beta), _p(y), _p(mean), _p(invstd), _p(c.nbt), NIMG * Ho * Wo, Cout, int(relu), _s())
    else:
        call("sbl_bn_eval_stats", _p(c.running_mean), _p(c.running_var), c.eps, _p(mean), _p(invstd), Cout, _s())
        call("sbl_bn_apply_fwd", _p(conv), _p(res), _p(mean), _p(invstd), _p(c.gamma), _p(c.beta), _p(y), NIMG * Ho * Wo, Cout,
             int(relu), _s())
    return conv, y, mean, invstd, w_dg


def bn_bwd_reduce(dy, y, bn):
    """The two fp64 backward sums per channel (sum g, sum g * xhat; g = dy * [y > 0], y None: no ReLU) of bn = (pre-BN
    output, mean, invstd), in a pass of their own: for a BatchNorm nobody's input-gradient epilogue reduced them for."""
    conv, mean, invstd = bn
    Cout = conv.size(-1)
    sums = torch.empty(2 * Cout, device=conv.device, dtype=torch.float64)
    call("sbl_bn_bwd_reduce", _p(dy), _p(y), _p(conv), _p(mean), _p(invstd), _p(sums), conv.numel() // Cout, Cout, int(y is not None),
         _workspace().data_ptr(), WS_BYTES, _s())
    return sums


def bn_bwd_apply(dy, y, bn, gamma, beta, sums, with_res):
    """BatchNorm (+ ReLU when y is given) backward from its sums -> (dconv, the residual branch's gradient or None, dgamma,
    dbeta).  With persistent gradient buffers the kernel adds dgamma / dbeta into them and None goes back to autograd."""
    conv, mean, invstd = bn
    Cout = conv.size(-1)
    dconv = torch.empty_like(conv)
    dres = torch.empty_like(conv) if with_res else None
    dgamma, dbeta = _gbuf(gamma), _gbuf(beta)
    acc = dgamma is not None and dbeta is not None
    if not acc:
        dgamma = torch.empty(Cout, device=conv.device, dtype=torch.float32)
        dbeta = torch.empty(Cout, device=conv.device, dtype=torch.float32)
    call("sbl_bn_bwd_apply", _p(dy), _p(y), _p(conv), _p(mean), _p(invstd), _p(gamma), _p(sums), _p(dconv), _p(dres),
         _p(dgamma), _p(dbeta), conv.numel() // Cout, Cout, int(y is not None), int(acc), _s())
    return (dconv, dres, None, None) if acc else (dconv, dres, dgamma, dbeta)


def conv_dgrad(dconv, w, w_dg, x, stride, addend=None, bn=None, bn_ds=None):
    """Input gradient of a trunk convolution and what rides on its epilogue -> (dx, sums or None).
    bn / bn_ds = (pre-BN output, mean, invstd) of the BatchNorm(s) + ReLU that produced x: their backward sums are
    reduced over the finished dx (2 * Cin fp64 each, bn's first).  addend: added to dx first - the residual branch's
    gradient, or the compact even/even-pixel gradient of a 1x1 / stride-2 shortcut.  Without an addend this is
    sbl_conv2d_dgrad_bnstats, with one sbl_conv2d_dgrad_fused; a block's backward has no use for the plain
    sbl_conv2d_dgrad."""
    Cin = x.size(-1)
    w_dg = _dgrad_weight(w, w_dg)
    dx = torch.empty_like(x)
    n_bn = (bn is not None) + (bn_ds is not None)
    sums, pooled = _zeros_or_empty(x.device, (2 * n_bn * Cin,), torch.float64) if n_bn else (None, False)
    head = (_p(dconv), _p(w_dg), _p(dx), *_conv_geom(x, w, stride), _workspace().data_ptr(), WS_BYTES)
    if addend is None:
        call("sbl_conv2d_dgrad_bnstats", *head, _p(x), *map(_p, bn), _p(sums), int(pooled), _s())
    else:
        call("sbl_conv2d_dgrad_fused", *head, _p(addend), _p(x if n_bn else None), *map(_p, bn or (None,) * 3), *map(_p, bn_ds or (None,) * 3),
             _p(sums), int(pooled), _s())
    return dx, sums


def conv_wgrad(x, dconv, w, stride):
    """Weight gradient of a trunk convolution -> dw (OIHW), or None after adding it into w's persistent gradient buffer.
    The weight gradient is off backward's dependency chain: with a persistent gradient buffer it is issued on the second
    stream, where its workgroups fill the CUs that the chain's kernels (tile-count quantisation: 522 workgroups on 256 CUs)
    leave idle; joined by an end-of-backward engine callback."""
    g = _conv_geom(x, w, stride)
    _, _, _, Cin, Cout, KH, KW, _, _ = g
    dev = x.device

    def launch(dw_ohwi, pooled, target, acc):
        call("sbl_conv2d_wgrad", _p(x), _p(dconv), _p(dw_ohwi), *g, int(pooled), _s())
        call("sbl_conv_wgrad_unpack", _p(dw_ohwi), _p(target), Cout, Cin, KH, KW, acc, _s())

    gw = _gbuf(w)
    if gw is None:
        dw = torch.empty_like(w)
        launch(torch.empty(Cout, KH, KW, Cin, device=dev, dtype=torch.float32), False, dw, 0)
        return dw
    side = side_stream(dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch(*_zeros_or_empty(dev, (Cout, KH, KW, Cin), torch.float32), gw, 1)
    x.record_stream(side)
    dconv.record_stream(side)
    _arm_side_join()
    return None


class BlockHandoff:
    """The one thing two consecutive BasicBlocks share.  It travels with the activation between them, as
    `y._sbl_handoff` on the producer's output, so nn.Sequential stages and forward pre-hooks need not know about it.

    Forward, the producer publishes: `bn2` and `bn_ds` - (pre-BN output, mean, invstd) of its bn2 and of its downsample
    BatchNorm (None without one) - and `act`, the identity of y.
    Backward, the consumer deposits: `sums` - the fp64 backward sums of those BatchNorms (bn2's 2 * C, then the
    downsample's), which its conv1 input-gradient epilogue reduced over its dx - and `dx_ptr`, the identity of that dx.
    The producer's backward takes the sums if its dy is that dx; otherwise (last block, a block on its own, a dy that
    autograd summed from several consumers) it falls back to sbl_bn_bwd_reduce.

    Only the ADDRESS of the activation is kept: the object hangs on y itself, a tensor in it would be a reference cycle
    that only the cyclic GC frees - ~1 GB of trunk activations per step.  take() drops the published tensors, so a
    second backward through the same graph finds nothing here and takes the fallbacks on both sides."""

    __slots__ = ("act", "bn2", "bn_ds", "sums", "dx_ptr")

    def __init__(self):
        self.act = self.bn2 = self.bn_ds = self.sums = self.dx_ptr = None

    def publish(self, y, bn2, bn_ds):
        self.act, self.bn2, self.bn_ds = y.data_ptr(), bn2, bn_ds

    def describes(self, x):
        return self.bn2 is not None and self.act == x.data_ptr()

    def deposit(self, sums, dx):
        self.sums, self.dx_ptr = sums, dx.data_ptr()

    def take(self, dy):
        if self.sums is None or self.dx_ptr != dy.data_ptr():
            return None
        sums = self.sums
        self.__init__()
        return sums


class BlockFn(torch.autograd.Function):
    """A BasicBlock (video_frontend.py:28-41) on NHWC activations as ONE tape node: conv1-bn1-relu, the 1x1 / stride-2
    conv-bn shortcut when there is one, conv2-bn2-(+shortcut)-relu.  Backward is the three convolutions' backward in
    reverse, with every BatchNorm's reduction pass but the last block's bn2 riding on an input-gradient epilogue."""

    @staticmethod
    def forward(ctx, x, prev, pub, c1, c2, ds, training, *params):
        """prev / pub: the BlockHandoff x came with / the one y will carry (None: none).  c1, c2, ds: ConvBN (ds None:
        identity shortcut); params repeats their (w, gamma, beta) so that autograd sees them."""
        _need_cuda(x, *params)
        x = x.contiguous()
        need_dx = ctx.needs_input_grad[0]
        conv1, out, mean1, invstd1, w_dg1 = conv_bn_fwd(x, c1, None, True, training, need_dx)
        res, bn_ds, saved_ds = x, None, ()
        if ds is not None:
            conv_ds, res, mean_ds, invstd_ds, w_dg_ds = conv_bn_fwd(x, ds, None, False, training, need_dx)
            bn_ds, saved_ds = (conv_ds, mean_ds, invstd_ds), (conv_ds, mean_ds, invstd_ds, w_dg_ds)
        need_dout = pub is not None and (need_dx or any(ctx.needs_input_grad[7:10]))       # conv1's output gets a gradient
        conv2, y, mean2, invstd2, w_dg2 = conv_bn_fwd(out, c2, res, True, training, need_dout)
        ctx.save_for_backward(x, conv1, out, mean1, invstd1, w_dg1, conv2, y, mean2, invstd2, w_dg2, *params, *saved_ds)
        ctx.training, ctx.strides, ctx.prev, ctx.pub = training, (c1.stride, ds.stride if ds is not None else None), prev, pub
        if pub is not None:
            pub.publish(y, (conv2, mean2, invstd2), bn_ds)
        return y

    @staticmethod
    @_bw
    def backward(ctx, dy):
        if not ctx.training:
            raise _lib.SblHipError("ConvBN backward is implemented for training-mode BatchNorm only")
        x, conv1, out, mean1, invstd1, w_dg1, conv2, y, mean2, invstd2, w_dg2, *params = ctx.saved_tensors
        w1, gamma1, beta1, w2, gamma2, beta2, *ds = params
        stride1, stride_ds = ctx.strides
        need_dx = ctx.needs_input_grad[0]
        bn1, bn2 = (conv1, mean1, invstd1), (conv2, mean2, invstd2)
        dy = dy.contiguous()
        # conv2 - bn2 - (+ shortcut) - relu.  The next block's conv1 epilogue reduced bn2's and the shortcut BN's sums over
        # dy (its dx, residual included); this one's dgrad epilogue reduces bn1's over dout.
        sums2 = ctx.pub.take(dy) if ctx.pub is not None else None
        sums_ds = None
        if sums2 is None:
            sums2 = bn_bwd_reduce(dy, y, bn2)
        elif ds:
            sums2, sums_ds = sums2[:sums2.numel() // 2], sums2[sums2.numel() // 2:]      # same g, each BN its own xhat
        dconv2, dres, dgamma2, dbeta2 = bn_bwd_apply(dy, y, bn2, gamma2, beta2, sums2, True)
        dout, sums1 = conv_dgrad(dconv2, w2, w_dg2, out, 1, bn=bn1)
        dw2 = conv_wgrad(out, dconv2, w2, 1)
        # the shortcut.  1x1 / stride-2: its input gradient lives on the even/even pixels; conv1's epilogue adds the
        # compact form instead of a zero-filled full-size tensor + an add
        grads_ds, addend = (), dres
        if ds:
            w_ds, gamma_ds, beta_ds, conv_ds, mean_ds, invstd_ds, w_dg_ds = ds
            bn_ds = (conv_ds, mean_ds, invstd_ds)
            if sums_ds is None:
                sums_ds = bn_bwd_reduce(dres, None, bn_ds)
            dconv_ds, _, dgamma_ds, dbeta_ds = bn_bwd_apply(dres, None, bn_ds, gamma_ds, beta_ds, sums_ds, False)
            if need_dx:
                NIMG, H, W, Cin = x.shape
                addend = torch.empty(NIMG, (H + 1) // 2, (W + 1) // 2, Cin, device=x.device, dtype=torch.float32)
                call("sbl_conv1x1s2_dgrad_compact", _p(dconv_ds), _p(_dgrad_weight(w_ds, w_dg_ds)), _p(addend), NIMG, H, W, Cin,
                     w_ds.size(0), _workspace().data_ptr(), WS_BYTES, _s())
            grads_ds = (conv_wgrad(x, dconv_ds, w_ds, stride_ds), dgamma_ds, dbeta_ds)
        # conv1 - bn1 - relu; its epilogue adds the shortcut's gradient and reduces the previous block's sums
        dconv1, _, dgamma1, dbeta1 = bn_bwd_apply(dout, out, bn1, gamma1, beta1, sums1, False)
        dx = None
        if need_dx:
            prev = ctx.prev if ctx.prev is not None and ctx.prev.describes(x) else None
            if prev is None:
                dx, _ = conv_dgrad(dconv1, w1, w_dg1, x, stride1, addend)
            else:
                dx, sums_prev = conv_dgrad(dconv1, w1, w_dg1, x, stride1, addend, prev.bn2, prev.bn_ds)
                prev.deposit(sums_prev, dx)
        dw1 = conv_wgrad(x, dconv1, w1, stride1)
        return (dx, None, None, None, None, None, None, dw1, dgamma1, dbeta1, dw2, dgamma2, dbeta2, *grads_ds)


def basic_block(x, c1, c2, ds, training):
    """BasicBlock forward; c1, c2, ds: ConvBN (ds None: identity shortcut).  Hands the BlockHandoff on from x to y."""
    pub = BlockHandoff() if training and torch.is_grad_enabled() else None
    y = BlockFn.apply(x, getattr(x, "_sbl_handoff", None), pub, c1, c2, ds, training, *c1[:3], *c2[:3], *(ds[:3] if ds is not None else ()))
    if pub is not None:
        y._sbl_handoff = pub
    return y


class AvgPoolFn(torch.autograd.Function):
    """AdaptiveAvgPool2d(1) + view on NHWC; video_frontend.py:87-88."""

    @staticmethod
    def forward(ctx, x):
        _need_cuda(x)
        x = x.contiguous()
        NIMG, H, W, C = x.shape
        y = torch.empty(NIMG, C, device=x.device, dtype=torch.float32)
        call("sbl_avgpool_fwd", _p(x), _p(y), NIMG, H * W, C, _s())
        ctx.shape = x.shape
        return y

    @staticmethod
    @_bw
    def backward(ctx, dy):
        NIMG, H, W, C = ctx.shape
        dy = dy.contiguous()
        dx = torch.empty(ctx.shape, device=dy.device, dtype=torch.float32)
        call("sbl_avgpool_bwd", _p(dy), _p(dx), NIMG, H * W, C, _s())
        return dx


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    """Fused Adam over flat fp32 buffers (SBL/train.py:75; optimizer.py:18-27)."""
    _need_cuda(p, g, m, v)
    call("sbl_adam_step", _p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, step, grad_scale, _s())


# Device-side optimizer step (include/sbl_hip.h): slots of the double[8] state buffer, and the launch geometry
OPT_STATE_SLOTS = 8
OPT_STEP, OPT_SKIPPED, OPT_GRAD_NORM, OPT_CLIP_COEF, OPT_LR, OPT_STEP_SIZE, OPT_INV_SQRT_BC2, OPT_SKIP = range(8)
OPT_MAX_BLOCKS = 2048


def opt_blocks(n):
    """Blocks (= partial sums) one sbl_grad_sumsq / sbl_adam_step_dev launch over n elements uses."""
    return max(1, min(OPT_MAX_BLOCKS, ((n + 3) // 4 + 255) // 256))


def grad_sumsq(g, partials, offset, grad_scale=1.0, clip_value=0.0):
    """Per-block sums of clamp(g * grad_scale, +-clip_value)^2 into partials[offset:]; returns the number written."""
    _need_cuda(g, partials)
    assert g.dtype == torch.float32 and partials.dtype == torch.float64 and g.is_contiguous() and partials.is_contiguous()
    call("sbl_grad_sumsq", _p(g), g.numel(), grad_scale, clip_value, _p(partials), partials.numel(), offset, _s())
    return opt_blocks(g.numel())


def opt_finalize(state, partials, nparts, max_norm=0.0, skip_nonfinite=False, noam=None, beta1=0.9, beta2=0.98):
    """partials[:nparts] -> norm, clip coefficient, and (unless the step is skipped) t, lr and the bias corrections."""
    _need_cuda(state, partials)
    assert state.dtype == torch.float64 and state.numel() == OPT_STATE_SLOTS and state.is_contiguous()
    assert partials.dtype == torch.float64 and 0 < nparts <= partials.numel()
    k, warmup = noam if noam is not None else (0.0, 0.0)
    call("sbl_opt_finalize", _p(state), _p(partials), nparts, max_norm, int(skip_nonfinite), k, warmup, beta1, beta2, _s())


def adam_step_dev(p, g, m, v, state, beta1, beta2, eps, grad_scale=1.0, clip_value=0.0):
    """Fused Adam over flat fp32 buffers with clip coefficient, step size, bias factor and skip flag read from `state`."""
    _need_cuda(p, g, m, v, state)
    assert state.dtype == torch.float64 and state.numel() == OPT_STATE_SLOTS
    assert g.numel() == m.numel() == v.numel() == p.numel()
    call("sbl_adam_step_dev", _p(p), _p(g), _p(m), _p(v), p.numel(), _p(state), beta1, beta2, eps, grad_scale, clip_value, _s())


def adam_ema_step_dev(p, g, m, v, e, state, beta1, beta2, eps, grad_scale=1.0, clip_value=0.0, ema_decay=0.9999, ema_warmup=True):
    """adam_step_dev plus, in the same launch, e += w * (p_new - e) with w = 1 - d_t derived from state[OPT_STEP]: d_t =
    min(ema_decay, (1 + t) / (10 + t)) under warm-up, else ema_decay.  A skipped step leaves e alone too."""
    _need_cuda(p, g, m, v, e, state)
    assert state.dtype == torch.float64 and state.numel() == OPT_STATE_SLOTS
    assert g.numel() == m.numel() == v.numel() == e.numel() == p.numel()
    call("sbl_adam_ema_step_dev", _p(p), _p(g), _p(m), _p(v), _p(e), p.numel(), _p(state), beta1, beta2, eps, grad_scale,
         clip_value, ema_decay, int(bool(ema_warmup)), _s())


def swap_(a, b):
    """Exchange the contents of two non-overlapping contiguous fp32 buffers in place (exact; one launch, no scratch)."""
    _need_cuda(a, b)
    assert a.dtype == b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous() and a.numel() == b.numel()
    call("sbl_swap_f32", _p(a), _p(b), a.numel(), _s())


_LUT = {}


def _lut(dev, mean, std):
    """The 256-entry normalisation table of a device, cached: float32((v/255. - mean)/std) in double, exactly the reference's
    numpy arithmetic.  Its first use on a device copies from the host, so it must not fall inside a graph capture."""
    key = (dev.index, mean, std)
    lut = _LUT.get(key)
    if lut is None:
        lut = _LUT[key] = torch.from_numpy(((_np.arange(256, dtype=_np.float64) / 255. - mean) / std).astype(_np.float32)).to(dev)
    return lut


class RawClips:
    """A batch of clips as the loader holds it: uint8 frames plus what SBL/data_gen.py:276-296 and cvtransforms.py:7-48 would do
    to them - the arguments of preprocess_clips, kept together.  StemFn and the models (Lipreading / Transformer.forward /
    recognize / validate, ClassifierTransformer.forward) take one wherever they take the (N,T,H,W) float clips; the stem then
    reads the bytes directly and the float clips are never built.  Immutable; the tensors may be overwritten in place (the
    static inputs of a captured graph).

    frames_u8 (N,Tin,Hin,Win) uint8; y1, x1, flip int32 (N,): crop origin and horizontal-flip flag per clip; src_frame int32
    (N,Tout): the source frame of every output frame, -1 = an all-zero frame (frame removal, padding to 30 frames, the CLS
    loader's 31st frame); crop = (Hc,Wc); mean / std of ColorNormalize.  All contiguous, all on one device.  While the index
    tensors are on the host their ranges are checked (0 <= y1, y1 + Hc <= Hin, likewise x, src_frame < Tin); device tensors
    are not read back - an index that leaves the frames reads as zero in the kernels."""
    __slots__ = ("frames_u8", "y1", "x1", "flip", "src_frame", "crop", "mean", "std", "_lut")

    def __init__(self, frames_u8, y1, x1, flip, src_frame, crop=(88, 88), mean=0.413621, std=0.1700239):
        def want(name, t, dtype, shape):
            if not isinstance(t, torch.Tensor) or t.dtype != dtype:
                raise TypeError("RawClips: %s must be a %s tensor (got %s)" % (name, dtype, getattr(t, "dtype", type(t).__name__)))
            if t.dim() != len(shape) or any(d is not None and t.size(i) != d for i, d in enumerate(shape)):
                raise ValueError("RawClips: %s must have shape (%s), got %s" % (name, ", ".join("*" if d is None else str(d) for d in shape), tuple(t.shape)))
            if not t.is_contiguous():
                raise ValueError("RawClips: %s must be contiguous" % name)
            if t.device != frames_u8.device:
                raise ValueError("RawClips: %s is on %s, the frames on %s" % (name, t.device, frames_u8.device))
        want("frames_u8", frames_u8, torch.uint8, (None, None, None, None))
        N, Tin, Hin, Win = frames_u8.shape
        for name, t in (("y1", y1), ("x1", x1), ("flip", flip)):
            want(name, t, torch.int32, (N,))
        want("src_frame", src_frame, torch.int32, (N, None))
        Hc, Wc = int(crop[0]), int(crop[1])
        if not (0 < Hc <= Hin and 0 < Wc <= Win and src_frame.size(1) > 0):
            raise ValueError("RawClips: crop %dx%d of %dx%d frames, %d output frames" % (Hc, Wc, Hin, Win, src_frame.size(1)))
        if not frames_u8.is_cuda:      # host tensors: a range check costs nothing (on the device it would be a sync)
            if N and (int(y1.min()) < 0 or int(y1.max()) + Hc > Hin):
                raise ValueError("RawClips: y1 outside [0, %d]" % (Hin - Hc))
            if N and (int(x1.min()) < 0 or int(x1.max()) + Wc > Win):
                raise ValueError("RawClips: x1 outside [0, %d]" % (Win - Wc))
            if N and int(src_frame.max()) >= Tin:
                raise ValueError("RawClips: src_frame >= Tin = %d" % Tin)
        for k, v in (("frames_u8", frames_u8), ("y1", y1), ("x1", x1), ("flip", flip), ("src_frame", src_frame), ("crop", (Hc, Wc)),
                     ("mean", float(mean)), ("std", float(std)),
                     ("_lut", _lut(frames_u8.device, float(mean), float(std)) if frames_u8.is_cuda else None)):
            object.__setattr__(self, k, v)

    def __setattr__(self, name, value):
        raise AttributeError("RawClips is immutable")

    @property
    def shape(self):
        """The logical clip shape (N,Tout,Hc,Wc)."""
        return torch.Size((self.frames_u8.size(0), self.src_frame.size(1)) + self.crop)

    @property
    def device(self):
        return self.frames_u8.device

    def dim(self):
        return 4

    def size(self, i=None):
        return self.shape if i is None else self.shape[i]

    def to(self, device):
        return RawClips(*(t.to(device) for t in (self.frames_u8, self.y1, self.x1, self.flip, self.src_frame)), crop=self.crop,
                        mean=self.mean, std=self.std)

    def tensors(self):
        """The six source arguments of sbl_stem_conv_fwd_u8 / sbl_stem_wgrad_u8, in order."""
        _need_cuda(self.frames_u8)
        return (self.frames_u8, self._lut, self.y1, self.x1, self.flip, self.src_frame)

    def src_dims(self):
        """(N, Tin, Hin, Win, Tout, Hc, Wc)"""
        return tuple(self.frames_u8.shape) + (self.src_frame.size(1),) + self.crop

    def materialize(self):
        """The fp32 clips (N,Tout,Hc,Wc) that preprocess_clips builds from the same arguments."""
        return preprocess_clips(self.frames_u8, self.y1, self.x1, self.flip, self.src_frame, Tout=self.src_frame.size(1),
                                crop=self.crop, mean=self.mean, std=self.std)


def preprocess_clips(frames_u8, y1, x1, flip, src_frame, Tout=30, crop=(88, 88), mean=0.413621, std=0.1700239):
    """Device input pipeline (SBL/data_gen.py:276-296 + cvtransforms.py): uint8 (N,Tin,Hin,Win) grayscale frames ->
    normalised, cropped, flipped, frame-mapped, zero-padded fp32 clips (N,Tout,Hc,Wc) in one kernel.  y1/x1/flip:
    int32 (N,) device tensors; src_frame: int32 (N,Tout), -1 = zero frame."""
    _need_cuda(frames_u8, y1, x1, flip, src_frame)
    assert frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous()
    N, Tin, Hin, Win = frames_u8.shape
    lut = _lut(frames_u8.device, mean, std)
    out = torch.empty(N, Tout, crop[0], crop[1], device=frames_u8.device, dtype=torch.float32)
    call("sbl_preprocess_clips", _p(frames_u8), _p(out), _p(lut), _p(y1.contiguous()), _p(x1.contiguous()), _p(flip.contiguous()),
         _p(src_frame.contiguous()), N, Tin, Hin, Win, Tout, crop[0], crop[1], _s())
    return out


# --------------------------------------------------------------------------- #
# validation scoring (sbl_seq_score)
# --------------------------------------------------------------------------- #
SCORE_COUNTERS = 37          # include/sbl_hip.h, SBL_SCORE_*: the counters of one direction
SCORE_N_SCORED, SCORE_N_EMPTY, SCORE_N_WORD_ERR, SCORE_SUM_DIST, SCORE_SUM_LEN = range(5)
SCORE_DIST_BY_LEN, SCORE_COUNT_BY_LEN = 5, 21
SCORE_MAX_TO, SCORE_WINDOW = 15, 16


def pack_names(names):
    """The name table of sbl_seq_score from a list of `vocab` short strings (one per token id): int64 (vocab,) CPU tensor,
    entry = length << 56 | the characters as a big-endian integer.  Checked here, on the host: ASCII without NUL, at most
    7 bytes each."""
    words = []
    for i, s in enumerate(names):
        try:
            b = s.encode("ascii")
        except (UnicodeEncodeError, AttributeError):
            raise ValueError("name %d (%r) is not an ASCII string" % (i, s))
        if len(b) > 7 or 0 in b:
            raise ValueError("name %d (%r): at most 7 bytes, none of them NUL" % (i, s))
        words.append(len(b) << 56 | int.from_bytes(b, "big"))
    if not words:
        raise ValueError("empty name table")
    return torch.tensor(words, dtype=torch.int64)


def _spelling_cpu(tok, kept, names):
    """(N, 112) uint8: the concatenated spelling of the kept ids of every row, zero padded (torch form of the kernel's rule:
    an id outside the table spells nothing)."""
    N, Wd = tok.shape
    inside = kept & (tok >= 0) & (tok < names.numel())
    w = names[torch.where(inside, tok, torch.zeros_like(tok))]
    length = torch.where(inside, (w >> 56) & 7, torch.zeros_like(w))
    q = torch.arange(7)
    ch = (w.unsqueeze(2) >> (8 * (length.unsqueeze(2) - 1 - q)).clamp(min=0)) & 0xFF      # (N, Wd, 7): character q
    valid = (q < length.unsqueeze(2)).reshape(N, Wd * 7)
    order = torch.argsort((~valid).to(torch.int8), dim=1, stable=True)                    # stable compaction to the left
    out = torch.gather(torch.where(valid, ch.reshape(N, Wd * 7), torch.zeros((), dtype=torch.int64)), 1, order)
    pad = out.new_zeros(N, SCORE_WINDOW * 7)
    pad[:, :Wd * 7] = out
    return pad.to(torch.uint8)


def _seq_score_cpu(ys, gold, sos, eos, ignore, names):
    """(dist, c, word_err) int64 (N,) of one direction: the definition of sbl_seq_score in vectorised torch (the kernel's
    dynamic program: stripped target entries are transparent columns, stripped predictions leave the row unchanged)."""
    N, To = gold.shape
    p = ys[:, :SCORE_WINDOW]
    gk = (gold != sos) & (gold != eos) & (gold != ignore)
    c = gk.sum(1)
    pk = (p != sos) & (p != eos) & (p != ignore) & (torch.arange(p.size(1)).unsqueeze(0) <= c.unsqueeze(1))
    D = torch.cat([c.new_zeros(N, 1), gk.cumsum(1)], 1)
    for i in range(p.size(1)):
        cols = [D[:, 0] + 1]
        for j in range(1, To + 1):
            cell = torch.minimum(torch.minimum(D[:, j], cols[-1]) + 1, D[:, j - 1] + (p[:, i] != gold[:, j - 1]).long())
            cols.append(torch.where(gk[:, j - 1], cell, cols[-1]))
        D = torch.where(pk[:, i:i + 1], torch.stack(cols, 1), D)
    dist = D[:, To]
    if names is None:
        werr = (dist != 0).long()
    else:
        werr = (_spelling_cpu(p, pk, names) != _spelling_cpu(gold, gk, names)).any(1).long()
    return dist, c, werr


def seq_score(ys_l2r, ys_r2l, gold_l2r, gold_r2l, acc, sos_id, eos_id, ignore_id, names=None, valid_rows=None, per_sample=None):
    """Score one batch of greedy decodes against its targets, both directions, and ADD the counters to `acc`
    (include/sbl_hip.h, sbl_seq_score: the definition, the reference lines and the three deviations).
    ys_*: int64 (N, Ly) rows of Transformer.recognize; gold_*: int64 (N, To <= 15) IGNORE_ID-padded targets; acc: int64
    (2, SCORE_COUNTERS); names: None or the int64 table of pack_names on the same device; valid_rows: None or int32[1] (rows
    at or beyond it are ignored); per_sample: None or int32 (2, 3, N), filled with dist / c / word_err per direction.
    On the GPU: one launch, no sync, no allocation.  CPU tensors take the same definition in vectorised torch, so that it can
    be pinned without a GPU; that is not a fallback of the GPU path, which raises without the library.  Returns acc."""
    N, Ly = ys_l2r.shape
    To = gold_l2r.size(1)
    toks = (ys_l2r, ys_r2l, gold_l2r, gold_r2l)
    if ys_r2l.shape != (N, Ly) or gold_l2r.shape != (N, To) or gold_r2l.shape != (N, To):
        raise ValueError("seq_score: shapes %s" % ([tuple(t.shape) for t in toks],))
    if not all(t.dtype == torch.int64 and t.is_contiguous() for t in toks):
        raise ValueError("seq_score: token tensors must be contiguous int64")
    if acc.shape != (2, SCORE_COUNTERS) or acc.dtype != torch.int64 or not acc.is_contiguous():
        raise ValueError("seq_score: acc must be a contiguous int64 (2, %d) tensor" % SCORE_COUNTERS)
    if names is not None and (names.dtype != torch.int64 or names.dim() != 1 or names.numel() < 1 or not names.is_contiguous()):
        raise ValueError("seq_score: names must be the int64 table of pack_names")
    if valid_rows is not None and (valid_rows.dtype != torch.int32 or valid_rows.numel() != 1):
        raise ValueError("seq_score: valid_rows must be an int32[1] tensor")
    if per_sample is not None and (per_sample.shape != (2, 3, N) or per_sample.dtype != torch.int32 or not per_sample.is_contiguous()):
        raise ValueError("seq_score: per_sample must be a contiguous int32 (2, 3, %d) tensor" % N)
    every = toks + (acc,) + tuple(t for t in (names, valid_rows, per_sample) if t is not None)
    if any(t.device != acc.device for t in every):
        raise ValueError("seq_score: tensors on different devices")
    if acc.is_cuda:
        call("sbl_seq_score", _p(ys_l2r), _p(ys_r2l), Ly, _p(gold_l2r), _p(gold_r2l), To, N, sos_id, eos_id, ignore_id, _p(names),
             0 if names is None else names.numel(), _p(valid_rows), _p(per_sample), _p(acc), _s())
        return acc
    if not 1 <= To <= SCORE_MAX_TO:
        raise ValueError("seq_score: target width To=%d outside 1..%d" % (To, SCORE_MAX_TO))
    live = torch.arange(N) < (N if valid_rows is None else min(max(int(valid_rows[0]), 0), N))
    for d, (ys, gold) in enumerate(((ys_l2r, gold_l2r), (ys_r2l, gold_r2l))):
        _score_accumulate_cpu(acc[d], None if per_sample is None else per_sample[d], live,
                              *_seq_score_cpu(ys, gold, sos_id, eos_id, ignore_id, names))
    return acc


def _score_accumulate_cpu(a, per, live, dist, c, werr):
    """Add one direction's per-sample (dist, c, word_err) to its counter row `a` (and write them to `per`, int32 (3, N))."""
    if per is not None:
        per.copy_(torch.where(live, torch.stack((dist, c, werr)), torch.full((), -1, dtype=torch.int64)).to(torch.int32))
    scored = live & (c > 0)
    a[SCORE_N_SCORED] += scored.sum()
    a[SCORE_N_EMPTY] += (live & (c == 0)).sum()
    a[SCORE_N_WORD_ERR] += werr[scored].sum()
    a[SCORE_SUM_DIST] += dist[scored].sum()
    a[SCORE_SUM_LEN] += c[scored].sum()
    a[SCORE_DIST_BY_LEN:SCORE_DIST_BY_LEN + 16].index_add_(0, c[scored], dist[scored])
    a[SCORE_COUNT_BY_LEN:SCORE_COUNT_BY_LEN + 16].index_add_(0, c[scored], torch.ones_like(c[scored]))


def seq_score1(ys, gold, acc, sos_id, eos_id, ignore_id, names=None, valid_rows=None, per_sample=None):
    """seq_score for ONE direction (include/sbl_hip.h, sbl_seq_score1; the single-direction model, LRW/train.py:245-260).
    ys int64 (N, Ly), gold int64 (N, To <= 15), acc int64 (SCORE_COUNTERS,), per_sample None or int32 (3, N).  On the GPU one
    launch, no sync, no allocation; CPU tensors take the same definition in vectorised torch.  Returns acc."""
    N, Ly = ys.shape
    To = gold.size(1)
    if gold.shape != (N, To) or not all(t.dtype == torch.int64 and t.is_contiguous() for t in (ys, gold)):
        raise ValueError("seq_score1: ys / gold must be contiguous int64 (N, Ly) / (N, To), got %s %s" % (tuple(ys.shape), tuple(gold.shape)))
    if acc.shape != (SCORE_COUNTERS,) or acc.dtype != torch.int64 or not acc.is_contiguous():
        raise ValueError("seq_score1: acc must be a contiguous int64 (%d,) tensor" % SCORE_COUNTERS)
    if names is not None and (names.dtype != torch.int64 or names.dim() != 1 or names.numel() < 1 or not names.is_contiguous()):
        raise ValueError("seq_score1: names must be the int64 table of pack_names")
    if valid_rows is not None and (valid_rows.dtype != torch.int32 or valid_rows.numel() != 1):
        raise ValueError("seq_score1: valid_rows must be an int32[1] tensor")
    if per_sample is not None and (per_sample.shape != (3, N) or per_sample.dtype != torch.int32 or not per_sample.is_contiguous()):
        raise ValueError("seq_score1: per_sample must be a contiguous int32 (3, %d) tensor" % N)
    every = (ys, gold, acc) + tuple(t for t in (names, valid_rows, per_sample) if t is not None)
    if any(t.device != acc.device for t in every):
        raise ValueError("seq_score1: tensors on different devices")
    if acc.is_cuda:
        call("sbl_seq_score1", _p(ys), Ly, _p(gold), To, N, sos_id, eos_id, ignore_id, _p(names),
             0 if names is None else names.numel(), _p(valid_rows), _p(per_sample), _p(acc), _s())
        return acc
    if not 1 <= To <= SCORE_MAX_TO:
        raise ValueError("seq_score1: target width To=%d outside 1..%d" % (To, SCORE_MAX_TO))
    live = torch.arange(N) < (N if valid_rows is None else min(max(int(valid_rows[0]), 0), N))
    _score_accumulate_cpu(acc, per_sample, live, *_seq_score_cpu(ys, gold, sos_id, eos_id, ignore_id, names))
    return acc


# --------------------------------------------------------------------------- #
# single-direction seq2seq decoder (LRW/transformer/decoder.py): scaled embedding, KV-cached greedy step
# --------------------------------------------------------------------------- #
class EmbedScalePEFn(torch.autograd.Function):
    """emb[tok] * scale + pe[:L]; LRW/transformer/decoder.py:111-112.  tok: int64 (B, L) (any row stride).  The gradient of
    `emb` is the scatter-add of scale * dy; when `emb` is also the output projection's weight (tgt_emb_prj_weight_sharing)
    autograd - or the shared flat gradient slice both kernels accumulate into - sums it with the projection's."""

    @staticmethod
    def forward(ctx, tok, emb, pe, scale):
        _need_cuda(tok, emb, pe)
        B, L = tok.shape
        V, D = emb.shape
        assert tok.dtype == torch.int64 and tok.stride(1) == 1 and pe.size(0) >= L and pe.is_contiguous() and emb.is_contiguous()
        out = torch.empty(B, L, D, device=emb.device, dtype=torch.float32)
        call("sbl_embed_scale_pe_fwd", _p(tok), tok.stride(0), _p(emb), _p(pe), _p(out), B, L, D, V, scale, 0, _s())
        ctx.tok, ctx.cfg = tok, (B, L, V, D, scale)
        ctx.gb = _gbuf(emb)
        return out

    @staticmethod
    @_bw
    def backward(ctx, dy):
        B, L, V, D, scale = ctx.cfg
        dy = dy.contiguous()
        demb, _, demb_ret = _target(ctx.gb, (V, D), dy.device, zero=True)
        call("sbl_embed_scale_bwd", _p(ctx.tok), ctx.tok.stride(0), _p(dy), _p(demb), B, L, D, V, scale, _s())
        return None, demb_ret, None, None


def _attn_step(q, k_new, v_new, k_cache, v_cache, Lcap, anc, out, W, H, n_prev, append, scale, kv_len=None):
    """The stride checks and the call behind decode_attn_step (W = None: every row owns its cache) and beam_attn_step.
    kv_len: None, or the device int32 key counts of the K/V entries (cross-attention only): the `_len` entries."""
    if kv_len is not None and append:
        raise _lib.SblHipError("decode / beam_attn_step: key counts go with the cross-attention (append = 0) only")
    S = q.size(0)
    ldc = k_cache.stride(-2)
    nc = S if append or W is None else S // W
    assert v_cache.stride(-2) == ldc and k_cache.stride(-1) == 1 and q.stride(1) == 1 and out.stride(1) == 1
    assert k_cache.dim() == 3 and k_cache.size(0) == nc and k_cache.size(1) == Lcap and k_cache.stride(0) == Lcap * ldc
    assert v_cache.shape == k_cache.shape and v_cache.stride(0) == Lcap * ldc and out.size(0) == S
    if append:
        assert k_new.stride(0) == v_new.stride(0) and k_new.stride(1) == 1 and v_new.stride(1) == 1
    head = (_p(q), q.stride(0), _p(k_new), _p(v_new), k_new.stride(0) if append else 0, _p(k_cache), _p(v_cache), ldc, Lcap)
    tail = (H, int(n_prev), int(bool(append)), scale)
    name, end = ("sbl_decode_attn_step", "sbl_beam_attn_step"), (_s(),)
    if kv_len is not None:
        name, end = (name[0] + "_len", name[1] + "_len"), (_counts(kv_len, nc, "kv_len"), _s())
    if W is None:
        call(name[0], *head, _p(out), out.stride(0), S, *tail, *end)
    else:
        if append:
            assert anc.dtype == torch.int32 and anc.dim() == 2 and anc.size(0) == S and anc.stride(1) == 1
        call(name[1], *head, _p(anc) if append else None, anc.stride(0) if append else 0, _p(out), out.stride(0), S,
             int(W), *tail, *end)
    return out


def decode_attn_step(q, k_new, v_new, k_cache, v_cache, Lcap, out, H, n_prev, append, scale=0.125, kv_len=None):
    """One (clip, head) wavefront each: the single new query row attends to the cache (include/sbl_hip.h,
    sbl_decode_attn_step).  q / k_new / v_new / out: (B, H*64) row views (column slices of wider buffers are fine);
    k_cache / v_cache: views whose first element is row 0 of clip 0, row stride .stride(-2), batch stride Lcap rows.
    kv_len (append = 0 only): None, or a device int32 (B,) tensor - clip b then sees the keys j < min(max(kv_len[b], 0),
    n_prev) and a clip without a visible key gets o = 0 (sbl_decode_attn_step_len)."""
    return _attn_step(q, k_new, v_new, k_cache, v_cache, Lcap, None, out, None, H, n_prev, append, scale, kv_len)


def decode_tail(y, w, ys, step, emb, pe, emb_scale, x_next=None, logits=None):
    """Greedy step tail in one launch (sbl_decode_tail): ys[:, step+1] = argmax(y w^T); x_next = emb[token] * emb_scale +
    pe[step+1] (the next step's input row) when given; logits (B, V) are written when given."""
    B, D = y.shape
    V = w.size(0)
    assert y.stride(1) == 1 and w.is_contiguous() and ys.dtype == torch.int64 and ys.stride(1) == 1
    assert x_next is None or (x_next.is_contiguous() and x_next.shape == (B, D) and pe.is_contiguous() and emb.is_contiguous())
    call("sbl_decode_tail", _p(y), y.stride(0), _p(w), _p(logits), 0 if logits is None else logits.stride(0), _p(ys), ys.stride(0),
         int(step), _p(emb), _p(pe), pe.size(0), emb_scale, _p(x_next), B, V, D, _s())


def beam_attn_step(q, k_new, v_new, k_cache, v_cache, Lcap, anc, out, W, H, n_prev, append, scale=0.125, kv_len=None):
    """decode_attn_step for beam slots (include/sbl_hip.h, sbl_beam_attn_step): q / k_new / v_new / out are (S, H*64) row views,
    S = clips * W.  append: k_cache / v_cache (S, Lcap, H*64) and anc (S, >= n_prev) int32 names the cache slot of every key;
    otherwise (cross-attention) k_cache / v_cache hold S / W clips and anc is None.  kv_len (append = 0 only): None, or the
    device int32 (S / W,) key counts of the clips (sbl_beam_attn_step_len)."""
    return _attn_step(q, k_new, v_new, k_cache, v_cache, Lcap, anc, out, W, H, n_prev, append, scale, kv_len)


class BeamState(object):
    """The device buffers of one beam search over N clips with W slots each (include/sbl_hip.h, sbl_beam_tail): allocated
    once per call; reset() restores the start (one hypothesis <sos> of score 0 per clip) with fill launches only.
    lex=True adds `node` (N, W) int32, the slots' trie nodes of the lexicon-constrained search (sbl_beam_tail_lex); reset()
    puts every slot at the root."""

    def __init__(self, N, W, maxlen, sos_id, device, lex=False):
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)      # noqa: E731
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=device)    # noqa: E731
        self.N, self.W, self.maxlen, self.sos_id = N, W, maxlen, sos_id
        self.score, self.last_tok = f32(N, W), i32(N, W)
        self.anc = i32(2, N * W, maxlen)
        self.hist_tok, self.hist_par, self.hist_flag = i32(N, maxlen, W), i32(N, maxlen, W), i32(N, maxlen, W)
        self.hist_score = f32(N, maxlen, W)
        self.end_score, self.end_ref, self.end_count = f32(N, W * maxlen), i32(N, W * maxlen), i32(N)
        self.node = i32(N, W) if lex else None
        self.reset()

    def reset(self):
        self.score.fill_(float("-inf"))
        self.score[:, 0] = 0.0
        self.last_tok.fill_(self.sos_id)
        if self.node is not None:
            self.node.zero_()

    def history(self):
        return self.hist_tok, self.hist_par, self.hist_score, self.hist_flag


def beam_tail(y, w, log_prior, st, step, eos_id, emb, pe, emb_scale, x_next=None, trie=None, clip_steps=None):
    """Tail of beam step `step` in one launch (sbl_beam_tail) on the rows y (N*W, 512): the best W candidates of every clip
    into the BeamState `st` (ancestry buffer step % 2 is read, the other one written), x_next = the next input rows.
    trie: None, or the (mask, first, word) tables of Lexicon.trie() - then the launch is sbl_beam_tail_lex, a candidate exists
    only where the slot's node st.node allows its token, and st.node is updated in place (st needs lex=True).
    clip_steps (without a trie): None, or the device int32 (N,) step counts of the clips - every kept hypothesis of clip n then
    ends at step clamp(clip_steps[n], 1, maxlen) - 1 (sbl_beam_tail_len)."""
    S, D = y.shape
    V = w.size(0)
    if trie is not None and clip_steps is not None:
        raise _lib.SblHipError("beam_tail: the lexicon search's step count does not depend on the clip (no clip_steps with a trie)")
    assert S == st.N * st.W and y.stride(1) == 1 and w.is_contiguous()
    assert log_prior is None or (log_prior.dtype == torch.float32 and log_prior.shape == (V, V) and log_prior.is_contiguous())
    assert x_next is None or (x_next.is_contiguous() and x_next.shape == (S, D) and pe.is_contiguous() and emb.is_contiguous())
    args = (_p(y), y.stride(0), _p(w), _p(log_prior), _p(st.score), _p(st.last_tok), _p(st.anc[step % 2]),
            _p(st.anc[1 - step % 2]), st.anc.stride(1), _p(st.hist_tok), _p(st.hist_par), _p(st.hist_score), _p(st.hist_flag),
            _p(st.end_score), _p(st.end_ref), _p(st.end_count), int(step), st.maxlen, int(eos_id), _p(emb), _p(pe), pe.size(0),
            emb_scale, _p(x_next), st.N, st.W, V, D)
    if clip_steps is not None:
        call("sbl_beam_tail_len", *args, _counts(clip_steps, st.N, "clip_steps"), _s())
        return
    if trie is None:
        call("sbl_beam_tail", *args, _s())
        return
    mask, first = trie[0], trie[1]
    if st.node is None:
        raise _lib.SblHipError("beam_tail: a trie needs a BeamState with a node buffer (lex=True)")
    _check_trie(mask, first, None, y.device)
    call("sbl_beam_tail_lex", *args, _p(mask), _p(first), mask.numel(), _p(st.node), _s())


def beam_finish(st, nbest, eos_id, clip_steps=None):
    """(yseq (N, nbest, maxlen+2) int64, lengths (N, nbest) int32, scores (N, nbest), n_hyps (N) int32): sbl_beam_finish.
    clip_steps: None, or the array beam_tail was given - a hypothesis that ended at clip n's last step then has length
    clip_steps[n] + 2 (sbl_beam_finish_len)."""
    dev = st.score.device
    yseq = torch.empty(st.N, nbest, st.maxlen + 2, dtype=torch.int64, device=dev)
    lengths = torch.empty(st.N, nbest, dtype=torch.int32, device=dev)
    scores = torch.empty(st.N, nbest, dtype=torch.float32, device=dev)
    n_hyps = torch.empty(st.N, dtype=torch.int32, device=dev)
    args = (_p(st.end_score), _p(st.end_ref), _p(st.end_count), _p(st.hist_tok), _p(st.hist_par), _p(yseq), _p(lengths), _p(scores),
            _p(n_hyps), st.N, st.W, st.maxlen, int(nbest), int(st.sos_id), int(eos_id))
    if clip_steps is None:
        call("sbl_beam_finish", *args, _s())
    else:
        call("sbl_beam_finish_len", *args, _counts(clip_steps, st.N, "clip_steps"), _s())
    return yseq, lengths, scores, n_hyps


class PairBeamState(object):
    """The device buffers of one beam search of the bidirectional SBL decoder over N clips with W slots each
    (include/sbl_hip.h, sbl_pair_beam_tail): total and per-direction scores, the two double-buffered prefix tables
    ys[d][k] (N*W, maxlen+1) int64 - step i reads k = i % 2 and writes the other - and the (N, maxlen, W) history.
    Allocated once per call; reset() restores the start (every prefix <sos>, slot 0 of every clip at score 0, the other
    slots dead) with fill launches only.
    lex=True adds the node buffers of the lexicon-constrained search (sbl_pair_beam_tail_lex): `node` (2, N, W) int32,
    double-buffered like the prefixes, and `hist_node` (N, maxlen, W); reset() puts every slot at the root.  row_len (>=
    maxlen + 1) widens the prefix rows: that search runs maxlen = Cmax + 1 steps on the 17-entry rows the decoder stage reads,
    and the entries behind maxlen keep reset()'s <eos>."""

    def __init__(self, N, W, maxlen, sos_id, eos_id, device, lex=False, row_len=None):
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)      # noqa: E731
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=device)    # noqa: E731
        self.N, self.W, self.maxlen, self.sos_id, self.eos_id = N, W, maxlen, sos_id, eos_id
        row_len = maxlen + 1 if row_len is None else int(row_len)
        if row_len < maxlen + 1:
            raise ValueError("PairBeamState: prefix rows of %d entries for maxlen = %d (+1)" % (row_len, maxlen))
        self.score, self.score_dir = f32(N, W), f32(N, W, 2)
        self.ys = torch.empty(2, 2, N * W, row_len, dtype=torch.int64, device=device)      # [direction][buffer]
        self.hist_tok_l, self.hist_tok_r, self.hist_par = i32(N, maxlen, W), i32(N, maxlen, W), i32(N, maxlen, W)
        self.hist_score = f32(N, maxlen, W)
        self.node, self.hist_node = (i32(2, N, W), i32(N, maxlen, W)) if lex else (None, None)
        self.reset()

    def reset(self):
        self.score.fill_(float("-inf"))
        self.score[:, 0] = 0.0
        self.score_dir.fill_(float("-inf"))
        self.score_dir[:, 0] = 0.0
        self.ys.fill_(self.eos_id)
        self.ys[:, :, :, 0] = self.sos_id
        if self.node is not None:
            self.node.zero_()

    def nodes(self, step):
        """The (N, W) trie nodes that step `step` reads (lex=True): what step - 1 wrote."""
        return self.node[step % 2]

    def prefixes(self, step):
        """(l2r, r2l) prefix tables that step `step` reads: what step - 1 wrote."""
        return self.ys[0, step % 2], self.ys[1, step % 2]

    def history(self):
        return self.hist_tok_l, self.hist_tok_r, self.hist_par, self.hist_score


def _pair_beam_tail(y_l, y_r, w_l, w_r, st, step, pair_trie):
    """The shape checks and the call behind pair_beam_tail (pair_trie = None) and pair_beam_tail_lex."""
    S, D = y_l.shape
    V = w_l.size(0)
    assert S == st.N * st.W and y_r.shape == y_l.shape and w_r.shape == w_l.shape
    assert y_l.stride(1) == 1 and y_r.stride(1) == 1 and y_l.stride(0) == y_r.stride(0) and w_l.is_contiguous() and w_r.is_contiguous()
    _need_cuda(y_l, y_r, w_l, w_r, st.score, *(pair_trie or ()))
    name, lex = "sbl_pair_beam_tail", ()
    if pair_trie is not None:
        begin, key, word = pair_trie
        if st.node is None:
            raise _lib.SblHipError("pair_beam_tail_lex: a pair trie needs a PairBeamState with node buffers (lex=True)")
        P, E = word.numel(), key.numel()
        ok = all(t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous() and t.device == y_l.device for t in pair_trie)
        if not ok or P < 1 or begin.numel() != P + 1:
            raise _lib.SblHipError("pair trie tables must be contiguous int32 vectors begin (P + 1) / key (E) / word (P) on %s" % y_l.device)
        name = "sbl_pair_beam_tail_lex"
        lex = (_p(begin), _p(key), _p(word), P, E, _p(st.node[step % 2]), _p(st.node[1 - step % 2]), _p(st.hist_node))
    old, new = st.ys[:, step % 2], st.ys[:, 1 - step % 2]
    call(name, _p(y_l), _p(y_r), y_l.stride(0), _p(w_l), _p(w_r), _p(st.score), _p(st.score_dir), _p(old[0]), _p(old[1]), _p(new[0]),
         _p(new[1]), st.ys.stride(2), _p(st.hist_tok_l), _p(st.hist_tok_r), _p(st.hist_par), _p(st.hist_score), int(step), st.maxlen,
         int(st.eos_id), st.N, st.W, V, D, *lex, _s())


def pair_beam_tail(y_l, y_r, w_l, w_r, st, step):
    """Tail of beam step `step` in one launch (sbl_pair_beam_tail) on the rows y_l / y_r (N*W, 512) the two heads read: the
    best W pair candidates of every clip into the PairBeamState `st` (prefix buffer step % 2 is read, the other written)."""
    _pair_beam_tail(y_l, y_r, w_l, w_r, st, step, None)


def pair_beam_tail_lex(y_l, y_r, w_l, w_r, st, step, pair_trie):
    """pair_beam_tail restricted to a word list, in one launch (include/sbl_hip.h, sbl_pair_beam_tail_lex).  pair_trie: the
    (begin (P + 1), key (P - 1), word (P)) int32 tables of Lexicon.pair_trie() on the same device; st: a PairBeamState with
    lex=True, whose node buffer step % 2 is read and the other one written, like the prefixes."""
    _pair_beam_tail(y_l, y_r, w_l, w_r, st, step, pair_trie)


# --------------------------------------------------------------------------- #
# closed-vocabulary word decode (sbl_lexicon_shortlist, sbl_pair_score_tail)
# --------------------------------------------------------------------------- #
LEXICON_MAX_WORD, LEXICON_MAX_WORDS, LEXICON_MAX_SHORTLIST = 15, 65536, 16

Shortlist = _collections.namedtuple("Shortlist", ("cand", "cand_dist", "cand_hyp", "cand_ys_l2r", "cand_ys_r2l", "n_pos"))


def lexicon_shortlist(ys_l2r, ys_r2l, lex, K, sos_id, eos_id, ignore_id):
    """The K lexicon words nearest to the hypotheses of every clip, in one launch (include/sbl_hip.h, sbl_lexicon_shortlist).
    ys_l2r / ys_r2l: int64 (N, 17) or (N, H, 17) rows of recognize / beam_search (views with any clip and hypothesis stride);
    lex: the uint8 (Wn, 16) table of transformer.lexicon.Lexicon on the same device.  Returns Shortlist(cand, cand_dist,
    cand_hyp (N, K) int32, cand_ys_l2r, cand_ys_r2l (N*K, 17) int64, n_pos (N*K) int32).  No sync."""
    if ys_l2r.dim() == 2:
        ys_l2r, ys_r2l = ys_l2r.unsqueeze(1), ys_r2l.unsqueeze(1)
    N, H, Ly = ys_l2r.shape
    K = int(K)
    _need_cuda(ys_l2r, ys_r2l, lex)
    if ys_r2l.shape != ys_l2r.shape or ys_l2r.dtype != torch.int64 or ys_r2l.dtype != torch.int64:
        raise ValueError("lexicon_shortlist: hypothesis rows %s / %s must be int64 of one shape" % (tuple(ys_l2r.shape), tuple(ys_r2l.shape)))
    if ys_l2r.stride() != ys_r2l.stride() or ys_l2r.stride(2) != 1:
        ys_l2r, ys_r2l = ys_l2r.contiguous(), ys_r2l.contiguous()
    if lex.dtype != torch.uint8 or lex.dim() != 2 or lex.size(1) != 16 or not lex.is_contiguous():
        raise ValueError("lexicon_shortlist: lex must be the contiguous uint8 (Wn, 16) table of Lexicon")
    Wn = lex.size(0)
    if not 1 <= K <= min(Wn, LEXICON_MAX_SHORTLIST):
        raise _lib.SblHipError("lexicon_shortlist: shortlist = %d outside 1..min(%d words, %d)" % (K, Wn, LEXICON_MAX_SHORTLIST))
    dev = ys_l2r.device
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)      # noqa: E731
    out = Shortlist(i32(N, K), i32(N, K), i32(N, K), torch.empty(N * K, Ly, dtype=torch.int64, device=dev),
                    torch.empty(N * K, Ly, dtype=torch.int64, device=dev), i32(N * K))
    call("sbl_lexicon_shortlist", _p(ys_l2r), _p(ys_r2l), ys_l2r.stride(0), ys_l2r.stride(1), Ly, _p(lex), Wn, N, H, K, int(sos_id),
         int(eos_id), int(ignore_id), *(_p(t) for t in out), _s())
    return out


def _check_trie(mask, first, word, device):
    """The tables of Lexicon.trie(): contiguous int64 / int32 / int32 vectors of one length P >= 1 on `device`."""
    P = mask.numel()
    ok = mask.dtype == torch.int64 and first.dtype == torch.int32 and mask.dim() == 1 and first.shape == mask.shape and P >= 1
    ok = ok and mask.is_contiguous() and first.is_contiguous() and mask.device == device and first.device == device
    if word is not None:
        ok = ok and word.dtype == torch.int32 and word.shape == mask.shape and word.is_contiguous() and word.device == device
    if not ok:
        raise _lib.SblHipError("trie tables must be contiguous int64 mask / int32 first / int32 word vectors of one length on %s" % device)


def lexicon_lookup(ys, trie, sos_id, eos_id, ignore_id):
    """Exact trie walk of token rows in one launch (include/sbl_hip.h, sbl_lexicon_lookup).  ys: int64 (..., Ly) rows of
    recognize / beam_search (the last dimension contiguous, the leading ones collapsible to one row stride, else copied);
    trie: the (mask, first, word) tables of Lexicon.trie() on the same device.  Returns (word, node), int32 of ys.shape[:-1]:
    the word index (-1: no such word) and the node reached (-1: a token without a child).  No sync."""
    mask, first, word = trie
    _need_cuda(ys, mask)
    if ys.dtype != torch.int64 or ys.dim() < 1 or ys.size(-1) < 1:
        raise ValueError("lexicon_lookup: ys must be int64 rows, got %s %s" % (ys.dtype, tuple(ys.shape)))
    _check_trie(mask, first, word, ys.device)
    lead, Ly = ys.shape[:-1], ys.size(-1)
    rows = ys.reshape(-1, Ly)      # a view where the strides allow it
    if rows.stride(1) != 1 or (rows.size(0) > 1 and rows.stride(0) < Ly):
        rows = rows.contiguous()
    R = rows.size(0)
    out_w = torch.empty(R, dtype=torch.int32, device=ys.device)
    out_n = torch.empty(R, dtype=torch.int32, device=ys.device)
    call("sbl_lexicon_lookup", _p(rows), max(rows.stride(0), Ly), Ly, R, _p(mask), _p(first), _p(word), mask.numel(), int(sos_id),
         int(eos_id), int(ignore_id), _p(out_w), _p(out_n), _s())
    return out_w.view(lead), out_n.view(lead)


def pair_score_tail(y_l, y_r, w_l, w_r, ys_l2r, ys_r2l, n_pos, G, logp, score_dir, score, best):
    """Pair scores of S slots in groups of G in one launch (sbl_pair_score_tail) on the rows y_l / y_r (16*S, 512) the two
    heads read at the last position of every prefix (GatherLastFn of the 16 segments 1..16): fills logp (S, 16, 2), score_dir
    (S, 2), score (S) and best (S/G) int32.  ys_l2r / ys_r2l: (S, 17) int64 token tables; n_pos: int32 (S) or None (16)."""
    S = ys_l2r.size(0)
    V, D = w_l.shape
    _need_cuda(y_l, y_r, w_l, w_r, ys_l2r, ys_r2l, score)
    assert y_l.shape == (16 * S, D) and y_r.shape == y_l.shape and w_r.shape == w_l.shape and ys_r2l.shape == ys_l2r.shape
    assert y_l.stride(1) == 1 and y_r.stride(1) == 1 and y_l.stride(0) == y_r.stride(0) and w_l.is_contiguous() and w_r.is_contiguous()
    assert ys_l2r.dtype == torch.int64 and ys_r2l.dtype == torch.int64 and ys_l2r.stride(1) == 1 and ys_l2r.stride() == ys_r2l.stride()
    assert n_pos is None or (n_pos.dtype == torch.int32 and n_pos.shape == (S,) and n_pos.is_contiguous())
    assert all(t.is_contiguous() for t in (logp, score_dir, score, best)) and best.dtype == torch.int32
    assert logp.shape == (S, 16, 2) and score_dir.shape == (S, 2) and score.shape == (S,) and best.numel() * G == S
    call("sbl_pair_score_tail", _p(y_l), _p(y_r), y_l.stride(0), _p(w_l), _p(w_r), _p(ys_l2r), _p(ys_r2l), ys_l2r.stride(0),
         _p(n_pos), _p(logp), _p(score_dir), _p(score), _p(best), S, int(G), V, D, _s())

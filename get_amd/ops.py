"""Autograd-aware host wrappers over the C-ABI (one ``torch.autograd.Function`` per fused op).

PyTorch supplies device memory, streams and the autograd tape; every numerical
step runs in libget_hip.so.  All tensors are fp32/contiguous on a ROCm device.
"""
from __future__ import annotations

import os
import weakref
from typing import Optional

import torch

from . import _lib
from ._lib import call, ptr, stream

# GET_AMD_CLAIM_STREAM=0 keeps the claim branch on the caller's stream (modules.Graph_basedSemantiStructure.forward)
CLAIM_SIDE_STREAM = os.environ.get("GET_AMD_CLAIM_STREAM", "1") != "0"
_SIDE_STREAMS: dict = {}


def side_stream(device) -> "torch.cuda.Stream":
    """One auxiliary HIP stream per device for work that is independent of the main chain of launches."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    s = _SIDE_STREAMS.get(idx)
    if s is None:
        s = torch.cuda.Stream(device=idx)
        _SIDE_STREAMS[idx] = s
    return s


# Weight gradients of the few-row layers (evidence-level attention, head) leave the critical path of backward: with a
# FlatTrainer (gradients accumulate straight into the flat bucket) they are issued on the auxiliary stream and joined
# at the end of the backward pass (and before any all-reduce).  GET_AMD_WGRAD_STREAM=0 keeps them in line.
WGRAD_SIDE_STREAM = os.environ.get("GET_AMD_WGRAD_STREAM", "1") != "0"
WGRAD_FEW_ROWS = 4096
_side_pending: set = set()


def side_join():
    """Make the current stream wait for everything issued on the auxiliary stream so far (no-op when nothing is)."""
    for idx in list(_side_pending):
        torch.cuda.current_stream(idx).wait_stream(_SIDE_STREAMS[idx])
        _side_pending.discard(idx)


def pending_side_stream():
    """The auxiliary stream of the current device if work of the running backward pass is pending on it, else None."""
    idx = torch.cuda.current_device() if torch.cuda.is_available() else None
    return _SIDE_STREAMS.get(idx) if idx in _side_pending else None


def side_mark_backward(device):
    """Called from inside a backward pass when work of that pass runs (or is about to run) on the auxiliary stream -- the
    claim branch's backward, which autograd replays on its forward stream: marks the device pending and queues the join
    for the end of the pass.  With a FlatTrainer the branch's backward returns no gradients to autograd (they land in
    the flat bucket directly), so the engine itself never learns about the side stream and would not join it."""
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx in _SIDE_STREAMS and idx not in _side_pending:
        _side_pending.add(idx)
        torch.autograd.Variable._execution_engine.queue_callback(side_join)


def _side_wgrad(dev, tensors, launch):
    """Run `launch()` (weight-gradient launches only) on the auxiliary stream after the current stream's work;
    `tensors` are the operands it reads.  The join is queued for the end of the running backward pass."""
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    side = side_stream(dev)
    main = torch.cuda.current_stream(idx)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        _lib.ensure_workspace(dev)
        launch()
    for t in tensors:
        if t is not None:
            t.record_stream(side)
    if idx not in _side_pending:
        _side_pending.add(idx)
        torch.autograd.Variable._execution_engine.queue_callback(side_join)


_WEIGHT_EPOCH = 0
_WT_CACHE: dict = {}


def bump_weight_epoch():
    """Invalidate EVERY cached derivative of the weights (transposes, bias sums, packed scalar gates, bf16 twins).  The
    public invalidation API: call it after writing parameters through `.data` / raw pointers (EMA swaps, hand-written
    optimisers) -- such writes do not bump `_version`, so nothing else can notice them."""
    global _WEIGHT_EPOCH
    _WEIGHT_EPOCH += 1
    _WT_CACHE.clear()
    _BF16_CACHE.clear()
    _DERIVED_CACHE.clear()
    if _lib.gemm_mode() == "fp32x3p":       # the library's pre-split weight images: drop them (weights may have been replaced)
        call("gh_fp32x3_clear")


def _bump_trainer_epoch():
    """FlatTrainer.step's own invalidation: the fused optimiser rewrites exactly the parameters of its bucket, so entries
    derived from tensors OUTSIDE the bucket (`frozen`: the never-trained GSL scorer's packed gates, the bf16 twin of a
    frozen embedding table) stay valid."""
    global _WEIGHT_EPOCH
    _WEIGHT_EPOCH += 1
    _WT_CACHE.clear()
    _BF16_CACHE.clear()
    for k in [k for k, v in _DERIVED_CACHE.items() if v[0][-1] != -1]:
        del _DERIVED_CACHE[k]
    if _lib.gemm_mode() == "fp32x3p":       # every image stale; refresh_transposes re-makes them all in one launch
        call("gh_weights_changed")


_X3P_SIG: dict = {}


def fp32x3p_guard(module):
    """gemm mode "fp32x3p" only: the library reads the weight operand of its activation-sized GEMMs from pre-split images
    and cannot see in-place updates by a torch optimiser.  Called at the top of the model's forward: when any parameter's
    `_version` or address moved since the last call, every image is marked stale (re-made by the launch that meets it).
    FlatTrainer rewrites parameters through raw pointers and tells the library itself (_bump_trainer_epoch)."""
    sig = 0
    for q in module.parameters():
        sig = (sig * 1000003 + q._version * 31 + q.data_ptr()) & 0xFFFFFFFFFFFF
    if _X3P_SIG.get(id(module)) != sig:
        _X3P_SIG[id(module)] = sig
        call("gh_weights_changed")


def _direct(p) -> bool:
    """True when gradients of `p` may be accumulated by the kernels straight into `p.grad` (a live view of
    the trainer's flat bucket, see dist.FlatTrainer) instead of being returned to autograd, which
    would add them there with one extra elementwise kernel per parameter."""
    if not getattr(p, "_gh_direct_grad", False):      # (first: a non-leaf view of a weight has no .grad to ask for)
        return False
    g = getattr(p, "grad", None)
    return g is not None and g.dtype == torch.float32 and g.is_contiguous() and g.shape == p.shape


def _f32(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def transposed(w: torch.Tensor) -> torch.Tensor:
    """W[n_out][n_in] -> Wt[n_in][n_out], cached per parameter OBJECT (weak reference), storage
    address, in-place version and weight epoch -- never by address alone, which the caching
    allocator recycles."""
    key = id(w)
    hit = _WT_CACHE.get(key)
    if hit is not None:
        ref, dptr, ver, epoch, wt = hit
        if ref() is w and dptr == w.data_ptr() and ver == w._version and epoch == _WEIGHT_EPOCH:
            return wt
    wc = _f32(w.detach())
    if _lib.gemm_mode() == "fp32x3p":
        # the library keys its pre-split images by operand address: keep the k-major copy in the parameter's persistent
        # buffer (as refresh_transposes does) so that the address stays, and mark the images stale
        hit_p = _WT_PERSIST.get(key)
        if hit_p is None or hit_p[0]() is not w or hit_p[1].shape != (wc.shape[1], wc.shape[0]) or hit_p[1].device != w.device:
            hit_p = (weakref.ref(w), torch.empty((wc.shape[1], wc.shape[0]), device=w.device, dtype=torch.float32))
            _WT_PERSIST[key] = hit_p
        wt = hit_p[1]
        call("gh_weights_changed")
    else:
        wt = torch.empty((wc.shape[1], wc.shape[0]), device=w.device, dtype=torch.float32)
    call("gh_transpose", ptr(wc), ptr(wt), wc.shape[0], wc.shape[1], stream())
    if len(_WT_CACHE) > 512:
        for k in [k for k, v in _WT_CACHE.items() if v[0]() is None]:
            del _WT_CACHE[k]
    _WT_CACHE[key] = (weakref.ref(w), w.data_ptr(), w._version, _WEIGHT_EPOCH, wt)
    return wt


_DERIVED_CACHE: dict = {}
_WT_PERSIST: dict = {}
# bf16 storage mode (BASELINE configs[4]): bf16 twins of a weight matrix and of its transpose, in persistent buffers (their
# addresses are part of the composite entry points' cached descriptor), validity tracked like the transposes'
_BF16_CACHE: dict = {}       # id(w) -> (ref, data_ptr, version, epoch, w16, wt16)
_BF16_PERSIST: dict = {}     # id(w) -> (ref, w16, wt16)


def _bf16_buffers(w: torch.Tensor):
    hit = _BF16_PERSIST.get(id(w))
    if hit is None or hit[0]() is not w or hit[1].shape != w.shape or hit[1].device != w.device:
        if len(_BF16_PERSIST) > 512:
            for k in [k for k, v in _BF16_PERSIST.items() if v[0]() is None]:
                del _BF16_PERSIST[k]
        hit = (weakref.ref(w), torch.empty(tuple(w.shape), device=w.device, dtype=torch.bfloat16),
               torch.empty((w.shape[1], w.shape[0]), device=w.device, dtype=torch.bfloat16))
        _BF16_PERSIST[id(w)] = hit
    return hit[1], hit[2]


def bf16_twins(w: torch.Tensor):
    """(bf16(W) [n_out][n_in], bf16(W^T) [n_in][n_out]) of a weight matrix, cached per parameter object / storage address /
    in-place version / weight epoch; re-made together with the fp32 transpose in ONE launch (gh_weights_refresh), by
    refresh_transposes after the optimiser step or here on a miss."""
    hit = _BF16_CACHE.get(id(w))
    if hit is not None:
        ref, dptr, ver, epoch, w16, wt16 = hit
        if ref() is w and dptr == w.data_ptr() and ver == w._version and epoch == _WEIGHT_EPOCH:
            return w16, wt16
    _bf16_buffers(w)
    refresh_transposes([w])
    hit = _BF16_CACHE[id(w)]
    return hit[4], hit[5]


def derived(tag: str, tensors, fn, frozen: bool = False):
    """Small per-parameter-set cache for values derived from weights (bias sums, packed scalar gates): recomputed only
    when one of the source tensors was replaced, modified in place (``_version``) or the weight epoch moved on (the
    fused optimiser updates parameters through raw pointers).  Saves a dozen tiny elementwise launches per step."""
    key = (tag,) + tuple(id(t) for t in tensors)
    # frozen: the sources are never touched by the optimiser (requires_grad False), so the weight epoch does not matter
    sig = tuple((t.data_ptr(), t._version) for t in tensors) + ((-1,) if frozen else (_WEIGHT_EPOCH,))
    hit = _DERIVED_CACHE.get(key)
    if hit is not None and hit[0] == sig and all(r() is t for r, t in zip(hit[1], tensors)):
        return hit[2]
    with torch.no_grad():
        val = fn()
    if len(_DERIVED_CACHE) > 512:
        for k in [k for k, v in _DERIVED_CACHE.items() if any(r() is None for r in v[1])]:
            del _DERIVED_CACHE[k]
    _DERIVED_CACHE[key] = (sig, tuple(weakref.ref(t) for t in tensors), val)
    return val


def refresh_transposes(weights):
    """Transpose many weight matrices in ONE launch and prime the cache (called by the trainer right
    after the optimiser step, so the next forward finds every k-major operand ready)."""
    import ctypes
    ws = [w for w in weights if w.dim() == 2]
    if not ws:
        return
    n = len(ws)
    # the transposed copies live in PERSISTENT buffers (one per parameter object, rewritten in place every step): their
    # addresses are part of the composite entry points' cached descriptor (get_amd/fused.py), and nothing is allocated
    wts = []
    for w in ws:
        hit = _WT_PERSIST.get(id(w))
        if hit is None or hit[0]() is not w or hit[1].shape != (w.shape[1], w.shape[0]) or hit[1].device != w.device:
            hit = (weakref.ref(w), torch.empty((w.shape[1], w.shape[0]), device=w.device, dtype=torch.float32))
            _WT_PERSIST[id(w)] = hit
        wts.append(hit[1])
    src = (ctypes.c_void_p * n)(*[w.data_ptr() for w in ws])
    dst = (ctypes.c_void_p * n)(*[t.data_ptr() for t in wts])
    rows = (ctypes.c_int * n)(*[w.shape[0] for w in ws])
    cols = (ctypes.c_int * n)(*[w.shape[1] for w in ws])
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    # bf16 twins ride in the same launch for every matrix that has them (i.e. that a bf16-storage cell has asked for)
    twins = [_BF16_PERSIST.get(id(w)) for w in ws]
    twins = [t if (t is not None and t[0]() is w and t[1].device == w.device) else None for t, w in zip(twins, ws)]
    if any(t is not None for t in twins):
        w16 = (ctypes.c_void_p * n)(*[(t[1].data_ptr() if t is not None else None) for t in twins])
        t16 = (ctypes.c_void_p * n)(*[(t[2].data_ptr() if t is not None else None) for t in twins])
        call("gh_weights_refresh", n, cast(src), cast(dst), cast(w16), cast(t16), cast(rows), cast(cols), stream())
        for w, t in zip(ws, twins):
            if t is not None:
                _BF16_CACHE[id(w)] = (weakref.ref(w), w.data_ptr(), w._version, _WEIGHT_EPOCH, t[1], t[2])
    else:
        call("gh_transpose_batch", n, cast(src), cast(dst), cast(rows), cast(cols), stream())
    if _lib.gemm_mode() == "fp32x3p":
        call("gh_fp32x3_refresh", stream())
    for w, wt in zip(ws, wts):
        _WT_CACHE[id(w)] = (weakref.ref(w), w.data_ptr(), w._version, _WEIGHT_EPOCH, wt)


# --------------------------------------------------------------------------- packed adjacency
class PackedAdj:
    """Adjacency of ``n`` graphs with ``r`` padded nodes in the library's packed form
    (include/get_hip.h): neighbour bit rows + either dinv (normalised binary graph built by
    ``graph_build``) or dense fp32 values (any adjacency the reference API hands over), plus an
    optional GSL keep-set."""

    __slots__ = ("bits", "dinv", "vals", "keep", "n", "r", "plan")

    def __init__(self, bits, dinv, vals, keep, n, r, plan=None):
        self.bits, self.dinv, self.vals, self.keep, self.n, self.r = bits, dinv, vals, keep, n, r
        self.plan = plan        # optional RaggedPlan (node-compact row layout) for callers that opt in

    @property
    def words(self):
        return (self.r + 63) // 64

    @property
    def device(self):
        return self.bits.device

    @staticmethod
    def from_dense(adj: torch.Tensor) -> "PackedAdj":
        """(N,R,R) float64/float32 -> packed (exact values kept, i.e. the reference's `.float()`)."""
        _lib.require_cuda(adj)
        assert adj.dim() == 3 and adj.shape[1] == adj.shape[2], "adjacency must be (N,R,R)"
        n, r, _ = adj.shape
        if adj.dtype not in (torch.float64, torch.float32):
            adj = adj.float()
        adj = adj.contiguous()
        w = (r + 63) // 64
        bits = torch.empty((n, r, w), device=adj.device, dtype=torch.int64)
        vals = torch.empty((n, r, r), device=adj.device, dtype=torch.float32)
        fn = "gh_adj_pack_f64" if adj.dtype == torch.float64 else "gh_adj_pack_f32"
        call(fn, ptr(adj), n, r, ptr(bits), ptr(vals), stream())
        return PackedAdj(bits, None, vals, None, n, r)

    def with_keep(self, keep: Optional[torch.Tensor]) -> "PackedAdj":
        return PackedAdj(self.bits, self.dinv, self.vals, keep, self.n, self.r, self.plan)

    def with_plan(self, plan: "RaggedPlan") -> "PackedAdj":
        return PackedAdj(self.bits, self.dinv, self.vals, self.keep, self.n, self.r, plan)

    def to_dense(self) -> torch.Tensor:
        out = torch.empty((self.n, self.r, self.r), device=self.device, dtype=torch.float32)
        call("gh_adj_unpack", ptr(self.bits), ptr(self.dinv), ptr(self.vals), ptr(self.keep), self.n, self.r,
             ptr(out), stream())
        return out

    def _args(self):
        return ptr(self.bits), ptr(self.dinv), ptr(self.vals), ptr(self.keep)


def graph_build(tokens: torch.Tensor, lengths: torch.Tensor, window: int):
    """interactions.py:334-351 on device.  tokens (N,R) raw ids, lengths (N,).

    Returns (PackedAdj, node_ids (N,R) int32, n_nodes (N,) int32)."""
    _lib.require_cuda(tokens, lengths)
    tokens = tokens.to(torch.int32).contiguous()
    lengths = lengths.to(torch.int32).contiguous()
    n, r = tokens.shape
    w = (r + 63) // 64
    dev = tokens.device
    node_ids = torch.empty((n, r), device=dev, dtype=torch.int32)
    n_nodes = torch.empty((n,), device=dev, dtype=torch.int32)
    bits = torch.empty((n, r, w), device=dev, dtype=torch.int64)
    dinv = torch.empty((n, r), device=dev, dtype=torch.float32)
    call("gh_graph_build", ptr(tokens), ptr(lengths), n, r, int(window), ptr(node_ids), ptr(n_nodes), ptr(bits),
         ptr(dinv), stream())
    return PackedAdj(bits, dinv, None, None, n, r), node_ids, n_nodes


def as_packed(adj) -> PackedAdj:
    return adj if isinstance(adj, PackedAdj) else PackedAdj.from_dense(adj)


class RaggedPlan:
    """Node-compact row layout of ``n`` graphs padded to ``r`` nodes (include/get_hip.h): the real nodes of
    all graphs back to back (graph g at rows ``goff[g] .. goff[g+1]``), every padding node after them.

    The reference runs all n*r padded rows through every layer (graph_based_semantic_structure.py:99-107);
    padding nodes have no edges and are masked out of the word attention (:180), so only the first cell's
    forward and the scorer (whose padding scores compete in GSL's top-k, wrapper.py:216-219) need them.
    ``m_real`` (sum of node counts) must be known on the HOST: it sizes the launches."""

    __slots__ = ("n", "r", "m_real", "m_tot", "goff", "rowg", "src", "cids", "maskf")

    def __init__(self, n_nodes: torch.Tensor, node_ids: torch.Tensor, m_real: int):
        _lib.require_cuda(n_nodes, node_ids)
        n, r = node_ids.shape
        dev = node_ids.device
        self.n, self.r, self.m_real, self.m_tot = int(n), int(r), int(m_real), int(n * r)
        assert 0 <= self.m_real <= self.m_tot
        n_nodes = n_nodes.to(torch.int32).contiguous()
        node_ids = node_ids.to(torch.int32).contiguous()
        self.goff = torch.empty((n + 1,), device=dev, dtype=torch.int32)
        self.rowg = torch.empty((n * r,), device=dev, dtype=torch.int32)
        self.src = torch.empty((n * r,), device=dev, dtype=torch.int32)
        self.cids = torch.empty((n * r,), device=dev, dtype=torch.int32)
        self.maskf = torch.empty((n * r,), device=dev, dtype=torch.float32)     # (cids >= 1): the word attention's mask
        call("gh_ragged_plan", ptr(n_nodes), ptr(node_ids), n, r, ptr(self.goff), ptr(self.rowg), ptr(self.src),
             ptr(self.cids), ptr(self.maskf), stream())

    @classmethod
    def empty(cls, n: int, r: int, m_real: int, device) -> "RaggedPlan":
        """Buffers of a plan that a later gh_get_prepare / gh_ragged_plan call fills (get_amd.batch.NativeBatch)."""
        self = cls.__new__(cls)
        self.n, self.r, self.m_real, self.m_tot = int(n), int(r), int(m_real), int(n * r)
        assert 0 <= self.m_real <= self.m_tot
        i32 = lambda k: torch.empty((k,), device=device, dtype=torch.int32)
        self.goff, self.rowg, self.src, self.cids = i32(n + 1), i32(n * r), i32(n * r), i32(n * r)
        self.maskf = torch.empty((n * r,), device=device, dtype=torch.float32)
        return self

    def to_padded(self, x: torch.Tensor, rows: Optional[int] = None) -> torch.Tensor:
        """Compact rows (m, ...) -> padded (n, r, ...) with zeros where no compact row was given."""
        m = x.shape[0] if rows is None else rows
        out = torch.zeros((self.m_tot,) + tuple(x.shape[1:]), device=x.device, dtype=x.dtype)
        out.index_copy_(0, self.src[:m].long(), x[:m])
        return out.view(self.n, self.r, *x.shape[1:])

    def from_padded(self, x: torch.Tensor, rows: Optional[int] = None) -> torch.Tensor:
        """Padded (n, r, ...) -> compact rows (m_tot or `rows`, ...)."""
        m = self.m_tot if rows is None else rows
        return x.reshape(self.m_tot, *x.shape[2:]).index_select(0, self.src[:m].long())


# --------------------------------------------------------------------------- aggregation (a = A x)
class _Spmm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, adj: PackedAdj, plan):
        x = _f32(x)
        h = x.shape[-1]
        if plan is not None:
            assert x.dim() == 2 and x.shape[0] == plan.m_real, "node-compact spmm takes the (m_real, h) real rows"
        else:
            assert x.dim() == 3 and x.shape[0] == adj.n and x.shape[1] == adj.r
        y = torch.empty_like(x)
        call("gh_spmm", *adj._args(), *_plan_args(plan), ptr(x), ptr(y), adj.n, adj.r, h, 0, 0, stream())
        ctx.adj, ctx.plan = adj, plan
        return y

    @staticmethod
    def backward(ctx, g):
        g = _f32(g)
        dx = torch.empty_like(g)
        call("gh_spmm", *ctx.adj._args(), *_plan_args(ctx.plan), ptr(g), ptr(dx), ctx.adj.n, ctx.adj.r, g.shape[-1], 1, 0,
             stream())
        return dx, None, None


def _plan_args(plan):
    """(goff, m_real) of the C-ABI: NULL/0 selects the padded layout."""
    return (None, 0) if plan is None else (ptr(plan.goff), plan.m_real)


def spmm(adj: PackedAdj, x: torch.Tensor, plan: "RaggedPlan" = None) -> torch.Tensor:
    return _Spmm.apply(x, adj, plan)


# --------------------------------------------------------------------------- GGNN cell
class _GGNNCell(torch.autograd.Function):
    """Models/BiDAF/wrapper.py:188-208 (without the input dropout, applied by the caller)."""

    @staticmethod
    def forward(ctx, x, ids, adj: PackedAdj, w_p, w_z0, b_z0, w_z1, b_z1, w_r0, b_r0, w_r1, b_r1, w_h0, b_h0, w_h1,
                b_h1, drop_p=0.0, drop_seed=0, plan=None, rows=0, score=None):
        x = _f32(x)
        n, r = adj.n, adj.r
        h, din = w_p.shape
        m = n * r if plan is None else int(rows)      # rows the forward computes (node-compact: m_real or m_tot)
        mb = n * r if plan is None else plan.m_real    # rows the backward computes
        if plan is not None:
            assert plan.n == n and plan.r == r and plan.m_real <= m <= plan.m_tot
        if ids is not None:
            assert ids.dtype == torch.int32 and ids.numel() >= m and x.dim() == 2 and x.shape[1] == din
            ids = ids.contiguous()
        elif plan is not None:
            assert x.dim() == 2 and x.shape[1] == din and x.shape[0] >= m, "node-compact cell takes (rows, din) features"
        else:
            assert x.numel() == m * din, f"x has {x.numel()} elements, expected {m}x{din}"
        dev = x.device
        # forward products x.W^T take the weights as stored; the backward's dX = g.W takes the cached transposes
        ws = [_f32(w.detach()) for w in (w_p, w_z0, w_z1, w_r0, w_r1, w_h0, w_h1)]
        wts = [transposed(w) for w in (w_p, w_z0, w_z1, w_r0, w_r1, w_h0, w_h1)]
        bs = [_f32(t.detach()) for t in (b_z0, b_z1, b_r0, b_r1, b_h0, b_h1)]      # the epilogues add b?0 + b?1
        # bf16 STORAGE pipeline (BASELINE configs[4], _lib.set_gemm_mode("bf16")): activations and weights of the cell live
        # in HBM as bf16, the GEMMs run v_mfma_f32_16x16x32_bf16 with fp32 accumulation; the fp32 cell output is kept for the
        # consumers outside the cell.  Only for shapes the bf16 kernels take (16-byte rows, activation-sized launches).
        bf = bf16_cell_ok(din, h, m, mb)
        ctx.bf = bf
        if bf:
            wkeys = (w_p, w_z0, w_z1, w_r0, w_r1, w_h0, w_h1)
            if all(t.dtype == torch.float32 and t.is_contiguous() for t in wkeys):
                tw = [bf16_twins(t) for t in wkeys]          # persistent buffers, refreshed with the transposes in one launch
                ws_b, wts_b = tuple(t[0] for t in tw), tuple(t[1] for t in tw)
            else:
                ws_b = derived("cell_w_bf16", wkeys, lambda: tuple(t.to(torch.bfloat16) for t in ws))
                wts_b = derived("cell_wt_bf16", wkeys, lambda: tuple(t.to(torch.bfloat16) for t in wts))
            if ids is not None:
                xb = derived("table_bf16", (x,), lambda: x.detach().to(torch.bfloat16), frozen=not x.requires_grad)
            else:
                xb = getattr(x, "_gh_bf16", None)
                if xb is None or xb.shape != x.shape:
                    xb = x.detach().to(torch.bfloat16)
            bufb = torch.empty((7, m, h), device=dev, dtype=torch.bfloat16)
            xp, a, z, rr, rx, hh, outb = bufb.unbind(0)
            out = torch.empty((m, h), device=dev, dtype=torch.float32)
            sx = None
            sc = (None, None, 0.0, 0)
            if score is not None:
                sw, sp, sseed = score
                sx = torch.empty((m,), device=dev, dtype=torch.float32)
                sc = (ptr(_f32(sw.detach().reshape(-1))), ptr(sx), float(sp), int(sseed))
            call("gh_ggnn_cell_fwd_bf16", *adj._args(), *_plan_args(plan), m, ptr(xb), ptr(ids), n, r, din, h,
                 *[ptr(t) for t in ws_b], *[ptr(t) for t in bs],
                 ptr(xp), ptr(a), ptr(z), ptr(rr), ptr(rx), ptr(hh), ptr(outb), ptr(out), float(drop_p), int(drop_seed), *sc,
                 stream())
            ctx.adj, ctx.ids, ctx.dims, ctx.plan, ctx.rows = adj, ids, (n, r, din, h), plan, (m, mb)
            ctx.drop = (float(drop_p), int(drop_seed))
            ctx.params = (w_p, w_z0, b_z0, w_z1, b_z1, w_r0, b_r0, w_r1, b_r1, w_h0, b_h0, w_h1, b_h1)
            ctx.save_for_backward(xb, bufb, *wts_b)
            ctx.x_needs_grad = ctx.needs_input_grad[0]
            ctx.x_shape = tuple(x.shape)
            res = out.view(n, r, h) if plan is None else out
            res._gh_bf16 = outb.view(n, r, h) if plan is None else outb        # bf16 twin for a following bf16 cell
            if score is not None:
                ctx.mark_non_differentiable(sx)
                return res, sx
            return res
        buf = torch.empty((7, m, h), device=dev, dtype=torch.float32)
        xp, a, z, rr, rx, hh, out = buf.unbind(0)
        sx = None
        sc = (None, None, 0.0, 0)
        if score is not None:      # (scorer proj weight (h,), dropout p, seed): projection fused into the last epilogue
            sw, sp, sseed = score
            sx = torch.empty((m,), device=dev, dtype=torch.float32)
            sc = (ptr(_f32(sw.detach().reshape(-1))), ptr(sx), float(sp), int(sseed))
        call("gh_ggnn_cell_fwd", *adj._args(), *_plan_args(plan), m, ptr(x), ptr(ids), n, r, din, h,
             *[ptr(t) for t in ws], *[ptr(t) for t in bs],
             ptr(xp), ptr(a), ptr(z), ptr(rr), ptr(rx), ptr(hh), ptr(out), float(drop_p), int(drop_seed), *sc, stream())
        ctx.adj, ctx.ids, ctx.dims, ctx.plan, ctx.rows = adj, ids, (n, r, din, h), plan, (m, mb)
        ctx.drop = (float(drop_p), int(drop_seed))
        ctx.params = (w_p, w_z0, b_z0, w_z1, b_z1, w_r0, b_r0, w_r1, b_r1, w_h0, b_h0, w_h1, b_h1)
        ctx.save_for_backward(x, buf, *wts)
        ctx.x_needs_grad = ctx.needs_input_grad[0]
        res = out.view(n, r, h) if plan is None else out
        if score is not None:
            ctx.mark_non_differentiable(sx)
            return res, sx
        return res

    @staticmethod
    def backward(ctx, g, *_unused):
        x, buf, w_p, w_z0, w_z1, w_r0, w_r1, w_h0, w_h1 = ctx.saved_tensors      # the TRANSPOSED weights
        xp, a, z, rr, rx, hh, _ = buf.unbind(0)
        n, r, din, h = ctx.dims
        m_fwd, m = ctx.rows                   # the backward runs on the real-node rows only (m == m_fwd when padded)
        plan = ctx.plan
        dev = g.device
        g = _f32(g).reshape(m_fwd, h)
        _lib.ensure_workspace(dev)
        bf = getattr(ctx, "bf", False)
        scratch = torch.empty((5, max(m, 1), h), device=dev, dtype=torch.bfloat16 if bf else torch.float32)
        dhp, dzp, drp, dxp, da = scratch.unbind(0)
        ids = ctx.ids
        want_dx = ctx.x_needs_grad
        dx = None
        if want_dx:
            x_rows = m if ids is not None else x.shape[0] if plan is not None else m
            if bf and ids is None and plan is None:
                x_rows = m
            dx = torch.empty((x_rows, din), device=dev, dtype=torch.float32)
            if x_rows > m:
                dx[m:].zero_()               # padding rows (and unused tail rows of x) get no gradient
        P = ctx.params
        direct = all(_direct(p) for p in P)
        if direct:     # weight/bias gradients land in the parameters' own .grad (flat bucket) -- no adds, no fills
            pw_p, pz0, bz0, pz1, bz1, pr0, br0, pr1, br1, ph0, bh0, ph1, bh1 = (p.grad for p in P)
            gw = [pw_p, pz0, pz1, pr0, pr1, ph0, ph1]
            gb = [bz0, br0, bh0, bz1, br1, bh1]
        else:
            dw_p = torch.zeros((h, din), device=dev, dtype=torch.float32)
            dws = torch.zeros((6, h, h), device=dev, dtype=torch.float32)
            dbs = torch.zeros((3, h), device=dev, dtype=torch.float32)
            gw = [dw_p] + [dws[i] for i in range(6)]
            gb = [dbs[0], dbs[1], dbs[2], None, None, None]
        call("gh_ggnn_cell_bwd_bf16" if bf else "gh_ggnn_cell_bwd", *ctx.adj._args(), *_plan_args(plan), ptr(x), ptr(ids), n, r, din, h,
             ptr(w_p), ptr(w_z0), ptr(w_z1), ptr(w_r0), ptr(w_r1), ptr(w_h0), ptr(w_h1),
             ptr(xp), ptr(a), ptr(z), ptr(rr), ptr(rx), ptr(hh), ptr(g),
             ptr(dhp), ptr(dzp), ptr(drp), ptr(dxp), ptr(da),
             ptr(dx), *[ptr(t) for t in gw], *[ptr(t) for t in gb], ctx.drop[0], ctx.drop[1], stream())
        if want_dx:
            if ids is not None:      # trainable embedding table: scatter the row gradients
                demb = torch.zeros(x.shape, device=dev, dtype=torch.float32)
                demb.index_add_(0, ids[:m].long(), dx)
                dx = demb
            else:
                dx = dx.view(ctx.x_shape if bf else x.shape)
        if direct:
            return (dx, None, None) + (None,) * 18
        dz0, dz1, dr0, dr1, dh0, dh1 = dws.unbind(0)
        bz, br, bh = dbs.unbind(0)
        return (dx, None, None, dw_p, dz0, bz, dz1, bz, dr0, br, dr1, br, dh0, bh, dh1, bh, None, None, None, None, None)


def ggnn_cell(adj: PackedAdj, x, ids, params, drop_p: float = 0.0, drop_seed: int = 0, plan: "RaggedPlan" = None,
              rows: int = 0, score=None):
    """params: (w_p, w_z0, b_z0, w_z1, b_z1, w_r0, b_r0, w_r1, b_r1, w_h0, b_h0, w_h1, b_h1).
    drop_p > 0 applies the cell's input dropout inside the first GEMM (stateless hash mask keyed by drop_seed).
    plan: node-compact layout -- x is (>= rows, din) (or table + ids), the forward computes the first `rows`
    rows (plan.m_real or plan.m_tot), the backward the plan.m_real real-node rows; returns (rows, h).
    score = (w (h,), p, seed): also returns the GSL word scorer's projection dropout_p(out) . w per row, produced by
    the last GEMM's epilogue (see `scorer_fusable`); the result is then (out, score_x)."""
    if plan is not None and not rows:
        rows = plan.m_real
    return _GGNNCell.apply(x, ids, adj, *params, drop_p, drop_seed, plan, rows, score)


def bf16_cell_ok(din: int, h: int, m_fwd: int, m_bwd: int) -> bool:
    """True when a cell call takes the bf16 storage pipeline: mode "bf16", 16-byte bf16 rows, activation-sized launches."""
    return (_lib.gemm_mode() == "bf16" and din % 8 == 0 and h % 8 == 0 and din <= h and min(m_fwd, m_bwd) >= 8192)


def scorer_fusable(h: int) -> bool:
    """The scorer projection rides in the h-gate GEMM's epilogue when a whole output row lives in one workgroup."""
    return h % 4 == 0 and 4 <= h <= 320


def fused_dropout_ok(din: int, h: int) -> bool:
    """The in-kernel dropout lives in the float4 fast path of the GEMM."""
    return din % 4 == 0 and h % 4 == 0 and 4 <= din <= h


def new_dropout_seed() -> int:
    """Fresh 31-bit seed from torch's CPU generator (follows torch.manual_seed, no device sync)."""
    return int(torch.randint(0, 2 ** 31 - 1, (1,)).item())


def dropout_mask_reference(seed: int, rows: int, cols: int, p: float):
    """Host replica of the kernels' stateless mask (tests): bool (rows, cols), True = kept."""
    import numpy as np
    idx = (np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(cols) + np.arange(cols, dtype=np.uint64)[None, :])
    x = (idx * np.uint64(0x9E3779B1) + np.uint64(seed)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    t = p * 4294967296.0
    thresh = np.uint64(4294967295 if t >= 4294967295.0 else int(t))
    return x >= thresh


# --------------------------------------------------------------------------- word scorer + GSL (no gradient)
@torch.no_grad()
def scorer_gsl(adj: PackedAdj, feat: torch.Tensor, w_p, gate12: torch.Tensor, k: int, drop_p: float = 0.0,
               drop_seed: int = 0, plan: "RaggedPlan" = None, collapsed: bool = False, score_x: torch.Tensor = None):
    """GGNN(h->1) score of every node and the top-k keep set (wrapper.py:167-168, :215-219).
    feat: (N,R,H), or node-compact (N*R, H) incl. the padding rows when `plan` is given; alternatively
    score_x (rows,) = the projections proj(dropout(feat)) already produced by ggnn_cell(..., score=...).
    Returns (score (N,R) fp32, keep (N,W) int64 bit words) -- both in padded node indexing."""
    src = score_x if score_x is not None else feat
    src = _f32(src.detach())
    if plan is not None:
        need = min(plan.m_real + 1, plan.m_tot) if collapsed else plan.m_tot
        assert src.shape[0] == need and src.dim() == (1 if score_x is not None else 2), \
            "the scorer needs the padding rows too (they compete in top-k)"
        assert not (collapsed and drop_p > 0.0), "collapsed padding rows are an evaluation-mode layout"
        n, r = plan.n, plan.r
    else:
        n, r = adj.n, adj.r
        assert src.numel() == n * r * (1 if score_x is not None else src.shape[-1])
    h = w_p.numel()
    score = torch.empty((n, r), device=src.device, dtype=torch.float32)
    keep = torch.empty((n, adj.words), device=src.device, dtype=torch.int64)
    w_p = _f32(w_p.detach().reshape(-1))
    gate12 = _f32(gate12.detach())
    call("gh_scorer_gsl", ptr(adj.bits), ptr(adj.dinv), ptr(adj.vals), _plan_args(plan)[0], 1 if (collapsed and plan is not None) else 0,
         None if score_x is not None else ptr(src), ptr(src) if score_x is not None else None, ptr(w_p), ptr(gate12), n, r, h,
         int(k), ptr(score), ptr(keep), float(drop_p), int(drop_seed), stream())
    return score, keep


@torch.no_grad()
def gsl_topk(score: torch.Tensor, k: int) -> torch.Tensor:
    score = _f32(score.detach())
    n, r = score.shape
    keep = torch.empty((n, (r + 63) // 64), device=score.device, dtype=torch.int64)
    call("gh_gsl_topk", ptr(score), n, r, int(k), ptr(keep), stream())
    return keep


# --------------------------------------------------------------------------- concat attention
class _ConcatAtt(torch.autograd.Function):
    """two_branches_attention.py:121-148 (left given) / self_attention.py:75-100 (left None)."""

    @staticmethod
    def forward(ctx, left, right, mask, w1, w2, plan=None):
        right = _f32(right)
        if plan is not None:     # node-compact: right (m_real, dr), mask (m_real,), weights come back (m_real, heads)
            assert right.dim() == 2 and right.shape[0] == plan.m_real and mask.numel() == plan.m_real
            b, l, dr = plan.n, plan.r, right.shape[1]
            m = plan.m_real
        else:
            b, l, dr = right.shape
            m = b * l
        ha, inp = w1.shape
        heads = w2.shape[0]
        xl = 0
        if left is not None:
            left = _f32(left)
            xl = left.shape[1]
        assert inp == xl + dr, "linear1 input width must equal left + right widths"
        dev = right.device
        maskf = _f32(mask.to(torch.float32))
        w1c, w2c = _f32(w1.detach()), _f32(w2.detach())
        w1t = transposed(w1)          # for the backward's dX products
        u = torch.empty((b, ha), device=dev, dtype=torch.float32)
        t = torch.empty((m, ha), device=dev, dtype=torch.float32)
        e = torch.empty((m, heads), device=dev, dtype=torch.float32)
        weights = torch.empty((m, heads) if plan is not None else (b, l, heads), device=dev, dtype=torch.float32)
        attended = torch.empty((b, dr, heads), device=dev, dtype=torch.float32)
        pl = (None, None, 0) if plan is None else (ptr(plan.goff), ptr(plan.rowg), plan.m_real)
        call("gh_concat_att_fwd", ptr(left), ptr(right), ptr(maskf), *pl, b, l, xl, dr, ha, heads, ptr(w1c), ptr(w2c),
             ptr(u), ptr(t), ptr(e), ptr(weights), ptr(attended), stream())
        ctx.dims = (b, l, xl, dr, ha, heads, m)
        ctx.plan = plan
        ctx.params = (w1, w2)
        ctx.has_left = left is not None
        ctx.save_for_backward(left if left is not None else right.new_empty(0), right, w1t, w2c, t, weights)
        return attended, weights

    @staticmethod
    def backward(ctx, g_att, g_w):
        left, right, w1t, w2, t, weights = ctx.saved_tensors
        b, l, xl, dr, ha, heads, m = ctx.dims
        plan = ctx.plan
        dev = right.device
        if not ctx.has_left:
            left = None
        _lib.ensure_workspace(dev)
        g_att = _f32(g_att) if g_att is not None else torch.zeros((b, dr, heads), device=dev)
        g_w = _f32(g_w) if g_w is not None else None
        de = torch.empty((m, heads), device=dev, dtype=torch.float32)
        dpre = torch.empty((m, ha), device=dev, dtype=torch.float32)
        du = torch.empty((b, ha), device=dev, dtype=torch.float32)
        dleft = torch.empty((b, xl), device=dev, dtype=torch.float32) if left is not None else None
        dright = torch.empty_like(right)
        direct = all(_direct(p) for p in ctx.params)
        if direct:
            dw1, dw2 = ctx.params[0].grad, ctx.params[1].grad
        else:
            dw1 = torch.zeros((ha, xl + dr), device=dev, dtype=torch.float32)
            dw2 = torch.zeros((heads, ha), device=dev, dtype=torch.float32)
        pa = (ptr(left), ptr(right), *_plan_args(plan), b, l, xl, dr, ha, heads, ptr(w1t), ptr(w2), ptr(t), ptr(weights),
              ptr(g_att), ptr(g_w), ptr(de), ptr(dpre), ptr(du), ptr(dleft))
        if direct and WGRAD_SIDE_STREAM and b * l <= WGRAD_FEW_ROWS and right.is_cuda:
            # evidence level: everything but dW1 in line, dW1 = dpre^T [left | right] on the auxiliary stream
            call("gh_concat_att_bwd", *pa, ptr(dright), None, ptr(dw2), stream())
            _side_wgrad(dev, (left, right, dpre, du),
                        lambda: call("gh_concat_att_bwd", *pa, None, ptr(dw1), ptr(dw2), stream()))
        else:
            call("gh_concat_att_bwd", *pa, ptr(dright), ptr(dw1), ptr(dw2), stream())
        if direct:
            return dleft, dright, None, None, None, None
        return dleft, dright, None, dw1, dw2, None


def concat_att(left, right, mask, w1, w2, plan: "RaggedPlan" = None):
    """plan: node-compact `right` (m_real, dr) / `mask` (m_real,); weights are returned compact (m_real, heads)."""
    return _ConcatAtt.apply(left, right, mask, w1, w2, plan)


# --------------------------------------------------------------------------- single-query attention ablations
def _mask_f32(mask: torch.Tensor) -> torch.Tensor:
    """Masks of any dtype are compared with zero (the reference's `mask == 0`): 1.0 = real, 0.0 = padding."""
    return (mask != 0).to(torch.float32).contiguous()


class _QueryAtt(torch.autograd.Function):
    """two_branches_attention.py:29-37 (Dot) / :62-69 (BiLinear, q = W(left)): csrc/attention_ops.hip gh_query_att_*."""

    @staticmethod
    def forward(ctx, q, right, mask):
        _lib.require_cuda(q, right, mask)
        q, right = _f32(q), _f32(right)
        b, l, d = right.shape
        assert q.shape == (b, d) and mask.shape == (b, l), "query_att: q (B,D), right (B,L,D), mask (B,L)"
        weights = torch.empty((b, l), device=right.device, dtype=torch.float32)
        avg = torch.empty((b, d), device=right.device, dtype=torch.float32)
        call("gh_query_att_fwd", ptr(q), ptr(right), ptr(_mask_f32(mask)), b, l, d, ptr(weights), ptr(avg), stream())
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(q, right, weights)
        return avg, weights

    @staticmethod
    def backward(ctx, g_avg, g_w):
        q, right, weights = ctx.saved_tensors
        b, l, d = right.shape
        g_avg = _f32(g_avg) if g_avg is not None else torch.zeros_like(q)
        g_w = _f32(g_w) if g_w is not None else None
        dq = torch.empty_like(q)
        dright = torch.empty_like(right)
        call("gh_query_att_bwd", ptr(q), ptr(right), ptr(weights), ptr(g_avg), ptr(g_w), b, l, d, ptr(dq), ptr(dright), stream())
        return dq, dright, None


def query_att(q, right, mask):
    """q (B,D), right (B,L,D), mask (B,L) -> avg (B,D), weights (B,L); both outputs are differentiable."""
    return _QueryAtt.apply(q, right, mask)


class _TanhAtt(torch.autograd.Function):
    """two_branches_attention.py:183-190 (BiLinearTanh) / self_attention.py:39-47, :143-150: gh_tanh_att_*."""

    @staticmethod
    def forward(ctx, pre, u, w2, mask, values):
        _lib.require_cuda(pre, u, w2, mask, values)
        pre, values = _f32(pre), _f32(values)
        b, l, ha = pre.shape
        heads, dv = w2.shape[0], values.shape[2]
        assert w2.shape[1] == ha and values.shape[:2] == (b, l) and mask.shape == (b, l), \
            "tanh_att: pre (B,L,H), w2 (C,H), mask (B,L), values (B,L,X)"
        if u is not None:
            u = _f32(u)
            assert u.shape == (b, ha), "tanh_att: u (B,H)"
        w2c = _f32(w2.detach())
        dev = pre.device
        t = torch.empty((b, l, ha), device=dev, dtype=torch.float32)
        weights = torch.empty((b, l, heads), device=dev, dtype=torch.float32)
        attended = torch.empty((b, heads, dv), device=dev, dtype=torch.float32)
        call("gh_tanh_att_fwd", ptr(pre), ptr(u), ptr(w2c), ptr(_mask_f32(mask)), ptr(values), b, l, ha, heads, dv, ptr(t),
             ptr(weights), ptr(attended), stream())
        ctx.set_materialize_grads(False)
        ctx.has_u = u is not None
        ctx.save_for_backward(t, w2c, weights, values)
        return attended, weights

    @staticmethod
    def backward(ctx, g_att, g_w):
        t, w2, weights, values = ctx.saved_tensors
        b, l, ha = t.shape
        heads, dv = w2.shape[0], values.shape[2]
        dev = t.device
        _lib.ensure_workspace(dev)      # the per-sequence dW2 partials
        g_att = _f32(g_att) if g_att is not None else torch.zeros((b, heads, dv), device=dev)
        g_w = _f32(g_w) if g_w is not None else None
        dpre = torch.empty_like(t)
        du = torch.empty((b, ha), device=dev, dtype=torch.float32) if ctx.has_u else None
        dw2 = torch.zeros((heads, ha), device=dev, dtype=torch.float32)
        dvalues = torch.empty_like(values)
        call("gh_tanh_att_bwd", ptr(t), ptr(w2), ptr(weights), ptr(values), ptr(g_att), ptr(g_w), b, l, ha, heads, dv, ptr(dpre),
             ptr(du), ptr(dw2), ptr(dvalues), stream())
        return dpre, du, dw2, None, dvalues


def tanh_att(pre, u, w2, mask, values):
    """pre (B,L,H), u (B,H) or None, w2 (C,H), mask (B,L), values (B,L,X) -> attended (B,C,X), weights (B,L,C):
    e = w2 tanh(pre + u), masked softmax over L per head, weighted sum of `values`.  Both outputs are differentiable."""
    return _TanhAtt.apply(pre, u, w2, mask, values)


# --------------------------------------------------------------------------- multi-head query/key/value attention
def _rows_ld(t: torch.Tensor) -> torch.Tensor:
    """(B, L, W) fp32 whose rows the kernels can read in place: unit stride along W and row r of batch i at (i * L + r) * ld
    -- a contiguous tensor or a column slice of one (ld = stride(1) > W); anything else is copied."""
    if t.dtype != torch.float32:
        t = t.float()
    if t.is_contiguous():
        return t
    s0, s1, s2 = t.stride()
    if s2 == 1 and s1 >= t.shape[2] and s0 == t.shape[1] * s1:
        return t
    return t.contiguous()


def _ld(t: torch.Tensor) -> int:
    return t.shape[2] if t.is_contiguous() else t.stride(1)


class _MhaSdpa(torch.autograd.Function):
    """two_branches_attention.py:334-341 + :414-421 (the head split, softmax(q k^T) v with the mask, the head merge):
    csrc/mha_ops.hip gh_mha_sdpa_*."""

    @staticmethod
    def forward(ctx, q, k, v, mask, heads):
        if mask is None:
            raise TypeError("mha_sdpa: mask is None; a bool mask (B,Lq,Lk) is required, as the reference's masked_fill requires it")
        _lib.require_cuda(q, k, v, mask)
        if mask.dtype != torch.bool:
            raise RuntimeError(f"mha_sdpa: the mask must be a bool tensor (True = masked), got {mask.dtype}")
        assert q.dim() == 3 and k.dim() == 3 and v.dim() == 3, "mha_sdpa: q (B,Lq,H*dk), k (B,Lk,H*dk), v (B,Lk,H*dv)"
        q, k, v = _rows_ld(q), _rows_ld(k), _rows_ld(v)
        b, lq, wq = q.shape
        lk, wv = k.shape[1], v.shape[2]
        assert k.shape == (b, lk, wq) and v.shape[:2] == (b, lk) and wq % heads == 0 and wv % heads == 0 and \
            mask.shape == (b, lq, lk), "mha_sdpa: q (B,Lq,H*dk), k (B,Lk,H*dk), v (B,Lk,H*dv), mask (B,Lq,Lk)"
        dk, dv = wq // heads, wv // heads
        m8 = mask.contiguous().view(torch.uint8)
        weights = torch.empty((heads * b, lq, lk), device=q.device, dtype=torch.float32)
        out = torch.empty((b, lq, heads * dv), device=q.device, dtype=torch.float32)
        call("gh_mha_sdpa_fwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), _ld(q), _ld(k), _ld(v), ptr(m8), b, heads, lq, lk, dk, dv,
             ptr(weights), ptr(out), heads * dv, stream())
        ctx.set_materialize_grads(False)
        ctx.dims = (b, heads, lq, lk, dk, dv)
        ctx.save_for_backward(q, k, v, weights)
        return out, weights

    @staticmethod
    def backward(ctx, g_out, g_w):
        q, k, v, weights = ctx.saved_tensors
        b, heads, lq, lk, dk, dv = ctx.dims
        g_out = _f32(g_out) if g_out is not None else torch.zeros((b, lq, heads * dv), device=q.device)
        g_w = _f32(g_w) if g_w is not None else None
        ds = torch.empty_like(weights)
        dq = torch.empty((b, lq, heads * dk), device=q.device, dtype=torch.float32)
        dkk = torch.empty((b, lk, heads * dk), device=q.device, dtype=torch.float32)
        dvv = torch.empty((b, lk, heads * dv), device=q.device, dtype=torch.float32)
        call("gh_mha_sdpa_bwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), _ld(q), _ld(k), _ld(v), ptr(weights), ptr(g_out), heads * dv,
             ptr(g_w), b, heads, lq, lk, dk, dv, ptr(ds), ptr(dq), heads * dk, ptr(dkk), heads * dk, ptr(dvv), heads * dv, stream())
        return dq, dkk, dvv, None, None


def mha_sdpa(q, k, v, mask, heads: int):
    """q (B,Lq,H*dk), k (B,Lk,H*dk), v (B,Lk,H*dv) with head h in the columns [h*d, (h+1)*d) (column slices of a wider tensor
    are read in place), mask (B,Lq,Lk) bool with True = masked, shared by the heads -> out (B,Lq,H*dv), weights (H*B,Lq,Lk) in
    the reference's head-major order.  softmax(q_h k_h^T) without a temperature; masked weights are exactly 0, a fully masked
    row is all zero.  Both outputs are differentiable."""
    return _MhaSdpa.apply(q, k, v, mask, heads)


class _AddLayerNorm(torch.autograd.Function):
    """two_branches_attention.py:345 layer_norm(output + residual) / :267 layer_norm(tmp): gh_add_layernorm_*."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, eps):
        _lib.require_cuda(x, res, weight, bias)
        x2 = _f32(x).reshape(-1, x.shape[-1])
        rows, d = x2.shape
        assert weight.shape == (d,) and bias.shape == (d,), "add_layernorm: weight (D,), bias (D,)"
        r2 = None
        if res is not None:
            assert res.shape == x.shape, "add_layernorm: res has the shape of x"
            r2 = _f32(res).reshape(rows, d)
        wc, bc = _f32(weight.detach()), _f32(bias.detach())
        y = torch.empty_like(x2)
        mean = torch.empty((rows,), device=x2.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        call("gh_add_layernorm_fwd", ptr(x2), ptr(r2), ptr(wc), ptr(bc), float(eps), rows, d, ptr(y), ptr(mean), ptr(rstd), stream())
        ctx.has_res = res is not None
        ctx.xshape = x.shape
        ctx.save_for_backward(x2, r2, wc, mean, rstd)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, g):
        x2, r2, wc, mean, rstd = ctx.saved_tensors
        rows, d = x2.shape
        _lib.ensure_workspace(x2.device)      # the per-workgroup dgamma / dbeta partials
        g2 = _f32(g).reshape(rows, d)
        dx = torch.empty_like(x2)
        dgamma = torch.zeros((d,), device=x2.device, dtype=torch.float32)
        dbeta = torch.zeros((d,), device=x2.device, dtype=torch.float32)
        call("gh_add_layernorm_bwd", ptr(x2), ptr(r2), ptr(wc), ptr(mean), ptr(rstd), ptr(g2), rows, d, ptr(dx), ptr(dgamma),
             ptr(dbeta), stream())
        dx = dx.view(ctx.xshape)
        return dx, (dx if ctx.has_res else None), dgamma, dbeta, None


def add_layernorm(x, res, weight, bias, eps: float = 1e-5):
    """LayerNorm(x + res) * weight + bias over the last axis (res may be None), biased variance."""
    return _AddLayerNorm.apply(x, res, weight, bias, eps)


# --------------------------------------------------------------------------- what the two recurrences share
def _rnn_args(who, G, gx0, gx1, w0, w1, lens, order, bias=False, b0=None, b1=None):
    """Shapes and dtypes of one layer's operands (G gates; bias: the cell has recurrent biases b0 / b1 of its own), then the
    fp32 contiguous tensors the kernels read: (n, t_in, h, dirs), gx pair, detached w_hh pair, detached b_hh pair, lens, order."""
    dirs = 1 if gx1 is None else 2
    shapes = "%s: gx (N,T,%dH), w_hh (%dH,H)%s per direction" % (who, G, G, ", b_hh (%dH,)" % G if bias else "")
    assert gx0.dim() == 3 and w0.dim() == 2 and (w1 is None) == (gx1 is None) and (b0 is not None) == bias and \
        (b1 is None) == (gx1 is None or not bias), shapes
    n, t_in, hg = gx0.shape
    h = w0.shape[1]
    assert hg == G * h and w0.shape[0] == hg and (b0 is None or b0.shape == (hg,)) and \
        (dirs == 1 or (gx1.shape == gx0.shape and w1.shape == w0.shape and (b0 is None or b1.shape == b0.shape))), shapes
    assert lens.dtype == torch.int32 and lens.shape == (n,) and (order is None or (order.dtype == torch.int32 and order.shape == (n,))), \
        who + ": lens and order are int32 (N,)"
    f32 = lambda t: _f32(t) if t is not None else None
    const = lambda t: _f32(t.detach()) if t is not None else None
    return (n, t_in, h, dirs), (f32(gx0), f32(gx1)), (const(w0), const(w1)), (const(b0), const(b1)), lens.contiguous(), \
        (order.contiguous() if order is not None else None)


def _rnn_alloc(dev, dims, t_out, G, save):
    """y (N,t_out,dirs*H), h_n (dirs,N,H) and, when a gradient is wanted, the saved gates (dirs,N,T_in,G*H), the cell's own
    saved row and h_prev (dirs,N,T_in,H each)."""
    n, t_in, h, dirs = dims
    new = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
    saved = (new(dirs, n, t_in, G * h), new(dirs, n, t_in, h), new(dirs, n, t_in, h)) if save else (None, None, None)
    return new(n, t_out, dirs * h), new(dirs, n, h), saved


def _rnn_wgrad(hprev, dpre, G, pw, pb, need_w, need_b):
    """dW_hh = dpre^T h_prev (and db_hh = colsum(dpre) for a cell with a recurrent bias pb) of one direction: ONE call of the
    weight-gradient GEMM (gh_linear_bwd without dx), straight into the parameters' .grad where _direct allows it for every
    wanted gradient.  Returns what autograd still has to add: (dw, db), None where nothing is left."""
    if not (need_w or need_b):
        return None, None
    _lib.ensure_workspace(dpre.device)
    h = hprev.shape[-1]
    direct = need_w and _direct(pw) and (pb is None or (need_b and _direct(pb)))
    if direct:
        dw, db = pw.grad, (pb.grad if pb is not None else None)
    else:
        dw = torch.zeros((G * h, h), device=dpre.device, dtype=torch.float32)
        db = torch.zeros((G * h,), device=dpre.device, dtype=torch.float32) if pb is not None else None
    call("gh_linear_bwd", ptr(hprev), None, None, ptr(dpre), hprev.shape[0] * hprev.shape[1], h, G * h, None, ptr(dw), ptr(db), stream())
    if direct:
        return None, None
    return (dw if need_w else None), (db if need_b else None)


# --------------------------------------------------------------------------- LSTM recurrence (wrapper.py:256-276)
class _LstmSeq(torch.autograd.Function):
    """One layer's recurrence, both directions in one launch: csrc/rnn_ops.hip gh_lstm_seq_*.  The weight gradient
    dW_hh = dgates^T h_prev is ONE call of the weight-gradient GEMM per direction (gh_linear_bwd without dx)."""

    @staticmethod
    def forward(ctx, gx0, gx1, w0, w1, lens, order, t_out):
        _lib.require_cuda(gx0, gx1, w0, w1, lens, order)
        dims, (gx0, gx1), (wc0, wc1), _, lens, order = _rnn_args("lstm_seq", 4, gx0, gx1, w0, w1, lens, order)
        n, t_in, h, dirs = dims
        y, hn, (gates, cs, hprev) = _rnn_alloc(gx0.device, dims, t_out, 4, any(ctx.needs_input_grad[:4]))
        cn = torch.empty_like(hn)
        call("gh_lstm_seq_fwd", ptr(gx0), ptr(gx1), 4 * h, ptr(wc0), ptr(wc1), ptr(lens), ptr(order), n, t_in, t_out, h, dirs, ptr(y),
             dirs * h, ptr(gates), ptr(cs), ptr(hprev), ptr(hn), ptr(cn), stream())
        ctx.dims = (n, t_in, t_out, h, dirs)
        ctx.params = (w0, w1)
        ctx.save_for_backward(wc0, wc1, lens, order, gates, cs, hprev)
        ctx.mark_non_differentiable(cn)
        ctx.set_materialize_grads(False)
        return y, hn, cn

    @staticmethod
    def backward(ctx, g_y, g_hn, _g_cn):
        wc0, wc1, lens, order, gates, cs, hprev = ctx.saved_tensors
        n, t_in, t_out, h, dirs = ctx.dims
        g_y = _f32(g_y) if g_y is not None else None
        g_hn = _f32(g_hn) if g_hn is not None else None
        dgates = torch.empty_like(gates)
        call("gh_lstm_seq_bwd", ptr(wc0), ptr(wc1), ptr(lens), ptr(order), n, t_in, t_out, h, dirs, ptr(g_y), dirs * h, ptr(g_hn),
             ptr(gates), ptr(cs), ptr(dgates), stream())
        dws = [None, None]
        for d in range(dirs):
            dws[d], _ = _rnn_wgrad(hprev[d], dgates[d], 4, ctx.params[d], None, ctx.needs_input_grad[2 + d], False)
        return dgates[0], (dgates[1] if dirs == 2 else None), dws[0], dws[1], None, None, None


def lstm_seq(gx, w_hh, lens, order, t_out: int):
    """The recurrence of one LSTM layer.  gx / w_hh: one tensor per direction (forward, then reverse) -- gx (N,T_in,4H) =
    x W_ih^T + b_ih + b_hh in torch's gate order i, f, g, o, w_hh (4H,H) as nn.LSTM stores it; lens (N,) int32 on the device
    (clamped into [0, min(T_in, t_out)]); order (N,) int32 or None: the processing order (a permutation sorted by length keeps
    a tile's sequences alike), outputs stay in the rows of the inputs.  Returns y (N,t_out,dirs*H) with exact zeros at
    t >= len, h_n and c_n (dirs,N,H); y and h_n are differentiable."""
    gx, w_hh = list(gx), list(w_hh)
    assert len(gx) == len(w_hh) and len(gx) in (1, 2), "lstm_seq: one or two directions"
    return _LstmSeq.apply(gx[0], gx[1] if len(gx) == 2 else None, w_hh[0], w_hh[1] if len(gx) == 2 else None, lens, order, int(t_out))


# --------------------------------------------------------------------------- GRU recurrence (wrapper.py:306-327)
class _GruSeq(torch.autograd.Function):
    """One layer's recurrence, both directions in one launch: csrc/rnn_ops.hip gh_gru_seq_*.  The backward kernel writes the
    gradient of gx and the gradient `da` of the recurrent pre-activations (they differ in the n third by the factor r);
    dW_hh = da^T h_prev and db_hh = colsum(da) are ONE call of the weight-gradient GEMM per direction (gh_linear_bwd without dx)."""

    @staticmethod
    def forward(ctx, gx0, gx1, w0, w1, b0, b1, lens, order, t_out):
        _lib.require_cuda(gx0, gx1, w0, w1, b0, b1, lens, order)
        dims, (gx0, gx1), (wc0, wc1), (bc0, bc1), lens, order = _rnn_args("gru_seq", 3, gx0, gx1, w0, w1, lens, order, True, b0, b1)
        n, t_in, h, dirs = dims
        y, hn, (gates, an, hprev) = _rnn_alloc(gx0.device, dims, t_out, 3, any(ctx.needs_input_grad[:6]))
        call("gh_gru_seq_fwd", ptr(gx0), ptr(gx1), 3 * h, ptr(wc0), ptr(wc1), ptr(bc0), ptr(bc1), ptr(lens), ptr(order), n, t_in, t_out, h,
             dirs, ptr(y), dirs * h, ptr(gates), ptr(an), ptr(hprev), ptr(hn), stream())
        ctx.dims = (n, t_in, t_out, h, dirs)
        ctx.params = (w0, w1, b0, b1)
        ctx.save_for_backward(wc0, wc1, lens, order, gates, an, hprev)
        ctx.set_materialize_grads(False)
        return y, hn

    @staticmethod
    def backward(ctx, g_y, g_hn):
        wc0, wc1, lens, order, gates, an, hprev = ctx.saved_tensors
        n, t_in, t_out, h, dirs = ctx.dims
        g_y = _f32(g_y) if g_y is not None else None
        g_hn = _f32(g_hn) if g_hn is not None else None
        dgx, da = torch.empty_like(gates), torch.empty_like(gates)
        call("gh_gru_seq_bwd", ptr(wc0), ptr(wc1), ptr(lens), ptr(order), n, t_in, t_out, h, dirs, ptr(g_y), dirs * h, ptr(g_hn),
             ptr(gates), ptr(an), ptr(hprev), ptr(dgx), ptr(da), stream())
        dws, dbs = [None, None], [None, None]
        for d in range(dirs):
            dws[d], dbs[d] = _rnn_wgrad(hprev[d], da[d], 3, ctx.params[d], ctx.params[2 + d], ctx.needs_input_grad[2 + d],
                                        ctx.needs_input_grad[4 + d])
        return dgx[0], (dgx[1] if dirs == 2 else None), dws[0], dws[1], dbs[0], dbs[1], None, None, None


def gru_seq(gx, w_hh, b_hh, lens, order, t_out: int):
    """The recurrence of one GRU layer.  gx / w_hh / b_hh: one tensor per direction (forward, then reverse) -- gx (N,T_in,3H) =
    x W_ih^T + b_ih ALONE in torch's gate order r, z, n; w_hh (3H,H) and b_hh (3H,) as nn.GRU stores them (b_hh stays with the
    kernel: its n third is multiplied by r); lens (N,) int32 on the device (clamped into [0, min(T_in, t_out)]); order (N,)
    int32 or None: the processing order, outputs stay in the rows of the inputs.  Returns y (N,t_out,dirs*H) with exact zeros
    at t >= len and h_n (dirs,N,H); differentiable in gx, w_hh and b_hh."""
    gx, w_hh, b_hh = list(gx), list(w_hh), list(b_hh)
    assert len(gx) == len(w_hh) == len(b_hh) and len(gx) in (1, 2), "gru_seq: one or two directions"
    two = len(gx) == 2
    return _GruSeq.apply(gx[0], gx[1] if two else None, w_hh[0], w_hh[1] if two else None, b_hh[0], b_hh[1] if two else None, lens, order,
                         int(t_out))


# --------------------------------------------------------------------------- BiDAF: attention flow and highway gate
class _OutBuffer:
    """The caller's destination of ops.att_flow, handed to the autograd function as a plain object: the buffer is where the
    output lives, not an input of the graph."""

    def __init__(self, t):
        self.t = t


class _AttFlow(torch.autograd.Function):
    """bidaf_model.py:72-104 (trilinear scores, both attentions, the four-way cat): csrc/bidaf_ops.hip gh_att_flow_*."""

    @staticmethod
    def forward(ctx, c, q, w_c, w_q, w_cq, b_c, b_q, b_cq, out):
        out = out.t
        _lib.require_cuda(c, q, w_c, w_q, w_cq, b_c, b_q, b_cq, out)
        assert c.dim() == 3 and q.dim() == 3 and c.shape[0] == q.shape[0] and c.shape[2] == q.shape[2], \
            "att_flow: c (B,Lc,D), q (B,Lq,D)"
        c, q = _rows_ld(c), _rows_ld(q)
        b, lc, d = c.shape
        lq = q.shape[1]
        assert w_c.numel() == d and w_q.numel() == d and w_cq.numel() == d and b_c.numel() == 1 and b_q.numel() == 1 and \
            b_cq.numel() == 1, "att_flow: w_c, w_q, w_cq hold D weights, b_c, b_q, b_cq one bias each"
        ws = [_f32(w.detach()).reshape(-1) for w in (w_c, w_q, w_cq)]
        bs = [_f32(t.detach()).reshape(-1) for t in (b_c, b_q, b_cq)]
        dev = c.device
        if out is None:
            x = torch.empty((b, lc, 4 * d), device=dev, dtype=torch.float32)
        else:
            x = out
            assert x.shape == (b, lc, 4 * d) and x.dtype == torch.float32 and _rows_ld(x) is x, \
                "att_flow: out is fp32 (B,Lc,4D), contiguous or a column slice of a contiguous tensor"
        a = torch.empty((b, lc, lq), device=dev, dtype=torch.float32)
        amax = torch.empty((b, lc), device=dev, dtype=torch.int32)
        m = torch.empty((b, lc), device=dev, dtype=torch.float32)
        beta = torch.empty((b, lc), device=dev, dtype=torch.float32)
        q2c = torch.empty((b, d), device=dev, dtype=torch.float32)
        call("gh_att_flow_fwd", c.data_ptr(), q.data_ptr(), _ld(c), _ld(q), ptr(ws[0]), ptr(ws[1]), ptr(ws[2]), ptr(bs[0]), ptr(bs[1]),
             ptr(bs[2]), b, lc, lq, d, x.data_ptr(), _ld(x), ptr(a), ptr(amax), ptr(m), ptr(beta), ptr(q2c), stream())
        ctx.dims = (b, lc, lq, d)
        ctx.shapes = tuple(t.shape for t in (w_c, w_q, w_cq, b_c, b_q, b_cq))
        ctx.save_for_backward(c, q, ws[0], ws[1], ws[2], x, a, amax, beta, q2c)
        return x

    @staticmethod
    def backward(ctx, g_x):
        c, q, w_c, w_q, w_cq, x, a, amax, beta, q2c = ctx.saved_tensors
        b, lc, lq, d = ctx.dims
        dev = c.device
        _lib.ensure_workspace(dev)      # the per-batch-element / per-tile dw partials
        g_x = _rows_ld(g_x)
        ds = torch.empty_like(a)
        dm = torch.empty_like(beta)
        dq2c = torch.empty_like(q2c)
        dc = torch.empty((b, lc, d), device=dev, dtype=torch.float32)
        dq = torch.empty((b, lq, d), device=dev, dtype=torch.float32)
        dws = [torch.zeros((d,), device=dev, dtype=torch.float32) for _ in range(3)]
        call("gh_att_flow_bwd", c.data_ptr(), q.data_ptr(), _ld(c), _ld(q), ptr(w_c), ptr(w_q), ptr(w_cq), x.data_ptr(), _ld(x), ptr(a),
             ptr(amax), ptr(beta), ptr(q2c), g_x.data_ptr(), _ld(g_x), b, lc, lq, d, ptr(ds), ptr(dm), ptr(dq2c), ptr(dc), d, ptr(dq), d,
             ptr(dws[0]), ptr(dws[1]), ptr(dws[2]), stream())
        sh = ctx.shapes
        # the three bias gradients are mathematically zero (sum_j dS_ij = dm_i, sum_i dm_i = 0): exact zeros, not None
        dbs = [torch.zeros(sh[3 + i], device=dev, dtype=torch.float32) for i in range(3)]
        return (dc, dq, dws[0].view(sh[0]), dws[1].view(sh[1]), dws[2].view(sh[2]), dbs[0], dbs[1], dbs[2], None)


def att_flow(c, q, w_c, w_q, w_cq, b_c, b_q, b_cq, out=None):
    """The attention-flow layer of bidaf_model.py:72-104.  c (B,Lc,D), q (B,Lq,D) (column slices of a wider tensor are read in
    place); w_c, w_q, w_cq: the D weights of the three Linear(D, 1) (any shape with D elements), b_c, b_q, b_cq their
    1-element biases -> x (B,Lc,4D) = [c, c2q, c * c2q, c * q2c], written into `out` (fp32, contiguous or a column slice of a
    contiguous tensor) when given; the buffer must not be overwritten before the backward, which re-reads c2q from it.  There
    is no mask, as in the reference: zero rows of c and q take part in both softmaxes.
    The row maximum behind q2c sends its gradient to the lowest index attaining it, as torch.max does.  The gradients of the
    three biases are mathematically zero and come back as exact zeros."""
    return _AttFlow.apply(c, q, w_c, w_q, w_cq, b_c, b_q, b_cq, _OutBuffer(out))


class _Highway(torch.autograd.Function):
    """bidaf_model.py:62 with the ReLU / Sigmoid of :22-24 folded in: gh_highway_*."""

    @staticmethod
    def forward(ctx, x, h_pre, g_pre):
        _lib.require_cuda(x, h_pre, g_pre)
        assert x.shape == h_pre.shape == g_pre.shape and x.dim() >= 1, "highway: x, h_pre and g_pre have one shape"
        x2, h2, g2 = (_f32(t).reshape(-1, t.shape[-1]) for t in (x, h_pre, g_pre))
        rows, d = x2.shape
        y = torch.empty_like(x2)
        call("gh_highway_fwd", ptr(x2), ptr(h2), ptr(g2), rows, d, ptr(y), stream())
        ctx.save_for_backward(x2, h2, g2)
        ctx.xshape = x.shape
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, g):
        x2, h2, g2 = ctx.saved_tensors
        rows, d = x2.shape
        gy = _f32(g).reshape(rows, d)
        dh, dg, dx = torch.empty_like(x2), torch.empty_like(x2), torch.empty_like(x2)
        call("gh_highway_bwd", ptr(x2), ptr(h2), ptr(g2), ptr(gy), rows, d, ptr(dh), ptr(dg), ptr(dx), stream())
        return dx.view(ctx.xshape), dh.view(ctx.xshape), dg.view(ctx.xshape)


def highway(x, h_pre, g_pre):
    """y = sigmoid(g_pre) * relu(h_pre) + (1 - sigmoid(g_pre)) * x, elementwise (one highway layer after its two projections).
    The gradient of x is the direct one only; the projections' share arrives through h_pre and g_pre."""
    return _Highway.apply(x, h_pre, g_pre)


# --------------------------------------------------------------------------- matchzoo/modules: soft alignment, matching, kernels
def _flag_bytes(t, shape, who):
    """A bool / uint8 flag tensor of `shape` as contiguous uint8 (nonzero = set), None stays None."""
    if t is None:
        return None
    assert t.dtype in (torch.bool, torch.uint8) and tuple(t.shape) == tuple(shape), \
        f"{who}: a bool (or uint8) tensor of shape {tuple(shape)} is expected, got {t.dtype} {tuple(t.shape)}"
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


class _SoftAlign(torch.autograd.Function):
    """matchzoo/modules/attention.py:50-63 and :99-105 (softmax(fill(q k^T)) v, the row zeroing, MatchModule's four-way cat):
    csrc/match_ops.hip gh_soft_align_*."""

    @staticmethod
    def forward(ctx, q, k, v, key_fill, row_zero, fill, fuse, out):
        out = out.t
        _lib.require_cuda(q, k, v, key_fill, row_zero, out)
        assert q.dim() == 3 and k.dim() == 3 and v.dim() == 3 and q.shape[0] == k.shape[0] == v.shape[0] and \
            q.shape[2] == k.shape[2] and k.shape[1] == v.shape[1], "soft_align: q (B,Lq,D), k (B,Lk,D), v (B,Lk,Dv)"
        q, k, v = _rows_ld(q), _rows_ld(k), _rows_ld(v)
        b, lq, d = q.shape
        lk, dv = v.shape[1], v.shape[2]
        kf = _flag_bytes(key_fill, (b, lk), "soft_align: key_fill")
        rz = _flag_bytes(row_zero, (b, lq), "soft_align: row_zero")
        fuse = int(bool(fuse))
        if fuse and (dv != d or rz is not None):
            raise RuntimeError(f"soft_align: fuse needs Dv == D (got {dv}, {d}) and no row_zero")
        wo = 4 * d if fuse else dv
        dev = q.device
        if out is None:
            x = torch.empty((b, lq, wo), device=dev, dtype=torch.float32)
        else:
            x = out
            assert x.shape == (b, lq, wo) and x.dtype == torch.float32 and _rows_ld(x) is x, \
                "soft_align: out is fp32 (B,Lq,Dv) -- (B,Lq,4D) with fuse --, contiguous or a column slice of a contiguous tensor"
        a = torch.empty((b, lq, lk), device=dev, dtype=torch.float32)
        call("gh_soft_align_fwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), _ld(q), _ld(k), _ld(v), ptr(kf), ptr(rz), float(fill), fuse,
             b, lq, lk, d, dv, ptr(a), x.data_ptr(), _ld(x), stream())
        ctx.dims = (b, lq, lk, d, dv, fuse)
        ctx.save_for_backward(q, k, v, kf, rz, a, x if fuse else None)
        ctx.mark_non_differentiable(a)
        return x, a

    @staticmethod
    def backward(ctx, g, _g_a):
        q, k, v, kf, rz, a, x = ctx.saved_tensors
        b, lq, lk, d, dv, fuse = ctx.dims
        dev = q.device
        g = _rows_ld(g)
        ds = torch.empty_like(a)
        dq = torch.empty((b, lq, d), device=dev, dtype=torch.float32)
        dk = torch.empty((b, lk, d), device=dev, dtype=torch.float32)
        dvv = torch.empty((b, lk, dv), device=dev, dtype=torch.float32)
        call("gh_soft_align_bwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), _ld(q), _ld(k), _ld(v), ptr(kf), ptr(rz), fuse, ptr(a),
             x.data_ptr() if fuse else None, _ld(x) if fuse else 0, g.data_ptr(), _ld(g), b, lq, lk, d, dv, ptr(ds), ptr(dq), d, ptr(dk), d,
             ptr(dvv), dv, stream())
        return dq, dk, dvv, None, None, None, None, None


def soft_align(q, k, v, key_fill, row_zero=None, fill=-1e-7, fuse=False, out=None):
    """Soft alignment between two sequences: q (B,Lq,D), k (B,Lk,D), v (B,Lk,Dv) (column slices of a wider tensor are read in
    place), key_fill (B,Lk) bool, row_zero (B,Lq) bool or None -> (out, weights (B,Lq,Lk)).
    S = q k^T with S[:, :, j] REPLACED by the constant `fill` (finite) where key_fill[:, j]: as in the reference's
    masked_fill(mask, -1e-7), a filled key is not excluded, it keeps a weight (and receives the gradient of v), only its score
    is a constant and sends nothing to q and k.  weights = softmax(S) over the keys; o = weights v, zero in the rows of
    row_zero.  out = o (B,Lq,Dv), or with fuse (Dv == D, no row_zero) [q, o, q - o, q * o] (B,Lq,4D); it is written into `out`
    when given (fp32, contiguous or a column slice of a contiguous tensor), which must not be overwritten before the backward
    when fuse is set.  Differentiable in q, k and v through `out`; `weights` is returned for inspection only."""
    return _SoftAlign.apply(q, k, v, key_fill, row_zero, fill, fuse, _OutBuffer(out))


LIN_ATT_MODES = (0, 1, 2)


class _LinAtt(torch.autograd.Function):
    """matchzoo/modules/attention.py:35-38: gh_lin_att_*."""

    @staticmethod
    def forward(ctx, x, w, mode):
        _lib.require_cuda(x, w)
        assert x.dim() == 3 and w.numel() == x.shape[2], "lin_att: x (B,L,D), w holds D weights"
        assert mode in LIN_ATT_MODES, "lin_att: mode is 0, 1 or 2"
        x = _f32(x)
        b, l, d = x.shape
        wc = _f32(w.detach()).reshape(-1)
        a = torch.empty((b, l), device=x.device, dtype=torch.float32)
        call("gh_lin_att_fwd", ptr(x), ptr(wc), int(mode), b, l, d, ptr(a), stream())
        ctx.save_for_backward(x, wc, a)
        ctx.wshape = w.shape
        return a

    @staticmethod
    def backward(ctx, g):
        x, wc, a = ctx.saved_tensors
        b, l, d = x.shape
        g = _f32(g)
        dx = torch.empty_like(x)
        part = torch.empty((b, d), device=x.device, dtype=torch.float32)
        dw = torch.empty((d,), device=x.device, dtype=torch.float32)
        call("gh_lin_att_bwd", ptr(x), ptr(wc), ptr(a), ptr(g), b, l, d, ptr(dx), ptr(part), ptr(dw), stream())
        return dx, dw.view(ctx.wshape), None


def lin_att(x, w, mode=0):
    """x (B,L,D), w: the D weights of a Linear(D, 1, bias=False) -> weights (B,L): the softmax of s = x w over the kept
    positions, exactly 0 elsewhere.  mode 0 excludes s == 0 (an all-zero row of x scores exactly 0), mode 1 excludes s != 1,
    mode 2 excludes nothing: the reference's (x != m) / (mask == m) pair for m == 0, m == 1 and any other m.  A sequence
    without a kept position gives NaN in its own row."""
    return _LinAtt.apply(x, w, mode)


class _MatchDot(torch.autograd.Function):
    """matchzoo/modules/matching.py:46-50: gh_match_dot_*."""

    @staticmethod
    def forward(ctx, x, y, normalize):
        _lib.require_cuda(x, y)
        assert x.dim() == 3 and y.dim() == 3 and x.shape[0] == y.shape[0] and x.shape[2] == y.shape[2], \
            "match_dot: x (B,L,D), y (B,R,D)"
        x, y = _rows_ld(x), _rows_ld(y)
        b, l, d = x.shape
        r = y.shape[1]
        dev = x.device
        normalize = int(bool(normalize))
        ix = torch.empty((b, l), device=dev, dtype=torch.float32) if normalize else None
        iy = torch.empty((b, r), device=dev, dtype=torch.float32) if normalize else None
        out = torch.empty((b, l, r), device=dev, dtype=torch.float32)
        call("gh_match_dot_fwd", x.data_ptr(), y.data_ptr(), _ld(x), _ld(y), normalize, b, l, r, d, ptr(ix), ptr(iy), ptr(out), stream())
        ctx.normalize = normalize
        ctx.save_for_backward(x, y, ix, iy)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y, ix, iy = ctx.saved_tensors
        b, l, d = x.shape
        r = y.shape[1]
        g = _f32(g)
        dx = torch.empty((b, l, d), device=x.device, dtype=torch.float32)
        dy = torch.empty((b, r, d), device=x.device, dtype=torch.float32)
        call("gh_match_dot_bwd", x.data_ptr(), y.data_ptr(), _ld(x), _ld(y), ctx.normalize, ptr(ix), ptr(iy), ptr(g), b, l, r, d, ptr(dx),
             ptr(dy), stream())
        return dx, dy, None


def match_dot(x, y, normalize=False):
    """x (B,L,D), y (B,R,D) (column slices are read in place) -> (B,L,R) = x y^T, of the L2-normalised rows (F.normalize, eps
    1e-12) with `normalize`.  A row with a norm <= 1e-12 is divided by 1e-12, and its gradient is of the order 1e12 times the
    upstream one, exactly as torch gives."""
    return _MatchDot.apply(x, y, normalize)


MATCH_BCAST_OPS = {"mul": 0, "plus": 1, "minus": 2, "concat": 3}


class _MatchBcast(torch.autograd.Function):
    """matchzoo/modules/matching.py:52-61: gh_match_bcast_*."""

    @staticmethod
    def forward(ctx, x, y, op):
        _lib.require_cuda(x, y)
        assert x.dim() == 3 and y.dim() == 3 and x.shape[0] == y.shape[0] and x.shape[2] == y.shape[2], \
            "match_bcast: x (B,L,D), y (B,R,D)"
        x, y = _f32(x), _f32(y)
        b, l, d = x.shape
        r = y.shape[1]
        out = torch.empty((b, l, r, 2 * d if op == 3 else d), device=x.device, dtype=torch.float32)
        call("gh_match_bcast_fwd", ptr(x), ptr(y), op, b, l, r, d, ptr(out), stream())
        ctx.op = op
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        b, l, d = x.shape
        r = y.shape[1]
        g = _f32(g)
        dx, dy = torch.empty_like(x), torch.empty_like(y)
        call("gh_match_bcast_bwd", ptr(x), ptr(y), ptr(g), ctx.op, b, l, r, d, ptr(dx), ptr(dy), stream())
        return dx, dy, None


def match_bcast(x, y, op: str):
    """x (B,L,D), y (B,R,D) -> (B,L,R,D) = x[:, :, None] op y[:, None] for op 'mul', 'plus', 'minus'; 'concat' gives
    (B,L,R,2D) = [x, y].  Written once, without the reference's two repeat copies."""
    if op not in MATCH_BCAST_OPS:
        raise ValueError("match_bcast: %s is not one of %s" % (op, list(MATCH_BCAST_OPS)))
    return _MatchBcast.apply(x, y, MATCH_BCAST_OPS[op])


class _GaussKernel(torch.autograd.Function):
    """matchzoo/modules/gaussian_kernel.py:34-36: gh_gauss_kernel_*."""

    @staticmethod
    def forward(ctx, x, mu, sigma):
        _lib.require_cuda(x)
        x = _f32(x)
        y = torch.empty_like(x)
        call("gh_gauss_kernel_fwd", ptr(x), float(mu), float(sigma), x.numel(), ptr(y), stream())
        ctx.params = (float(mu), float(sigma))
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        g = _f32(g)
        dx = torch.empty_like(x)
        call("gh_gauss_kernel_bwd", ptr(x), ptr(y), ptr(g), ctx.params[0], ctx.params[1], x.numel(), ptr(dx), stream())
        return dx, None, None


def gauss_kernel(x, mu: float, sigma: float):
    """exp(-0.5 (x - mu)^2 / sigma^2), elementwise; sigma == 0 is refused."""
    return _GaussKernel.apply(x, mu, sigma)


# --------------------------------------------------------------------------- linear
class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        x2 = _f32(x).reshape(-1, x.shape[-1])
        m, k = x2.shape
        n = w.shape[0]
        wc = _f32(w.detach())
        y = torch.empty((m, n), device=x.device, dtype=torch.float32)
        bc = _f32(b.detach()) if b is not None else None
        call("gh_linear_fwd", ptr(x2), ptr(wc), ptr(bc), ptr(y), m, k, n, stream())
        ctx.save_for_backward(x2, transposed(w), wc)
        ctx.params = (w, b)
        ctx.has_bias = b is not None
        ctx.xshape = x.shape
        return y.view(*x.shape[:-1], n)

    @staticmethod
    def backward(ctx, g):
        x2, wt, wc = ctx.saved_tensors
        m, k = x2.shape
        n = wt.shape[1]
        g2 = _f32(g).reshape(m, n)
        _lib.ensure_workspace(g.device)
        dx = torch.empty((m, k), device=g.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        pw, pb = ctx.params
        direct = _direct(pw) and (pb is None or _direct(pb))
        if direct:
            dw, db = pw.grad, (pb.grad if pb is not None else None)
        else:
            dw = torch.zeros((n, k), device=g.device, dtype=torch.float32)
            db = torch.zeros((n,), device=g.device, dtype=torch.float32) if ctx.has_bias else None
        if direct and WGRAD_SIDE_STREAM and m <= WGRAD_FEW_ROWS and g2.is_cuda:
            if dx is not None:
                call("gh_linear_bwd", ptr(x2), ptr(wt), ptr(wc), ptr(g2), m, k, n, ptr(dx), None, None, stream())
            _side_wgrad(g2.device, (x2, g2),
                        lambda: call("gh_linear_bwd", ptr(x2), ptr(wt), ptr(wc), ptr(g2), m, k, n, None, ptr(dw), ptr(db), stream()))
        else:
            call("gh_linear_bwd", ptr(x2), ptr(wt), ptr(wc), ptr(g2), m, k, n, ptr(dx), ptr(dw), ptr(db), stream())
        dxo = dx.view(ctx.xshape) if dx is not None else None
        if direct:
            return dxo, None, None
        return dxo, dw, db


def linear(x, w, b=None):
    return _Linear.apply(x, w, b)


def linear_wgrad_bf16(g16: torch.Tensor, x16: torch.Tensor, dw: torch.Tensor, db: torch.Tensor = None):
    """dw[n][k] += g16^T x16, db[n] += colsum(g16) for bf16 activations / upstream gradients [m][n], [m][k] (row views with a
    leading dimension are taken as they are) and fp32 accumulators -- gh_linear_wgrad_bf16, the weight-gradient GEMM of the
    bf16 storage pipeline (gh_ggnn_cell_bwd_bf16) on its own.  Returns dw."""
    assert g16.dtype == torch.bfloat16 and x16.dtype == torch.bfloat16 and dw.dtype == torch.float32
    assert g16.dim() == 2 and x16.dim() == 2 and g16.shape[0] == x16.shape[0] and g16.stride(1) == 1 and x16.stride(1) == 1
    m, n = g16.shape
    k = x16.shape[1]
    assert tuple(dw.shape) == (n, k) and dw.stride(1) == 1 and (db is None or (db.dtype == torch.float32 and db.numel() == n and db.is_contiguous()))
    _lib.ensure_workspace(g16.device)
    # (row views with a leading dimension: the raw addresses, `ptr` insists on contiguous tensors)
    call("gh_linear_wgrad_bf16", g16.data_ptr(), g16.stride(0), x16.data_ptr(), x16.stride(0), m, n, k, dw.data_ptr(), dw.stride(0), ptr(db), stream())
    return dw


# --------------------------------------------------------------------------- graph encoders (wrapper.py:7-151 GAT, GCN)
class _FeatDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, seed):
        x = _f32(x)
        y = torch.empty_like(x)
        cols = x.shape[-1]
        call("gh_feat_dropout", ptr(x), ptr(y), x.numel() // cols, cols, float(p), int(seed), stream())
        ctx.p, ctx.seed = p, seed
        return y

    @staticmethod
    def backward(ctx, g):
        g = _f32(g)
        dx = torch.empty_like(g)
        cols = g.shape[-1]
        call("gh_feat_dropout", ptr(g), ptr(dx), g.numel() // cols, cols, float(ctx.p), int(ctx.seed), stream())
        return dx, None, None


def feat_dropout(x, p: float, seed: int):
    """F.dropout(x, p) with the stateless mask: element (row, col) of x viewed as (numel/cols, cols) is kept iff
    dropout_mask_reference(seed, numel/cols, cols, p)[row, col]."""
    if p <= 0:
        return x
    return _FeatDropout.apply(x, p, seed)


def gat_dropout_mask(seed: int, layer: int, heads: int, n: int, r: int, p: float):
    """Host replica (tests) of gh_gat_layer_fwd's attention dropout: bool (heads, n, r, r), True = kept."""
    m = dropout_mask_reference(seed, (layer + 1) * heads * n * r, r, p)
    return m[layer * heads * n * r:].reshape(heads, n, r, r)


def _gat_operands(heads):
    """(W_cat^T [H*f][din], W_cat [din][H*f], a [H][2f]) of a list of GraphAttentionLayer-like modules (.W [din][f],
    .a [2f][1]), cached like the transposes: recomputed only when a weight is replaced, written in place or the weight
    epoch moves on."""
    ws = tuple(m.W for m in heads)
    as_ = tuple(m.a for m in heads)

    def make_lin():
        if _lib.gemm_mode() == "fp32x3p":
            call("gh_weights_changed")
        return torch.cat([_f32(w.detach()).t() for w in ws], 0).contiguous()

    w_lin = derived("gat_w_lin", ws, make_lin)
    w_cat = derived("gat_w_cat", ws, lambda: torch.cat([_f32(w.detach()) for w in ws], 1).contiguous())
    a_cat = derived("gat_a", as_, lambda: torch.cat([_f32(a.detach()).reshape(1, -1) for a in as_], 0).contiguous())
    return w_lin, w_cat, a_cat


GAT_OUTPUT, GAT_ELU, GAT_PLAIN = 0, 1, 2      # gh_gat_layer_fwd modes


class _GATLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, adj: PackedAdj, cfg, w_lin, w_cat, a_cat, *params):
        heads, f, alpha, mode, layer, drop_p, seed = cfg
        n, r = adj.n, adj.r
        x2 = _f32(x).reshape(-1, x.shape[-1])
        assert x2.shape[0] == n * r, f"GAT input has {x2.shape[0]} rows, the adjacency {n} x {r} nodes"
        din, F = x2.shape[1], heads * f
        dev = x.device
        e = lambda *s: torch.empty(s, device=dev, dtype=torch.float32)
        h, s, stats, hp = e(n * r, F), e(n * r, heads, 2), e(n * r, heads, 2), e(n * r, F)
        out = e(n * r, f) if mode == GAT_OUTPUT else e(n * r, F)
        call("gh_gat_layer_fwd", ptr(adj.bits), ptr(adj.vals), ptr(adj.keep), ptr(x2), ptr(w_lin), ptr(a_cat), n, r, din,
             heads, f, float(alpha), mode, layer, float(drop_p), int(seed), ptr(h), ptr(s), ptr(stats), ptr(hp), ptr(out),
             stream())
        ctx.save_for_backward(x2, h, s, stats, hp, out)
        ctx.adj, ctx.cfg, ctx.w_cat, ctx.a_cat, ctx.xshape = adj, cfg, w_cat, a_cat, x.shape
        return out.view(*x.shape[:-1], out.shape[-1])

    @staticmethod
    def backward(ctx, g):
        x2, h, s, stats, hp, out = ctx.saved_tensors
        heads, f, alpha, mode, layer, drop_p, seed = ctx.cfg
        adj = ctx.adj
        n, r = adj.n, adj.r
        din, F = x2.shape[1], heads * f
        g2 = _f32(g).reshape(out.shape)
        dev = g.device
        _lib.ensure_workspace(dev)
        dh = torch.empty_like(h)
        da_part = torch.empty((n, heads, 2 * f), device=dev, dtype=torch.float32)
        dx = torch.empty_like(x2) if ctx.needs_input_grad[0] else None
        dw = torch.zeros((din, F), device=dev, dtype=torch.float32)
        da = torch.zeros((heads, 2 * f), device=dev, dtype=torch.float32)
        call("gh_gat_layer_bwd", ptr(adj.bits), ptr(adj.vals), ptr(adj.keep), ptr(x2), ptr(ctx.w_cat), ptr(ctx.a_cat), n, r,
             din, heads, f, float(alpha), mode, layer, float(drop_p), int(seed), ptr(h), ptr(s), ptr(stats), ptr(hp),
             ptr(out), ptr(g2), ptr(dh), ptr(da_part), ptr(dx), ptr(dw), ptr(da), stream())
        dws = [dw[:, k * f:(k + 1) * f].contiguous() for k in range(heads)]
        das = [da[k].reshape(2 * f, 1) for k in range(heads)]
        return (dx.view(ctx.xshape) if dx is not None else None, None, None, None, None, None, *dws, *das)


def gat_layer(x, adj: PackedAdj, heads, mode: int, layer: int = 0, drop_p: float = 0.0, seed: int = 0):
    """All heads of one GAT layer (GraphAttentionLayer-like modules sharing alpha and width) in one projection GEMM and
    one aggregation launch.  x (N,R,din) -> (N,R,H*f) (modes GAT_ELU / GAT_PLAIN, heads concatenated) or (N,R,f)
    (GAT_OUTPUT: relu(sum of the heads / R)).  drop_p/seed: the attention dropout (gat_dropout_mask replays it)."""
    f = heads[0].W.shape[1]
    alpha = float(heads[0].alpha)
    assert all(m.W.shape == heads[0].W.shape and float(m.alpha) == alpha for m in heads)
    w_lin, w_cat, a_cat = _gat_operands(heads)
    cfg = (len(heads), f, alpha, int(mode), int(layer), float(drop_p), int(seed))
    return _GATLayer.apply(x, adj, cfg, w_lin, w_cat, a_cat, *[m.W for m in heads], *[m.a for m in heads])


def gat_pattern(adj) -> PackedAdj:
    """GAT adjacency: a dense (N,R,R) tensor is packed with its values (the kernels keep the entries > 0, as the
    reference's `adj > 0` does); a PackedAdj is used as it is (its refined bit pattern, values > 0 where it has values)."""
    return as_packed(adj)


def gcn_scale(adj: PackedAdj) -> torch.Tensor:
    """Per-row scale of the GCN normalisation D^-1/2 A D^-1/2 (gh_gcn_norm), (N, R)."""
    scale = torch.empty((adj.n, adj.r), device=adj.device, dtype=torch.float32)
    call("gh_gcn_norm", ptr(adj.bits), ptr(adj.dinv) if adj.vals is None else None, ptr(adj.vals), ptr(adj.keep), adj.n,
         adj.r, ptr(scale), stream())
    return scale


class _ScaleRows(torch.autograd.Function):
    """y = x * scale[row] (scale carries no gradient); the backward is the same scaling."""

    @staticmethod
    def forward(ctx, x, scale):
        x = _f32(x)
        y = torch.empty_like(x)
        call("gh_scale_rows", ptr(x), ptr(scale), None, ptr(y), scale.numel(), x.numel() // scale.numel(), stream())
        ctx.scale = scale
        return y

    @staticmethod
    def backward(ctx, g):
        g = _f32(g)
        dx = torch.empty_like(g)
        call("gh_scale_rows", ptr(g), ptr(ctx.scale), None, ptr(dx), ctx.scale.numel(), g.numel() // ctx.scale.numel(),
             stream())
        return dx, None


class _Relu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _f32(x)
        y = torch.empty_like(x)
        cols = x.shape[-1]
        call("gh_scale_rows", ptr(x), None, ptr(x), ptr(y), x.numel() // cols, cols, stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        g = _f32(g)
        dx = torch.empty_like(g)
        cols = g.shape[-1]
        call("gh_scale_rows", ptr(g), None, ptr(y), ptr(dx), g.numel() // cols, cols, stream())
        return dx


def relu(x):
    return _Relu.apply(x)


class GCNAdj:
    """A_hat = D^-1/2 A D^-1/2 of a packed adjacency, applied without forming it: the normalised graph's A_hat is again a
    normalised graph (bits + per-row scale), a weighted one is scale . A . scale around the fp32 aggregation."""

    __slots__ = ("adj", "scale")

    def __init__(self, adj: PackedAdj):
        self.scale = gcn_scale(adj)
        if adj.vals is None:
            adj = PackedAdj(adj.bits, self.scale, None, adj.keep, adj.n, adj.r)
        self.adj = adj

    def apply(self, x):
        """A_hat @ x for x (N,R,D) (the backward uses A_hat^T through gh_spmm's transposed mode)."""
        if self.adj.vals is None:
            return spmm(self.adj, x)
        return _ScaleRows.apply(spmm(self.adj, _ScaleRows.apply(x, self.scale)), self.scale)


# --------------------------------------------------------------------------- ragged helpers
class Segments:
    """Claim -> evidence-pair segmentation of one batch (prefix sums live on the device)."""

    def __init__(self, counts: torch.Tensor, b1: int, n_max: int):
        _lib.require_cuda(counts)
        counts = counts.to(torch.int64).contiguous()
        self.b = counts.shape[0]
        self.b1 = int(b1)
        self.n_max = int(n_max)
        self.offsets = torch.empty((self.b + 1,), device=counts.device, dtype=torch.int32)
        self.pair2claim = torch.empty((max(self.b1, 1),), device=counts.device, dtype=torch.int32)
        self.has = torch.empty((self.b, 1), device=counts.device, dtype=torch.float32)      # 1.0 where the claim has evidences
        call("gh_seg_offsets", ptr(counts), self.b, ptr(self.offsets), ptr(self.pair2claim), self.b1, ptr(self.has), stream())


class _SegBroadcast(torch.autograd.Function):       # basic_fc_model.py:80-92 _pad_left_tensor
    @staticmethod
    def forward(ctx, src, seg: Segments):
        src = _f32(src)
        x = src.shape[1]
        dst = torch.empty((seg.b1, x), device=src.device, dtype=torch.float32)
        call("gh_seg_broadcast", ptr(src), ptr(seg.pair2claim), ptr(dst), seg.b1, x, stream())
        ctx.seg = seg
        return dst

    @staticmethod
    def backward(ctx, g):
        g = _f32(g)
        seg = ctx.seg
        x = g.shape[1]
        d = torch.empty((seg.b, x), device=g.device, dtype=torch.float32)
        call("gh_seg_sum", ptr(g), ptr(seg.offsets), ptr(d), seg.b, x, stream())
        return d, None


class _SegPad(torch.autograd.Function):             # basic_fc_model.py:94-121 _pad_right_tensor
    @staticmethod
    def forward(ctx, src, seg: Segments):
        src = _f32(src)
        x = src.shape[1]
        dst = torch.empty((seg.b, seg.n_max, x), device=src.device, dtype=torch.float32)
        call("gh_seg_pad", ptr(src), ptr(seg.offsets), ptr(dst), seg.b, seg.n_max, x, x, stream())
        ctx.seg = seg
        return dst

    @staticmethod
    def backward(ctx, g):
        g = _f32(g)
        seg = ctx.seg
        x = g.shape[2]
        d = torch.zeros((seg.b1, x), device=g.device, dtype=torch.float32)     # rows no slot maps to (counts > n_max) get 0
        call("gh_seg_unpad", ptr(g), ptr(seg.offsets), ptr(d), seg.b, seg.n_max, x, x, stream())
        return d, None


def seg_broadcast(src, seg):
    return _SegBroadcast.apply(src, seg)


def seg_pad(src, seg):
    return _SegPad.apply(src, seg)


class _EvdAssemble(torch.autograd.Function):
    """graph_based_semantic_structure.py:157-170,195-215: pad_right(avg) ++ article_source_embs(sources) and the slot mask."""

    @staticmethod
    def forward(ctx, avg, table, seg: Segments, sources, document):
        avg = _f32(avg)
        xa = avg.shape[1]
        b, n = seg.b, seg.n_max
        ds = 0
        tb = None
        if table is not None:
            tb = _f32(table.detach())
            ds = tb.shape[1]
            if sources.dtype not in (torch.int32, torch.int64):
                sources = sources.long()
            sources = sources.contiguous()
            assert sources.numel() == b * n
        if document.dtype not in (torch.int32, torch.int64):
            document = document.long()
        document = document.contiguous()
        r = document.shape[-1]
        assert document.numel() == b * n * r
        right = torch.empty((b, n, xa + ds), device=avg.device, dtype=torch.float32)
        mask = torch.empty((b, n), device=avg.device, dtype=torch.float32)
        call("gh_evd_assemble_fwd", ptr(avg), ptr(seg.offsets), ptr(tb), tb.shape[0] if tb is not None else 0,
             ptr(sources) if table is not None else None,
             1 if (table is not None and sources.dtype == torch.int64) else 0, ptr(document),
             1 if document.dtype == torch.int64 else 0, b, n, xa, ds, r, ptr(right), ptr(mask), stream())
        ctx.seg, ctx.dims, ctx.table = seg, (xa, ds), table
        ctx.sources = sources if table is not None else None
        ctx.mark_non_differentiable(mask)
        return right, mask

    @staticmethod
    def backward(ctx, g, _gm):
        seg = ctx.seg
        xa, ds = ctx.dims
        g = _f32(g)
        table = ctx.table
        # rows no slot maps to (a claim with more than n_max evidences, reachable through the dense compatibility shim) get 0
        d_avg = torch.zeros((seg.b1, xa), device=g.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        d_table = None
        ret_table = None
        if table is not None and table.requires_grad:
            if _direct(table):
                d_table = table.grad
            else:
                d_table = torch.zeros_like(table, dtype=torch.float32)
                ret_table = d_table
        src = ctx.sources
        call("gh_evd_assemble_bwd", ptr(g), ptr(seg.offsets), ptr(src), 1 if (src is not None and src.dtype == torch.int64) else 0,
             table.shape[0] if table is not None else 0, seg.b, seg.n_max, xa, ds, ptr(d_avg), ptr(d_table), stream())      # ds is also g's row pitch: always the real width
        return d_avg, ret_table, None, None, None


def evd_assemble(avg, table, seg, sources, document):
    """-> (right (B, n, Xa + Ds), mask (B, n) float).  table: the article-source embedding weight or None."""
    return _EvdAssemble.apply(avg, table, seg, sources, document)


class _MaskedMean(torch.autograd.Function):         # graph_based_semantic_structure.py:145,153
    @staticmethod
    def forward(ctx, hid, ids, lens):
        hid = _f32(hid)
        b, l, h = hid.shape
        lens = _f32(lens.to(torch.float32))
        ids = ids.to(torch.int32).contiguous()
        dst = torch.empty((b, h), device=hid.device, dtype=torch.float32)
        call("gh_masked_mean_fwd", ptr(hid), ptr(ids), ptr(lens), ptr(dst), b, l, h, stream())
        ctx.save_for_backward(ids, lens)
        ctx.dims = (b, l, h)
        return dst

    @staticmethod
    def backward(ctx, g):
        ids, lens = ctx.saved_tensors
        b, l, h = ctx.dims
        g = _f32(g)
        d = torch.empty((b, l, h), device=g.device, dtype=torch.float32)
        call("gh_masked_mean_bwd", ptr(g), ptr(ids), ptr(lens), ptr(d), b, l, h, stream())
        return d, None, None


def masked_mean(hid, ids, lens):
    return _MaskedMean.apply(hid, ids, lens)


def cross_entropy(phi, labels):
    """Mean cross-entropy (losses.py:29-32) with its gradient in one launch; see get_amd.fused.cross_entropy."""
    from .fused import cross_entropy as _ce
    return _ce(phi, labels)


def backward(loss):
    """loss.backward() without autograd's root fill + scale launches (get_amd.fused.backward)."""
    from .fused import backward as _bw
    _bw(loss)


# --------------------------------------------------------------------------- evaluation
CLS_EXTRA = 8            # slots of gh_cls_metrics' `out` behind the c x c confusion matrix


def cls_metrics(phi, labels, pos_class: int = 1):
    """The integers of the fitter's metrics (char_man_fitter_query_repr1.py:353-362, 381-401) in one launch, no read-back.

    phi (n, c) float32 logits -- rows may be a column slice of a wider row-major tensor (unit column stride) --, labels (n,)
    int64 or int32.  Returns (out (c*c + 8,) int64, pred (n,) int32) on the device; include/get_hip.h (gh_cls_metrics) lists
    the slots of `out`: confusion counts [label][prediction], then U2, n_pos, n_neg, bad labels, NaN rows."""
    _lib.require_cuda(phi, labels)
    if phi.dim() != 2 or labels.dim() != 1 or labels.shape[0] != phi.shape[0]:
        raise ValueError(f"cls_metrics: phi (n, c) and labels (n,) expected, got {tuple(phi.shape)} and {tuple(labels.shape)}")
    phi = phi.detach()
    n, c = phi.shape
    if phi.dtype != torch.float32 or phi.stride(1) != 1 or phi.stride(0) < c or phi.data_ptr() % 4:
        phi = phi.float().contiguous()
    if labels.dtype not in (torch.int64, torch.int32):
        labels = labels.to(torch.int64)
    labels = labels.contiguous()
    if phi.device != labels.device or phi.device.index != _lib._get_device():
        raise RuntimeError("get_amd: cls_metrics wants phi and labels on the current device")
    out = torch.empty((c * c + CLS_EXTRA,), device=phi.device, dtype=torch.int64)
    pred = torch.empty((n,), device=phi.device, dtype=torch.int32)
    call("gh_cls_metrics", phi.data_ptr(), phi.stride(0) if n > 1 else c, ptr(labels), 1 if labels.dtype == torch.int64 else 0,
         n, c, int(pos_class), ptr(pred), ptr(out), stream())
    return out, pred


# --------------------------------------------------------------------------- optimiser
def adam_step_flat(p, g, m, v, step, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3, grad_scale=1.0):
    """One Adam step on flat fp32 buffers (declare_fitter.py:58-61 semantics)."""
    call("gh_adam_step", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), float(lr), float(betas[0]), float(betas[1]),
         float(eps), float(weight_decay), int(step), float(grad_scale), stream())
    _bump_trainer_epoch()

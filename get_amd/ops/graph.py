"""Front of csrc/graph_build_ops.hip, spmm_ops.hip, gsl_ops.hip, ragged_ops.hip (the node-compact plan), cell_ops.hip and
encoder_ops.hip: the packed adjacency and the node-compact plan, the
aggregation, the GGNN cell, the word scorer with GSL, and the GAT / GCN encoders."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from .._lib import call, ptr, stream
from ._util import _f32
from .embed import table_grad
from .weights import _direct, bf16_twins, derived, transposed


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
            ctx.table = x if ids is not None else None      # (what is saved below is its bf16 twin)
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
        ctx.table = x if ids is not None else None
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
            if ids is not None:      # trainable embedding table: the row gradients summed by id in a fixed order
                dx = table_grad(ctx.table, dx, ids[:m])      # (None: added straight into the table's .grad)
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
    t = float(np.float32(p)) * 4294967296.0      # the C-ABI takes p as a float: (double)drop_p * 2^32, as the launchers form it
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

"""Front of csrc/dense_ops.hip, ragged_ops.hip, eval_ops.hip and param_ops.hip: the linear layer, the claim / evidence
segment helpers, the loss and backward shortcuts, the evaluation counts and the optimiser step."""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import call, ptr, stream
from . import streams
from ._util import _f32
from .weights import _bump_trainer_epoch, _direct, transposed


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
        if direct and streams.WGRAD_SIDE_STREAM and m <= streams.WGRAD_FEW_ROWS and g2.is_cuda:
            if dx is not None:
                call("gh_linear_bwd", ptr(x2), ptr(wt), ptr(wc), ptr(g2), m, k, n, ptr(dx), None, None, stream())
            streams._side_wgrad(g2.device, (x2, g2),
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
    from ..fused import cross_entropy as _ce
    return _ce(phi, labels)


def backward(loss):
    """loss.backward() without autograd's root fill + scale launches (get_amd.fused.backward)."""
    from ..fused import backward as _bw
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

"""Front of the concat attention (entry points in csrc/dense_ops.hip, kernels in concat_att_ops.hip), of attention_ops.hip (the
single-query ablations) and of mha_ops.hip (the multi-head query/key/value attention and the residual layer norm)."""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import call, ptr, stream
from . import streams
from ._util import _f32
from .graph import _plan_args
from .weights import _direct, transposed


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
        if direct and streams.WGRAD_SIDE_STREAM and b * l <= streams.WGRAD_FEW_ROWS and right.is_cuda:
            # evidence level: everything but dW1 in line, dW1 = dpre^T [left | right] on the auxiliary stream
            call("gh_concat_att_bwd", *pa, ptr(dright), None, ptr(dw2), stream())
            streams._side_wgrad(dev, (left, right, dpre, du),
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

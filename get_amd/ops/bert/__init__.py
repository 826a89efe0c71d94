"""Front of csrc/bert_ops.hip: the BERT encoder's self-attention (probabilities never in HBM), its activations and the
embedding sum + LayerNorm (pytorch_transformers/modeling_bert.py)."""
from __future__ import annotations

import torch

from ... import _lib
from ..._lib import call, ptr, stream
from .._util import _f32
from ..attention import _ld, _rows_ld
from ..embed import _ids32, table_grad

ACT_GELU, ACT_TANH = 0, 1        # GH_ACT_GELU / GH_ACT_TANH of include/get_hip.h


class _BertAttention(torch.autograd.Function):
    """modeling_bert.py:203-228 (head split, softmax(q k^T / sqrt(dh) + mask), dropout, context, head merge):
    gh_bert_attention_*.  Saved for the backward: q, k, v, bias, out and lse (B,H,Lq); delta is scratch of lse's size."""

    @staticmethod
    def forward(ctx, q, k, v, bias, heads, scale, p, seed):
        _lib.require_cuda(q, k, v, bias)
        assert q.dim() == 3 and k.dim() == 3 and v.dim() == 3, "bert_attention: q (B,Lq,H*dh), k, v (B,Lk,H*dh)"
        q, k, v = _rows_ld(q), _rows_ld(k), _rows_ld(v)
        b, lq, w = q.shape
        lk = k.shape[1]
        assert k.shape == (b, lk, w) and v.shape == (b, lk, w) and w % heads == 0, \
            "bert_attention: q (B,Lq,H*dh), k, v (B,Lk,H*dh) of one width that the heads divide"
        if bias is not None:
            assert bias.shape == (b, lk), "bert_attention: bias (B,Lk)"
            bias = _f32(bias)
        dh = w // heads
        out = torch.empty((b, lq, w), device=q.device, dtype=torch.float32)
        lse = torch.empty((b, heads, lq), device=q.device, dtype=torch.float32)
        call("gh_bert_attention_fwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), _ld(q), _ld(k), _ld(v), ptr(bias), b, heads, lq, lk, dh,
             float(scale), float(p), int(seed), ptr(out), w, ptr(lse), stream())
        ctx.dims = (b, heads, lq, lk, dh, float(scale), float(p), int(seed))
        ctx.has_bias = bias is not None
        ctx.save_for_backward(q, k, v, bias if bias is not None else q.new_empty(0), out, lse)
        return out

    @staticmethod
    def backward(ctx, g_out):
        q, k, v, bias, out, lse = ctx.saved_tensors
        b, heads, lq, lk, dh, scale, p, seed = ctx.dims
        w = heads * dh
        g_out = _f32(g_out)
        delta = torch.empty_like(lse)
        dq = torch.empty((b, lq, w), device=q.device, dtype=torch.float32)
        dk = torch.empty((b, lk, w), device=q.device, dtype=torch.float32)
        dv = torch.empty((b, lk, w), device=q.device, dtype=torch.float32)
        call("gh_bert_attention_bwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), _ld(q), _ld(k), _ld(v),
             ptr(bias) if ctx.has_bias else None, ptr(out), w, ptr(lse), ptr(g_out), w, b, heads, lq, lk, dh, scale, p, seed,
             ptr(delta), ptr(dq), w, ptr(dk), w, ptr(dv), w, stream())
        return dq, dk, dv, None, None, None, None, None


def bert_attention(q, k, v, bias, heads: int, scale: float, p: float = 0.0, seed: int = 0):
    """q (B,Lq,H*dh), k, v (B,Lk,H*dh) with head h in the columns [h*dh, (h+1)*dh) (column slices of a wider tensor are read
    in place), bias (B,Lk) added to every query row's scaled scores, or None -> (B,Lq,H*dh) =
    dropout(softmax(scale q_h k_h^T + bias), p) v_h.  Element (b, h, i, j) of the probabilities is kept iff
    dropout_mask_reference(seed, B*H*Lq, Lk, p)[(b*H + h)*Lq + i, j].  Differentiable in q, k and v; the probabilities are never
    materialised."""
    return _BertAttention.apply(q, k, v, bias, heads, scale, p, seed)


class _Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mode):
        _lib.require_cuda(x)
        x = _f32(x)
        y = torch.empty_like(x)
        if x.numel():
            call("gh_act_fwd", ptr(x), ptr(y), x.numel() // x.shape[-1], x.shape[-1], mode, stream())
        ctx.mode = mode
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        g = _f32(g)
        dx = torch.empty_like(x)
        if x.numel():
            call("gh_act_bwd", ptr(x), ptr(g), ptr(dx), x.numel() // x.shape[-1], x.shape[-1], ctx.mode, stream())
        return dx, None


def gelu(x):
    """x * 0.5 * (1 + erf(x / sqrt(2))), the erf form of modeling_bert.py:126."""
    return _Act.apply(x, ACT_GELU)


def tanh_act(x):
    """tanh(x) (the pooler's activation, modeling_bert.py:373)."""
    return _Act.apply(x, ACT_TANH)


class _BertEmbed(torch.autograd.Function):
    """modeling_bert.py:156-169: gh_bert_embed_fwd; the backward is gh_add_layernorm_bwd on the saved sum, then one
    deterministic table gradient per table (ops.embed.table_grad), the word table's without its padding row 0."""

    @staticmethod
    def forward(ctx, word, pos, type_, ids, pos_ids, type_ids, gamma, beta, eps):
        _lib.require_cuda(word, pos, type_, ids, pos_ids, type_ids, gamma, beta)
        assert ids.dim() == 2, "bert_embed: ids (B,L)"
        b, l = ids.shape
        vocab, d = word.shape
        assert pos.shape[1] == d and type_.shape[1] == d and gamma.shape == (d,) and beta.shape == (d,), \
            "bert_embed: the three tables and the LayerNorm share one width"
        for t in (pos_ids, type_ids):
            assert t is None or t.shape == ids.shape, "bert_embed: pos_ids and type_ids have the shape of ids"
        rows = b * l
        ids32 = _ids32(ids, vocab)
        pos32 = _ids32(pos_ids, pos.shape[0]) if pos_ids is not None else None
        type32 = _ids32(type_ids, type_.shape[0]) if type_ids is not None else None
        gc = _f32(gamma.detach())
        dev = word.device
        s = torch.empty((rows, d), device=dev, dtype=torch.float32)
        y = torch.empty((rows, d), device=dev, dtype=torch.float32)
        mean = torch.empty((rows,), device=dev, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        if rows:
            call("gh_bert_embed_fwd", ptr(_f32(word.detach())), ptr(_f32(pos.detach())), ptr(_f32(type_.detach())), ptr(ids32), ptr(pos32),
                 ptr(type32), ptr(gc), ptr(_f32(beta.detach())), float(eps), rows, l, d, vocab, pos.shape[0], type_.shape[0], ptr(s),
                 ptr(y), ptr(mean), ptr(rstd), stream())
        ctx.tables = (word, pos, type_)
        ctx.ids = (ids32, pos32, type32)
        ctx.l = l
        ctx.save_for_backward(s, gc, mean, rstd)
        return y.view(b, l, d)

    @staticmethod
    def backward(ctx, g):
        s, gc, mean, rstd = ctx.saved_tensors
        rows, d = s.shape
        if rows == 0:
            return (None,) * 9
        _lib.ensure_workspace(s.device)      # the per-workgroup dgamma / dbeta partials
        g2 = _f32(g).reshape(rows, d)
        dx = torch.empty_like(s)
        dgamma = torch.zeros((d,), device=s.device, dtype=torch.float32)
        dbeta = torch.zeros((d,), device=s.device, dtype=torch.float32)
        call("gh_add_layernorm_bwd", ptr(s), None, ptr(gc), ptr(mean), ptr(rstd), ptr(g2), rows, d, ptr(dx), ptr(dgamma), ptr(dbeta),
             stream())
        word, pos, type_ = ctx.tables
        ids32, pos32, type32 = ctx.ids
        need = ctx.needs_input_grad
        if pos32 is None and need[1]:
            pos32 = torch.arange(ctx.l, device=s.device, dtype=torch.int32).repeat(rows // ctx.l)
        if type32 is None and need[2]:
            type32 = torch.zeros((rows,), device=s.device, dtype=torch.int32)
        dword = table_grad(word, dx, ids32, 0) if need[0] else None      # (nn.Embedding(..., padding_idx=0), :147)
        dpos = table_grad(pos, dx, pos32, -1) if need[1] else None
        dtype_ = table_grad(type_, dx, type32, -1) if need[2] else None
        return dword, dpos, dtype_, None, None, None, dgamma, dbeta, None


def bert_embed(word, pos, type_, ids, pos_ids, type_ids, gamma, beta, eps: float = 1e-12):
    """ids (B,L) int32 or int64, pos_ids / type_ids of the same shape or None (the column index / row 0) ->
    LayerNorm(word[ids] + pos[pos_ids] + type[type_ids]) * gamma + beta, (B,L,D).  Differentiable in the three tables (row 0
    of the word table, its padding row, receives no gradient), gamma and beta; the table gradients are the deterministic
    row sums of ops.embedding_backward."""
    return _BertEmbed.apply(word, pos, type_, ids, pos_ids, type_ids, gamma, beta, eps)

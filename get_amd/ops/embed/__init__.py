"""Front of csrc/embed_ops.hip: the embedding lookup and the gradient of a trainable table as a segmented row sum in a fixed
order (include/get_hip.h, gh_embed_bwd) -- no floating-point atomics, two backward passes give the same bits."""
from __future__ import annotations

import torch

from ... import _lib
from ..._lib import call, ptr, stream
from .._util import _f32
from ..weights import _direct

EMBED_CHUNK = 128         # GH_EMBED_CHUNK of include/get_hip.h: sorted positions per chunk of the summation order


def _ids32(ids: torch.Tensor, vocab: int) -> torch.Tensor:
    """ids of any shape, int32 or int64 -> flat int32.  An int64 id beyond int32 would wrap into the table: ids are first
    limited to [-1, vocab], which keeps every id outside the table outside it."""
    if ids.dtype == torch.int32:
        return ids.reshape(-1).contiguous()
    if ids.dtype != torch.int64:
        raise TypeError(f"get_amd: embedding ids are int32 or int64, got {ids.dtype}")
    return ids.reshape(-1).clamp(-1, int(vocab)).to(torch.int32)


def embed_plan(ids: torch.Tensor, vocab: int):
    """(sorted_ids, perm), both (m,) int32 on the device: the ids in ascending order and the row each sorted position came
    from, equal ids in ascending row order -- what gh_embed_bwd sums by.  A stable device sort, no host synchronisation."""
    _lib.require_cuda(ids)
    sorted_ids, perm = torch.sort(_ids32(ids, vocab), stable=True)
    return sorted_ids, perm.to(torch.int32)


def embed_workspace_floats(m: int, d: int) -> int:
    """Scratch of gh_embed_bwd for m rows of width d: two partial rows per chunk."""
    return 2 * ((m + EMBED_CHUNK - 1) // EMBED_CHUNK) * d


def embedding_backward(dx: torch.Tensor, plan, dtable: torch.Tensor, padding_idx: int = -1) -> torch.Tensor:
    """dtable (V,D) += the rows of dx (m,D) summed by id, in the fixed order of gh_embed_bwd; plan = embed_plan(ids, V).
    dx may be a row view with a leading dimension (stride(0) >= D).  Rows with padding_idx or an id outside the table add
    nothing; rows of dtable that no id names are not touched.  Returns dtable."""
    sorted_ids, perm = plan
    _lib.require_cuda(dx, sorted_ids, perm, dtable)
    if dtable.dim() != 2 or dtable.dtype != torch.float32 or not dtable.is_contiguous():
        raise ValueError("embedding_backward: dtable is a contiguous fp32 (V,D) tensor")
    vocab, d = dtable.shape
    m = sorted_ids.numel()
    if dx.dim() != 2 or tuple(dx.shape) != (m, d) or perm.numel() != m:
        raise ValueError(f"embedding_backward: dx {(m, d)} is expected for {m} ids, got {tuple(dx.shape)}")
    if sorted_ids.dtype != torch.int32 or perm.dtype != torch.int32:
        raise TypeError("embedding_backward: the plan holds int32 tensors (embed_plan)")
    if m == 0:
        return dtable
    if dx.dtype != torch.float32 or not (dx.stride(1) == 1 and dx.stride(0) >= d or m == 1 and dx.stride(1) == 1):
        dx = _f32(dx)
    ldx = d if dx.is_contiguous() else dx.stride(0)
    pad = -1 if padding_idx is None else int(padding_idx)
    ws = torch.empty((embed_workspace_floats(m, d),), device=dx.device, dtype=torch.float32)
    call("gh_embed_bwd", dx.data_ptr(), ldx, ptr(sorted_ids.contiguous()), ptr(perm.contiguous()), m, d, vocab, pad, ptr(dtable), ptr(ws),
         ws.numel(), stream())
    return dtable


def table_grad(weight: torch.Tensor, dx: torch.Tensor, ids: torch.Tensor, padding_idx: int = -1):
    """The gradient of table `weight` from the row gradients dx (m,D) of the lookups `ids` (m,), for an autograd backward to
    return: None after accumulating straight into weight.grad where that is the trainer's flat bucket (ops.weights._direct;
    no (V,D) temporary), else one zeroed (V,D) tensor that received the sums.
    A table is read by lookups on more than one stream (the claim branch runs on the auxiliary one) and both accumulate into
    the same rows: every direct accumulation waits for the one before it, through an event kept on the parameter."""
    vocab = weight.shape[0]
    plan = embed_plan(ids, vocab)
    if _direct(weight):
        cur = torch.cuda.current_stream(dx.device)
        done = getattr(weight, "_gh_embed_done", None)
        if done is None:
            done = weight._gh_embed_done = torch.cuda.Event()
        else:
            cur.wait_event(done)
        embedding_backward(dx, plan, weight.grad, padding_idx)
        done.record(cur)
        return None
    g = torch.zeros(tuple(weight.shape), device=dx.device, dtype=torch.float32)
    return embedding_backward(dx, plan, g, padding_idx)


class _Embedding(torch.autograd.Function):
    """torch.nn.functional.embedding on gh_embed_fwd / gh_embed_bwd."""

    @staticmethod
    def forward(ctx, weight, ids, padding_idx):
        _lib.require_cuda(weight, ids)
        if weight.dim() != 2:
            raise ValueError(f"embedding: a (V,D) table is expected, got {tuple(weight.shape)}")
        vocab, d = weight.shape
        flat = _ids32(ids, vocab)
        m = flat.numel()
        out = torch.empty((m, d), device=weight.device, dtype=torch.float32)
        if m:
            call("gh_embed_fwd", ptr(_f32(weight.detach())), ptr(flat), ptr(out), m, d, vocab, stream())
        ctx.weight, ctx.ids, ctx.padding_idx = weight, flat, padding_idx
        return out.view(*ids.shape, d)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        weight = ctx.weight
        g = g.reshape(-1, weight.shape[1])
        return table_grad(weight, g, ctx.ids, ctx.padding_idx), None, None


def embedding(weight: torch.Tensor, ids: torch.Tensor, padding_idx=None) -> torch.Tensor:
    """weight (V,D) fp32, ids of any shape (int32 or int64) -> (*ids.shape, D) = weight[ids].  Differentiable in weight: the
    gradient is the deterministic row sum of embedding_backward, without the rows of padding_idx (None = no such row)."""
    vocab = weight.shape[0]
    pad = -1
    if padding_idx is not None:      # (as torch: a negative index counts from the end of the table)
        pad = int(padding_idx) + (vocab if int(padding_idx) < 0 else 0)
        if not 0 <= pad < vocab:
            raise ValueError(f"embedding: padding_idx {padding_idx} is outside the {vocab}-row table")
    return _Embedding.apply(weight, ids, pad)

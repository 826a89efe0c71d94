"""Front of csrc/loss_ops.hip: softmax cross-entropy with an ignore index over rows of any width, the CrossEntropyLoss every
BERT task model ends in (pytorch_transformers/modeling_bert.py :698 :765 :822 :890 :996 :1056 :1142)."""
from __future__ import annotations

import math

import torch
from torch.autograd.function import once_differentiable

from ... import _lib
from ..._lib import call, stream


def _row_layout(x):
    """(rows, ldx, cs) when element (r, j) of x (..., c), its leading dimensions flattened to r, sits at r * ldx + j * cs floats
    from its first one, else None: what gh_softmax_xent_* read in place."""
    c = x.shape[-1]
    cs = x.stride(-1) if c > 1 else 1
    lead = [(n, s) for n, s in zip(x.shape[:-1], x.stride()[:-1]) if n != 1]
    span = (c - 1) * cs + 1
    if cs < 1:
        return None
    if not lead:
        return 1, span, cs
    for (_, outer), (n, inner) in zip(lead[:-1], lead[1:]):
        if outer != n * inner:
            return None
    ldx = lead[-1][1]
    if ldx < span:
        return None
    return math.prod(n for n, _ in lead), ldx, cs


def _current_device(t):
    if t.device.index != _lib._get_device():
        raise RuntimeError(f"get_amd: tensor on cuda:{t.device.index} but the current device is cuda:{_lib._get_device()}; "
                           "launches go to the current device's stream -- use `with torch.cuda.device(tensor.device):`")


class _SoftmaxXent(torch.autograd.Function):
    """gh_softmax_xent_fwd / _bwd.  Saved for the backward: the logits (as handed in, no copy), the labels, one log-sum-exp
    per row (two floats) and the count of kept rows -- never a second tensor of the logits' size."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index):
        x = logits.detach()
        layout = _row_layout(x) if x.data_ptr() % 4 == 0 else None
        if layout is None:
            x = x.contiguous()
            layout = _row_layout(x)
        rows, ldx, cs = layout
        c = x.shape[-1]
        labels = labels.reshape(-1).contiguous()
        _current_device(x)
        dev = x.device
        lse = torch.empty((2, rows), device=dev, dtype=torch.float32)      # the log-sum-exp and its rounding residual
        row_loss = torch.empty((rows,), device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        n_kept = torch.empty((1,), device=dev, dtype=torch.int64)
        call("gh_softmax_xent_fwd", x.data_ptr(), ldx, cs, labels.data_ptr(), int(labels.dtype == torch.int64), int(ignore_index), rows, c,
             lse[0].data_ptr(), lse[1].data_ptr(), row_loss.data_ptr(), loss.data_ptr(), n_kept.data_ptr(), stream())
        ctx.layout = (rows, ldx, cs, c, int(ignore_index))
        ctx.save_for_backward(x, labels, lse, n_kept)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, labels, lse, n_kept = ctx.saved_tensors
        rows, ldx, cs, c, ignore_index = ctx.layout
        g = g.to(torch.float32).contiguous()
        dx = torch.empty(x.shape, device=x.device, dtype=torch.float32)
        call("gh_softmax_xent_bwd", x.data_ptr(), ldx, cs, labels.data_ptr(), int(labels.dtype == torch.int64), ignore_index, rows, c,
             lse[0].data_ptr(), lse[1].data_ptr(), g.data_ptr(), n_kept.data_ptr(), dx.data_ptr(), c, 1, stream())
        return dx, None, None


def softmax_cross_entropy(logits, labels, ignore_index: int = -100):
    """torch.nn.functional.cross_entropy(logits.view(-1, c), labels.view(-1), ignore_index=ignore_index): the mean over the rows
    whose label is not ignore_index of log sum exp(logits) - logits[label], a scalar; NaN when no row is kept.

    logits (..., c) float32; a view whose rows lie one stride apart and whose classes lie one stride apart (a column slice, one
    column of a (B, L, 2) tensor seen as (B, L)) is read in place, anything else is made contiguous.  labels: logits' leading
    shape, int64 or int32.  A label outside [0, c) other than ignore_index, for which torch raises, drops its row and is
    counted (gh_clamp_events_n, slot 4).  Differentiable in logits; the backward recomputes the probabilities from the logits
    and one saved log-sum-exp per row."""
    _lib.require_cuda(logits, labels)
    if logits.dim() < 1 or logits.shape[-1] < 1:
        raise ValueError(f"softmax_cross_entropy: logits (..., c) with c >= 1 expected, got {tuple(logits.shape)}")
    if logits.dtype != torch.float32:
        raise ValueError(f"softmax_cross_entropy: float32 logits expected, got {logits.dtype}")
    if labels.dtype not in (torch.int64, torch.int32):
        raise ValueError(f"softmax_cross_entropy: int64 or int32 labels expected, got {labels.dtype}")
    if labels.numel() != logits.numel() // logits.shape[-1] or (labels.dim() > 1 and tuple(labels.shape) != tuple(logits.shape[:-1])):
        raise ValueError(f"softmax_cross_entropy: labels {tuple(labels.shape)} do not match the rows of logits {tuple(logits.shape)}")
    if labels.numel() == 0:      # the mean over no row, with a zero gradient of the logits' (empty) shape
        return logits.sum() * float("nan")
    return _SoftmaxXent.apply(logits, labels, ignore_index)

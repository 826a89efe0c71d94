"""Front of csrc/rank_ops.hip: the ranking metrics of a ragged batch of groups and the two pair-wise ranking losses."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from ... import _lib
from ..._lib import call, ptr, stream

RANK_MAX_GROUP = 1024     # GH_RANK_MAX_GROUP: items of one group
RANK_MAX_KS = 8           # GH_RANK_MAX_KS
RANK_INT_FIXED = 3        # group_int: count, n_rel, first relevant position; then hits per k
RANK_F64_FIXED = 3        # group_f64: ap, map, mrr; then precision, dcg, ndcg per k
HINGE_REDUCTIONS = {"none": 0, "mean": 1, "sum": 2}


def _host_offsets(offsets):
    """(device int32 tensor or None, host int32 array) of a group-offsets argument: a host sequence / array / CPU tensor is
    the sync-free form; a device tensor is copied to the host once (the limits are checked there before the launch)."""
    if torch.is_tensor(offsets):
        if offsets.dim() != 1 or offsets.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"rank_metrics: offsets (g + 1,) int32 / int64 expected, got {offsets.dtype} {tuple(offsets.shape)}")
        host = offsets.detach().cpu().numpy()
        dev = offsets.to(torch.int32).contiguous() if offsets.is_cuda else None
    else:
        host, dev = np.asarray(offsets), None
        if host.ndim != 1 or host.dtype.kind not in "iu":
            raise ValueError("rank_metrics: offsets is a 1-d sequence of integers")
    if host.size < 2:
        raise ValueError("rank_metrics: offsets holds g + 1 >= 2 entries")
    if host.min() < 0 or host.max() > 2 ** 31 - 1:
        raise ValueError("rank_metrics: offsets outside the int32 range")
    return dev, np.ascontiguousarray(host, dtype=np.int32)


def rank_metrics(scores, labels, offsets, ks, threshold=0.):
    """The six matchzoo ranking metrics of every group, and every item's rank inside its group, in one launch; no read-back.

    scores (n,) and labels (n,) on the device; group q is the items offsets[q] .. offsets[q + 1] (g + 1 non-decreasing
    integers from 0 to n; empty groups are legal, a group holds at most 1024 items).  `offsets` as a host sequence, numpy
    array or CPU tensor is uploaded; a device tensor is used as it is and copied to the host once for the limit checks.
    Scores are read as fp32 or fp64 as given (fp16 / bf16 and integers are widened to fp32); labels of any dtype are converted
    to float64, which is exact for integers and fp32 -- a graded label such as 0.1 never passes through fp32.
    ks: 1 to 8 cut-offs k >= 1.  An item is relevant when label > threshold.

    Returns (rank (n,) int32, group_int (g, 3 + nk) int32, group_f64 (g, 3 + 3 nk) float64, nan_count (2,) int32) on the
    device; include/get_hip.h (gh_rank_metrics) lists the slots."""
    _lib.require_cuda(scores, labels)
    if scores.dim() != 1 or labels.dim() != 1 or labels.shape[0] != scores.shape[0]:
        raise ValueError(f"rank_metrics: scores (n,) and labels (n,) expected, got {tuple(scores.shape)} and {tuple(labels.shape)}")
    if scores.device != labels.device or scores.device.index != _lib._get_device():
        raise RuntimeError("get_amd: rank_metrics wants scores and labels on the current device")
    ks = [int(k) for k in ks]
    off_dev, off_host = _host_offsets(offsets)
    if off_dev is None:
        off_dev = torch.from_numpy(off_host).to(scores.device)
    _lib.require_cuda(off_dev)
    scores = scores.detach()
    if scores.dtype not in (torch.float32, torch.float64):
        scores = scores.float()
    scores = scores.contiguous()
    labels = labels.detach().to(torch.float64).contiguous()
    n, g, nk = scores.shape[0], off_host.shape[0] - 1, len(ks)
    dev = scores.device
    rank = torch.empty((n,), device=dev, dtype=torch.int32)
    gi = torch.empty((g, RANK_INT_FIXED + nk), device=dev, dtype=torch.int32)
    gd = torch.empty((g, RANK_F64_FIXED + 3 * nk), device=dev, dtype=torch.float64)
    nan_count = torch.empty((2,), device=dev, dtype=torch.int32)
    ks_host = (ctypes.c_int32 * max(nk, 1))(*ks)
    call("gh_rank_metrics", ptr(scores), 1 if scores.dtype == torch.float64 else 0, ptr(labels), ptr(off_dev),
         off_host.ctypes.data, n, g, float(threshold), ctypes.cast(ks_host, ctypes.c_void_p), nk, ptr(rank), ptr(gi), ptr(gd),
         ptr(nan_count), stream())
    return rank, gi, gd, nan_count


def _rows(t: torch.Tensor, who: str) -> torch.Tensor:
    """(rows, c) fp32 whose rows the kernels read in place: unit stride along c, rows stride(0) >= c floats apart (a
    contiguous tensor or a column slice of one); anything else is copied."""
    if t.dim() != 2:
        raise ValueError(f"{who}: a (rows, c) tensor is expected, got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        t = t.float()
    if t.is_contiguous() or (t.stride(1) == 1 and t.stride(0) >= t.shape[1]):
        return t
    return t.contiguous()


def _row_ld(t: torch.Tensor) -> int:
    return t.shape[1] if t.is_contiguous() else t.stride(0)


def _instances(rows: int, num_neg: int, who: str) -> int:
    if rows < 1 or rows % (num_neg + 1):
        raise ValueError(f"{who}: {rows} rows are no (positive) multiple of num_neg + 1 = {num_neg + 1}")
    return rows // (num_neg + 1)


class _RankHinge(torch.autograd.Function):
    """matchzoo/losses/rank_hinge_loss.py:54-66: gh_rank_hinge_*."""

    @staticmethod
    def forward(ctx, y_pred, num_neg, margin, reduction):
        _lib.require_cuda(y_pred)
        y = _rows(y_pred, "rank_hinge")
        rows, c = y.shape
        nb = _instances(rows, num_neg, "rank_hinge")
        dev = y.device
        neg_mean = torch.empty((nb,), device=dev, dtype=torch.float32)
        if reduction == 0:
            out = torch.empty((nb, c), device=dev, dtype=torch.float32)
            call("gh_rank_hinge_fwd", y.data_ptr(), _row_ld(y), rows, c, num_neg, float(margin), 0, ptr(neg_mean), ptr(out), None, None,
                 stream())
        else:
            out = torch.empty((), device=dev, dtype=torch.float32)
            part = torch.empty((nb,), device=dev, dtype=torch.float32)
            call("gh_rank_hinge_fwd", y.data_ptr(), _row_ld(y), rows, c, num_neg, float(margin), reduction, ptr(neg_mean), None, ptr(part),
                 ptr(out), stream())
        ctx.args = (num_neg, float(margin), reduction)
        ctx.save_for_backward(y, neg_mean)
        return out

    @staticmethod
    def backward(ctx, g):
        y, neg_mean = ctx.saved_tensors
        num_neg, margin, reduction = ctx.args
        rows, c = y.shape
        g = g.float().contiguous()
        dy = torch.empty((rows, c), device=y.device, dtype=torch.float32)
        call("gh_rank_hinge_bwd", y.data_ptr(), _row_ld(y), rows, c, num_neg, margin, reduction, ptr(neg_mean), ptr(g), ptr(dy), stream())
        return dy, None, None, None


def rank_hinge(y_pred, num_neg: int = 1, margin: float = 1., reduction: str = "mean"):
    """y_pred (rows, c), rows = B (num_neg + 1): row b (num_neg + 1) is the positive of instance b, the num_neg rows behind it
    its negatives (a column slice of a wider tensor is read in place).  Element (b, j) = max(0, margin - (pos[b][j] -
    neg_mean[b])) with neg_mean[b] the mean of the instance's num_neg c negative entries; 'none' gives (B, c), 'mean' and
    'sum' a scalar.  Differentiable in y_pred."""
    if reduction not in HINGE_REDUCTIONS:
        raise ValueError("rank_hinge: %s is not one of %s" % (reduction, list(HINGE_REDUCTIONS)))
    return _RankHinge.apply(y_pred, int(num_neg), margin, HINGE_REDUCTIONS[reduction])


class _RankCrossEntropy(torch.autograd.Function):
    """matchzoo/losses/rank_cross_entropy_loss.py:29-38: gh_rank_ce_*."""

    @staticmethod
    def forward(ctx, y_pred, y_true, num_neg):
        _lib.require_cuda(y_pred, y_true)
        y, yt = _rows(y_pred, "rank_cross_entropy"), _rows(y_true.detach(), "rank_cross_entropy")
        if y.shape != yt.shape:
            raise ValueError(f"rank_cross_entropy: y_pred {tuple(y.shape)} and y_true {tuple(yt.shape)} differ in shape")
        rows, c = y.shape
        nb = _instances(rows, num_neg, "rank_cross_entropy")
        dev = y.device
        lse = torch.empty((nb,), device=dev, dtype=torch.float32)
        part = torch.empty((nb,), device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        call("gh_rank_ce_fwd", y.data_ptr(), _row_ld(y), yt.data_ptr(), _row_ld(yt), rows, c, num_neg, ptr(lse), ptr(part), ptr(loss), stream())
        ctx.num_neg = num_neg
        ctx.save_for_backward(y, yt, lse)
        return loss

    @staticmethod
    def backward(ctx, g):
        y, yt, lse = ctx.saved_tensors
        rows, c = y.shape
        g = g.float().contiguous()
        dy = torch.empty((rows, c), device=y.device, dtype=torch.float32)
        call("gh_rank_ce_bwd", y.data_ptr(), _row_ld(y), yt.data_ptr(), _row_ld(yt), rows, c, ctx.num_neg, ptr(lse), ptr(g), ptr(dy), stream())
        return dy, None, None


def rank_cross_entropy(y_pred, y_true, num_neg: int = 1):
    """y_pred, y_true (rows, c), rows = B (num_neg + 1): the logits of instance b are its num_neg + 1 rows side by side, the
    labels the same entries of y_true.  -mean_b sum_j labels log_softmax(logits), a scalar; differentiable in y_pred, the
    labels are constants.  The log-softmax is the stable one: a logit far below its row maximum gives a finite value where
    the reference's log(softmax(x)) gives -inf (and NaN under a zero label)."""
    return _RankCrossEntropy.apply(y_pred, y_true, int(num_neg))

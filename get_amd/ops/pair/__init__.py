"""Front of csrc/pair_ops.hip: the pairwise Euclidean and L1 distances, the windowed mean and the batched matching histogram.
Callers outside reach these as ``ops.pair.NAME(...)``."""
from __future__ import annotations

import torch

from ... import _lib
from ..._lib import call, ptr, stream
from .._util import _f32
from ..attention import _ld, _rows_ld

PAIR_MAX_L = 1024         # rows of either side of pair_l2 / pair_l1, ids per side of match_hist
PAIR_MAX_D = 2048
WINDOW_MAX = 1024         # window, left and right of window_mean
HIST_MAX_BINS = 256
HIST_MODES = {"CH": 0, "NH": 1, "LCH": 2}


def _pair_operands(a, b, who):
    if a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0] or a.shape[2] != b.shape[2]:
        raise ValueError(f"{who}: a (B,L,D) and b (B,R,D) are expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    _lib.require_cuda(a, b)
    return _rows_ld(a), _rows_ld(b)


class _PairL2(torch.autograd.Function):
    """torch_utils.py:311-329: gh_pair_l2_*."""

    @staticmethod
    def forward(ctx, a, b, eps):
        a, b = _pair_operands(a, b, "pair_l2")
        bn, l, d = a.shape
        r = b.shape[1]
        dev = a.device
        out = torch.empty((bn, l, r), device=dev, dtype=torch.float32)
        ctx.dims = (bn, l, r, d)
        if out.numel() == 0 or d == 0:
            ctx.save_for_backward(a, b, None, None)
            return out.fill_(float(eps) ** 0.5) if out.numel() else out
        a2 = torch.empty((bn, l), device=dev, dtype=torch.float32)
        b2 = torch.empty((bn, r), device=dev, dtype=torch.float32)
        sgn = torch.empty((bn, l, r), device=dev, dtype=torch.int8)
        call("gh_pair_l2_fwd", a.data_ptr(), b.data_ptr(), _ld(a), _ld(b), float(eps), bn, l, r, d, ptr(a2), ptr(b2), ptr(out), ptr(sgn),
             stream())
        ctx.save_for_backward(a, b, out, sgn)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b, out, sgn = ctx.saved_tensors
        bn, l, r, d = ctx.dims
        if out is None:
            return torch.zeros_like(a), torch.zeros_like(b), None
        g = _f32(g)
        da = torch.empty((bn, l, d), device=a.device, dtype=torch.float32)
        db = torch.empty((bn, r, d), device=a.device, dtype=torch.float32)
        call("gh_pair_l2_bwd", a.data_ptr(), b.data_ptr(), _ld(a), _ld(b), ptr(out), ptr(sgn), ptr(g), bn, l, r, d, ptr(da), ptr(db), stream())
        return da, db, None


def pair_l2(a, b, eps=1e-10):
    """a (B,L,D), b (B,R,D) (column slices are read in place) -> (B,L,R) = sqrt(|A2 - 2 a.b + B2| + eps), the reference's
    `cosine_distance`, which is the Euclidean distance.  The terms are added in the reference's order, so coincident rows
    give rounding noise under the root, as there; an entry whose inner value is exactly 0 sends no gradient."""
    return _PairL2.apply(a, b, eps)


class _PairL1(torch.autograd.Function):
    """torch_utils.py:332-348: gh_pair_l1_*."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _pair_operands(a, b, "pair_l1")
        bn, l, d = a.shape
        r = b.shape[1]
        out = torch.empty((bn, l, r), device=a.device, dtype=torch.float32)
        ctx.dims = (bn, l, r, d)
        ctx.save_for_backward(a, b)
        if out.numel() == 0 or d == 0:
            return out.zero_()
        call("gh_pair_l1_fwd", a.data_ptr(), b.data_ptr(), _ld(a), _ld(b), bn, l, r, d, ptr(out), stream())
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        bn, l, r, d = ctx.dims
        if bn * l * r * d == 0:
            return torch.zeros_like(a), torch.zeros_like(b)
        g = _f32(g)
        da = torch.empty((bn, l, d), device=a.device, dtype=torch.float32)
        db = torch.empty((bn, r, d), device=a.device, dtype=torch.float32)
        call("gh_pair_l1_bwd", a.data_ptr(), b.data_ptr(), _ld(a), _ld(b), ptr(g), bn, l, r, d, ptr(da), ptr(db), stream())
        return da, db


def pair_l1(a, b):
    """a (B,L,D), b (B,R,D) (column slices are read in place) -> (B,L,R) = sum_k |a_lk - b_rk|, without the reference's
    (B,L,R,D) difference tensor.  The gradient takes sign(0) = 0, as torch's norm(p=1) does."""
    return _PairL1.apply(a, b)


def window_out_len(l, window, left=0, right=0):
    """Rows of window_mean's result: l + left + right - window + 1, or 0 where the window is longer than the padded sequence."""
    return max(l + left + right - window + 1, 0)


class _WindowMean(torch.autograd.Function):
    """torch_utils.py:292-308, :351-376 and layers.py:42-66: gh_window_mean_*."""

    @staticmethod
    def forward(ctx, x, window, left, right, mask):
        _lib.require_cuda(x, mask)
        x = _rows_ld(x)
        bn, l, d = x.shape
        lo = window_out_len(l, window, left, right)
        out = torch.empty((bn, lo, d), device=x.device, dtype=torch.float32)
        ctx.args = (bn, l, d, lo, window, left, right)
        ctx.save_for_backward(mask)
        if out.numel() == 0:
            return out
        call("gh_window_mean_fwd", x.data_ptr(), _ld(x), ptr(mask), bn, l, d, window, left, right, ptr(out), stream())
        return out

    @staticmethod
    def backward(ctx, g):
        mask, = ctx.saved_tensors
        bn, l, d, lo, window, left, right = ctx.args
        dx = torch.empty((bn, l, d), device=g.device, dtype=torch.float32)
        if dx.numel() == 0 or lo == 0:
            return dx.zero_(), None, None, None, None
        g = _rows_ld(g)
        call("gh_window_mean_bwd", g.data_ptr(), _ld(g), ptr(mask), bn, l, d, window, left, right, ptr(dx), stream())
        return dx, None, None, None, None


def window_mean(x, window, left=0, right=0, mask=None):
    """x (B,L,D) (a column slice is read in place) -> (B,L_out,D), L_out = L + left + right - window + 1:
    out[:, t] = mask[:, t] / window * the sum of the rows t - left .. t - left + window - 1 of x, the `left` rows before and the
    `right` rows behind the sequence counting as zeros.  mask (B,L_out) of any dtype (read as fp32) or None; a row whose mask
    is 0 is an exact zero and sends an exact-zero gradient.  A window longer than the padded sequence gives (B,0,D) without a
    launch.  Differentiable in x."""
    window, left, right = int(window), int(left), int(right)
    if x.dim() != 3:
        raise ValueError(f"window_mean: x (B,L,D) is expected, got {tuple(x.shape)}")
    if window < 1 or left < 0 or right < 0:
        raise ValueError(f"window_mean: window >= 1 and left, right >= 0 are expected, got {window}, {left}, {right}")
    if max(window, left, right) > WINDOW_MAX and window_out_len(x.shape[1], window, left, right) > 0:
        raise ValueError(f"window_mean: window, left and right are limited to {WINDOW_MAX}, got {window}, {left}, {right}")
    if mask is not None:
        lo = window_out_len(x.shape[1], window, left, right)
        if tuple(mask.shape) != (x.shape[0], lo):
            raise ValueError(f"window_mean: mask {(x.shape[0], lo)} is expected, got {tuple(mask.shape)}")
        mask = mask.detach().to(torch.float32).contiguous()
    return _WindowMean.apply(x, window, left, right, mask)


def match_hist(table, inv_norm, ids_left, ids_right, len_right, bins, mode):
    """The DRMM matching histogram of a batch: table (V,D) fp32 on the device (a column slice is read in place), inv_norm (V)
    or None (the products are scaled by inv_norm[left] inv_norm[right]), ids_left (B,Lq), ids_right (B,Ld) and len_right (B)
    integers on the device -> (B,Lq,bins) fp32.  Entry (i, bin) is 1 plus the number of right ids j < len_right with
    int((table[left_i] . table[right_j] + 1) / 2 * (bins - 1)) == bin; mode 'CH' leaves the counts, 'NH' divides by the row
    total, 'LCH' takes the logarithm.  Right ids at or beyond len_right are ignored; an id outside [0, V) raises (the ids are
    checked on the device first, which synchronises the stream).  Not differentiable."""
    if mode not in HIST_MODES:
        raise ValueError("match_hist: %s is not one of %s" % (mode, list(HIST_MODES)))
    _lib.require_cuda(table, inv_norm, ids_left, ids_right, len_right)
    if table.dim() != 2 or ids_left.dim() != 2 or ids_right.dim() != 2 or len_right.dim() != 1 or \
            not ids_left.shape[0] == ids_right.shape[0] == len_right.shape[0]:
        raise ValueError("match_hist: table (V,D), ids_left (B,Lq), ids_right (B,Ld), len_right (B) are expected")
    if inv_norm is not None and tuple(inv_norm.shape) != (table.shape[0],):
        raise ValueError(f"match_hist: inv_norm ({table.shape[0]},) is expected, got {tuple(inv_norm.shape)}")
    for t in (ids_left, ids_right, len_right):
        if t.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"match_hist: ids and lengths are int32 / int64, got {t.dtype}")
    bins = int(bins)
    table = table.detach()
    if table.dtype != torch.float32:
        table = table.float()
    if not (table.is_contiguous() or (table.stride(1) == 1 and table.stride(0) >= table.shape[1])):
        table = table.contiguous()
    ldt = table.shape[1] if table.is_contiguous() else table.stride(0)
    inv = None if inv_norm is None else _f32(inv_norm.detach())
    bn, lq = ids_left.shape
    ld = ids_right.shape[1]
    dev = table.device
    out = torch.empty((bn, lq, bins), device=dev, dtype=torch.float32)
    if bn * lq == 0:
        return out
    if ld == 0:          # nothing to count: every bin keeps its 1 (one dummy right id that no length reaches)
        ids_right = torch.zeros((bn, 1), device=dev, dtype=torch.int32)
        len_right = torch.zeros((bn,), device=dev, dtype=torch.int32)
        ld = 1
    il, ir = ids_left.to(torch.int32).contiguous(), ids_right.to(torch.int32).contiguous()
    ln = len_right.to(torch.int32).contiguous()
    flag = torch.empty((1,), device=dev, dtype=torch.int32)
    call("gh_match_hist", table.data_ptr(), ldt, ptr(inv), table.shape[0], table.shape[1], ptr(il), ptr(ir), ptr(ln), bn, lq, ld, bins,
         HIST_MODES[mode], ptr(out), ptr(flag), stream())
    return out

"""Front of csrc/rnn_ops.hip: the LSTM and GRU recurrences and what they share."""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import call, ptr, stream
from ._util import _f32
from .weights import _direct


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

"""Front of csrc/bidaf_ops.hip: the attention-flow layer and the highway gate."""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import call, ptr, stream
from ._util import _f32
from .attention import _ld, _rows_ld


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

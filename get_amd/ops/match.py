"""Front of csrc/match_ops.hip: soft alignment, the matching layers and the Gaussian kernel."""
from __future__ import annotations

import torch

from .. import _lib
from .._lib import call, ptr, stream
from ._util import _f32
from .attention import _ld, _rows_ld
from .bidaf import _OutBuffer


# --------------------------------------------------------------------------- matchzoo/modules: soft alignment, matching, kernels
def _flag_bytes(t, shape, who):
    """A bool / uint8 flag tensor of `shape` as contiguous uint8 (nonzero = set), None stays None."""
    if t is None:
        return None
    assert t.dtype in (torch.bool, torch.uint8) and tuple(t.shape) == tuple(shape), \
        f"{who}: a bool (or uint8) tensor of shape {tuple(shape)} is expected, got {t.dtype} {tuple(t.shape)}"
    t = t.contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


class _SoftAlign(torch.autograd.Function):
    """matchzoo/modules/attention.py:50-63 and :99-105 (softmax(fill(q k^T)) v, the row zeroing, MatchModule's four-way cat):
    csrc/match_ops.hip gh_soft_align_*."""

    @staticmethod
    def forward(ctx, q, k, v, key_fill, row_zero, fill, fuse, out):
        out = out.t
        _lib.require_cuda(q, k, v, key_fill, row_zero, out)
        assert q.dim() == 3 and k.dim() == 3 and v.dim() == 3 and q.shape[0] == k.shape[0] == v.shape[0] and \
            q.shape[2] == k.shape[2] and k.shape[1] == v.shape[1], "soft_align: q (B,Lq,D), k (B,Lk,D), v (B,Lk,Dv)"
        q, k, v = _rows_ld(q), _rows_ld(k), _rows_ld(v)
        b, lq, d = q.shape
        lk, dv = v.shape[1], v.shape[2]
        kf = _flag_bytes(key_fill, (b, lk), "soft_align: key_fill")
        rz = _flag_bytes(row_zero, (b, lq), "soft_align: row_zero")
        fuse = int(bool(fuse))
        if fuse and (dv != d or rz is not None):
            raise RuntimeError(f"soft_align: fuse needs Dv == D (got {dv}, {d}) and no row_zero")
        wo = 4 * d if fuse else dv
        dev = q.device
        if out is None:
            x = torch.empty((b, lq, wo), device=dev, dtype=torch.float32)
        else:
            x = out
            assert x.shape == (b, lq, wo) and x.dtype == torch.float32 and _rows_ld(x) is x, \
                "soft_align: out is fp32 (B,Lq,Dv) -- (B,Lq,4D) with fuse --, contiguous or a column slice of a contiguous tensor"
        a = torch.empty((b, lq, lk), device=dev, dtype=torch.float32)
        call("gh_soft_align_fwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), _ld(q), _ld(k), _ld(v), ptr(kf), ptr(rz), float(fill), fuse,
             b, lq, lk, d, dv, ptr(a), x.data_ptr(), _ld(x), stream())
        ctx.dims = (b, lq, lk, d, dv, fuse)
        ctx.save_for_backward(q, k, v, kf, rz, a, x if fuse else None)
        ctx.mark_non_differentiable(a)
        return x, a

    @staticmethod
    def backward(ctx, g, _g_a):
        q, k, v, kf, rz, a, x = ctx.saved_tensors
        b, lq, lk, d, dv, fuse = ctx.dims
        dev = q.device
        g = _rows_ld(g)
        ds = torch.empty_like(a)
        dq = torch.empty((b, lq, d), device=dev, dtype=torch.float32)
        dk = torch.empty((b, lk, d), device=dev, dtype=torch.float32)
        dvv = torch.empty((b, lk, dv), device=dev, dtype=torch.float32)
        call("gh_soft_align_bwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), _ld(q), _ld(k), _ld(v), ptr(kf), ptr(rz), fuse, ptr(a),
             x.data_ptr() if fuse else None, _ld(x) if fuse else 0, g.data_ptr(), _ld(g), b, lq, lk, d, dv, ptr(ds), ptr(dq), d, ptr(dk), d,
             ptr(dvv), dv, stream())
        return dq, dk, dvv, None, None, None, None, None


def soft_align(q, k, v, key_fill, row_zero=None, fill=-1e-7, fuse=False, out=None):
    """Soft alignment between two sequences: q (B,Lq,D), k (B,Lk,D), v (B,Lk,Dv) (column slices of a wider tensor are read in
    place), key_fill (B,Lk) bool, row_zero (B,Lq) bool or None -> (out, weights (B,Lq,Lk)).
    S = q k^T with S[:, :, j] REPLACED by the constant `fill` (finite) where key_fill[:, j]: as in the reference's
    masked_fill(mask, -1e-7), a filled key is not excluded, it keeps a weight (and receives the gradient of v), only its score
    is a constant and sends nothing to q and k.  weights = softmax(S) over the keys; o = weights v, zero in the rows of
    row_zero.  out = o (B,Lq,Dv), or with fuse (Dv == D, no row_zero) [q, o, q - o, q * o] (B,Lq,4D); it is written into `out`
    when given (fp32, contiguous or a column slice of a contiguous tensor), which must not be overwritten before the backward
    when fuse is set.  Differentiable in q, k and v through `out`; `weights` is returned for inspection only."""
    return _SoftAlign.apply(q, k, v, key_fill, row_zero, fill, fuse, _OutBuffer(out))


LIN_ATT_MODES = (0, 1, 2)


class _LinAtt(torch.autograd.Function):
    """matchzoo/modules/attention.py:35-38: gh_lin_att_*."""

    @staticmethod
    def forward(ctx, x, w, mode):
        _lib.require_cuda(x, w)
        assert x.dim() == 3 and w.numel() == x.shape[2], "lin_att: x (B,L,D), w holds D weights"
        assert mode in LIN_ATT_MODES, "lin_att: mode is 0, 1 or 2"
        x = _f32(x)
        b, l, d = x.shape
        wc = _f32(w.detach()).reshape(-1)
        a = torch.empty((b, l), device=x.device, dtype=torch.float32)
        call("gh_lin_att_fwd", ptr(x), ptr(wc), int(mode), b, l, d, ptr(a), stream())
        ctx.save_for_backward(x, wc, a)
        ctx.wshape = w.shape
        return a

    @staticmethod
    def backward(ctx, g):
        x, wc, a = ctx.saved_tensors
        b, l, d = x.shape
        g = _f32(g)
        dx = torch.empty_like(x)
        part = torch.empty((b, d), device=x.device, dtype=torch.float32)
        dw = torch.empty((d,), device=x.device, dtype=torch.float32)
        call("gh_lin_att_bwd", ptr(x), ptr(wc), ptr(a), ptr(g), b, l, d, ptr(dx), ptr(part), ptr(dw), stream())
        return dx, dw.view(ctx.wshape), None


def lin_att(x, w, mode=0):
    """x (B,L,D), w: the D weights of a Linear(D, 1, bias=False) -> weights (B,L): the softmax of s = x w over the kept
    positions, exactly 0 elsewhere.  mode 0 excludes s == 0 (an all-zero row of x scores exactly 0), mode 1 excludes s != 1,
    mode 2 excludes nothing: the reference's (x != m) / (mask == m) pair for m == 0, m == 1 and any other m.  A sequence
    without a kept position gives NaN in its own row."""
    return _LinAtt.apply(x, w, mode)


class _MatchDot(torch.autograd.Function):
    """matchzoo/modules/matching.py:46-50: gh_match_dot_*."""

    @staticmethod
    def forward(ctx, x, y, normalize):
        _lib.require_cuda(x, y)
        assert x.dim() == 3 and y.dim() == 3 and x.shape[0] == y.shape[0] and x.shape[2] == y.shape[2], \
            "match_dot: x (B,L,D), y (B,R,D)"
        x, y = _rows_ld(x), _rows_ld(y)
        b, l, d = x.shape
        r = y.shape[1]
        dev = x.device
        normalize = int(bool(normalize))
        ix = torch.empty((b, l), device=dev, dtype=torch.float32) if normalize else None
        iy = torch.empty((b, r), device=dev, dtype=torch.float32) if normalize else None
        out = torch.empty((b, l, r), device=dev, dtype=torch.float32)
        call("gh_match_dot_fwd", x.data_ptr(), y.data_ptr(), _ld(x), _ld(y), normalize, b, l, r, d, ptr(ix), ptr(iy), ptr(out), stream())
        ctx.normalize = normalize
        ctx.save_for_backward(x, y, ix, iy)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y, ix, iy = ctx.saved_tensors
        b, l, d = x.shape
        r = y.shape[1]
        g = _f32(g)
        dx = torch.empty((b, l, d), device=x.device, dtype=torch.float32)
        dy = torch.empty((b, r, d), device=x.device, dtype=torch.float32)
        call("gh_match_dot_bwd", x.data_ptr(), y.data_ptr(), _ld(x), _ld(y), ctx.normalize, ptr(ix), ptr(iy), ptr(g), b, l, r, d, ptr(dx),
             ptr(dy), stream())
        return dx, dy, None


def match_dot(x, y, normalize=False):
    """x (B,L,D), y (B,R,D) (column slices are read in place) -> (B,L,R) = x y^T, of the L2-normalised rows (F.normalize, eps
    1e-12) with `normalize`.  A row with a norm <= 1e-12 is divided by 1e-12, and its gradient is of the order 1e12 times the
    upstream one, exactly as torch gives."""
    return _MatchDot.apply(x, y, normalize)


MATCH_BCAST_OPS = {"mul": 0, "plus": 1, "minus": 2, "concat": 3}


class _MatchBcast(torch.autograd.Function):
    """matchzoo/modules/matching.py:52-61: gh_match_bcast_*."""

    @staticmethod
    def forward(ctx, x, y, op):
        _lib.require_cuda(x, y)
        assert x.dim() == 3 and y.dim() == 3 and x.shape[0] == y.shape[0] and x.shape[2] == y.shape[2], \
            "match_bcast: x (B,L,D), y (B,R,D)"
        x, y = _f32(x), _f32(y)
        b, l, d = x.shape
        r = y.shape[1]
        out = torch.empty((b, l, r, 2 * d if op == 3 else d), device=x.device, dtype=torch.float32)
        call("gh_match_bcast_fwd", ptr(x), ptr(y), op, b, l, r, d, ptr(out), stream())
        ctx.op = op
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        b, l, d = x.shape
        r = y.shape[1]
        g = _f32(g)
        dx, dy = torch.empty_like(x), torch.empty_like(y)
        call("gh_match_bcast_bwd", ptr(x), ptr(y), ptr(g), ctx.op, b, l, r, d, ptr(dx), ptr(dy), stream())
        return dx, dy, None


def match_bcast(x, y, op: str):
    """x (B,L,D), y (B,R,D) -> (B,L,R,D) = x[:, :, None] op y[:, None] for op 'mul', 'plus', 'minus'; 'concat' gives
    (B,L,R,2D) = [x, y].  Written once, without the reference's two repeat copies."""
    if op not in MATCH_BCAST_OPS:
        raise ValueError("match_bcast: %s is not one of %s" % (op, list(MATCH_BCAST_OPS)))
    return _MatchBcast.apply(x, y, MATCH_BCAST_OPS[op])


class _GaussKernel(torch.autograd.Function):
    """matchzoo/modules/gaussian_kernel.py:34-36: gh_gauss_kernel_*."""

    @staticmethod
    def forward(ctx, x, mu, sigma):
        _lib.require_cuda(x)
        x = _f32(x)
        y = torch.empty_like(x)
        call("gh_gauss_kernel_fwd", ptr(x), float(mu), float(sigma), x.numel(), ptr(y), stream())
        ctx.params = (float(mu), float(sigma))
        ctx.save_for_backward(x, y)
        return y

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        g = _f32(g)
        dx = torch.empty_like(x)
        call("gh_gauss_kernel_bwd", ptr(x), ptr(y), ptr(g), ctx.params[0], ctx.params[1], x.numel(), ptr(dx), stream())
        return dx, None, None


def gauss_kernel(x, mu: float, sigma: float):
    """exp(-0.5 (x - mu)^2 / sigma^2), elementwise; sigma == 0 is refused."""
    return _GaussKernel.apply(x, mu, sigma)

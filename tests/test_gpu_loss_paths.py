"""Every path of gh_softmax_xent_fwd / gh_softmax_xent_bwd (csrc/loss_ops.hip), called through the C-ABI on NaN-fenced buffers and
compared with the float64 restatement of tests/heads_ref.py at tests.util.TOL = 1e-4 of the largest entry of the float64 result
(the loss, the log-sum-exps, the gradient).

Paths by the row width c (the constants tests/test_bert_heads_cpu.py reads out of the .hip file): c <= LANE_MAX_C one lane per
row, c <= WAVE_MAX_C one wave per row, wider one workgroup per row; each wide path as float4 accesses (cs == 1, 16-byte base and
row stride), float2 accesses (8-byte base and row stride: a contiguous 30522-wide matrix, 30522 = 2 mod 4) or element by element.  No path stages a row in LDS (the log-sum-exp is a running maximum and sum), so there is no
LDS bound to step over; the widest case is 3 x 30522.

The logits sit at their strides inside a buffer of random values, the gradient inside a buffer of NaN: after the calls the
logits' buffer holds the bits it held, every float of the gradient's buffer outside the (row, class) positions is still NaN,
ignored rows are exact zeros, the fences are intact, and a second pair of calls gives the same bits."""
import ctypes
import math

import pytest
import torch

from tests import heads_ref
from tests.util import DEV, TOL, _Fenced, _ops, bits_equal, rel_close

pytestmark = pytest.mark.gpu

LANE_MAX_C, WAVE_MAX_C = 32, 2048      # XENT_LANE_MAX_C, XENT_WAVE_MAX_C of csrc/loss_ops.hip
WIDTHS = sorted({1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099} |
                {t + d for t in (LANE_MAX_C, WAVE_MAX_C) for d in (-1, 0, 1)})
ROWS = (1, 2, 7, 65, 257)


def _clamp_events(reset=False):
    _lib, _ = _ops()
    buf = (ctypes.c_int64 * 5)()
    _lib.call("gh_clamp_events_n", ctypes.cast(buf, ctypes.c_void_p), 5, 1 if reset else 0)
    return list(buf)


def _logits(rows, c, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, c, generator=g) * 3.0
    return x


def _labels(rows, c, seed, ignore, how="some"):
    """how: none | some | ends | all rows carry the ignore index."""
    g = torch.Generator().manual_seed(seed + 1)
    y = torch.randint(0, c, (rows,), generator=g)
    if how == "some":
        y[torch.rand(rows, generator=g) < 0.3] = ignore
    elif how == "ends":
        y[0] = ignore
        y[-1] = ignore
    elif how == "all":
        y[:] = ignore
    return y


class _Run:
    """One forward and one backward on fenced buffers.  x (rows, c) float32 and y (rows,) int64 on the CPU; pad / dpad: floats
    between a row's span and the next row; mis: the logits' and the gradient's base 4 bytes past a 16-byte boundary."""

    def __init__(self, x, y, ignore, cs=1, pad=0, dcs=1, dpad=0, mis=False, i64=True, g=1.0):
        _lib, _ = _ops()
        rows, c = x.shape
        self.rows, self.c, self.ignore, self.gval = rows, c, ignore, g
        ldx, lddx = c * cs + pad, c * dcs + dpad
        F = self.F = _Fenced()
        gen = torch.Generator().manual_seed(99)
        xb = torch.randn(rows * ldx, generator=gen)
        xb.view(rows, ldx)[:, :c * cs:cs] = x
        self.xbuf = F.put("x", xb, mis=mis)
        self.x_before = self.xbuf.clone()
        self.dbuf = F.put("dx", shape=(rows * lddx,), mis=mis)
        self.lse = F.put("lse", shape=(rows,))
        self.lse_lo = F.put("lse_lo", shape=(rows,))
        self.row_loss = F.put("row_loss", shape=(rows,))
        self.loss = F.put("loss", shape=(1,))
        self.g = F.put("g", torch.tensor([g]))
        self.n_kept = torch.tensor([-7, -7, -7], dtype=torch.int64, device=DEV)
        self.labels = (y if i64 else y.to(torch.int32)).to(DEV)
        self.dview = self.dbuf.view(rows, lddx)[:, :c * dcs:dcs]
        self.touched = torch.zeros(rows, lddx, dtype=torch.bool)
        self.touched[:, :c * dcs:dcs] = True
        self.fwd_args = (self.xbuf.data_ptr(), ldx, cs, self.labels.data_ptr(), int(i64), ignore, rows, c, self.lse.data_ptr(),
                         self.lse_lo.data_ptr(), self.row_loss.data_ptr(), self.loss.data_ptr(), self.n_kept[1:].data_ptr(), _lib.stream())
        self.bwd_args = (self.xbuf.data_ptr(), ldx, cs, self.labels.data_ptr(), int(i64), ignore, rows, c, self.lse.data_ptr(),
                         self.lse_lo.data_ptr(), self.g.data_ptr(), self.n_kept[1:].data_ptr(), self.dbuf.data_ptr(), lddx, dcs, _lib.stream())
        self.x, self.y = x, y

    def call(self):
        _lib, _ = _ops()
        _lib.call("gh_softmax_xent_fwd", *self.fwd_args)
        _lib.call("gh_softmax_xent_bwd", *self.bwd_args)
        torch.cuda.synchronize()
        return self.loss.clone(), self.lse.clone(), self.dbuf.clone(), self.n_kept.clone()

    def check(self, what):
        first = self.call()
        loss, lse, dbuf, n_kept = first
        self.F.check(what)
        bits_equal(self.xbuf, self.x_before, what + ": the logits' buffer")
        assert n_kept[0] == -7 and n_kept[2] == -7, what + ": around n_kept"
        x64 = self.x.double()
        want_loss, want_lse, n = heads_ref.xent(x64, self.y, self.ignore)
        assert int(n_kept[1]) == n, (what, int(n_kept[1]), n)
        rel_close(lse, want_lse, TOL, what + " lse", fam="softmax_xent")
        if n == 0:
            assert bool(torch.isnan(loss).all()) and math.isnan(float(want_loss)), what + ": no kept row gives a NaN loss"
        else:
            rel_close(loss[0], want_loss, TOL, what + " loss", fam="softmax_xent")
        want_dx = heads_ref.xent_grad(x64, self.y, want_lse, n, self.gval, self.ignore)
        got = self.dview.cpu()
        rel_close(got, want_dx, TOL, what + " dx", fam="softmax_xent")
        dropped = ~heads_ref.kept_rows(self.y, self.c, self.ignore)
        assert bool((got[dropped] == 0).all()), what + ": rows without a kept label are exact zeros"
        flat = dbuf.cpu().view(self.rows, -1)
        assert bool(torch.isnan(flat[~self.touched]).all()), what + ": the gradient's buffer was written between its elements"
        for a, b, k in zip(first, self.call(), ("loss", "lse", "dx", "n_kept")):
            bits_equal(a.view(torch.float32) if a.dtype == torch.int64 else a, b.view(torch.float32) if b.dtype == torch.int64 else b,
                       f"{what}: {k} of two calls")
        return first


@pytest.mark.parametrize("c", WIDTHS)
def test_widths_and_row_counts(c):
    """Every width of the grid at every row count; the layout, the label type, the ignore index and which rows are ignored
    rotate with the case so that each width meets several of them."""
    for i, rows in enumerate(ROWS):
        k = i + c
        ignore = (-1, -100, c)[k % 3]
        how = ("none", "some", "ends", "some", "all")[(i + c // 7) % 5]
        x, y = _logits(rows, c, 7 * c + rows), _labels(rows, c, c + rows, ignore, how)
        run = _Run(x, y, ignore, cs=1 + k % 2, pad=(0, 3, 4)[k % 3], dcs=1 + (k // 2) % 2, dpad=(4, 0, 5)[k % 3], mis=k % 5 == 0,
                   i64=k % 2 == 0, g=(1.0, 0.37, -2.5)[k % 3])
        run.check(f"c={c} rows={rows} ignore={ignore} ({how})")


@pytest.mark.parametrize("c", [5, 257, 4099])
def test_every_layout_on_every_path(c):
    """One width per path: cs in {1, 2}, a row stride without a gap and with gaps that make it 0, 2 and 3 modulo 4 floats (float4,
    float2 and element-wise accesses at cs = 1), an aligned and a misaligned base, and a gradient whose strides differ from the
    logits'.  The results of all layouts agree bit for bit."""
    rows, ignore = 7, -100
    x, y = _logits(rows, c, c), _labels(rows, c, c, ignore, "ends")
    seen = []
    for cs in (1, 2):
        for pad in (0, 8 - (c * cs) % 4, 6 - (c * cs) % 4 + 4, 3 - (c * cs) % 4 + 4):
            for mis in (False, True):
                for dcs, dpad in ((cs, pad), (3 - cs, pad + 1)):
                    run = _Run(x, y, ignore, cs=cs, pad=pad, dcs=dcs, dpad=dpad, mis=mis, g=0.5)
                    loss, lse, _, _ = run.check(f"c={c} cs={cs} pad={pad} mis={mis} dcs={dcs} dpad={dpad}")
                    seen.append((loss, lse, run.dview.clone()))
    for loss, lse, dx in seen[1:]:
        bits_equal(loss, seen[0][0], f"c={c}: loss across layouts")
        bits_equal(lse, seen[0][1], f"c={c}: lse across layouts")
        bits_equal(dx, seen[0][2], f"c={c}: dx across layouts")


@pytest.mark.parametrize("rows", [1, 3])
def test_vocabulary_wide_rows(rows):
    c = 30522
    x, y = _logits(rows, c, rows), _labels(rows, c, rows, -1, "none")
    if rows == 3:
        y[1] = -1
    assert c % 4 == 2
    runs = [_Run(x, y, -1, g=1.7).check(f"c={c} rows={rows} contiguous: row stride 2 mod 4, float2"),
            _Run(x, y, -1, pad=2, dpad=2, g=1.7).check(f"c={c} rows={rows} row stride {c + 2}: float4"),
            _Run(x, y, -1, pad=1, dpad=1, g=1.7).check(f"c={c} rows={rows} odd row stride: element by element"),
            _Run(x, y, -1, pad=2, dpad=0, g=1.7).check(f"c={c} rows={rows} float4 logits, float2 gradient")]
    for loss, lse, _, _ in runs[1:]:
        bits_equal(loss, runs[0][0], f"c={c}: loss across access widths")
        bits_equal(lse, runs[0][1], f"c={c}: lse across access widths")


@pytest.mark.parametrize("c", [2, 9, 384, 4099])
@pytest.mark.parametrize("ignore", [-1, -100, "c"])
@pytest.mark.parametrize("how", ["none", "some", "ends", "all"])
def test_ignore_indices_and_label_types(c, ignore, how):
    ignore = c if ignore == "c" else ignore
    rows = 9
    x, y = _logits(rows, c, c + 3), _labels(rows, c, c + 3, ignore, how)
    a = _Run(x, y, ignore, i64=True, g=0.25).check(f"c={c} ignore={ignore} {how} int64")
    b = _Run(x, y, ignore, i64=False, g=0.25).check(f"c={c} ignore={ignore} {how} int32")
    for u, v, k in zip(a[:3], b[:3], ("loss", "lse", "dx")):
        bits_equal(u, v, f"int32 against int64 labels: {k}")


@pytest.mark.parametrize("c", [3, 300, 2500])
def test_extreme_logit_values(c):
    """A row mixing +1e4 and -1e4, a row of equal values, and labels on a row's maximum and on its minimum."""
    x = _logits(6, c, c)
    x[0, ::2], x[0, 1::2] = 1e4, -1e4
    x[1, ::2], x[1, 1::2] = 1e4, -1e4
    x[2, :] = 0.75
    x[3, :] = -1e4
    y = torch.tensor([0, 1, c - 1, 0, int(x[4].argmax()), int(x[5].argmin())])
    _Run(x, y, -100, g=1.0).check(f"c={c} extreme values")
    _Run(x, y, -100, cs=2, pad=1, g=1.0).check(f"c={c} extreme values, element path")


@pytest.mark.parametrize("c", [4, 100, 3000])
def test_a_label_outside_the_classes_drops_its_row_and_is_counted(c):
    rows = 5
    x, y = _logits(rows, c, c), _labels(rows, c, c, -100, "none")
    y[1], y[3] = -100, c + 2
    _clamp_events(reset=True)
    run = _Run(x, y, -100)
    run.call()
    assert _clamp_events() == [0, 0, 0, 0, 1], "one forward counts the label once; the backward counts nothing"
    _clamp_events(reset=True)
    run.check(f"c={c} label {c + 2}")
    y[3] = -5
    _Run(x, y, -100, i64=False).check(f"c={c} label -5")
    assert _clamp_events(reset=True)[4] == 4      # two forward calls per check


def test_refusals_write_nothing():
    _lib, _ = _ops()
    x, y = _logits(4, 10, 1), _labels(4, 10, 1, -100, "none")
    run = _Run(x, y, -100, pad=2)
    fwd, bwd = list(run.fwd_args), list(run.bwd_args)

    def refused(name, args, i, value, match):
        a = list(args)
        a[i] = value
        with pytest.raises(RuntimeError, match=match):
            _lib.call(name, *a)

    for i in (0, 3, 8, 9, 10, 11, 12):
        refused("gh_softmax_xent_fwd", fwd, i, None, "NULL")
    for i in (0, 3, 8, 9, 10, 11, 12):
        refused("gh_softmax_xent_bwd", bwd, i, None, "NULL")
    for name, args in (("gh_softmax_xent_fwd", fwd), ("gh_softmax_xent_bwd", bwd)):
        refused(name, args, 6, 0, "rows=0")
        refused(name, args, 6, -3, "rows=-3")
        refused(name, args, 7, 0, "c=0")
        refused(name, args, 7, -1, "c=-1")
        refused(name, args, 2, 0, "element stride 0")
        refused(name, args, 1, 9, "row stride 9")
    refused("gh_softmax_xent_bwd", bwd, 14, 0, "element stride 0 of dx")
    refused("gh_softmax_xent_bwd", bwd, 13, 9, "row stride 9 of dx")
    torch.cuda.synchronize()
    run.F.check("refused calls")
    for t in (run.dbuf, run.lse, run.lse_lo, run.row_loss, run.loss):
        assert bool(torch.isnan(t).all()), "a refused call wrote an output"
    run.check("after the refusals")


def test_the_op_reads_views_in_place_and_refuses_what_the_fronts_refuse():
    """ops.softmax_cross_entropy on the strided columns of a (B, L, 2) tensor and on a column slice: the result and the gradient
    are those of the contiguous copy, bit for bit; empty input gives NaN and an empty gradient."""
    _, ops = _ops()
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(4, 37, 2, generator=g).to(DEV).requires_grad_(True)
    pos = torch.tensor([0, 36, 37, 5]).to(DEV)
    wide = torch.randn(6, 50, generator=g).to(DEV).requires_grad_(True)
    lab = torch.tensor([0, 3, -100, 29, 1, 2]).to(DEV)
    for view, labels, ignore, leaf in ((lambda t: t[..., 0], pos, 37, logits), (lambda t: t[..., 1], pos, 37, logits),
                                       (lambda t: t[:, 10:40], lab, -100, wide)):
        v = view(leaf)
        assert not v.is_contiguous()
        loss = ops.softmax_cross_entropy(v, labels, ignore_index=ignore)
        grad, = torch.autograd.grad(loss * 3.0, leaf)
        copy = view(leaf.detach()).contiguous().requires_grad_(True)
        loss_c = ops.softmax_cross_entropy(copy, labels, ignore_index=ignore)
        grad_c, = torch.autograd.grad(loss_c * 3.0, copy)
        bits_equal(loss.detach().reshape(1), loss_c.detach().reshape(1), "view against copy: loss")
        bits_equal(view(grad), grad_c, "view against copy: gradient")
        want = torch.nn.functional.cross_entropy(copy.detach().double().cpu(), labels.cpu(), ignore_index=ignore)
        rel_close(loss, want, TOL, "view: loss against torch in float64")
    empty = torch.zeros(0, 5, device=DEV, requires_grad=True)
    loss = ops.softmax_cross_entropy(empty, torch.zeros(0, dtype=torch.long, device=DEV))
    assert bool(torch.isnan(loss)) and torch.autograd.grad(loss, empty)[0].shape == (0, 5)
    with pytest.raises(ValueError, match="float32"):
        ops.softmax_cross_entropy(wide.double(), lab)
    with pytest.raises(ValueError, match="labels"):
        ops.softmax_cross_entropy(wide, lab[:5])
    with pytest.raises(ValueError, match="int64 or int32"):
        ops.softmax_cross_entropy(wide, lab.float())

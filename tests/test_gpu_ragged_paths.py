"""Every path of the ragged claim <-> evidence helpers of csrc/ragged_ops.hip (gh_seg_offsets / gh_seg_sum / gh_seg_pad /
gh_seg_unpad, gh_masked_mean_fwd / _bwd, gh_evd_assemble_fwd / _bwd) against the plain numpy restatements of tests/util.py
(checked on their own against the oracle's pad_left / pad_right by tests/test_concat_restatement_cpu.py).

The C-ABI entries are called directly.  Every float operand and output sits in a NaN-fenced allocation of its own, every
integer output between runs of a sentinel; outputs start as NaN (the sentinel) and whatever the header documents as
written must come back finite.  Copies are exact (np.array_equal); sums are held to TOL = 1e-4 of the float64 result's
largest entry (family "ragged").  What is documented as NOT written -- the gap columns of a padded row wider than x, the
rows of a claim's evidences beyond n_max in gh_seg_unpad -- must still be NaN."""
import ctypes

import numpy as np
import pytest
import torch

from tests.util import (DEV, _Fenced, _ops, _rel, r_clamp_sources, r_evd_assemble, r_evd_assemble_bwd, r_masked_mean,
                        r_masked_mean_bwd, r_seg_offsets, r_seg_pad, r_seg_sum, r_seg_unpad)

pytestmark = pytest.mark.gpu

FAM = "ragged"
SENT = -123457


class _IntFenced:
    """Integer outputs between 64 sentinels on either side, filled with the sentinel themselves."""

    def __init__(self):
        self.items = []

    def put(self, name, n, dtype=torch.int32):
        buf = torch.full((n + 128,), SENT, device=DEV, dtype=dtype)
        self.items.append((name, buf, n))
        return buf[64:64 + n]

    def check(self, what):
        for name, buf, n in self.items:
            assert bool((buf[:64] == SENT).all() & (buf[64 + n:] == SENT).all()), f"{what}: the fence around {name} was written"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _offsets(counts):
    return r_seg_offsets(counts, int(np.sum(counts)))[0]


# ----------------------------------------------------------------------------- gh_seg_offsets
def _counts(b, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 4, size=b).astype(np.int64)
    if b > 1:
        c[0], c[-1], c[b // 2] = 0, 0, 3
    else:
        c[0] = 3
    return c


@pytest.mark.parametrize("with_has", [True, False])
@pytest.mark.parametrize("delta", [0, 5, -3], ids=["b1=sum", "b1>sum", "b1<sum"])
@pytest.mark.parametrize("b", [1, 257])
def test_seg_offsets(b, delta, with_has):
    """b = 257: the 256-thread loop over the claims wraps; counts are 0 for the first and the last claim.  b1 above the sum:
    the tail maps to claim 0; b1 below the sum: nothing is written past pair2claim[b1)."""
    _lib, _ = _ops()
    counts = _counts(b, 40 + b)
    b1 = int(counts.sum()) + delta
    what = f"seg_offsets b={b} b1={b1} (sum {int(counts.sum())})"
    fi, ff = _IntFenced(), _Fenced()
    offsets, p2c = fi.put("offsets", b + 1), fi.put("pair2claim", b1)
    has = ff.put("has", shape=(b,)) if with_has else None
    cd = _dev(counts)                                    # (kept in a variable: a temporary would be freed before the launch)
    _lib.call("gh_seg_offsets", _lib.ptr(cd), b, _lib.ptr(offsets), _lib.ptr(p2c), b1, _lib.ptr(has), _lib.stream())
    torch.cuda.synchronize()
    fi.check(what)
    ff.check(what)
    want_off, want_p2c, want_has = r_seg_offsets(counts, b1)
    assert np.array_equal(_np(offsets), want_off), what
    assert np.array_equal(_np(p2c), want_p2c), what
    if with_has:
        assert np.array_equal(_np(has), want_has), what


# ----------------------------------------------------------------------------- gh_seg_sum
@pytest.mark.parametrize("x", [1, 256, 300])
def test_seg_sum(x):
    """Counts on either side of the unroll of eight rows; an empty claim gives exact zeros; x = 300: the column loop wraps."""
    _lib, _ = _ops()
    counts = np.array([0, 1, 7, 8, 9, 17, 0], dtype=np.int64)
    offsets = _offsets(counts)
    gen = torch.Generator().manual_seed(50 + x)
    src = 0.2 * torch.randn((int(counts.sum()), x), generator=gen)
    f = _Fenced()
    s, dst = f.put("src", src), f.put("dst", shape=(len(counts), x))
    od = _dev(offsets)
    _lib.call("gh_seg_sum", _lib.ptr(s), _lib.ptr(od), _lib.ptr(dst), len(counts), x, _lib.stream())
    torch.cuda.synchronize()
    f.check(f"seg_sum x={x}")
    _rel(dst, r_seg_sum(src.numpy(), offsets), f"seg_sum x={x}", FAM)
    got = _np(dst)
    assert not got[0].any() and not got[-1].any(), "an empty claim's sum is not exactly 0"
    assert np.array_equal(got[1], src.numpy()[0]), "a single row is not copied exactly"


# ----------------------------------------------------------------------------- gh_seg_pad / gh_seg_unpad
@pytest.mark.parametrize("x,ld", [(5, 8), (300, 304), (300, 300)])
def test_seg_pad_and_unpad(x, ld):
    """Counts 0, n_max and above n_max; a row pitch wider than x leaves the gap columns alone; unpad writes the rows that
    have a slot and no other."""
    _lib, _ = _ops()
    n_max = 4
    counts = np.array([2, 0, 4, 6, 1], dtype=np.int64)
    b, b1 = len(counts), int(counts.sum())
    offsets = _offsets(counts)
    gen = torch.Generator().manual_seed(60 + x)
    src = 0.2 * torch.randn((b1, x), generator=gen)
    what = f"seg_pad x={x} ld={ld}"
    f = _Fenced()
    s, dst = f.put("src", src), f.put("dst", shape=(b, n_max, ld))
    od = _dev(offsets)
    _lib.call("gh_seg_pad", _lib.ptr(s), _lib.ptr(od), _lib.ptr(dst), b, n_max, x, ld, _lib.stream())
    torch.cuda.synchronize()
    f.check(what)
    got = _np(dst)
    assert np.array_equal(got[:, :, :x], r_seg_pad(src.numpy(), offsets, n_max)), what
    assert np.isnan(got[:, :, x:]).all(), f"{what}: a gap column was written"
    # unpad from a fully finite padded tensor of the same pitch
    padded = 0.2 * torch.randn((b, n_max, ld), generator=gen)
    f = _Fenced()
    p, back = f.put("padded", padded), f.put("unpadded", shape=(b1, x))
    _lib.call("gh_seg_unpad", _lib.ptr(p), _lib.ptr(od), _lib.ptr(back), b, n_max, x, ld, _lib.stream())
    torch.cuda.synchronize()
    f.check(what + " unpad")
    want = r_seg_unpad(padded.numpy()[:, :, :x], offsets, np.full((b1, x), np.nan, np.float32))
    assert np.isnan(want[offsets[3] + n_max:offsets[4]]).all() and np.isfinite(want).sum() == (b1 - 2) * x
    assert np.array_equal(_np(back), want, equal_nan=True), what + " unpad"


# ----------------------------------------------------------------------------- gh_masked_mean_fwd / _bwd
@pytest.mark.parametrize("h", [1, 256, 300])
@pytest.mark.parametrize("l", [1, 8, 9, 30])
def test_masked_mean(l, h):
    """l on either side of the unroll of eight tokens; sequence 1 has a single live token; the backward writes every row
    and exact zeros on the rows of masked tokens."""
    _lib, _ = _ops()
    b = 4
    rng = np.random.default_rng(70 + l)
    ids = rng.integers(0, 3, size=(b, l)).astype(np.int32)
    ids[0, :] = 5
    ids[1, :] = 0
    ids[1, l - 1] = 2                                    # one live token, the last one
    ids[2, 0] = 1
    ids[3, l // 2] = 7
    lens = (ids > 0).sum(1).astype(np.float32)
    assert lens.min() >= 1 and lens[1] == 1
    gen = torch.Generator().manual_seed(71 + l + h)
    hid, g = 0.2 * torch.randn((b, l, h), generator=gen), 0.2 * torch.randn((b, h), generator=gen)
    what = f"masked_mean l={l} h={h}"
    f = _Fenced()
    hd, gd, ld_ = f.put("hid", hid), f.put("g", g), f.put("lens", torch.from_numpy(lens))
    dst, dhid = f.put("dst", shape=(b, h)), f.put("dhid", shape=(b, l, h))
    idd = _dev(ids)
    _lib.call("gh_masked_mean_fwd", _lib.ptr(hd), _lib.ptr(idd), _lib.ptr(ld_), _lib.ptr(dst), b, l, h, _lib.stream())
    _lib.call("gh_masked_mean_bwd", _lib.ptr(gd), _lib.ptr(idd), _lib.ptr(ld_), _lib.ptr(dhid), b, l, h, _lib.stream())
    torch.cuda.synchronize()
    f.check(what)
    _rel(dst, r_masked_mean(hid.numpy(), ids, lens), what + " fwd", FAM)
    _rel(dhid, r_masked_mean_bwd(g.numpy(), ids, lens), what + " bwd", FAM)
    assert np.array_equal(_np(dst)[1], hid.numpy()[1, l - 1]), what + ": the single live token is not its own mean"
    assert not _np(dhid)[ids == 0].any(), what + ": the gradient row of a masked token is not exactly 0"


# ----------------------------------------------------------------------------- gh_evd_assemble_fwd
def _clamp_events(reset):
    _lib, _ = _ops()
    buf = (ctypes.c_int64 * 4)()
    _lib.call("gh_clamp_events", ctypes.cast(buf, ctypes.c_void_p), 1 if reset else 0)
    return [int(v) for v in buf]


@pytest.mark.parametrize("r", [1, 64, 65, 100])
@pytest.mark.parametrize("src64,doc64", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=["s32d32", "s32d64", "s64d32", "s64d64"])
def test_evd_assemble_fwd(src64, doc64, r):
    """The four (sources, document) id types; source -1 reads row 0 uncounted, ids beyond the table are clamped and counted
    once each; r around the 64 lanes of the mask reduction; a slot of zeros (mask 0) and a slot whose only id sits in the
    last column (mask 1)."""
    _lib, _ = _ops()
    n_max, xa, ds, rows = 4, 12, 8, 6
    counts = np.array([2, 0, 4, 6, 1], dtype=np.int64)
    b, b1 = len(counts), int(counts.sum())
    offsets = _offsets(counts)
    rng = np.random.default_rng(80 + r)
    sources = rng.integers(0, rows, size=(b, n_max))
    sources[0, 1], sources[1, 0] = -1, -1                # the padding id, on a real and on a padding slot
    sources[2, 0], sources[2, 3], sources[4, 2] = rows, rows + 40, -2      # outside the table: clamped and counted
    document = rng.integers(0, 4, size=(b, n_max, r))
    document[0, 0] = 0                                   # mask 0
    document[0, 1] = 0
    document[0, 1, r - 1] = 1                            # one id, in the last column
    gen = torch.Generator().manual_seed(81 + r)
    avg, table = 0.2 * torch.randn((b1, xa), generator=gen), 0.2 * torch.randn((rows, ds), generator=gen)
    what = f"evd_assemble_fwd r={r} sources int{64 if src64 else 32} document int{64 if doc64 else 32}"
    f = _Fenced()
    a, t = f.put("avg", avg), f.put("table", table)
    right, mask = f.put("right", shape=(b, n_max, xa + ds)), f.put("mask", shape=(b, n_max))
    sd = _dev(sources.astype(np.int64 if src64 else np.int32))
    dd = _dev(document.astype(np.int64 if doc64 else np.int32))
    od = _dev(offsets)
    _clamp_events(reset=True)
    _lib.call("gh_evd_assemble_fwd", _lib.ptr(a), _lib.ptr(od), _lib.ptr(t), rows, _lib.ptr(sd), src64, _lib.ptr(dd), doc64,
              b, n_max, xa, ds, r, _lib.ptr(right), _lib.ptr(mask), _lib.stream())
    events = _clamp_events(reset=True)
    f.check(what)
    want_right, want_mask, want_clamped = r_evd_assemble(avg.numpy(), offsets, table.numpy(), sources, document, n_max)
    assert np.array_equal(_np(right), want_right), what
    assert np.array_equal(_np(mask), want_mask), what
    assert want_mask[0, 0] == 0.0 and want_mask[0, 1] == 1.0
    assert want_clamped == 3 and events[2] == 3, f"{what}: {events[2]} clamped article-source ids counted, 3 handed in"
    assert np.array_equal(want_right[0, 1, xa:], table.numpy()[0]) and np.array_equal(want_right[2, 3, xa:], table.numpy()[rows - 1])


def test_evd_assemble_fwd_without_a_table():
    _lib, _ = _ops()
    n_max, xa, r = 3, 300, 7
    counts = np.array([1, 3, 0], dtype=np.int64)
    b, b1 = len(counts), int(counts.sum())
    offsets = _offsets(counts)
    gen = torch.Generator().manual_seed(90)
    avg = 0.2 * torch.randn((b1, xa), generator=gen)
    document = np.random.default_rng(90).integers(0, 2, size=(b, n_max, r)).astype(np.int32)
    f = _Fenced()
    a, right, mask = f.put("avg", avg), f.put("right", shape=(b, n_max, xa)), f.put("mask", shape=(b, n_max))
    od, dd = _dev(offsets), _dev(document)
    _lib.call("gh_evd_assemble_fwd", _lib.ptr(a), _lib.ptr(od), None, 0, None, 0, _lib.ptr(dd), 0,
              b, n_max, xa, 0, r, _lib.ptr(right), _lib.ptr(mask), _lib.stream())
    torch.cuda.synchronize()
    f.check("evd_assemble_fwd ds=0")
    want_right, want_mask, _ = r_evd_assemble(avg.numpy(), offsets, None, None, document, n_max)
    assert np.array_equal(_np(right), want_right) and np.array_equal(_np(mask), want_mask)


# ----------------------------------------------------------------------------- gh_evd_assemble_bwd
def _assemble_bwd_case(b, n_max, xa, ds, rows, seed):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, n_max + 3, size=b).astype(np.int64)        # empty claims, full claims, claims over n_max
    counts[0] = max(counts[0], 1)
    sources = rng.integers(-1, rows + 1, size=(b, n_max))               # few rows: ids repeat within and across claims and
    gen = torch.Generator().manual_seed(seed)                           # ballot words; -1 and `rows` are clamped as in the forward
    g = 0.2 * torch.randn((b, n_max, xa + ds), generator=gen)           # (padding slots carry gradient AND ids real slots carry)
    d_table0 = 0.2 * torch.randn((rows, ds), generator=gen)
    return counts, sources, g, d_table0


def _assemble_bwd(b, n_max, xa, ds, rows, seed, src64, with_avg=True, with_table=True):
    _lib, _ = _ops()
    counts, sources, g, d_table0 = _assemble_bwd_case(b, n_max, xa, ds, rows, seed)
    offsets = _offsets(counts)
    what = f"evd_assemble_bwd b={b} n_max={n_max} int{64 if src64 else 32}{'' if with_avg else ' d_avg NULL'}{'' if with_table else ' d_table NULL'}"
    real = np.arange(n_max)[None, :] < np.minimum(counts, n_max)[:, None]
    table_row = r_clamp_sources(sources, rows)[0]
    assert b * n_max < 60 or np.isin(table_row[~real], table_row[real]).any(), "no padding slot shares a source with a real slot"
    f = _Fenced()
    gd = f.put("g", g)
    d_avg = f.put("d_avg", shape=(int(offsets[-1]), xa)) if with_avg else None
    d_table = f.put("d_table", d_table0) if with_table else None
    sd, od = _dev(sources.astype(np.int64 if src64 else np.int32)), _dev(offsets)
    _lib.call("gh_evd_assemble_bwd", _lib.ptr(gd), _lib.ptr(od), _lib.ptr(sd), src64, rows, b, n_max, xa, ds,
              _lib.ptr(d_avg), _lib.ptr(d_table), _lib.stream())
    torch.cuda.synchronize()
    f.check(what)
    want_avg, want_table = r_evd_assemble_bwd(g.numpy(), offsets, sources, rows, xa, d_table0.numpy() if with_table else None)
    if with_avg:
        assert np.array_equal(_np(d_avg), want_avg), what + ": d_avg"
    if with_table:
        _rel(d_table, want_table, what + " d_table", FAM)
    return d_table


@pytest.mark.parametrize("src64", [0, 1], ids=["int32", "int64"])
@pytest.mark.parametrize("b,n_max", [(1, 1), (9, 7), (8, 8), (13, 5), (13, 10)], ids=["1", "63", "64", "65", "130"])
def test_evd_assemble_bwd_slot_counts(b, n_max, src64):
    """n_slots 1, 63, 64, 65, 130 against the 64-slot ballot words; d_table starts from non-zero values; sources repeat
    within a claim, across claims and across ballot words; padding slots carry ids of real slots and must not join; two
    calls agree bit for bit (slot order, no atomics)."""
    a = _assemble_bwd(b, n_max, 12, 8, 5, 100 + b * n_max, src64)
    again = _assemble_bwd(b, n_max, 12, 8, 5, 100 + b * n_max, src64)
    assert torch.equal(a, again)


def test_evd_assemble_bwd_null_outputs():
    _assemble_bwd(9, 7, 12, 8, 5, 163, 0, with_avg=False)
    _assemble_bwd(9, 7, 12, 8, 5, 163, 1, with_table=False)


def test_evd_assemble_bwd_lds_opt_in_and_the_slot_limit():
    """420 claims x 30 slots = 12 600 slot ids + 197 ballot words = 51 976 B of dynamic LDS, above the 48 KB a kernel gets
    without the attribute; 38 001 slots are refused by the host check before any launch."""
    _lib, _ = _ops()
    _assemble_bwd(420, 30, 4, 4, 50, 171, 0)
    offsets = _dev(np.zeros(38002, np.int32))
    g = torch.zeros((38001, 1, 8), device=DEV)
    src = torch.zeros((38001, 1), device=DEV, dtype=torch.int32)
    d_avg, d_table = torch.zeros((1, 4), device=DEV), torch.zeros((2, 4), device=DEV)
    with pytest.raises(RuntimeError, match=r"evd_assemble_bwd: 38001 claim x evidence slots"):
        _lib.call("gh_evd_assemble_bwd", _lib.ptr(g), _lib.ptr(offsets), _lib.ptr(src), 0, 2, 38001, 1, 4, 4, _lib.ptr(d_avg),
                  _lib.ptr(d_table), _lib.stream())
    torch.cuda.synchronize()

"""The pairwise helpers on the GPU (csrc/pair_ops.hip, ops.pair and get_amd.pairwise): the reference's goldens on the public
functions, the two distances and the windowed mean against the float64 restatements of tests/pair_ref.py on every tiling path,
L1 bit for bit on a dyadic grid (which pins sign(0) = 0), the Euclidean distance at coincident rows, the histogram's counts
(exactly where every value is exact, within the derived fragility margin elsewhere), and once per kernel the NaN fences,
the repeatability and the limits.  The ratios the tests print (WORST) are the ones quoted in DESIGN.md 4.24."""
import math

import numpy as np
import pytest
import torch

from tests import pair_ref as R
from tests.test_pair_cpu import GOLDEN_TOL, HIST_MODES, archive, arr, cases_of, check_golden, window_args
from tests.util import TOL, WORST, _Fenced, bits_equal, rel_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-10


def _up(gen, shape):
    return torch.randint(-16, 17, tuple(shape), generator=gen).float() / 16


def _run(fn, inputs, g, *extra):
    """fn(*inputs on the device as given, *extra) and its gradients under g: (out, grads...)."""
    args = [t.detach().requires_grad_(True) for t in inputs]
    out = fn(*args, *extra)
    if out.numel():
        out.backward(g.to(DEV))
    return (out.detach(),) + tuple(a.grad for a in args)


def _wide(t, extra, off):
    """t as a column slice of a wider device tensor whose base lies 4 bytes past a 16-byte boundary."""
    n, l, wd = t.shape
    flat = torch.full((n * l * (wd + extra) + 1,), 7.0, device=DEV)
    v = flat[1:].view(n, l, wd + extra)[:, :, off:off + wd]
    v.copy_(t)
    assert flat[1:].data_ptr() % 16 == 4 and not v.is_contiguous()
    return v


# ----------------------------------------------------------------------------- goldens on the public functions
@pytest.mark.parametrize("key", cases_of(("l2", "l1")))
def test_distances_match_reference_goldens(golden_dir, key):
    from get_amd import pairwise
    z, _ = archive(golden_dir)
    fn = pairwise.cosine_distance if key.startswith("l2::") else pairwise.l1_distance
    out, da, db = _run(fn, (arr(z, key, "a").to(DEV), arr(z, key, "b").to(DEV)), arr(z, key, "g"))
    check_golden(z, key, {"out": out, "grad::a": da, "grad::b": db}, "drop-in")


@pytest.mark.parametrize("key", cases_of(("ma", "mod", "ctx")))
def test_window_means_match_reference_goldens(golden_dir, key):
    from get_amd import pairwise
    z, meta = archive(golden_dir)
    w = meta["params"][key]["window"]
    x, g = arr(z, key, "x").to(DEV), arr(z, key, "g")
    if key.startswith("ctx::"):
        mask = arr(z, key, "mask").to(DEV)
        out, dx = _run(lambda t: pairwise._get_doc_context_copacrr(t, mask, w), (x,), g)
        assert bool((out[mask == 0] == 0).all())
    elif key.startswith("mod::"):
        out, dx = _run(pairwise.MovingAverage(w, 1), (x,), g)
    else:
        out, dx = _run(lambda t: pairwise.moving_average(t, w, 1), (x,), g)
    if key == "ma::over":
        assert tuple(out.shape) == (x.shape[0], 0, x.shape[2]) and dx is None
        return
    check_golden(z, key, {"out": out, "grad::x": dx}, "drop-in")


def _fragile(scaled, bins, d):
    """(nearest integer, is-fragile) of float64 scaled values: within (bins - 1) / 2 (D + 2) 2^-23 of an integer -- the fp32
    dot-product bound (D products and sums of |terms| <= 1, two more roundings for the scaling), carried to the scaled value."""
    k = np.round(scaled)
    return k.astype(np.int64), np.abs(scaled - k) <= (bins - 1) / 2 * (d + 2) * 2.0 ** -23


def _count_bounds(scaled, bins, d):
    """(lower, upper) int64 (Lq, bins) of one sample's counts: 1 + the robust pairs of a bin, plus the fragile pairs next to it."""
    k, frag = _fragile(scaled, bins, d)
    idx = R.hist_bins(scaled, bins)
    lower, extra = np.ones((scaled.shape[0], bins), np.int64), np.zeros((scaled.shape[0], bins), np.int64)
    for i in range(scaled.shape[0]):
        for j in range(scaled.shape[1]):
            if not frag[i, j]:
                lower[i, idx[i, j]] += 1
            else:
                for b in {int(np.clip(k[i, j] - 1, 0, bins - 1)), int(np.clip(k[i, j], 0, bins - 1))}:
                    extra[i, b] += 1
    return lower, lower + extra, int(frag.sum())


@pytest.mark.parametrize("key", cases_of(("hist",)))
def test_matching_histogram_matches_reference_goldens(golden_dir, key):
    from get_amd import pairwise
    z, meta = archive(golden_dir)
    p = meta["params"][key]
    (V, D, Lq, Ld), bins = p["shape"], p["bins"]
    table = arr(z, key, "table").double().numpy()
    il, ir, ln = z[f"{key}::ids_left"], z[f"{key}::ids_right"], z[f"{key}::len_right"]
    scaled = z[f"{key}::scaled"]
    units = {m: pairwise.MatchingHistogram(bins, table, p["normalize"], m) for m in HIST_MODES}
    got = {m: u.transform_batch(torch.from_numpy(il).to(DEV), torch.from_numpy(ir), ln).cpu().double().numpy() for m, u in units.items()}
    counts = got["CH"]
    assert counts.shape == (len(ln), Lq, bins) and np.array_equal(counts, np.round(counts))
    assert np.array_equal(counts.sum(2), np.repeat(ln[:, None] + bins, Lq, axis=1))          # every row total, exactly
    n_frag = 0
    for i, n in enumerate(ln):
        if key == "hist::shared":       # cosine 1 sits exactly on the top edge: either of the top two bins
            same = (il[i][:, None] == ir[i][None, :n]).sum(1)
            assert int(same.sum()) >= min(Lq, n)
            assert (counts[i][:, bins - 2:].sum(1) - 2 >= same).all(), (key, i)
            continue
        lower, upper, nf = _count_bounds(scaled[i, :, :n], bins, D)
        n_frag += nf
        assert (lower <= counts[i]).all() and (counts[i] <= upper).all(), (key, i)
        if key == "hist::dyadic":       # every value exact in fp32 and float64: the reference's counts
            assert nf == int((scaled[i, :, :n] == np.round(scaled[i, :, :n])).sum())
            assert np.array_equal(counts[i], z[f"{key}::out::CH"][i].astype(np.float64)), (key, i)
    for m in ("NH", "LCH"):             # the other two modes on equal counts
        rel_close(got[m], np.stack([R.hist_mode(c, m) for c in counts]), TOL, f"{key} {m} of the device's counts", fam="match_hist")
    if key == "hist::dyadic":
        for m in HIST_MODES:
            rel_close(got[m], z[f"{key}::out::{m}"], GOLDEN_TOL, f"{key} {m}", fam="match_hist")
    elif key != "hist::shared":
        share = n_frag / max(int(ln.sum()) * Lq, 1)
        print(f"{key}: {n_frag} fragile pairs of {int(ln.sum()) * Lq} ({100 * share:.2f} %)")
        assert share <= 0.03
    # transform() of one pair is the batch of one
    one = units["CH"].transform([il[0].tolist(), ir[0][:ln[0]].tolist()])
    assert isinstance(one, list) and np.array_equal(np.asarray(one), counts[0])


# ----------------------------------------------------------------------------- the distances against float64
PAIR_SHAPES = [(2, 5, 3, 6),            # below one tile, depth no multiple of 4
               (3, 21, 9, 10),          # two row tiles
               (2, 37, 35, 70),         # ragged tiles both ways, two depth chunks of the L1 kernels
               (2, 30, 100, 300),       # the project's shape: three MFMA depth blocks, two L1 column tiles
               (1, 19, 20, 700),        # more depth blocks than column tiles of a wave
               (1, 1024, 1024, 8)]      # the length limits
FAMS = {"l2": ("pair_l2", R.pair_l2_grads64), "l1": ("pair_l1", R.pair_l1_grads64)}


def _pair_inputs(shape, seed):
    b, l, r, d = shape
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, l, d, generator=g), torch.randn(b, r, d, generator=g), _up(g, (b, l, r))


@pytest.mark.parametrize("fam", list(FAMS))
@pytest.mark.parametrize("shape", PAIR_SHAPES)
def test_distances_against_float64(shape, fam):
    from get_amd import ops
    a, b, g = _pair_inputs(shape, 101)
    want = FAMS[fam][1](a, b, g)
    got = _run(getattr(ops.pair, FAMS[fam][0]), (a.to(DEV), b.to(DEV)), g)
    for name, u, w in zip(("out", "da", "db"), got, want):
        rel_close(u, w, TOL, f"{FAMS[fam][0]} {shape} {name}", fam=FAMS[fam][0])


@pytest.mark.parametrize("fam", list(FAMS))
@pytest.mark.parametrize("shape", [(3, 21, 9, 10), (2, 37, 35, 70)])
def test_distance_operands_are_read_in_place(shape, fam):
    """Both operands as column slices of wider tensors from a base 4 bytes past a 16-byte boundary: within TOL of float64 and
    bit-identical to the run on contiguous copies."""
    from get_amd import ops
    a, b, g = _pair_inputs(shape, 102)
    fn = getattr(ops.pair, FAMS[fam][0])
    ref = _run(fn, (a.to(DEV), b.to(DEV)), g)
    got = _run(fn, (_wide(a, 3, 1), _wide(b, 5, 2)), g)
    for name, u, v, w in zip(("out", "da", "db"), got, ref, FAMS[fam][1](a, b, g)):
        rel_close(u, w, TOL, f"{FAMS[fam][0]} {shape} sliced {name}", fam=FAMS[fam][0])
        bits_equal(u.contiguous(), v, f"{FAMS[fam][0]} {shape} {name} sliced against contiguous")


def test_l1_is_exact_on_a_dyadic_grid():
    """Inputs on the 1/16 grid in [-2, 2] and gradients of integer / 16: every sum is exact in fp32, and exact ties a == b
    occur, so the output and both gradients equal the float64 result bit for bit -- which pins sign(0) = 0."""
    from get_amd import ops
    b, l, r, d = 2, 21, 9, 70
    g = torch.Generator().manual_seed(103)
    a = torch.randint(-32, 33, (b, l, d), generator=g).float() / 16
    bb = torch.randint(-32, 33, (b, r, d), generator=g).float() / 16
    gu = _up(g, (b, l, r))
    ties = int((a.unsqueeze(2) == bb.unsqueeze(1)).sum())
    print(f"l1 exactness: {ties} exact ties")
    assert ties >= 100
    want = R.pair_l1_grads64(a, bb, gu)
    got = _run(ops.pair.pair_l1, (a.to(DEV), bb.to(DEV)), gu)
    for name, u, w in zip(("out", "da", "db"), got, want):
        assert torch.equal(w.float().double(), w), name           # the float64 result is an fp32 number
        bits_equal(u.cpu() + 0.0, w.float() + 0.0, f"pair_l1 exact {name}")      # + 0.0: -0.0 and 0.0 are the same sum


def test_l2_at_coincident_rows():
    """A few rows of a copied into b.  Away from those pairs the output holds TOL; at them it is finite, at least
    sqrt(eps) (1 - 1e-6) and at most sqrt(eps + 2 (D + 4) 2^-24 (A2 + B2)), the worst-case fp32 summation error of the
    three terms under the root (each a sum of D products, two more roundings to combine them); the gradients are finite
    everywhere and hold TOL in the rows that meet no coincident pair."""
    from get_amd import ops
    b, l, r, d = 2, 37, 35, 70
    a, bb, g = _pair_inputs((b, l, r, d), 104)
    pairs = [(0, 3, 5), (0, 20, 34), (1, 36, 0), (1, 16, 16)]
    hit = torch.zeros(b, l, r, dtype=torch.bool)
    for n, i, j in pairs:
        bb[n, j] = a[n, i]
        hit[n, i, j] = True
    want = R.pair_l2_grads64(a, bb, g)
    got = [t.cpu() for t in _run(ops.pair.pair_l2, (a.to(DEV), bb.to(DEV)), g)]
    rel_close(got[0][~hit], want[0][~hit], TOL, "pair_l2 away from the coincident pairs", fam="pair_l2")
    a2, b2 = (a.double() ** 2).sum(-1), (bb.double() ** 2).sum(-1)
    for n, i, j in pairs:
        o = float(got[0][n, i, j])
        hi = math.sqrt(EPS + 2 * (d + 4) * 2.0 ** -24 * float(a2[n, i] + b2[n, j]))
        print(f"pair_l2 coincident ({n},{i},{j}): {o:.3e} in [{math.sqrt(EPS):.3e}, {hi:.3e}]")
        assert math.isfinite(o) and math.sqrt(EPS) * (1 - 1e-6) <= o <= hi
    assert all(bool(torch.isfinite(t).all()) for t in got)
    clean_a, clean_b = ~hit.any(2), ~hit.any(1)
    rel_close(got[1][clean_a], want[1][clean_a], TOL, "pair_l2 da of the rows without a coincident pair", fam="pair_l2")
    rel_close(got[2][clean_b], want[2][clean_b], TOL, "pair_l2 db of the rows without a coincident pair", fam="pair_l2")


# ----------------------------------------------------------------------------- the windowed mean against float64
WM_SHAPES = [(2, 7, 6, 1),              # the identity window
             (2, 7, 6, 7),              # the window is the sequence
             (3, 9, 5, 2),
             (3, 21, 10, 3),
             (2, 100, 300, 5),          # four row tiles, five column blocks, the last one partial
             (2, 100, 300, 4),          # an even context window: left != right
             (1, 1024, 8, 64)]          # a long sequence, narrow columns


def _ragged_mask(b, l):
    """Lengths in [0, l]: the first sequence full, the last one (of more than one) all masked."""
    lens = [l] + [max(1, (l * (i + 1)) // (b + 1)) for i in range(1, b)]
    if b > 1:
        lens[-1] = 0
    return torch.arange(l)[None, :] < torch.tensor(lens)[:, None]


@pytest.mark.parametrize("form", ["plain", "context"])
@pytest.mark.parametrize("shape", WM_SHAPES)
def test_window_mean_against_float64(shape, form):
    from get_amd import ops
    b, l, d, w = shape
    gen = torch.Generator().manual_seed(105)
    x = torch.randn(b, l, d, generator=gen)
    left, right = (w // 2, w - w // 2 - 1) if form == "context" else (0, 0)
    lo = R.window_out_len(l, w, left, right)
    mask = _ragged_mask(b, lo) if form == "context" else None
    g = _up(gen, (b, lo, d))
    md = None if mask is None else mask.to(DEV)
    out, dx = _run(lambda t: ops.pair.window_mean(t, w, left, right, md), (x.to(DEV),), g)
    assert tuple(out.shape) == (b, lo, d)
    rel_close(out, R.window_mean64(x, w, left, right, mask), TOL, f"window_mean {shape} {form} out", fam="window_mean")
    rel_close(dx, R.window_mean_bwd64(g, l, w, left, right, mask), TOL, f"window_mean {shape} {form} dx", fam="window_mean")
    if mask is not None:
        assert bool((out.cpu()[~mask] == 0).all())                                  # masked rows are exact zeros
        only = g * (~mask).unsqueeze(2)                                             # and send exact-zero gradient
        assert b == 1 or float(only.abs().max()) > 0
        _, dx0 = _run(lambda t: ops.pair.window_mean(t, w, left, right, md), (x.to(DEV),), only)
        assert bool((dx0 == 0).all())
        if b > 1:
            assert bool((dx.cpu()[-1] == 0).all())                                  # the all-masked sequence


def test_window_mean_reads_a_column_slice_and_handles_the_empty_result():
    from get_amd import ops
    b, l, d, w = 3, 21, 10, 3
    gen = torch.Generator().manual_seed(106)
    x, g = torch.randn(b, l, d, generator=gen), _up(gen, (b, l - w + 1, d))
    ref = _run(lambda t: ops.pair.window_mean(t, w), (x.to(DEV),), g)
    got = _run(lambda t: ops.pair.window_mean(t, w), (_wide(x, 3, 1),), g)
    bits_equal(got[0], ref[0], "window_mean out from a column slice")
    bits_equal(got[1].contiguous(), ref[1], "window_mean dx from a column slice")
    gw = _wide(g, 2, 1)                                                             # the upstream gradient as a slice, too
    xd = x.to(DEV).requires_grad_(True)
    ops.pair.window_mean(xd, w).backward(gw)
    bits_equal(xd.grad, ref[1], "window_mean dx from a sliced gradient")
    xd = x.to(DEV).requires_grad_(True)
    out = ops.pair.window_mean(xd, l + 1)                                           # w > L: (B, 0, D), nothing launched
    assert tuple(out.shape) == (b, 0, d) and out.requires_grad
    out.sum().backward()
    assert bool((xd.grad == 0).all())
    assert tuple(ops.pair.window_mean(xd, 2000).shape) == (b, 0, d)                 # also beyond the kernel's window limit


# ----------------------------------------------------------------------------- hygiene, once per kernel
def _bytes_in_fence(F, name, n):
    """n int8 / int32 bytes inside a NaN-fenced fp32 allocation (the fence class fills with NaN, which integers do not hold)."""
    v = F.put(name, shape=((n + 3) // 4,))
    return v, v.view(torch.int8)[:n]


def test_fences_and_repeatability_of_the_distance_kernels():
    from get_amd import _lib
    b, l, r, d = 2, 37, 35, 70
    a, bb, g = _pair_inputs((b, l, r, d), 107)
    st = _lib.stream()
    runs = []
    for rep in range(2):
        F = _Fenced()
        ad, bd, gd = F.put("a", a, mis=True), F.put("b", bb), F.put("g", g, mis=True)
        a2, b2, out = F.put("a2", shape=(b, l)), F.put("b2", shape=(b, r)), F.put("out", shape=(b, l, r), mis=True)
        raw, sgn = _bytes_in_fence(F, "sgn", b * l * r)
        tail = raw.view(torch.int8)[b * l * r:].clone()
        da, db = F.put("da", shape=(b, l, d)), F.put("db", shape=(b, r, d), mis=True)
        _lib.call("gh_pair_l2_fwd", ad.data_ptr(), bd.data_ptr(), d, d, EPS, b, l, r, d, a2.data_ptr(), b2.data_ptr(), out.data_ptr(),
                  sgn.data_ptr(), st)
        _lib.call("gh_pair_l2_bwd", ad.data_ptr(), bd.data_ptr(), d, d, out.data_ptr(), sgn.data_ptr(), gd.data_ptr(), b, l, r, d,
                  da.data_ptr(), db.data_ptr(), st)
        o1, da1, db1 = F.put("l1 out", shape=(b, l, r)), F.put("l1 da", shape=(b, l, d), mis=True), F.put("l1 db", shape=(b, r, d))
        _lib.call("gh_pair_l1_fwd", ad.data_ptr(), bd.data_ptr(), d, d, b, l, r, d, o1.data_ptr(), st)
        _lib.call("gh_pair_l1_bwd", ad.data_ptr(), bd.data_ptr(), d, d, gd.data_ptr(), b, l, r, d, da1.data_ptr(), db1.data_ptr(), st)
        torch.cuda.synchronize()
        F.check("pair_l2 / pair_l1")
        assert torch.equal(raw.view(torch.int8)[b * l * r:], tail), "bytes behind sgn were written"
        assert bool(((sgn >= -1) & (sgn <= 1)).all())
        outs = (a2, b2, out, da, db, o1, da1, db1)
        assert all(bool(torch.isfinite(t).all()) for t in outs), "an output element was not written"
        runs.append([t.clone() for t in outs] + [sgn.clone().float()])
    for i, (u, v) in enumerate(zip(*runs)):
        bits_equal(u, v, f"distance kernels: output {i} of two calls")
    want = R.pair_l2_grads64(a, bb, g) + R.pair_l1_grads64(a, bb, g)
    for name, u, w in zip(("l2 out", "l2 da", "l2 db", "l1 out", "l1 da", "l1 db"), runs[0][2:8], want):
        rel_close(u, w, TOL, f"direct call {name}")


def test_fences_and_repeatability_of_window_mean():
    from get_amd import _lib
    b, l, d, w, left, right = 3, 21, 10, 4, 2, 1
    lo = l + left + right - w + 1
    gen = torch.Generator().manual_seed(108)
    x, g, mask = torch.randn(b, l, d, generator=gen), _up(gen, (b, lo, d)), _ragged_mask(b, lo).float()
    st = _lib.stream()
    runs = []
    for rep in range(2):
        F = _Fenced()
        xd, gd, md = F.put("x", x, mis=True), F.put("g", g), F.put("mask", mask, mis=True)
        out, dx = F.put("out", shape=(b, lo, d), mis=True), F.put("dx", shape=(b, l, d))
        _lib.call("gh_window_mean_fwd", xd.data_ptr(), d, md.data_ptr(), b, l, d, w, left, right, out.data_ptr(), st)
        _lib.call("gh_window_mean_bwd", gd.data_ptr(), d, md.data_ptr(), b, l, d, w, left, right, dx.data_ptr(), st)
        torch.cuda.synchronize()
        F.check("window_mean")
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dx).all())
        runs.append((out.clone(), dx.clone()))
    bits_equal(runs[0][0], runs[1][0], "window_mean out of two calls")
    bits_equal(runs[0][1], runs[1][1], "window_mean dx of two calls")
    rel_close(runs[0][0], R.window_mean64(x, w, left, right, mask), TOL, "direct call window_mean out")
    rel_close(runs[0][1], R.window_mean_bwd64(g, l, w, left, right, mask), TOL, "direct call window_mean dx")


def test_fences_and_repeatability_of_match_hist():
    from get_amd import _lib
    V, D, bn, lq, ld, bins = 40, 10, 3, 7, 33, 30
    gen = torch.Generator().manual_seed(109)
    table = torch.randn(V, D, generator=gen)
    inv = 1.0 / table.norm(dim=1)
    il = torch.randint(0, V // 2, (bn, lq), generator=gen).int().to(DEV)
    ir = torch.randint(V // 2, V, (bn, ld), generator=gen).int().to(DEV)
    ir[:, 20:] = 10 ** 6                     # ids at or beyond every length are never read through
    ln = torch.tensor([20, 0, 7], dtype=torch.int32, device=DEV)
    st = _lib.stream()
    runs = []
    for rep in range(2):
        F = _Fenced()
        td, nd = F.put("table", table, mis=True), F.put("inv_norm", inv)
        out = F.put("out", shape=(bn, lq, bins), mis=True)
        raw, flag8 = _bytes_in_fence(F, "flag", 4)
        _lib.call("gh_match_hist", td.data_ptr(), D, nd.data_ptr(), V, D, il.data_ptr(), ir.data_ptr(), ln.data_ptr(), bn, lq, ld, bins, 0,
                  out.data_ptr(), flag8.data_ptr(), st)
        torch.cuda.synchronize()
        F.check("match_hist")
        assert bool(torch.isfinite(out).all()) and int(raw.view(torch.int32)[0]) == 0
        runs.append(out.clone())
    bits_equal(runs[0], runs[1], "match_hist of two calls")
    counts = runs[0].cpu().double().numpy()
    assert np.array_equal(counts.sum(2), np.repeat(ln.cpu().numpy()[:, None] + bins, lq, axis=1))
    t64 = R.normalize_table64(table.double().numpy())
    for i, n in enumerate(ln.tolist()):
        # the inv_norm form rounds more often than the dot product alone: two fp32 inverse norms of a few roundings each and
        # the two products with them, on top of the D + 2 of the margin
        lower, upper, _ = _count_bounds(R.hist_scaled64(t64, il[i].cpu().numpy(), ir[i, :n].cpu().numpy(), bins), bins, D + 8)
        assert (lower <= counts[i]).all() and (counts[i] <= upper).all()


@pytest.mark.parametrize("shape,match", [((1, 1025, 3, 4), "l=1025"), ((1, 3, 1025, 4), "r=1025"), ((1, 3, 3, 2049), "d=2049")])
def test_distance_limits_raise_instead_of_launching(shape, match):
    from get_amd import ops
    b, l, r, d = shape
    a, bb = torch.zeros(b, l, d, device=DEV), torch.zeros(b, r, d, device=DEV)
    for fn in (ops.pair.pair_l2, ops.pair.pair_l1):
        with pytest.raises(RuntimeError, match=match):
            fn(a, bb)


def test_window_and_histogram_limits_raise_instead_of_launching():
    from get_amd import _lib, ops, pairwise
    x = torch.zeros(1, 2000, 4, device=DEV)
    out = torch.full((1, 976, 4), 5.0, device=DEV)
    with pytest.raises(RuntimeError, match="window=1025"):
        _lib.call("gh_window_mean_fwd", x.data_ptr(), 4, None, 1, 2000, 4, 1025, 0, 0, out.data_ptr(), _lib.stream())
    with pytest.raises(RuntimeError, match="d=2049"):
        ops.pair.window_mean(torch.zeros(1, 4, 2049, device=DEV), 2)
    with pytest.raises(RuntimeError, match="longer than the padded sequence"):
        _lib.call("gh_window_mean_fwd", x.data_ptr(), 4, None, 1, 3, 4, 5, 0, 0, out.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    table = torch.randn(8, 4, device=DEV)
    ids = torch.zeros(2, 3, dtype=torch.int64, device=DEV)
    ln = torch.full((2,), 3, dtype=torch.int64, device=DEV)
    with pytest.raises(RuntimeError, match="bins=257"):
        ops.pair.match_hist(table, None, ids, ids, ln, 257, "CH")
    with pytest.raises(RuntimeError, match="lq=1025|l=1025"):
        ops.pair.match_hist(table, None, torch.zeros(2, 1025, dtype=torch.int64, device=DEV), ids, ln, 30, "CH")
    for bad_left, bad_right in (((0, 1, 8), None), ((0, -1, 2), None), (None, (1, 2, 8)), (None, (-3, 0, 0))):
        left, right = ids.clone(), ids.clone()
        if bad_left is not None:
            left[1] = torch.tensor(bad_left)
        else:
            right[0] = torch.tensor(bad_right)
        with pytest.raises(RuntimeError, match="outside the table"):
            ops.pair.match_hist(table, None, left, right, ln, 30, "CH")
    right = ids.clone()
    right[:, 2] = 99                           # beyond the length: ignored, not an error
    got = ops.pair.match_hist(table, None, ids, right, torch.full((2,), 2, dtype=torch.int64, device=DEV), 30, "CH")
    assert float(got.sum()) == 2 * 3 * (30 + 2)
    unit = pairwise.MatchingHistogram(30, table.cpu().numpy(), True, "CH")
    assert np.asarray(unit.transform([[1, 2], []])).tolist() == np.ones((2, 30)).tolist()      # no right text: every bin keeps its 1
    print("WORST", {k: f"{v:.3e}" for k, v in WORST.items()})

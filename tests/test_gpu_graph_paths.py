"""Every dispatch path of the graph kernels (csrc/spmm_ops.hip: gh_spmm / gh_spmm_bf16 with the edge-list, matrix-pipe
and scalar aggregation kernels; gsl_ops.hip: gh_gsl_topk, gh_scorer_gsl; graph_build_ops.hip: gh_graph_build, gh_adj_pack_* /
gh_adj_unpack, gh_ref_depad; ragged_ops.hip: gh_ragged_plan; and gh_get_prepare of csrc/model_ops.hip) against plain numpy /
float64 references on the CPU.

The C-ABI entries are called directly.  Every output sits inside a larger allocation of its own, filled with NaN (floating
point) or a sentinel (integers), at least 256 bytes of it on either side; what an entry documents as not written must
still hold the fill afterwards.  The references never come from a kernel under test: dense adjacencies are built from
oracle.get_oracle.convert_text or from the numpy array that is handed over and packed to bit words in numpy, keep-sets are
numpy rankings (descending score, ties to the lower index), products are float64 (for bf16: of the same bf16 values).
tests/util.py holds these restatements; tests/test_graph_restatements_cpu.py checks them against the reference's goldens.

Bounds: integer and bit outputs exact; fp32 aggregation and scorer scores 1e-4 of the float64 result's largest entry on
every written element (tests.util._rel); bf16 aggregation |err| <= 2^-8 |ref| + 4e-6 (|A| |x| + |y0|) per element.

No path counter exists for these kernels: the path named in a case's label follows from its shape by reading spmm_plan
(csrc/spmm_plan.h, the arithmetic of launch_spmm) and launch_ragged_plan.  The evidence that a label is right is a mutation check on a scratch copy of the library (one
change per path, the cases with that label fail), listed in DESIGN.md 4.8."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import get_oracle as O
from tests.util import (TOL, WORST, _rel, g_dense_pattern, g_depad, g_dinv, g_pack_bits, g_plan, g_refined64, g_scorer64,
                        g_text_graphs, g_topk, g_words)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
NAN = float("nan")
FENCE = 256                      # bytes of fill on either side of every output, at the least
SENT = {torch.int32: -1515870811, torch.int64: -6510615555426900571}      # 0xA5A5... as a signed value
CASES = [0]


def _lib():
    from get_amd import _lib
    return _lib


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ----------------------------------------------------------------------------- fenced buffers
class _Fenced:
    """Tensors inside allocations of their own that are filled with NaN / a sentinel; check() asserts that the fences on
    either side still hold the fill.  fresh(v): the elements of v that still hold the fill."""

    def __init__(self):
        self.items = []

    def put(self, name, src=None, shape=None, dtype=torch.float32, mis=False):
        if src is not None and not torch.is_tensor(src):
            src = torch.from_numpy(np.ascontiguousarray(src))
        shape = tuple(src.shape if shape is None else shape)
        n = int(np.prod(shape, dtype=np.int64))
        es = torch.empty((), dtype=dtype).element_size()
        pad = FENCE // es
        fill = NAN if dtype.is_floating_point else SENT[dtype]
        buf = torch.full((n + 2 * pad + 16,), fill, device=DEV, dtype=dtype)
        off = pad
        while (buf.data_ptr() + off * es) % 16 != (4 if mis else 0):
            off += 1
        v = buf[off:off + n].view(shape)
        if src is not None:
            v.copy_(src.to(dtype))
        assert v.is_contiguous() and v.data_ptr() % 16 == (4 if mis else 0)
        self.items.append((name, buf, off, n, fill))
        return v

    @staticmethod
    def fresh(v):
        return torch.isnan(v) if v.dtype.is_floating_point else v == SENT[v.dtype]

    def check(self, what):
        for name, buf, off, n, fill in self.items:
            for part in (buf[:off], buf[off + n:]):
                ok = torch.isnan(part).all() if buf.dtype.is_floating_point else (part == fill).all()
                assert bool(ok), f"{what}: the fence around {name} was written"


def _untouched(v, what):
    assert bool(_Fenced.fresh(v).all()), f"{what}: written, but documented as left alone"


def _exact(got, want, what):
    got = got.detach().cpu().numpy()
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype.kind == "f":                    # bit for bit
        got, want = got.view(np.int32), np.ascontiguousarray(want.astype(np.float32)).view(np.int32)
    bad = np.argwhere(got != want.astype(got.dtype))
    assert bad.size == 0, f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}: " \
                          f"{got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


# ----------------------------------------------------------------------------- graph fixtures (host side)
def _batch(pattern, nn, dinv=None, vals=None):
    n, r = pattern.shape[:2]
    nn = np.asarray(nn, np.int32)
    for g in range(n):                           # a node beyond the graph's count has no edge (node-compact layout)
        assert not pattern[g, nn[g]:, :].any() and not pattern[g, :, nn[g]:].any()
    return SimpleNamespace(n=n, r=r, pattern=pattern, nn=nn, dinv=dinv, vals=vals, plan=g_plan(nn, r), dev={})


@functools.lru_cache(maxsize=None)
def _texts(n, r, window, seed, kinds=True):
    """Random texts with repeated tokens and one frequent token; with `kinds` text 0 is empty, text 1 all distinct (a full
    graph: as many nodes as rows), text 2 one token repeated, the others of random length."""
    rng = np.random.default_rng(seed)
    toks = rng.integers(2, max(4, 3 * r), size=(n, r)).astype(np.int32)
    toks[:, ::5] = 1 + (np.arange(n)[:, None] % 3 == 0)
    lens = rng.integers(max(1, r // 3), r + 1, size=(n,)).astype(np.int32)
    if kinds:
        lens[0] = 0
        if n > 1:
            toks[1], lens[1] = np.arange(r) + 7, r
        if n > 2:
            toks[2], lens[2] = 5, r
    return toks, lens


@functools.lru_cache(maxsize=None)
def _word_batch(n, r, window=3, seed=0):
    """Normalised word graphs from convert_text: an empty graph, a full one and short ones in the same batch."""
    toks, lens = _texts(n, r, window, 1000 * r + seed)
    _, nn, pattern, dinv, _ = g_text_graphs(toks, lens, r, window, O.convert_text)
    return _batch(pattern, nn, dinv=dinv)


@functools.lru_cache(maxsize=None)
def _many(n):
    """The first n of 520 word graphs at r = 64 (the launch-mode switches depend on n alone)."""
    if n == 520:
        return _word_batch(520, 64, 3, 7)
    b = _many(520)
    lo = 3 if n == 1 else 0                      # (graph 0 is the empty one: a single graph should have rows)
    return _batch(b.pattern[lo:lo + n], b.nn[lo:lo + n], dinv=b.dinv[lo:lo + n])


@functools.lru_cache(maxsize=None)
def _dense_batch(n, r, seed=0, density=None, counts=None):
    """Weighted hand-over with an ASYMMETRIC pattern (values, not d^-1/2 products) on the first nn[g] nodes of every
    graph; graph 0 full, the last one empty when there are three or more.  density None: about 3 entries per row, so
    that the united pattern (about 7 per row with the heavy row below) stays on the edge list; 0.3: beyond its capacity."""
    rng = np.random.default_rng(5000 + 10 * r + seed)
    if counts is None:
        nn = rng.integers(max(1, r // 3), r + 1, size=(n,))
        nn[0] = r
        if n > 2:
            nn[n - 1] = 0
    else:
        nn = np.asarray(counts)
    a = np.zeros((n, r, r), np.float32)
    for g in range(n):
        k = int(nn[g])
        blk = rng.standard_normal((k, k)) * (rng.random((k, k)) < (min(1.0, 3.0 / max(k, 1)) if density is None else density))
        blk[np.arange(k), np.arange(k)] = 1.0
        if k > 2:
            blk[:, k - 1] = 0.0                   # a column present only through the transposed side ...
            blk[k - 1, : k // 2] = 0.5           # ... of a heavy row
        a[g, :k, :k] = blk
    return _batch(g_dense_pattern(a), nn, vals=a)


def _sym(r, pairs, diag):
    p = np.zeros((r, r), bool)
    for i, j in pairs:
        p[i, j] = p[j, i] = True
    for i in diag:
        p[i, i] = True
    return p


@functools.lru_cache(maxsize=None)
def _cap_batch(r, weighted, which):
    """Edge counts placed entry by entry.  which = "at": exactly 10 r, the list's capacity, next to a sparse graph (both
    listed); "past": 10 r + 1 alone (the bit walk inside the list kernel); "both": all three in one launch."""
    rng = np.random.default_rng(77 + r)
    iu = np.argwhere(np.triu(np.ones((r, r), bool), 1))
    pick = iu[rng.permutation(len(iu))[:5 * r]]
    pats = [_sym(r, pick, []), _sym(r, pick, [r // 2]), _sym(r, pick[:r], range(0, r, 3))]
    assert [int(p.sum()) for p in pats[:2]] == [10 * r, 10 * r + 1]
    pattern = np.stack({"at": [pats[0], pats[2]], "past": [pats[1]], "both": pats}[which])
    nn = [r] * len(pattern)
    if weighted:
        vals = (rng.standard_normal(pattern.shape) * pattern).astype(np.float32)
        vals[vals == 0] += pattern[vals == 0] * 0.25
        return _batch(g_dense_pattern(vals), nn, vals=vals)
    return _batch(pattern, nn, dinv=g_dinv(pattern))


def _split_plan(pattern_g, nn, r, bf16=False):
    """What the edge-list kernel's scheduling comes to for one graph without a keep-set: (hub rows split, mid rows split)."""
    deg = pattern_g[:nn].sum(-1)
    grp = -(-deg // 8)
    hub, mid = deg > 32, (deg > 16) & (deg <= 32)
    spare = (r - nn) // 2 if bf16 else r - nn
    nnz_ok = int(deg.sum()) <= 10 * r
    h, m = int(grp[hub].sum()), int(grp[mid].sum())
    return (nnz_ok and 0 < h <= spare, nnz_ok and m > 0 and h + m <= spare)


@functools.lru_cache(maxsize=None)
def _hub_batch(r=128):
    """One pattern -- a hub row of 40 edges (5 groups of 8), two mid rows of 22 (3 groups each), a ring -- in graphs whose
    spare rows r - nn fit: hubs and mids (nn = 100), hubs alone (nn = r - 6), neither (nn = r - 3); plus an empty graph, and
    a hub-free full graph (nn = r)."""
    def graph(nn, hubs=True):
        pairs = [(i, (i + 1) % nn) for i in range(nn)]
        if hubs:
            pairs += [(0, j) for j in range(2, 40)] + [(1, j) for j in range(40, 59)] + [(60, j) for j in range(62, 81)]
        return _sym(r, pairs, range(nn))
    nn = [100, r - 6, r - 3, 0, r, 100]
    pattern = np.stack([graph(100), graph(r - 6), graph(r - 3), np.zeros((r, r), bool), graph(r, False), graph(100)])
    want = [(True, True), (True, False), (False, False), (False, False), (False, False), (True, True)]
    assert [_split_plan(pattern[g], nn[g], r) for g in range(6)] == want
    return _batch(pattern, nn, dinv=g_dinv(pattern))


def _upload(G):
    if not G.dev:
        G.dev = dict(bits=T(g_pack_bits(G.pattern)), dinv=None if G.dinv is None else T(G.dinv),
                     vals=None if G.vals is None else T(G.vals), goff=T(G.plan["goff"]))
    return SimpleNamespace(**G.dev)


@functools.lru_cache(maxsize=None)
def _keep_for(n, r, k, seed=3):
    rng = np.random.default_rng(seed + 31 * r + n)
    keep = g_topk(rng.standard_normal((n, r)), k)
    if n > 1:
        keep[1] = False                           # a graph that keeps nothing
    return keep


# ----------------------------------------------------------------------------- aggregation
def _spmm_run(G, h, compact, keep, tr, acc, mis, bf16, what):
    """One launch (twice, into separately fenced outputs: bit-identical).  Returns (y as written, float64 reference,
    float64 scale |A| |x| + |y0|), rows = the layout's."""
    lib = _lib()
    D = _upload(G)
    n, r = G.n, G.r
    gen = torch.Generator().manual_seed(97 * n + 7 * r + h)
    dt = torch.bfloat16 if bf16 else torch.float32
    xp = torch.randn(n * r, h, generator=gen).to(dt)            # padded-layout values; the compact rows are gathered from them
    y0p = torch.randn(n * r, h, generator=gen).to(dt)
    m_real = int(G.plan["goff"][n])
    rows = torch.from_numpy(G.plan["src"][:m_real].astype(np.int64)) if compact else torch.arange(n * r)
    live = torch.zeros(n * r, dtype=torch.bool)
    live[torch.from_numpy(G.plan["src"][:m_real].astype(np.int64))] = True
    # float64 reference on the padded layout (absent nodes have no edge: their x never counts), then the layout's rows
    A = torch.from_numpy(g_refined64(G.pattern, keep, G.dinv, G.vals, bool(tr)))
    x64 = (xp.double() * live[:, None]).view(n, r, h)
    ref = (A @ x64).view(n * r, h)
    scale = (A.abs() @ x64.abs()).view(n * r, h)
    if acc:
        ref, scale = ref + y0p.double(), scale + y0p.double().abs()
    keep_d = None if keep is None else T(g_pack_bits(keep))
    outs = []
    for _ in range(2):
        f = _Fenced()
        x = f.put("x", xp[rows], dtype=dt, mis=mis == "x")
        y = f.put("y", y0p[rows] if acc else None, shape=(len(rows), h), dtype=dt, mis=mis == "y")
        lib.call("gh_spmm_bf16" if bf16 else "gh_spmm", lib.ptr(D.bits), lib.ptr(D.dinv), lib.ptr(D.vals), lib.ptr(keep_d),
                 lib.ptr(D.goff) if compact else None, m_real if compact else 0, lib.ptr(x), lib.ptr(y), n, r, h, tr, acc,
                 lib.stream())
        torch.cuda.synchronize()
        f.check(what)
        outs.append(y)
    assert torch.equal(outs[0].view(torch.int16 if bf16 else torch.int32), outs[1].view(torch.int16 if bf16 else torch.int32)), \
        f"{what}: two calls differ"
    return outs[0], ref[rows], scale[rows]


def _spmm_case(G, h, label, compact=False, keep_k=None, tr=0, acc=0, mis=None, bf16=False):
    """label: the kernel the launch takes (list | list-walk | scalar | mfma | list16), which names the error family."""
    CASES[0] += 1
    keep = None if keep_k is None else _keep_for(G.n, G.r, keep_k)
    mode = "weighted" if G.vals is not None else "normalised"
    what = (f"spmm{'_bf16' if bf16 else ''} {label} n={G.n} r={G.r} h={h} {mode} {'compact' if compact else 'padded'}"
            f"{'' if keep is None else f' keep {keep_k}'}{' A^T' if tr else ''}{' +=' if acc else ''}{f' {mis} misaligned' if mis else ''}")
    y, ref, scale = _spmm_run(G, h, compact, keep, tr, acc, mis, bf16, what)
    if not bf16:
        if ref.numel():
            _rel(y, ref, what, f"spmm {label}")
        return y
    got = y.double().cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements not written / not finite"
    err, tol = (got - ref).abs(), ref.abs() * 2.0 ** -8 + scale * 4e-6 + 1e-30
    ratio = float((err / tol).max()) if ref.numel() else 0.0
    fam = f"spmm_bf16 {label}"
    WORST[fam] = max(WORST.get(fam, 0.0), ratio)
    print(f"{what}: worst err / bound {ratio:.3f} (worst {fam}: {WORST[fam]:.3f})")
    assert bool((err <= tol).all()), f"{what}: {int((err > tol).sum())} elements beyond the bound, worst {ratio:.3f} x"
    return y


# keep / transpose / accumulate, together and apart
COMBOS = [dict(), dict(keep_k=5), dict(tr=1), dict(acc=1), dict(keep_k=5, tr=1, acc=1)]


def _kk(G, kw):
    """keep_k of a combination scaled to the graph size: about r / 3 nodes kept (at least one where there are two)."""
    kw = dict(kw)
    if "keep_k" in kw:
        kw["keep_k"] = max(1, G.r // 3) if G.r > 1 else 0
    return kw


@pytest.mark.parametrize("r", [1, 2, 63, 64, 65, 128, 129, 192, 193, 255, 256])
def test_spmm_list_every_row_count(r):
    """Edge-list kernel, one to four bit words per row, st[R] at R = 256, trow = min(tid, R - 1); h = 44 is 11 float4
    columns: an odd count over two columns per thread."""
    for G in (_word_batch(9, r), _dense_batch(9, r)):
        for kw in COMBOS:
            for compact in (False, True):
                _spmm_case(G, 44, "list", compact=compact, **_kk(G, kw))


@pytest.mark.parametrize("h,why", [(4, "one column: TPR = 1, no magic"), (8, "two columns: TPR = 1"), (12, "three columns"),
                                   (280, "slabs of 24, 24, 22 columns"), (300, "three even slabs"),
                                   (768, "whole-line slabs of 32 columns")])
def test_spmm_list_every_width(h, why):
    for G in (_word_batch(9, 65), _dense_batch(9, 65)):
        for kw in (dict(), dict(keep_k=5, tr=1, acc=1)):
            for compact in (False, True):
                _spmm_case(G, h, "list", compact=compact, **_kk(G, kw))
    if h in (4, 768):
        _spmm_case(_word_batch(9, 256), h, "list", compact=True, keep_k=80, acc=1)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 13, 255, 256, 257])
def test_spmm_list_every_graph_count(n):
    """The 1-D grid's decode (8 XCD queues, n not a multiple of 8) and the slabs-per-workgroup switch at n = 256: one
    slab per workgroup below it, all three of r = 64, h = 300 from it on."""
    G = _many(n)
    _spmm_case(G, 300, "list", compact=False)
    _spmm_case(G, 300, "list", compact=True, keep_k=20, acc=1)


def test_spmm_list_520_compact_graphs_on_24k_slabs():
    """Node-compact, n >= 512, r <= 128: the 24 KB slab cap -- four slabs of 19, 19, 19, 18 columns at r = 64, h = 300
    instead of three of 25 -- walked by one workgroup per graph."""
    G = _many(520)
    _spmm_case(G, 300, "list", compact=True)
    _spmm_case(G, 300, "list", compact=True, keep_k=20, tr=1, acc=1)
    _spmm_case(G, 300, "list", compact=False)                     # the same count on 32 KB slabs


@pytest.mark.parametrize("which,label", [("at", "list"), ("past", "list-walk"), ("both", "list-walk")])
@pytest.mark.parametrize("weighted", [False, True])
def test_spmm_list_capacity_switch(weighted, which, label):
    """nnz == cap stays on the list, nnz == cap + 1 walks the bit rows inside the same kernel.  (Mutation check: a wrong
    walk fails "past" and "both" and passes "at"; a wrong list fails "at" and "both" and passes "past".)"""
    for r in (64, 129):
        G = _cap_batch(r, weighted, which)
        for kw in (dict(), dict(tr=1, acc=1)):
            _spmm_case(G, 44, label, **kw)
        _spmm_case(G, 300, label, acc=1)
        if which == "both":
            _spmm_case(G, 44, "list", keep_k=r // 2)            # refined below the capacity: every graph listed


def test_spmm_list_walk_on_dense_hand_overs():
    G = _dense_batch(9, 65, density=0.3)          # every graph of more than 46 nodes beyond the capacity
    assert (G.pattern.sum((1, 2)) > 650).sum() >= 3
    for kw in (dict(), dict(tr=1, acc=1)):
        for compact in (False, True):
            _spmm_case(G, 300, "list-walk", compact=compact, **kw)


@pytest.mark.parametrize("h", [44, 300])
def test_spmm_list_row_splitting_never_changes_a_bit(h):
    """Hub and mid rows handed to work items of their own as far as the spare rows reach (hubs and mids / hubs alone /
    neither, an empty and a full graph in the same launch): the node-compact result, where rows split, equals the padded
    one, where none can, bit for bit -- and both meet the float64 bound."""
    G = _hub_batch()
    m_real = int(G.plan["goff"][G.n])
    rows = torch.from_numpy(G.plan["src"][:m_real].astype(np.int64)).to(DEV)
    for kw in (dict(), dict(acc=1), dict(keep_k=50, acc=1)):
        yp = _spmm_case(G, h, "list", compact=False, **kw)
        yc = _spmm_case(G, h, "list", compact=True, **kw)
        assert torch.equal(yp[rows].view(torch.int32), yc.view(torch.int32)), f"h={h} {kw}: compact and padded results differ"


def test_spmm_compact_equals_padded_bit_for_bit_on_word_graphs():
    for G, h in ((_word_batch(9, 128, 5), 300), (_word_batch(9, 256, 5), 44), (_many(257), 300), (_dense_batch(9, 129), 44)):
        m_real = int(G.plan["goff"][G.n])
        rows = torch.from_numpy(G.plan["src"][:m_real].astype(np.int64)).to(DEV)
        for kw in (dict(), dict(keep_k=G.r // 3, tr=1)):
            yp = _spmm_case(G, h, "list", compact=False, **kw)
            yc = _spmm_case(G, h, "list", compact=True, **kw)
            assert torch.equal(yp[rows].view(torch.int32), yc.view(torch.int32)), f"r={G.r} h={h} {kw}: compact != padded"


@pytest.mark.parametrize("h", [1, 3, 30, 130, 301])
def test_spmm_scalar_every_width(h):
    """spmm_kernel<1>: h % 4 != 0.  130 and 301 take two and three slabs at r = 65."""
    for G in (_word_batch(9, 65), _dense_batch(9, 65)):
        for kw in COMBOS:
            for compact in (False, True):
                _spmm_case(G, h, "scalar", compact=compact, **_kk(G, kw))


@pytest.mark.parametrize("mis", ["x", "y"])
def test_spmm_scalar_through_one_misaligned_operand(mis):
    """h % 4 == 0, but x alone / y alone sits one float past a 16-byte boundary."""
    for G in (_word_batch(9, 65), _dense_batch(9, 65)):
        for kw in (dict(), dict(keep_k=20, tr=1, acc=1)):
            for compact in (False, True):
                _spmm_case(G, 12, "scalar", compact=compact, mis=mis, **kw)
    _spmm_case(_word_batch(9, 256), 300, "scalar", compact=True, mis=mis, keep_k=80, acc=1)


def test_spmm_scalar_at_256_rows_over_several_slabs():
    for G in (_word_batch(9, 256), _dense_batch(9, 256)):
        for kw in (dict(), dict(keep_k=80, tr=1, acc=1)):
            for compact in (False, True):
                _spmm_case(G, 130, "scalar", compact=compact, **kw)


# ---- bf16
@pytest.mark.parametrize("r", [1, 16, 17, 31, 32, 33, 64, 65, 96, 127, 128])
def test_spmm_bf16_mfma_every_row_count(r):
    """Matrix-pipe kernel: row tiles of 16, k-steps of 32, one and two bit words; h = 136: a full slab and one of 8 columns."""
    for G in (_word_batch(13, r), _dense_batch(13, r)):
        for kw in COMBOS:
            for compact in (False, True):
                _spmm_case(G, 136, "mfma", compact=compact, bf16=True, **_kk(G, kw))


@pytest.mark.parametrize("h", [8, 128, 136, 392, 768])
@pytest.mark.parametrize("n", [1, 13, 256, 257])
def test_spmm_bf16_mfma_every_width_and_graph_count(n, h):
    """One slab, a partial last slab, four slabs and six: from n = 256 on a workgroup walks three slabs (4 = 3 + 1, 6 = 3 + 3)."""
    for G in (_word_batch(n, 33), _dense_batch(n, 33)):
        _spmm_case(G, h, "mfma", compact=False, bf16=True)
        _spmm_case(G, h, "mfma", compact=True, bf16=True, keep_k=11, tr=1, acc=1)


def test_spmm_bf16_mfma_node_counts_at_and_past_tile_edges():
    counts = (16, 17, 32, 33, 48, 49, 64, 65, 96, 97, 112, 113, 128, 0, 1)
    G = _dense_batch(len(counts), 128, counts=counts)
    Gn = _batch(G.pattern, G.nn, dinv=g_dinv(G.pattern))
    for B in (G, Gn):
        for kw in (dict(), dict(keep_k=40), dict(keep_k=40, tr=1, acc=1)):
            _spmm_case(B, 136, "mfma", compact=True, bf16=True, **kw)


@pytest.mark.parametrize("r", [129, 200, 256])
@pytest.mark.parametrize("h", [8, 264, 768])
def test_spmm_bf16_list_large_graphs(r, h):
    """r > 128: the edge-list kernel on a bf16 slab image, three columns per thread."""
    for G in (_word_batch(9, r), _dense_batch(9, r)):
        for kw in (dict(), dict(keep_k=r // 3), dict(tr=1, acc=1)):
            for compact in (False, True):
                _spmm_case(G, h, "list16", compact=compact, bf16=True, **kw)


def test_spmm_bf16_list_row_splitting():
    """Hub rows split over the (R - NR) / 2 spare bf16 rows at r = 200."""
    r = 200
    def graph(nn):
        pairs = [(i, (i + 1) % nn) for i in range(nn)] + [(0, j) for j in range(2, 40)] + [(1, j) for j in range(40, 59)]
        return _sym(r, pairs, range(nn))
    nn = [150, r - 12, r - 6]
    pattern = np.stack([graph(k) for k in nn])
    assert [_split_plan(pattern[g], nn[g], r, True) for g in range(3)] == [(True, True), (True, False), (False, False)]
    G = _batch(pattern, nn, dinv=g_dinv(pattern))
    for kw in (dict(), dict(acc=1)):
        _spmm_case(G, 264, "list16", compact=True, bf16=True, **kw)


# ----------------------------------------------------------------------------- GSL: top-k alone
def _score_fixture(r):
    """Rows of r scores: random, all equal, equal values straddling every word boundary, +-0.0 mixed, +-inf at either end."""
    rng = np.random.default_rng(900 + r)
    rows = [rng.standard_normal(r), np.full(r, 0.25), rng.standard_normal(r), np.where(np.arange(r) % 2 == 0, 0.0, -0.0),
            rng.standard_normal(r), rng.standard_normal(r)]
    for b in range(63, r, 64):                    # the best value four times around bit 63 / 64 of every word boundary
        rows[2][max(b - 1, 0):b + 3] = 9.0
    rows[3][r // 2:] = np.where(np.arange(r - r // 2) % 3 == 0, -0.0, 0.0)
    rows[4][0], rows[4][r - 1] = -np.inf, np.inf
    rows[5][::3] = np.inf
    rows[5][1::3] = -np.inf
    return np.stack(rows).astype(np.float32)


@pytest.mark.parametrize("r", [1, 63, 64, 65, 128, 129, 256])
def test_gsl_topk_keep_words_exact(r):
    lib = _lib()
    s = _score_fixture(r)
    n, W = s.shape[0], g_words(r)
    sd = T(s)
    for k in sorted({0, 1, max(r - 1, 0), r, r + 5, 2, min(r, 65)}):
        CASES[0] += 1
        what = f"gsl_topk r={r} k={k}"
        f = _Fenced()
        keep = f.put("keep", shape=(n, W), dtype=torch.int64)
        lib.call("gh_gsl_topk", lib.ptr(sd), n, r, k, lib.ptr(keep), lib.stream())
        torch.cuda.synchronize()
        f.check(what)
        _exact(keep, g_pack_bits(g_topk(s, k)), what)          # (g_pack_bits leaves bits >= r zero: so must the kernel)


# ----------------------------------------------------------------------------- GSL: scorer + top-k
def _pick_k(s64, bound, want_tie=False):
    """A k (nearest to r / 2) at which every graph's float64 scores have a gap of more than 2 * bound on both sides of the
    k-th place among distinct values (and, want_tie, the k-th place of some graph falls inside a run of equal scores).
    Decided from the reference alone."""
    n, r = s64.shape

    def ok(k):
        tie = False
        for row in s64:
            v = np.sort(row)[::-1]
            a, b = v[k - 1], v[k]
            if a != b:
                if not a - b > 2 * bound:
                    return False
            else:
                tie = True
                above, below = v[v > a], v[v < a]
                if (above.size and not above.min() - a > 2 * bound) or (below.size and not a - below.max() > 2 * bound):
                    return False
        return tie or not want_tie
    for k in sorted(range(1, r), key=lambda k: (abs(k - r // 2), k)):
        if ok(k):
            return k
    assert r == 1 or not want_tie, "no k with the required gap"
    assert r == 1, "no k with the required gap"
    return 1


def _scorer_fixture(G, h, compact, collapsed, drop_p, use_score_x, seed=0):
    """Host side of a scorer case: inputs in the layout's row order, the float64 scores and the k they allow."""
    from get_amd import ops
    n, r = G.n, G.r
    rng = np.random.default_rng(321 + 7 * r + h + seed)
    m_real = int(G.plan["goff"][n])
    # feature rows of the layout; frow[g][j] = the row node j of graph g reads
    if compact and collapsed:
        rows_tot = m_real + 1
        frow = np.full((n, r), m_real, np.int64)
        for g in range(n):
            frow[g, :G.nn[g]] = G.plan["goff"][g] + np.arange(G.nn[g])
    elif compact:
        rows_tot = n * r
        frow = np.empty(n * r, np.int64)
        frow[G.plan["src"]] = np.arange(n * r)
        frow = frow.reshape(n, r)
    else:
        rows_tot = n * r
        frow = np.arange(n * r).reshape(n, r)
    feat = (rng.standard_normal((rows_tot, h)) * 0.5).astype(np.float32)
    w_p = (rng.standard_normal(h) / np.sqrt(h)).astype(np.float32)
    gate = rng.uniform(-1.2, 1.2, size=12).astype(np.float32)
    drop_seed = 12345 + r
    f64 = feat.astype(np.float64)
    if drop_p > 0:
        mask = ops.dropout_mask_reference(drop_seed, rows_tot, h, drop_p)
        f64 = f64 * mask * float(np.float32(1.0 / (1.0 - drop_p)))
    xrows = f64 @ w_p.astype(np.float64)                            # (rows_tot,)
    if use_score_x:
        xrows = xrows.astype(np.float32).astype(np.float64)         # projected on the host, rounded to fp32, handed over
    A = g_refined64(G.pattern, None, G.dinv, G.vals)
    s64 = g_scorer64(A, xrows[frow], gate)
    scale = np.abs(s64).max() + 1e-12
    k = _pick_k(s64, TOL * scale, want_tie=collapsed)
    return SimpleNamespace(feat=feat, w_p=w_p, gate=gate, drop_seed=drop_seed, xrows=xrows, s64=s64, k=k)


def _scorer_case(G, h, label, compact=False, collapsed=False, drop_p=0.0, mis=None, use_score_x=False, seed=0):
    """label: float4 | scalar | score_x -- the projection path."""
    CASES[0] += 1
    lib = _lib()
    D = _upload(G)
    n, r, W = G.n, G.r, g_words(G.r)
    fx = _scorer_fixture(G, h, compact, collapsed, drop_p, use_score_x, seed)
    feat, w_p, gate, drop_seed, xrows, s64, k = fx.feat, fx.w_p, fx.gate, fx.drop_seed, fx.xrows, fx.s64, fx.k
    mode = "weighted" if G.vals is not None else "normalised"
    what = (f"scorer_gsl {label} n={n} r={r} h={h} k={k} {mode} {'compact' if compact else 'padded'}{' collapsed' if collapsed else ''}"
            f"{f' dropout {drop_p}' if drop_p else ''}{f' {mis} misaligned' if mis else ''}")
    f = _Fenced()
    fd = wd = xd = None
    if use_score_x:
        xd = f.put("score_x", xrows.astype(np.float32))
    else:
        fd, wd = f.put("feat", feat, mis=mis == "feat"), f.put("w_p", w_p, mis=mis == "w_p")
    gd = T(gate)
    score, keep = f.put("score", shape=(n, r)), f.put("keep", shape=(n, W), dtype=torch.int64)
    lib.call("gh_scorer_gsl", lib.ptr(D.bits), lib.ptr(D.dinv), lib.ptr(D.vals), lib.ptr(D.goff) if compact else None,
             1 if collapsed else 0, lib.ptr(fd), lib.ptr(xd), lib.ptr(wd), lib.ptr(gd), n, r, h, k, lib.ptr(score), lib.ptr(keep),
             float(drop_p), drop_seed, lib.stream())
    torch.cuda.synchronize()
    f.check(what)
    _rel(score, torch.from_numpy(s64), what, f"scorer {label}")
    _exact(keep, g_pack_bits(g_topk(score.cpu().numpy(), k)), what + " (top-k of the returned scores)")
    _exact(keep, g_pack_bits(g_topk(s64, k)), what + " (top-k of the float64 scores)")


@pytest.mark.parametrize("r", [1, 64, 65, 100, 256])
def test_scorer_gsl_every_projection_path_and_layout(r):
    Gn, Gw = _word_batch(6, r, 3, 1), _dense_batch(6, r, seed=1)
    for G in (Gn, Gw):
        _scorer_case(G, 300, "float4")
        _scorer_case(G, 300, "float4", compact=True)                       # compact with padding rows that compete
        _scorer_case(G, 300, "float4", compact=True, collapsed=True)       # every padding node ties: the lower index wins
        _scorer_case(G, 30, "scalar")                                      # h % 4 != 0
        _scorer_case(G, 30, "scalar", compact=True)
        _scorer_case(G, 44, "scalar", mis="feat")
        _scorer_case(G, 44, "scalar", mis="w_p", compact=True)
        _scorer_case(G, 300, "float4", drop_p=0.3)
        _scorer_case(G, 300, "float4", drop_p=0.3, compact=True)           # mask indexed by the compact row
        _scorer_case(G, 30, "scalar", drop_p=0.3, compact=True)
        _scorer_case(G, 300, "score_x", use_score_x=True)
        _scorer_case(G, 300, "score_x", use_score_x=True, compact=True)
        _scorer_case(G, 300, "score_x", use_score_x=True, compact=True, collapsed=True)


# ----------------------------------------------------------------------------- batch preparation, all bit-exact
def _build_texts(n, r, seed):
    """Texts with repeats whose node indices straddle bit 63 / 64, and lengths -3, 0, r, r + 7 among random ones."""
    toks, lens = _texts(n, r, 0, seed, kinds=False)
    toks, lens = toks.copy(), lens.copy()
    for g, ln in zip(range(4), (-3, 0, r, r + 7)):
        if g < n:
            lens[g] = ln
    if n > 5 and r >= 3:
        toks[4] = np.arange(r) + 10                  # all distinct: node i = position i ...
        toks[4, r - 1], toks[4, r - 2] = toks[4, min(63, r - 3)], toks[4, min(64, r - 3)]      # ... then nodes 63 and 64 again
        lens[4] = r
        toks[5, :] = np.arange(r) % 2 + 3            # two nodes, every position
        lens[5] = r
    return toks, lens


def _graph_build_once(toks, lens, r, window, what):
    lib = _lib()
    n, W = len(toks), g_words(r)
    f = _Fenced()
    ids, nn = f.put("node_ids", shape=(n, r), dtype=torch.int32), f.put("n_nodes", shape=(n,), dtype=torch.int32)
    bits, dinv = f.put("bits", shape=(n, r, W), dtype=torch.int64), f.put("dinv", shape=(n, r))
    td, ld = T(toks), T(lens)
    lib.call("gh_graph_build", lib.ptr(td), lib.ptr(ld), n, r, window, lib.ptr(ids), lib.ptr(nn), lib.ptr(bits), lib.ptr(dinv), lib.stream())
    torch.cuda.synchronize()
    f.check(what)
    return ids, nn, bits, dinv


@pytest.mark.parametrize("r", [1, 63, 64, 65, 200, 256])
def test_graph_build_against_convert_text(r):
    for window in sorted({1, 3, r}):
        CASES[0] += 1
        what = f"graph_build r={r} window={window}"
        toks, lens = _build_texts(12, r, 40 + r)
        e_ids, e_nn, e_pat, e_dinv, _ = g_text_graphs(toks, lens, r, window, O.convert_text)
        ids, nn, bits, dinv = _graph_build_once(toks, lens, r, window, what)
        _exact(ids, e_ids, what + " node_ids")
        _exact(nn, e_nn, what + " n_nodes")
        _exact(bits, g_pack_bits(e_pat), what + " bits")
        _exact(dinv, e_dinv, what + " dinv")            # float32(1 / sqrt(float64(deg))), bit for bit


def test_graph_build_a_thousand_texts_in_one_launch():
    CASES[0] += 1
    r, window, n = 64, 3, 1000
    toks, lens = _build_texts(n, r, 9)
    e_ids, e_nn, e_pat, e_dinv, _ = g_text_graphs(toks, lens, r, window, O.convert_text)
    ids, nn, bits, dinv = _graph_build_once(toks, lens, r, window, "graph_build 1000 texts")
    _exact(ids, e_ids, "node_ids"); _exact(nn, e_nn, "n_nodes"); _exact(bits, g_pack_bits(e_pat), "bits"); _exact(dinv, e_dinv, "dinv")


@pytest.mark.parametrize("r", [1, 65, 256])
def test_adj_pack_and_unpack(r):
    lib = _lib()
    G = _dense_batch(5, r, seed=2)
    W, n = g_words(r), G.n
    a64 = G.vals.astype(np.float64) * (1.0 + 2.0 ** -30)          # float64 values that round to fp32 on the way in
    for entry, src in (("gh_adj_pack_f32", G.vals), ("gh_adj_pack_f64", a64)):
        CASES[0] += 1
        what = f"{entry} r={r}"
        f = _Fenced()
        bits, vals = f.put("bits", shape=(n, r, W), dtype=torch.int64), f.put("vals", shape=(n, r, r))
        ad = T(src)
        lib.call(entry, lib.ptr(ad), n, r, lib.ptr(bits), lib.ptr(vals), lib.stream())
        torch.cuda.synchronize()
        f.check(what)
        _exact(bits, g_pack_bits(g_dense_pattern(src)), what + " bits")
        _exact(vals, src.astype(np.float32), what + " vals")
    D = _upload(G)
    Gn = _word_batch(5, r, 3, 2)
    Dn = _upload(Gn)
    for B, Dv in ((G, D), (Gn, Dn)):
        for keep in (None, _keep_for(n, r, max(1, r // 3))):
            CASES[0] += 1
            what = f"gh_adj_unpack r={r} {'weighted' if B.vals is not None else 'normalised'}{'' if keep is None else ' keep'}"
            f = _Fenced()
            adj = f.put("adj", shape=(n, r, r))
            kd = None if keep is None else T(g_pack_bits(keep))
            lib.call("gh_adj_unpack", lib.ptr(Dv.bits), lib.ptr(Dv.dinv), lib.ptr(Dv.vals), lib.ptr(kd), n, r, lib.ptr(adj), lib.stream())
            torch.cuda.synchronize()
            f.check(what)
            if B.vals is not None:
                _exact(adj, g_refined64(B.pattern, keep, None, B.vals).astype(np.float32), what)
            else:                                      # the fp32 product of two fp32 dinv
                on = g_refined64(B.pattern, keep, B.dinv) != 0
                _exact(adj, np.where(on, B.dinv[:, :, None] * B.dinv[:, None, :], np.float32(0)), what)


def _plan_counts(n, r, seed):
    rng = np.random.default_rng(seed)
    nn = rng.integers(0, r + 1, size=n).astype(np.int32)
    nn[::7] = r + 3                                    # clamped to r
    nn[3::11] = -2                                     # clamped to 0
    return nn


def _plan_call(nn, ids, n, r, with_ids, what):
    lib = _lib()
    f = _Fenced()
    goff = f.put("goff", shape=(n + 1,), dtype=torch.int32)
    rowg, src = f.put("rowg", shape=(n * r,), dtype=torch.int32), f.put("src", shape=(n * r,), dtype=torch.int32)
    cids = f.put("cids", shape=(n * r,), dtype=torch.int32) if with_ids else None
    maskf = f.put("maskf", shape=(n * r,)) if with_ids else None
    nd, idd = T(nn), T(ids)
    lib.call("gh_ragged_plan", lib.ptr(nd), lib.ptr(idd) if with_ids else None, n, r, lib.ptr(goff), lib.ptr(rowg), lib.ptr(src),
             lib.ptr(cids), lib.ptr(maskf), lib.stream())
    torch.cuda.synchronize()
    f.check(what)
    return goff, rowg, src, cids, maskf


@pytest.mark.parametrize("n,label", [(1, "one launch"), (4096, "one launch"), (4097, "scan + fill"), (5000, "scan + fill")])
def test_ragged_plan_against_numpy(n, label):
    r = 4
    nn = _plan_counts(n, r, 60 + n)
    ids = np.random.default_rng(n).integers(0, 50, size=(n, r)).astype(np.int32)
    for with_ids in (True, False):
        CASES[0] += 1
        what = f"ragged_plan n={n} {label}{'' if with_ids else ' cids / maskf NULL'}"
        e = g_plan(nn, r, ids)
        goff, rowg, src, cids, maskf = _plan_call(nn, ids, n, r, with_ids, what)
        _exact(goff, e["goff"], what + " goff"); _exact(rowg, e["rowg"], what + " rowg"); _exact(src, e["src"], what + " src")
        if with_ids:
            _exact(cids, e["cids"], what + " cids"); _exact(maskf, e["maskf"], what + " maskf")


@pytest.mark.parametrize("b,b1,l,r,plan,label", [(3, 7, 30, 65, True, "small batch: scatter rides along"),
                                                 (3, 7, 30, 65, False, "m_real < 0: scatter kernel, no plan"),
                                                 (5, 4100, 8, 4, True, "b1 > 4096: scan + fill, scatter kernel")])
def test_get_prepare_against_the_separate_entries(b, b1, l, r, plan, label):
    CASES[0] += 1
    lib = _lib()
    window, n_max = 3, -(-b1 // b) + 1
    what = f"get_prepare b={b} b1={b1} r={r} {label}"
    qt, ql = _build_texts(b, l, 70 + l)
    dt, dl = _build_texts(b1, r, 71 + r)
    q_e = g_text_graphs(qt, ql, l, window, O.convert_text)
    d_e = g_text_graphs(dt, dl, r, window, O.convert_text)
    slot_np = np.random.default_rng(b1).permutation(b * n_max)[:b1].astype(np.int64)      # distinct rows of document, not in order
    f = _Fenced()
    q = [f.put("q_ids", shape=(b, l), dtype=torch.int32), f.put("q_n", shape=(b,), dtype=torch.int32),
         f.put("q_bits", shape=(b, l, g_words(l)), dtype=torch.int64), f.put("q_dinv", shape=(b, l))]
    d = [f.put("d_ids", shape=(b1, r), dtype=torch.int32), f.put("d_n", shape=(b1,), dtype=torch.int32),
         f.put("d_bits", shape=(b1, r, g_words(r)), dtype=torch.int64), f.put("d_dinv", shape=(b1, r))]
    pl = [f.put("goff", shape=(b1 + 1,), dtype=torch.int32), f.put("rowg", shape=(b1 * r,), dtype=torch.int32),
          f.put("src", shape=(b1 * r,), dtype=torch.int32), f.put("cids", shape=(b1 * r,), dtype=torch.int32), f.put("maskf", shape=(b1 * r,))]
    doc = f.put("document", torch.zeros(b * n_max, r, dtype=torch.int32), dtype=torch.int32)
    m_real = int(np.clip(d_e[1], 0, r).sum()) if plan else -1
    tens = [T(qt), T(ql), T(dt), T(dl), T(slot_np)]
    lib.call("gh_get_prepare", lib.ptr(tens[0]), lib.ptr(tens[1]), b, l, lib.ptr(tens[2]), lib.ptr(tens[3]), b1, r, window,
             *[lib.ptr(t) for t in q], *[lib.ptr(t) for t in d], m_real, *[lib.ptr(t) for t in pl], lib.ptr(tens[4]), lib.ptr(doc),
             lib.stream())
    torch.cuda.synchronize()
    f.check(what)
    for got, e, name in ((q, q_e, "claim"), (d, d_e, "evidence")):
        _exact(got[0], e[0], f"{what} {name} node_ids"); _exact(got[1], e[1], f"{what} {name} n_nodes")
        _exact(got[2], g_pack_bits(e[2]), f"{what} {name} bits"); _exact(got[3], e[3], f"{what} {name} dinv")
    # the separate entries give the same, bit for bit
    s_ids, s_nn, s_bits, s_dinv = _graph_build_once(dt, dl, r, window, what + " (gh_graph_build)")
    assert torch.equal(s_ids, d[0]) and torch.equal(s_nn, d[1]) and torch.equal(s_bits, d[2]) and torch.equal(s_dinv.view(torch.int32), d[3].view(torch.int32))
    if plan:
        e = g_plan(d_e[1], r, d_e[0])
        for t, key in zip(pl, ("goff", "rowg", "src", "cids", "maskf")):
            _exact(t, e[key], f"{what} {key}")
        sep = _plan_call(d_e[1], d_e[0], b1, r, True, what + " (gh_ragged_plan)")
        for t, u in zip(pl, sep):
            assert torch.equal(t.view(torch.int32), u.view(torch.int32)), what
    else:
        for t in pl:
            _untouched(t, f"{what} plan output")
    e_doc = np.zeros((b * n_max, r), np.int32)
    e_doc[slot_np] = d_e[0]
    _exact(doc, e_doc, what + " document")


# ---- gh_ref_depad
def _depad_batch(b, n_max, r, seed, kind="normalised"):
    """counts (with 0, a negative one and one above n_max), ids (b, n_max, r) and float64 adjacency (b, n_max, r, r): word
    graphs as convert_text hands them over (float64 D^-1/2 A D^-1/2)."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, n_max + 1, size=b).astype(np.int64)
    if b >= 4:
        counts[0], counts[1], counts[2], counts[3] = n_max, 0, -3, n_max + 5
    toks, lens = _texts(b * n_max, r, 3, seed, kinds=False)
    lens = lens.copy()
    lens[::5] = 0
    ids32, _, _, _, adj = g_text_graphs(toks, lens, r, 3, O.convert_text)
    return counts, ids32.reshape(b, n_max, r).astype(np.int64), adj.reshape(b, n_max, r, r).copy()


def _depad_case(counts, ids, adj, i64, force, what, want_bad=None, want_weighted=None):
    CASES[0] += 1
    lib = _lib()
    b, n_max, r = ids.shape
    W, tot = g_words(r), b * n_max
    e = g_depad(counts, n_max, r, ids, adj)
    pairs = len(e["ids"])
    f = _Fenced()
    d_ids, bits = f.put("d_ids", shape=(tot, r), dtype=torch.int32), f.put("bits", shape=(tot, r, W), dtype=torch.int64)
    vals, dinv = f.put("vals", shape=(tot, r, r)), f.put("dinv", shape=(tot, r))
    nn, stats = f.put("n_nodes", shape=(tot,), dtype=torch.int32), f.put("stats", shape=(5,), dtype=torch.int64)
    cd, idd, ad = T(counts), T(ids if i64 else ids.astype(np.int32)), T(adj)
    lib.call("gh_ref_depad", lib.ptr(cd), b, n_max, r, lib.ptr(idd), 1 if i64 else 0, lib.ptr(ad), lib.ptr(d_ids), lib.ptr(bits),
             lib.ptr(vals), lib.ptr(dinv), lib.ptr(nn), lib.ptr(stats), 1 if force else 0, lib.stream())
    torch.cuda.synchronize()
    f.check(what)
    n_bad, n_w = int(np.sum(e["bad"])), int(np.sum(e["weighted"]))
    if want_bad is not None:
        assert (n_bad, n_w) == (want_bad, want_weighted), f"{what}: the fixture has {n_bad} bad and {n_w} weighted pairs"
    _exact(stats, np.array([pairs, int(np.sum(e["n_nodes"])), n_bad, n_w, 0], np.int64), what + " stats")
    if pairs:
        _exact(d_ids[:pairs], np.stack(e["ids"]), what + " ids"); _exact(nn[:pairs], np.array(e["n_nodes"], np.int32), what + " n_nodes")
        _exact(bits[:pairs], g_pack_bits(np.stack(e["pattern"])), what + " bits"); _exact(dinv[:pairs], np.stack(e["dinv"]), what + " dinv")
    for p in range(pairs):
        if e["weighted"][p] or force:
            _exact(vals[p], e["vals"][p], f"{what} vals of pair {p}")
        else:
            _untouched(vals[p], f"{what} vals of recognised pair {p}")
    for t in (d_ids, bits, vals, dinv, nn):            # rows >= pairs of every output
        _untouched(t[pairs:], f"{what} rows >= pairs")


@pytest.mark.parametrize("r", [1, 100, 256])
@pytest.mark.parametrize("i64", [True, False])
def test_ref_depad_recognised_normalised_graphs(r, i64):
    counts, ids, adj = _depad_batch(6 if r < 256 else 4, 3 if r < 256 else 2, r, 80 + r)
    what = f"ref_depad r={r} {'int64' if i64 else 'int32'} ids"
    _depad_case(counts, ids, adj, i64, False, what + " recognised", want_bad=0, want_weighted=0)      # stats[3] == 0, vals still NaN
    _depad_case(counts, ids, adj, i64, True, what + " force_vals", want_bad=0, want_weighted=0)


def test_ref_depad_pair_index_over_more_than_256_counts():
    counts, ids, adj = _depad_batch(300, 2, 8, 5)
    assert (np.clip(counts, 0, 2)[:290] > 0).sum() > 150
    _depad_case(counts, ids, adj, True, False, "ref_depad b=300 n_max=2 r=8")
    _depad_case(counts, ids, adj, False, True, "ref_depad b=300 n_max=2 r=8 int32 force_vals")


def test_ref_depad_recognition_and_layout_flags():
    r = 100
    counts, ids, adj = _depad_batch(4, 2, r, 31)
    counts[:] = 2
    full = [(c, j) for c in range(4) for j in range(2) if (ids[c, j] >= 1).sum() >= 4]
    assert len(full) >= 5
    (c0, j0), (c1, j1), (c2, j2), (c3, j3), (c4, j4) = full[:5]
    a = adj.copy(); a[c0, j0] *= 1.0 + 1e-7
    _depad_case(counts, ids, a, True, False, "ref_depad values x (1 + 1e-7): recognised", want_bad=0, want_weighted=0)
    a = adj.copy(); a[c1, j1] *= 1.0 + 1e-5
    _depad_case(counts, ids, a, True, False, "ref_depad values x (1 + 1e-5): weighted", want_bad=0, want_weighted=1)
    a = adj.copy()
    i, j = np.argwhere(np.triu(a[c2, j2] != 0, 1))[0]
    a[c2, j2, i, j] = 0.0                                  # an entry present on one side only
    _depad_case(counts, ids, a, True, False, "ref_depad one-sided entry: weighted", want_bad=0, want_weighted=1)
    i2 = ids.copy(); i2[c3, j3, 1] = 0                     # a zero in the middle of the ids
    _depad_case(counts, i2, adj, False, False, "ref_depad ids with a hole", want_bad=1, want_weighted=0)
    a = adj.copy()
    nn4 = int((ids[c4, j4] >= 1).sum())
    assert nn4 < r
    a[c4, j4, nn4, nn4] = 1.0                              # a padding node carrying an edge (a self loop: still normalised)
    _depad_case(counts, ids, a, True, False, "ref_depad edge on a padding node", want_bad=1, want_weighted=0)


def test_zz_report():
    """Prints the worst ratios and the number of cases of this file (DESIGN.md 4.8 quotes one run)."""
    print(f"cases so far: {CASES[0]}")
    for fam in sorted(WORST):
        if fam.startswith(("spmm", "scorer")):
            print(f"worst {fam}: {WORST[fam]:.3e}")

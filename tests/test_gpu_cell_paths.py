"""Every dispatch path of the GGNN cell entries (csrc/cell_ops.hip: gh_ggnn_cell_fwd, gh_ggnn_cell_bwd and their _bf16 twins)
and of the streaming kernels only the cell reaches (csrc/stream_ops.hip: gate_bwd_pre, gather_rows) against the float64
restatement of the cell in tests/util.py (cell_forward_f64 / cell_backward_f64, checked on their own by
tests/test_cell_restatement_cpu.py).

The four C-ABI entries are called directly with the argument lists of get_amd/ops/graph.py.  Every floating-point operand, saved
stream, scratch tensor and output sits inside a NaN-filled allocation of its own (tests/util.py _Fenced; the integer inputs --
bit rows, keep words, ids, goff -- are plain tensors: there is no NaN to fence them with), the workspace is NaN before every call
and the path counters are reset.  Adjacencies are built in numpy and packed with g_pack_bits / g_dinv (PackedAdj.from_dense only
for the weighted variant); a batch holds full, short and single-node graphs.  What a stream that starts as NaN proves: a row the
contract says is written comes back finite, a row, column or contraction element outside an operand that reaches a sum comes
back NaN, a partial tile summed without having been written comes back NaN, a store outside an output breaks a fence.

Shapes are (n, r, din, h): graphs, padded nodes per graph, input width, hidden width.  Layouts: padded (n r rows), or node-compact
(tests/util.py g_plan) on the first m_rows rows, m_real <= m_rows <= n r.  On the node-compact layout with m_rows > m_real the
rows >= m_real of rr and hh are undefined (include/get_hip.h) and not compared; those rows of xp, a, z, rx and out are (a padding
row has no neighbours) -- except the rows of `a` beyond the partial zero fill of the fast path, ((m_real + 127) / 128 + 1) * 128,
which stay the NaN they were: the written rows of the other streams being right shows that the tile skip reads none of them.

Forward: every stream from the original inputs.  Backward: the saved streams handed in are the float64 forward rounded to fp32,
not the kernel's own, the seven dw and six db start from non-zero pre-fills and are compared with pre + reference, dx starts as
NaN; once with db_?1 NULL and once given.  Two calls into separately prepared buffers agree bit for bit in every compared output:
no case here orders a sum by an fp32 atomic (a weight gradient of one K chunk adds once per element; several chunks go through the
workspace and reduce_partials_kernel; the column sums take the workspace kernels or, at <= 256 rows, one row block; the scorer's
two column blocks add two addends onto zero).

Bounds.  fp32 entries: tests.util.TOL (1e-4 of the float64 result's largest entry) on every written element, in exact fp32 and
-- the NT launches -- in fp32x3p.  bf16 entries, stage by stage: a stored bf16 stream against the float64 value of that stage
computed from the bf16 values the kernel stored upstream (read back) and the bf16 weights, |err| <= 2^-8 |ref| + TOL max|ref|
(one round-to-nearest bf16 store -- half an ulp of 8 significant bits, which is 2^-9 of a value just below a power of two and
2^-8 of one just above it, so a single store alone comes to 0.95 of this bound -- plus the fp32 accumulation); their
fp32 outputs (out32, dx, dw, db) at TOL against float64 of the stored bf16 operands.  The bf16 cases drop with p = 0.5: the
loaders round the masked, scaled operand to bf16 again, which 1 / (1 - p) = 2 makes exact, so a stage stays one store.  In the
bf16 backward da and dxp are stored, re-read and stored again by up to four launches; their intermediate values are overwritten, so
a per-stage reference does not exist for them: dxp is read back only as the operand of dx and dw_p, da not at all (the backward
ends with the gathered rows in it).

The plan named next to a case is the planner's (csrc/gemm_plan.h): tools/gemm_plan_sweep.cpp restates the launches of both entries
and asserts tile, split, chunk count, finish shape, fast / generic, workspace / atomic and fused / separate column sums of every
launch of every case below on the CPU (tests/test_gemm_plan_cpu.py; the names there are the ones in the comments here).  A run
itself verifies the fast / generic counts and the launch total (gh_gemm_path_counters), whether partial tiles and column-sum
partials reached the workspace (_ws_written) and the fences.  Which epilogue implementation ran is not visible from outside; a
mutation check on scratch copies of the library (one value-only change per implementation) showed it: every
unsplit fast launch in exact fp32, on all three tiles, runs the straight-line epilogue of gemm_nt_epi32.hip.h; fp32x3p runs `pass`
of gemm_nt.hip.h; the bf16 64 x 320 and 128 x 256 tiles `pass8`; the 256 x 256 tile the fast epilogue of gemm_nt_pp_epi.hip.h;
split launches nt_finish_kernel; generic launches gemm.hip.h.

Not reachable through the public entries, so without a case: the backward on a second stream, the fused next cell (EPI_GATE_PRE)
and the second row buffer (one weight-gradient launch) -- model_ops.hip passes them, tests/test_gpu_cell_bwd_nodx.py covers that
composite; score_parts (more than two column blocks of a scorer projection); gather_rows_bf16's 4-wide loop (the bf16 entries
require din % 8 == 0 and the destination is the 16-byte aligned row buffer `da`, so only a misaligned table would reach it, which
the bf16 contract does not allow).  No fp32 shape below 30 000 rows other than 251 x 100 reaches the occupancy switch to 32-row
tiles in the z / r pair; the projection and the h gate (one problem, or the narrow tile) never do below 50 000 rows."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.util import (CELL_B, CELL_SAVED, CELL_W, DEV, TOL, WORST, _Fenced, _f64, _ops, _poison, _rel, _same, _workspace,
                        _ws_written, cell_backward_f64, cell_forward_f64, g_dinv, g_pack_bits, g_plan, g_refined64)

pytestmark = pytest.mark.gpu

VOCAB = 128
SEED, SCORE_SEED = 90210, 4711
OUT_STREAMS = CELL_SAVED + ("out",)


# ----------------------------------------------------------------------------- graphs, numbers
def _counts(n, r, kind):
    """mixed: full, short (a third) and single-node graphs in turn; tail: all full but the last four (short, 1, short, 1)."""
    short = max(r // 3, 1)
    if kind == "mixed":
        return [(r, short, 1)[g % 3] for g in range(n)]
    assert kind == "tail" and n > 4
    return [r] * (n - 4) + [short, 1, short, 1]


@functools.lru_cache(maxsize=None)
def _graph(n, r, kind):
    """Symmetric patterns with self loops on the real nodes, node ids (>= 1 real, 0 padding), dinv, the node-compact plan, the
    weighted variant's fp32 values (asymmetric) and a keep set."""
    rng = np.random.default_rng(1000 * n + r + (7 if kind == "tail" else 0))
    counts = _counts(n, r, kind)
    pattern = np.zeros((n, r, r), bool)
    ids = np.zeros((n, r), np.int32)
    for g, c in enumerate(counts):
        on = rng.random((c, c)) < min(0.5, 6.0 / c)
        pattern[g, :c, :c] = on | on.T | np.eye(c, dtype=bool)
        ids[g, :c] = rng.integers(1, VOCAB, c)
    dinv = g_dinv(pattern)
    vals = (g_refined64(pattern, dinv=dinv) * (1.0 + 0.3 * rng.standard_normal((n, r, r)))).astype(np.float32)
    keep = rng.random((n, r)) < 0.4
    keep[:, 0] = True
    return SimpleNamespace(n=n, r=r, counts=counts, m_real=int(sum(counts)), pattern=pattern, ids=ids, dinv=dinv, vals=vals, keep=keep,
                           plan=g_plan(np.asarray(counts), r, ids))


@functools.lru_cache(maxsize=None)
def _numbers(rows, din, h):
    gen = torch.Generator().manual_seed(7919 * din + h)
    rn = lambda *s: torch.randn(*s, generator=gen)
    w = {"p": rn(h, din) / din ** 0.5}
    w.update({k: rn(h, h) / h ** 0.5 for k in CELL_W[1:]})
    b = {k: 0.1 * rn(h) for k in CELL_B}
    pre_w = {k: 0.3 * rn(*v.shape) for k, v in w.items()}
    pre_b = {k: 0.3 * rn(h) for k in CELL_B}
    return SimpleNamespace(table=rn(VOCAB, din), w=w, b=b, pre_w=pre_w, pre_b=pre_b, score_w=rn(h) / h ** 0.5,
                           g=torch.randn(rows, h, generator=torch.Generator().manual_seed(rows + h)))


def _adj64(G, variant):
    if variant == "weighted":
        return g_refined64(G.pattern | np.swapaxes(G.pattern, -1, -2), vals=G.vals)
    return g_refined64(G.pattern, keep=G.keep if variant == "keep" else None, dinv=G.dinv)


def _adj_args(f, G, variant):
    """(bits, dinv, vals, keep) of the C-ABI; the tensors are kept alive by the returned list."""
    _lib, ops = _ops()
    if variant == "weighted":
        padj = ops.PackedAdj.from_dense(torch.from_numpy(G.vals).to(DEV))
        assert np.array_equal(padj.bits.cpu().numpy(), g_pack_bits(G.pattern)), "from_dense packed another pattern"
        vals = f.put("vals", padj.vals)
        return [padj.bits, None, vals, None]
    bits = torch.from_numpy(g_pack_bits(G.pattern)).to(DEV)
    dinv = f.put("dinv", torch.from_numpy(G.dinv))
    keep = torch.from_numpy(g_pack_bits(G.keep)).to(DEV) if variant == "keep" else None
    return [bits, dinv, None, keep]


def C(n, r, din, h, **kw):
    """A case.  adj: pattern | weighted | keep; ids: table + ids instead of x; drop: input dropout p; compact: None (padded),
    "real", "tot" or m_rows; score: None or the scorer's dropout p; mis: the operand one float off a 16-byte boundary; counts:
    _counts kind; generic: launches on the generic kernel (of 3 forward launches / of the backward's); tiles: partial tiles reach
    the workspace; fam: the family the errors are recorded under."""
    d = dict(n=n, r=r, din=din, h=h, adj="pattern", ids=False, drop=0.0, compact=None, score=None, mis=None, counts="mixed",
             generic=0, tiles=False, fam="cell fwd 32x320", dx=True, ws="default", sums=None, bf=False)
    d.update(kw)
    return SimpleNamespace(**d)


def _name(c):
    bits = [f"{c.n}x{c.r}-{c.din}-{c.h}", c.adj]
    bits += ["ids"] if c.ids else []
    bits += [f"drop{c.drop}"] if c.drop else []
    bits += [f"compact-{c.compact}"] if c.compact is not None else []
    bits += [f"score{c.score}"] if c.score is not None else []
    bits += [f"mis-{c.mis}"] if c.mis else []
    bits += ["nodx"] if not c.dx else []
    bits += [f"ws-{c.ws}"] if c.ws != "default" else []
    return "-".join(bits)


def _layout(c, G, backward=False):
    """(src: padded row of every row of the call, m_real, m_rows)."""
    if c.compact is None:
        return np.arange(c.n * c.r), c.n * c.r, c.n * c.r
    m_rows = G.m_real if (c.compact == "real" or backward) else c.n * c.r if c.compact == "tot" else int(c.compact)
    return G.plan["src"][:m_rows].astype(np.int64), G.m_real, m_rows


def _key(c):
    return (c.n, c.r, c.din, c.h, c.adj, c.drop, c.compact, c.score, c.counts, c.bf)


def _mask(seed, rows, cols, p):
    from get_amd import ops
    return torch.from_numpy(ops.dropout_mask_reference(seed, rows, cols, p)).double() / (1.0 - p)


def _pad(t, src, total):
    out = torch.zeros((total,) + tuple(t.shape[1:]), dtype=torch.float64)
    out[torch.from_numpy(src)] = t.double()
    return out


def _fresh_weights():
    """The weights of every call sit in newly allocated buffers: tell the library, as a caller that replaces its weights must.
    (fp32x3p keeps pre-split images of the weights by address; without this a second call whose allocations come back in
    another order would multiply with the image of another matrix.)"""
    _, ops = _ops()
    ops.bump_weight_epoch()


# ----------------------------------------------------------------------------- forward, fp32
_FWD_REF = {}


def _fwd_ref(c):
    """The float64 streams of the call's rows (and score_x), once per case whatever its alignment, mode and ids / x form."""
    k = _key(c)
    if k not in _FWD_REF:
        G, (src, m_real, m_rows) = _graph(c.n, c.r, c.counts), _layout(c, _graph(c.n, c.r, c.counts))
        num = _numbers(c.n * c.r, c.din, c.h)
        x = num.table[torch.from_numpy(G.ids.reshape(-1)[src]).long()].double()
        if c.drop:
            x = x * _mask(SEED, m_rows, c.din, c.drop)
        adj = torch.from_numpy(_adj64(G, c.adj))
        full = cell_forward_f64(adj, _pad(x, src, c.n * c.r).view(c.n, c.r, c.din), num.w, num.b)
        ref = {k2: v.reshape(c.n * c.r, c.h)[torch.from_numpy(src)] for k2, v in full.items()}
        if c.score is not None:
            o = ref["out"] * (_mask(SCORE_SEED, m_rows, c.h, c.score) if c.score > 0 else 1.0)
            ref["score_x"] = o @ num.score_w.double()
        _FWD_REF[k] = ref
    return _FWD_REF[k]


def _fwd_once(c, what):
    _lib, _ = _ops()
    G = _graph(c.n, c.r, c.counts)
    src, m_real, m_rows = _layout(c, G)
    num = _numbers(c.n * c.r, c.din, c.h)
    f = _Fenced()
    adj = _adj_args(f, G, c.adj)
    row_ids = torch.from_numpy(G.ids.reshape(-1)[src].astype(np.int32))
    if c.ids:
        x, ids = f.put("table", num.table, mis=c.mis == "x"), row_ids.to(DEV)
    else:
        x, ids = f.put("x", num.table[row_ids.long()], mis=c.mis == "x"), None
    w = [f.put("w_" + k, num.w[k], mis=(c.mis == "w" and k == "z0")) for k in CELL_W]
    b = [f.put("b_" + k, num.b[k], mis=(c.mis == "bias" and k == "r0")) for k in CELL_B]
    st = {k: f.put(k, shape=(m_rows, c.h), mis=c.mis == k) for k in OUT_STREAMS}
    sw = f.put("score_w", num.score_w) if c.score is not None else None
    sx = f.put("score_x", shape=(m_rows,)) if c.score is not None else None
    goff = torch.from_numpy(G.plan["goff"]).to(DEV) if c.compact is not None else None
    _poison()
    _fresh_weights()
    _lib.gemm_path_counters(reset=True)
    try:
        _lib.call("gh_ggnn_cell_fwd", *[_lib.ptr(t) for t in adj], _lib.ptr(goff), m_real if goff is not None else 0, m_rows,
                  _lib.ptr(x), _lib.ptr(ids), c.n, c.r, c.din, c.h, *[_lib.ptr(t) for t in w], *[_lib.ptr(t) for t in b],
                  *[_lib.ptr(st[k]) for k in OUT_STREAMS], float(c.drop), SEED, _lib.ptr(sw), _lib.ptr(sx),
                  float(c.score or 0.0), SCORE_SEED, _lib.stream())
    finally:
        torch.cuda.synchronize()
        cnt = _lib.gemm_path_counters()
        f.check(what)
    st["score_x"] = sx
    return st, cnt, _ws_written()


def _fwd_views(c, st):
    """(name, the rows of the stream the contract says are written)."""
    G = _graph(c.n, c.r, c.counts)
    _, m_real, m_rows = _layout(c, G)
    views = []
    for k in OUT_STREAMS + (("score_x",) if c.score is not None else ()):
        rows = m_rows
        if k in ("rr", "hh"):
            rows = m_real
        elif k == "a" and m_rows > m_real and not c.generic and c.h % 4 == 0 and c.h >= 4 and c.mis is None:
            rows = min(m_rows, ((m_real + 127) // 128 + 1) * 128)          # cell_fwd_impl partial_zero
            if rows < m_rows:
                assert bool(torch.isnan(st["a"][rows:]).all()), "rows of `a` beyond the partial zero fill were written"
        views.append((k, rows))
    return views


def _fwd_case(c, identical=True):
    what = "fwd " + _name(c)
    st, cnt, (tiles, _) = _fwd_once(c, what)
    ref = _fwd_ref(c)
    views = _fwd_views(c, st)
    for k, rows in views:
        _rel(st[k][:rows], ref[k][:rows], f"{what} {k}", c.fam)
    assert cnt["generic_large"] == 0 and cnt["generic"] == c.generic and cnt["fast"] == 3 - c.generic, \
        f"{what}: expected {3 - c.generic} fast and {c.generic} generic launches, counted {cnt}"
    assert tiles == c.tiles, f"{what}: partial tiles {'were' if tiles else 'were not'} written to the workspace"
    if identical:
        again, _, _ = _fwd_once(c, what)
        _same([st[k][:rows] for k, rows in views], [again[k][:rows] for k, rows in views], what)
    return st


SMALL = [(3, 20, 8, 8), (3, 20, 12, 20)]


@pytest.mark.parametrize("ids,drop", [(False, 0.0), (True, 0.0), (False, 0.2), (True, 0.2)], ids=["x", "ids", "x-drop", "ids-drop"])
@pytest.mark.parametrize("adj", ["pattern", "weighted", "keep"])
@pytest.mark.parametrize("shape", SMALL, ids=["8-8", "12-20"])
def test_fwd_few_rows_unsplit(shape, adj, ids, drop, arith_mode):
    """A1.  60 rows, K of 8 to 40: three unsplit launches on the 32 x 320 tile (sweep: fwd (3,20,8,8) x / ids drop, fwd (3,20,12,20)
    x / ids drop / fp32x3p); rows from x and gathered from a table, the dropout mask in the projection's loader, all three
    adjacency forms."""
    _, ops = _ops()
    ops.bump_weight_epoch()
    _fwd_case(C(*shape, adj=adj, ids=ids, drop=drop))


FWD_SPLIT = [
    C(2, 100, 64, 64, tiles=True, fam="cell fwd split-K finish"),              # z/r pair and h gate x2(4), wave per row; projection unsplit
    C(2, 100, 300, 300, tiles=True, fam="cell fwd split-K finish"),            # projection x4(5), gates x8(5) (9 K tiles of 16 + 19 ... per segment), wave per row
    C(3, 20, 64, 512, tiles=True, fam="cell fwd split-K finish"),              # two column blocks per gate, x16(4), a workgroup per row
    C(2, 100, 64, 64, compact="tot", fam="cell fwd 32x320"),                   # seg0_rows > 0: no launch splits
    C(2, 100, 64, 64, score=0.2, tiles=True, fam="cell fwd split-K finish"),   # the h gate with score_w does not split (the pair still does)
    C(2, 100, 64, 64, drop=0.2, tiles=True, fam="cell fwd split-K finish"),    # (the projection is unsplit at K = 64 anyway)
    C(2, 100, 300, 300, drop=0.2, tiles=True, fam="cell fwd split-K finish"),  # the projection with dropout does not split: x4 -> unsplit
]


@pytest.mark.parametrize("c", FWD_SPLIT, ids=_name)
def test_fwd_few_rows_split_k(c, arith_mode):
    """A2.  NT split-K with the gate epilogues in nt_finish_kernel (sweep: fwd (2,100,64,64) split / compact / score / drop,
    fwd (2,100,300,300) split / drop, fwd (3,20,64,512) split), and the three conditions of nt_split_plan that keep a launch whole."""
    _, ops = _ops()
    ops.bump_weight_epoch()
    _fwd_case(c)


FWD_GENERIC = [
    C(3, 20, 300, 1, generic=3, fam="cell fwd generic"),
    C(3, 20, 6, 6, generic=3, fam="cell fwd generic"),
    C(3, 20, 12, 30, generic=3, fam="cell fwd generic"),
    C(3, 20, 12, 30, generic=3, compact="tot", fam="cell fwd generic"),        # every padding row of `a` zeroed: partial_zero is false
    C(3, 20, 8, 8, mis="w", generic=1, fam="cell fwd generic"),                # w_z0: the pair's launch
    C(3, 20, 8, 8, mis="bias", generic=1, fam="cell fwd generic"),             # b_r0: the pair's launch
    C(3, 20, 8, 8, mis="xp", generic=3, fam="cell fwd generic"),               # the projection's C, an operand of both gate launches
    C(3, 20, 8, 8, mis="out", generic=1, fam="cell fwd generic"),              # the h gate's second output
]


@pytest.mark.parametrize("c", FWD_GENERIC, ids=_name)
def test_fwd_generic_kernel(c):
    """A3.  Widths that are no multiple of 4, h = 1, and one operand at a time one float off a 16-byte boundary send the launches
    that touch it to gemm_kernel (sweep: fwd (3,20,300,1) / (3,20,6,6) / (3,20,12,30) generic [compact], fwd (3,20,8,8) w / bias /
    xp / out misaligned).  Node-compact with padding rows on a generic shape: all of them are zero in `a` and the entry's
    internal check (a generic launch after a partial zero fill) does not trip."""
    st = _fwd_case(c)
    if c.compact is not None:
        G = _graph(c.n, c.r, c.counts)
        assert bool((st["a"][G.m_real:] == 0).all())


@pytest.mark.parametrize("c,msg", [(C(3, 20, 6, 6, drop=0.2), "fused dropout needs float4-shaped rows"),
                                   (C(3, 20, 6, 6, score=0.0), "the fused scorer projection needs h % 4 == 0 and h <= 320"),
                                   (C(3, 20, 8, 480, score=0.0), "the fused scorer projection needs h % 4 == 0 and h <= 320")],
                         ids=["drop-din6", "score-h6", "score-h480"])
def test_fwd_rejections_write_nothing(c, msg):
    """A3.  Dropout on a generic shape is refused by the first launch: no stream is written.  The scorer projection on h = 6
    (generic) and h = 480 (more than one 320-column block on a few-row tile) is refused by the h gate's launch: hh, out and
    score_x stay NaN.  The fences hold in all three."""
    what = "fwd rejected " + _name(c)
    _lib, _ = _ops()
    G, num = _graph(c.n, c.r, c.counts), _numbers(c.n * c.r, c.din, c.h)
    f = _Fenced()
    adj = _adj_args(f, G, c.adj)
    x = f.put("x", num.table[torch.from_numpy(G.ids.reshape(-1)).long()])
    w = [f.put("w_" + k, num.w[k]) for k in CELL_W]
    b = [f.put("b_" + k, num.b[k]) for k in CELL_B]
    st = {k: f.put(k, shape=(c.n * c.r, c.h)) for k in OUT_STREAMS}
    sw = f.put("score_w", num.score_w) if c.score is not None else None
    sx = f.put("score_x", shape=(c.n * c.r,)) if c.score is not None else None
    with pytest.raises(RuntimeError) as e:
        _lib.call("gh_ggnn_cell_fwd", *[_lib.ptr(t) for t in adj], None, 0, c.n * c.r, _lib.ptr(x), None, c.n, c.r, c.din, c.h,
                  *[_lib.ptr(t) for t in w], *[_lib.ptr(t) for t in b], *[_lib.ptr(st[k]) for k in OUT_STREAMS], float(c.drop), SEED,
                  _lib.ptr(sw), _lib.ptr(sx), 0.0, SCORE_SEED, _lib.stream())
    torch.cuda.synchronize()
    assert msg in str(e.value), str(e.value)
    f.check(what)
    untouched = OUT_STREAMS if c.drop else ("hh", "out")
    for k in untouched:
        assert bool(torch.isnan(st[k]).all()), f"{what}: {k} was written"
    if sx is not None:
        assert bool(torch.isnan(sx).all()), f"{what}: score_x was written"


FWD_BIG = [
    C(82, 100, 48, 160, fam="cell fwd 64x160"),                                              # one block per problem
    C(82, 100, 300, 300, adj="weighted", fam="cell fwd 64x160"),                             # two blocks, 160 + 140
    C(82, 100, 300, 300, score=0.2, fam="cell fwd 64x160 scorer"),                           # padded: two blocks add into score_x after a memset
    C(82, 100, 300, 300, score=0.2, compact=8192, counts="tail", fam="cell fwd 64x160 scorer"),   # rows % 4 == 0: the zero fill rides on the aggregation
    C(82, 100, 300, 300, score=0.0, compact=8198, counts="tail", fam="cell fwd 64x160 scorer"),   # rows % 4 != 0: memset
    C(82, 100, 48, 160, adj="keep", compact=8192, counts="tail", fam="cell fwd 64x160"),     # m_real = 7868 inside a tile; `a` zeroed up to row 8064 only
    C(250, 100, 300, 300, fam="cell fwd 64x320"),                                            # > 24 576 rows: projection and pair on 64 x 320, h gate narrow
    C(251, 100, 300, 300, fam="cell fwd 64x320"),                                            # 393 x 2 tiles = 1.023 rounds: the pair on 32-row tiles (occupancy)
]


@pytest.mark.parametrize("c", FWD_BIG, ids=_name)
def test_fwd_activation_sized(c):
    """A4.  >= 8192 rows: the 64 x 160 tile with one and two column blocks, the two-block scorer projection with both zero
    fills, the seg0_rows tile skip over rows of `a` that are NaN, the 64 x 320 tile above 24 576 rows and the occupancy
    rule (sweep: fwd (82,100,48,160), fwd (82,100,300,300) [score [compact 8192 / 8198]], fwd (82,100,48,160) compact 8192,
    fwd (250,100,300,300), fwd (251,100,300,300))."""
    _fwd_case(c, identical=c.n <= 82)


@pytest.mark.parametrize("c", [C(82, 100, 300, 300, fam="cell fwd fp32x3p"), C(120, 100, 48, 160, fam="cell fwd fp32x3p")], ids=_name)
def test_fwd_activation_sized_fp32x3p(c):
    """A4 in fp32x3p, which switches the narrow tile off: at 8200 rows the occupancy rule then takes 32-row tiles for all three
    launches (129 and 258 tiles of 64 rows are 0.17 and 0.34 rounds); at 12 000 rows the pair runs on 64 x 320 (376 tiles, 0.49
    rounds) -- sweep: fwd (82,100,300,300) fp32x3p, fwd (120,100,48,160) fp32x3p."""
    _lib, ops = _ops()
    _lib.set_gemm_mode("fp32x3p")
    ops.bump_weight_epoch()
    try:
        _fwd_case(c, identical=False)
    finally:
        ops.bump_weight_epoch()
        _lib.set_gemm_mode("fp32")


@pytest.mark.parametrize("shape", [(3, 20, 12, 20), (82, 100, 300, 300)], ids=["12-20", "300-300"])
def test_fwd_padded_against_node_compact(shape):
    """A5.  The same graphs through both layouts: the real rows of the node-compact call (m_rows == m_real and m_rows == m_tot)
    are the padded call's rows of those nodes, within the bound (sweep: fwd (3,20,12,20) compact 28 / 60 of 28,
    fwd (82,100,300,300) compact 3718 / 8200 of 3718)."""
    big = shape[0] > 3
    fam = "cell fwd 64x160" if big else "cell fwd 32x320"
    padded = _fwd_case(C(*shape, fam=fam), identical=False)
    G = _graph(shape[0], shape[1], "mixed")
    for compact in ("real", "tot"):
        c = C(*shape, compact=compact, fam=fam if compact == "tot" else "cell fwd 32x320")
        got = _fwd_case(c, identical=False)
        src = torch.from_numpy(G.plan["src"][:G.m_real]).to(DEV)
        for k in OUT_STREAMS:
            _rel(got[k][:G.m_real], _f64(padded[k][src]), f"fwd {_name(c)} vs padded {k}", "cell fwd layouts")


# ----------------------------------------------------------------------------- backward, fp32
_BWD_REF = {}


def _bwd_ref(c):
    """Saved streams (float64 forward rounded to fp32, the call's rows), g, and the float64 gradients from them."""
    k = _key(c)
    if k not in _BWD_REF:
        G = _graph(c.n, c.r, c.counts)
        src, _, m = _layout(c, G, backward=True)
        num = _numbers(c.n * c.r, c.din, c.h)
        total, tsrc = c.n * c.r, torch.from_numpy(src)
        x = num.table[torch.from_numpy(G.ids.reshape(-1)[src]).long()].double()
        mask = _mask(SEED, m, c.din, c.drop) if c.drop else None
        xm = x * mask if c.drop else x
        adj = torch.from_numpy(_adj64(G, c.adj))
        xpad = _pad(xm, src, total).view(c.n, c.r, c.din)
        fwd = cell_forward_f64(adj, xpad, num.w, num.b)
        saved = {k2: fwd[k2].reshape(total, c.h)[tsrc].float() for k2 in CELL_SAVED}
        g = num.g[:m]
        scratch = {}
        dw, db, dx = cell_backward_f64(adj, xpad, _pad(g, src, total).view(c.n, c.r, c.h), num.w, num.b,
                                       saved={k2: _pad(v, src, total).view(c.n, c.r, c.h) for k2, v in saved.items()}, scratch=scratch)
        dx = dx.reshape(total, c.din)[tsrc]
        _BWD_REF[k] = SimpleNamespace(saved=saved, g=g, dw=dw, db=db, dx=dx * mask if c.drop else dx,
                                      scratch={k2: v.reshape(total, c.h)[tsrc] for k2, v in scratch.items()})
    return _BWD_REF[k]


def _bwd_once(c, what, db1):
    _lib, _ = _ops()
    G = _graph(c.n, c.r, c.counts)
    src, m_real, m = _layout(c, G, backward=True)
    num = _numbers(c.n * c.r, c.din, c.h)
    ref = _bwd_ref(c)
    f = _Fenced()
    adj = _adj_args(f, G, c.adj)
    row_ids = torch.from_numpy(G.ids.reshape(-1)[src].astype(np.int32))
    if c.ids:
        x, ids = f.put("table", num.table, mis=c.mis == "x"), row_ids.to(DEV)
    else:
        x, ids = f.put("x", num.table[row_ids.long()], mis=c.mis == "x"), None
    wt = [f.put("wt_" + k, num.w[k].t().contiguous()) for k in CELL_W]
    saved = [f.put(k, ref.saved[k], mis=c.mis == k) for k in CELL_SAVED]
    g = f.put("g", ref.g)
    scratch = {k: f.put(k, shape=(m, c.h)) for k in ("dhp", "dzp", "drp", "dxp", "da")}
    dx = f.put("dx", shape=(m, c.din)) if c.dx else None
    dw = {k: f.put("dw_" + k, num.pre_w[k]) for k in CELL_W}
    db = {k: f.put("db_" + k, num.pre_b[k]) for k in CELL_B}
    goff = torch.from_numpy(G.plan["goff"]).to(DEV) if c.compact is not None else None
    _poison()
    _fresh_weights()
    _lib.gemm_path_counters(reset=True)
    _lib.call("gh_ggnn_cell_bwd", *[_lib.ptr(t) for t in adj], _lib.ptr(goff), m_real if goff is not None else 0,
              _lib.ptr(x), _lib.ptr(ids), c.n, c.r, c.din, c.h, *[_lib.ptr(t) for t in wt], *[_lib.ptr(t) for t in saved], _lib.ptr(g),
              *[_lib.ptr(scratch[k]) for k in ("dhp", "dzp", "drp", "dxp", "da")], _lib.ptr(dx), *[_lib.ptr(dw[k]) for k in CELL_W],
              _lib.ptr(db["z0"]), _lib.ptr(db["r0"]), _lib.ptr(db["h0"]),
              *[_lib.ptr(db[k]) if db1 else None for k in ("z1", "r1", "h1")], float(c.drop), SEED, _lib.stream())
    torch.cuda.synchronize()
    cnt = _lib.gemm_path_counters()
    f.check(what)
    return SimpleNamespace(dx=dx, dw=dw, db=db, scratch=scratch), cnt, _ws_written()


def _bwd_case(c):
    """GEMM launches of a call: 4 with dx (two NT pairs, dX, the weight gradients), 3 without dx on either chain; c.generic of
    them on the generic kernel; c.tiles / c.sums: partial tiles / column-sum partials in the workspace."""
    _, ops = _ops()
    ops.bump_weight_epoch()
    num, ref = _numbers(c.n * c.r, c.din, c.h), _bwd_ref(c)
    runs = []
    for db1 in (False, True):
        what = f"bwd {_name(c)}{' db1' if db1 else ''}"
        got, cnt, (tiles, sums) = _bwd_once(c, what, db1)
        if c.dx:
            _rel(got.dx, ref.dx, f"{what} dx", c.fam)
        for k in CELL_W:
            _rel(got.dw[k], num.pre_w[k].double() + ref.dw[k], f"{what} dw_{k}", c.fam)
        for k in CELL_B:
            want = num.pre_b[k].double() + (ref.db[k] if (db1 or k.endswith("0")) else 0.0)
            _rel(got.db[k], want, f"{what} db_{k}", c.fam)
        for k in ("dhp", "dzp", "drp"):
            _rel(got.scratch[k], ref.scratch[k], f"{what} {k}", c.fam)
        if c.dx or c.reassoc is False:      # the da / dxp chain leaves the whole dxp behind
            _rel(got.scratch["dxp"], ref.scratch["dxp"], f"{what} dxp", c.fam)
        launches = 4 if c.dx else 3
        assert cnt["generic_large"] == 0 and cnt["generic"] == c.generic and cnt["fast"] == launches - c.generic, \
            f"{what}: expected {launches - c.generic} fast and {c.generic} generic launches, counted {cnt}"
        assert tiles == c.tiles, f"{what}: partial tiles {'were' if tiles else 'were not'} written to the workspace"
        if c.sums is not None:
            assert sums == c.sums, f"{what}: column-sum partials {'were' if sums else 'were not'} written to the workspace"
        runs.append(got)
    # the second call differs only in db_?1: everything else must come back bit for bit
    a, b = runs
    _same([a.dx] + [a.dw[k] for k in CELL_W] + [a.db[k] for k in ("z0", "r0", "h0")] + [a.scratch[k] for k in ("dhp", "dzp", "drp")],
          [b.dx] + [b.dw[k] for k in CELL_W] + [b.db[k] for k in ("z0", "r0", "h0")] + [b.scratch[k] for k in ("dhp", "dzp", "drp")],
          f"bwd {_name(c)}")
    return runs[1]


def B(*a, **kw):
    kw.setdefault("fam", "cell bwd 32x320")
    kw.setdefault("reassoc", None)
    return C(*a, **kw)


BWD_DX = [
    B(3, 20, 12, 20, sums=True),                                                             # gate_bwd_pre float4; three unsplit NT launches; TN k1
    B(3, 20, 12, 20, adj="weighted", sums=True),                                             # A_hat^T of asymmetric values
    B(3, 20, 12, 20, adj="keep", compact="real", sums=True),
    B(2, 100, 64, 64, tiles=True, sums=True, fam="cell bwd split-K finish"),                 # the accumulate pair x2(4): `accumulate` in nt_finish_kernel
    B(3, 20, 16, 128, tiles=True, sums=True, fam="cell bwd split-K finish"),                 # EPI_BWD_DRX in nt_finish_kernel, x2 / x4 / x2
    B(82, 100, 300, 300, tiles=True, sums=False, fam="cell bwd 64x160"),                     # narrow tile at sites 3, 4, 5; TN k24 via workspace, column sums fused
    B(3, 20, 12, 20, drop=0.2, sums=True),                                                   # drop_mode 3 on the dx epilogue; gather_rows without ids, with the mask
    B(3, 20, 12, 20, ids=True, sums=True),                                                   # gather_rows four-chain float4 with ids, no mask
    B(3, 20, 12, 20, ids=True, drop=0.2, sums=True),                                         # ... ids and mask
    B(3, 20, 12, 20, ids=True, drop=0.2, mis="x", sums=True),                                # table one float off: gather_rows' single-float loop at din % 4 == 0
    B(3, 20, 12, 20, mis="z", sums=True),                                                    # one of gate_bwd_pre's seven streams misaligned: scalar kernel
    B(3, 20, 6, 6, generic=4, sums=False, fam="cell bwd generic"),                           # 360 elements (a multiple of 4): gate_bwd_pre float4 on h = 6; atomic column sums
    B(3, 7, 6, 6, ids=True, generic=4, sums=False, fam="cell bwd generic"),                  # 126 elements: scalar gate_bwd_pre; gather_rows at din = 6
    B(3, 20, 12, 30, generic=4, sums=False, fam="cell bwd generic"),
    B(3, 20, 20, 12, sums=True),                                                             # din > h from x: the TN loader reads x itself
    B(3, 20, 20, 12, ids=True, generic=1, sums=True, fam="cell bwd generic"),                # din > h with ids: the TN loader gathers -> generic launch
]


@pytest.mark.parametrize("c", BWD_DX, ids=_name)
def test_bwd_with_input_gradient(c):
    """B1, B3.  The da / dxp chain: four GEMM launches (sweep: bwd dx ...)."""
    _bwd_case(c)


@pytest.mark.parametrize("c", [B(3, 20, 12, 20), B(2, 100, 64, 64, tiles=True, fam="cell bwd split-K finish")], ids=_name)
def test_bwd_with_input_gradient_fp32x3p(c):
    """The NT launches of B1 in fp32x3p at the same bound (the weight gradients stay exact fp32)."""
    _lib, _ = _ops()
    _lib.set_gemm_mode("fp32x3p")
    try:
        _bwd_case(c)
    finally:
        _, ops = _ops()
        ops.bump_weight_epoch()
        _lib.set_gemm_mode("fp32")


def test_bwd_dropout_with_din_above_h_is_rejected():
    """B1.  din > h with dropout: no scratch buffer is wide enough for the masked rows."""
    c = B(3, 20, 20, 12, drop=0.2)
    with pytest.raises(RuntimeError) as e:
        _bwd_once(c, "bwd rejected", False)
    assert "fused dropout needs din" in str(e.value), str(e.value)
    torch.cuda.synchronize()


BWD_NODX = [
    B(82, 100, 300, 300, ids=True, drop=0.2, dx=False, tiles=True, sums=False, reassoc=True, fam="cell bwd re-associated"),
    B(82, 100, 48, 160, ids=True, dx=False, tiles=True, sums=False, reassoc=True, fam="cell bwd re-associated"),
    B(3, 20, 12, 20, ids=True, dx=False, sums=True, reassoc=True, fam="cell bwd re-associated"),
    # back to the da / dxp chain: two NT launches and one TN launch
    B(3, 20, 20, 12, ids=True, dx=False, generic=1, sums=True, reassoc=False, fam="cell bwd generic"),       # din > h (the TN loader gathers)
    B(3, 20, 6, 8, ids=True, dx=False, generic=1, sums=True, reassoc=False, fam="cell bwd generic"),         # din % 4: dw_p's problem is not float4-shaped
    B(3, 20, 12, 30, ids=True, dx=False, generic=3, sums=False, reassoc=False, fam="cell bwd generic"),      # h % 4
    B(3, 20, 12, 20, ids=True, dx=False, ws="none", sums=False, reassoc=False),
    B(3, 20, 300, 300, ids=True, dx=False, ws="small", tiles=True, sums=None, reassoc=False, fam="cell bwd split-K finish"),   # 512 KiB < 20 h din = 1.8 MB; the first NT pair x4(5)
]


@pytest.mark.parametrize("c", BWD_NODX, ids=_name)
def test_bwd_without_input_gradient(c):
    """B2.  dx == NULL with ids: the re-associated path of DESIGN 4.20 at activation size, and each condition that sends the
    call back to the da / dxp chain.  Both take three GEMM launches; what tells them apart from outside is the dxp scratch: the
    chain leaves d loss / d xp in it, the re-associated path overwrites its first din columns' worth with A_hat X (sweep: bwd nodx ...)."""
    ctx = _workspace(None) if c.ws == "none" else _workspace(1) if c.ws == "small" else None
    if ctx is None:
        got = _bwd_case(c)
    else:
        with ctx:
            got = _bwd_case(c)
    ref = _bwd_ref(c)
    err = (_f64(got.scratch["dxp"]) - ref.scratch["dxp"]).abs().max().item() / (ref.scratch["dxp"].abs().max().item() + 1e-12)
    on_chain = bool(torch.isfinite(got.scratch["dxp"]).all()) and err <= TOL
    assert on_chain == (not c.reassoc), f"bwd {_name(c)}: dxp {'holds' if on_chain else 'does not hold'} d loss / d xp (err {err:.3e})"


# ----------------------------------------------------------------------------- bf16 entries
def _bf(t):
    return t.to(torch.bfloat16)


def _stage(got, ref, what, fam):
    """A stored bf16 stream against the float64 value of its stage: |err| <= 2^-8 |ref| + TOL max|ref| per element."""
    got, ref = _f64(got), _f64(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements not written / not finite"
    scale = ref.abs().max().item() + 1e-12
    bound = 2.0 ** -8 * ref.abs() + TOL * scale
    ratio = ((got - ref).abs() / bound).max().item()
    WORST[fam] = max(WORST.get(fam, 0.0), ratio)
    print(f"{what}: worst |err| / (2^-8 |ref| + 1e-4 max|ref|) = {ratio:.3f} (worst {fam}: {WORST[fam]:.3f})")
    assert ratio <= 1.0, f"{what}: {ratio:.3f} of the bf16 stage bound"


def _bf_inputs(c):
    G = _graph(c.n, c.r, c.counts)
    num = _numbers(c.n * c.r, c.din, c.h)
    w16 = {k: _bf(v) for k, v in num.w.items()}
    return G, num, w16, _bf(num.table)


def _bf_fwd(c):
    """gh_ggnn_cell_fwd_bf16: every stored stream stage by stage, out32 at TOL."""
    _lib, _ = _ops()
    G, num, w16, table16 = _bf_inputs(c)
    src, m_real, m_rows = _layout(c, G)
    what, fam = "bf16 fwd " + _name(c), c.fam
    f = _Fenced()
    adj = _adj_args(f, G, c.adj)
    row_ids = torch.from_numpy(G.ids.reshape(-1)[src].astype(np.int32))
    if c.ids:
        x, ids = f.put("table", table16, dtype=torch.bfloat16), row_ids.to(DEV)
    else:
        x, ids = f.put("x", table16[row_ids.long()], dtype=torch.bfloat16), None
    w = [f.put("w_" + k, w16[k], dtype=torch.bfloat16) for k in CELL_W]
    b = [f.put("b_" + k, num.b[k]) for k in CELL_B]
    st = {k: f.put(k, shape=(m_rows, c.h), dtype=torch.bfloat16) for k in OUT_STREAMS}
    out32 = f.put("out32", shape=(m_rows, c.h))
    goff = torch.from_numpy(G.plan["goff"]).to(DEV) if c.compact is not None else None
    _poison()
    _lib.gemm_path_counters(reset=True)
    _lib.call("gh_ggnn_cell_fwd_bf16", *[_lib.ptr(t) for t in adj], _lib.ptr(goff), m_real if goff is not None else 0, m_rows,
              _lib.ptr(x), _lib.ptr(ids), c.n, c.r, c.din, c.h, *[_lib.ptr(t) for t in w], *[_lib.ptr(t) for t in b],
              *[_lib.ptr(st[k]) for k in OUT_STREAMS], _lib.ptr(out32), float(c.drop), SEED, None, None, 0.0, 0, _lib.stream())
    torch.cuda.synchronize()
    cnt = _lib.gemm_path_counters()
    f.check(what)
    assert cnt["generic"] == 0 and cnt["fast"] == 3, f"{what}: counted {cnt}"
    # stage references from what the kernel stored upstream; rows in the padded layout for the aggregation
    total, tsrc = c.n * c.r, torch.from_numpy(src)
    W = {k: v.double() for k, v in w16.items()}
    B_ = {k: v.double() for k, v in num.b.items()}
    xs = table16[row_ids.long()].double()
    if c.drop:
        xs = xs * _mask(SEED, m_rows, c.din, c.drop)
    got = {k: _f64(st[k]) for k in ("xp", "a", "z", "rx")}
    got["rr"], got["hh"] = _f64(st["rr"][:m_real]), _f64(st["hh"][:m_real])
    _stage(st["xp"], xs @ W["p"].t(), f"{what} xp", fam)
    adj64 = torch.from_numpy(_adj64(G, c.adj))
    a_ref = (adj64 @ _pad(got["xp"], src, total).view(c.n, c.r, c.h)).reshape(total, c.h)[tsrc]
    a_rows = m_rows if m_rows == m_real else min(m_rows, ((m_real + 127) // 128 + 1) * 128)
    _stage(st["a"][:a_rows], a_ref[:a_rows], f"{what} a", fam)
    a = torch.where(torch.arange(m_rows)[:, None] < m_real, torch.nan_to_num(got["a"]), torch.zeros(()).double())      # padding rows: no neighbours
    xp = got["xp"]
    z_ref = torch.sigmoid(a @ W["z0"].t() + B_["z0"] + xp @ W["z1"].t() + B_["z1"])
    r_ref = torch.sigmoid(a @ W["r0"].t() + B_["r0"] + xp @ W["r1"].t() + B_["r1"])
    _stage(st["z"], z_ref, f"{what} z", fam)
    _stage(st["rr"][:m_real], r_ref[:m_real], f"{what} rr", fam)
    _stage(st["rx"], r_ref * xp, f"{what} rx", fam)
    h_ref = torch.tanh(a @ W["h0"].t() + B_["h0"] + got["rx"] @ W["h1"].t() + B_["h1"])
    _stage(st["hh"][:m_real], h_ref[:m_real], f"{what} hh", fam)
    out_ref = h_ref * got["z"] + xp * (1 - got["z"])
    _rel(out32, out_ref, f"{what} out32", fam + " fp32 outputs")
    _stage(st["out"], out_ref, f"{what} out", fam)
    return [st[k] for k in ("xp", "z", "rx", "out")] + [st["a"][:a_rows], st["rr"][:m_real], st["hh"][:m_real], out32]


def _bf_bwd(c):
    """gh_ggnn_cell_bwd_bf16 from the float64 forward rounded to bf16: dhp, dzp, drp stage by stage; dx, dw, db at TOL against
    float64 of the stored bf16 operands."""
    _lib, _ = _ops()
    G, num, w16, table16 = _bf_inputs(c)
    src, m_real, m = _layout(c, G, backward=True)
    what, fam = "bf16 bwd " + _name(c), c.fam
    total, tsrc = c.n * c.r, torch.from_numpy(src)
    row_ids = torch.from_numpy(G.ids.reshape(-1)[src].astype(np.int32))
    xs = table16[row_ids.long()].double()
    mask = _mask(SEED, m, c.din, c.drop) if c.drop else None
    if c.drop:
        xs = xs * mask
    adj64 = torch.from_numpy(_adj64(G, c.adj))
    w64 = {k: v.float() for k, v in w16.items()}
    fwd = cell_forward_f64(adj64, _pad(xs, src, total).view(c.n, c.r, c.din), w64, num.b)
    saved16 = {k: _bf(fwd[k].reshape(total, c.h)[tsrc].float()) for k in CELL_SAVED}
    g = num.g[:m]
    f = _Fenced()
    adj = _adj_args(f, G, c.adj)
    if c.ids:
        x, ids = f.put("table", table16, dtype=torch.bfloat16), row_ids.to(DEV)
    else:
        x, ids = f.put("x", table16[row_ids.long()], dtype=torch.bfloat16), None
    wt = [f.put("wt_" + k, w16[k].t().contiguous(), dtype=torch.bfloat16) for k in CELL_W]
    saved = [f.put(k, saved16[k], dtype=torch.bfloat16) for k in CELL_SAVED]
    gd = f.put("g", g)
    scratch = {k: f.put(k, shape=(m, c.h), dtype=torch.bfloat16) for k in ("dhp", "dzp", "drp", "dxp", "da")}
    dx = f.put("dx", shape=(m, c.din))
    dw = {k: f.put("dw_" + k, num.pre_w[k]) for k in CELL_W}
    db = {k: f.put("db_" + k, num.pre_b[k]) for k in CELL_B}
    goff = torch.from_numpy(G.plan["goff"]).to(DEV) if c.compact is not None else None
    _poison()
    _lib.gemm_path_counters(reset=True)
    _lib.call("gh_ggnn_cell_bwd_bf16", *[_lib.ptr(t) for t in adj], _lib.ptr(goff), m_real if goff is not None else 0,
              _lib.ptr(x), _lib.ptr(ids), c.n, c.r, c.din, c.h, *[_lib.ptr(t) for t in wt], *[_lib.ptr(t) for t in saved], _lib.ptr(gd),
              *[_lib.ptr(scratch[k]) for k in ("dhp", "dzp", "drp", "dxp", "da")], _lib.ptr(dx), *[_lib.ptr(dw[k]) for k in CELL_W],
              _lib.ptr(db["z0"]), _lib.ptr(db["r0"]), _lib.ptr(db["h0"]), _lib.ptr(db["z1"]), _lib.ptr(db["r1"]), _lib.ptr(db["h1"]),
              float(c.drop), SEED, _lib.stream())
    torch.cuda.synchronize()
    cnt = _lib.gemm_path_counters()
    f.check(what)
    assert cnt["generic"] == 0 and cnt["fast"] == 4, f"{what}: counted {cnt}"
    tiles, _ = _ws_written()
    assert tiles, f"{what}: the weight gradients did not go through the workspace"
    s = {k: v.double() for k, v in saved16.items()}
    gg = g.double()
    _stage(scratch["dhp"], gg * s["z"] * (1 - s["hh"] * s["hh"]), f"{what} dhp", fam)
    _stage(scratch["dzp"], gg * (s["hh"] - s["xp"]) * s["z"] * (1 - s["z"]), f"{what} dzp", fam)
    dhp, dzp, drp, dxp = (_f64(scratch[k]) for k in ("dhp", "dzp", "drp", "dxp"))
    W = {k: v.double() for k, v in w16.items()}
    _stage(scratch["drp"], (dhp @ W["h1"]) * s["xp"] * s["rr"] * (1 - s["rr"]), f"{what} drp", fam)
    assert bool(torch.isfinite(dxp).all()), f"{what}: dxp not written"
    fo = fam + " fp32 outputs"
    dx_ref = dxp @ W["p"]
    _rel(dx, dx_ref * mask if c.drop else dx_ref, f"{what} dx", fo)
    tn = lambda p, q: p.t() @ q
    dw_ref = {"p": tn(dxp, xs), "z0": tn(dzp, s["a"]), "z1": tn(dzp, s["xp"]), "r0": tn(drp, s["a"]), "r1": tn(drp, s["xp"]),
              "h0": tn(dhp, s["a"]), "h1": tn(dhp, s["rx"])}
    for k in CELL_W:
        _rel(dw[k], num.pre_w[k].double() + dw_ref[k], f"{what} dw_{k}", fo)
    for k, v in (("z", dzp), ("r", drp), ("h", dhp)):
        for i in "01":
            _rel(db[k + i], num.pre_b[k + i].double() + v.sum(0), f"{what} db_{k}{i}", fo)
    return [dx] + [dw[k] for k in CELL_W] + [db[k] for k in CELL_B] + [scratch[k] for k in ("dhp", "dzp", "drp", "dxp")]


BF16 = [
    C(82, 100, 48, 160, bf=True, fam="cell bf16 64x320"),                                         # the 64 x 320 bf16 tile through pass8
    C(82, 100, 256, 256, bf=True, adj="weighted", fam="cell bf16 128x256"),
    C(328, 100, 256, 256, bf=True, fam="cell bf16 256x256"),                                      # ping-pong NT tile and epilogue; ping-pong TN k31
    C(328, 100, 256, 256, bf=True, drop=0.5, fam="cell bf16 128x256"),                            # the projection with dropout falls back to 128 x 256
    C(82, 100, 64, 192, bf=True, ids=True, drop=0.5, fam="cell bf16 64x320"),                     # K no multiple of 64; gather_rows_bf16 8-wide with ids and mask
    C(90, 100, 48, 160, bf=True, ids=True, adj="keep", compact="tot", counts="tail", fam="cell bf16 64x320"),   # node-compact: 9000 rows of 8668 real
]


@pytest.mark.parametrize("c", BF16, ids=_name)
def test_bf16_forward(c):
    """C.  sweep: bf16 fwd ...  Two calls into separately prepared buffers agree bit for bit."""
    first = _bf_fwd(c)
    if c.n <= 90:
        _same([t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) for t in first],
              [t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) for t in _bf_fwd(c)], "bf16 fwd " + _name(c))


@pytest.mark.parametrize("c", BF16, ids=_name)
def test_bf16_backward(c):
    """C.  sweep: bf16 bwd ...  Two calls agree bit for bit: the weight gradients go through the workspace, the bias gradients
    ride in those launches."""
    first = _bf_bwd(c)
    if c.n <= 90:
        _same([t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) for t in first],
              [t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32) for t in _bf_bwd(c)], "bf16 bwd " + _name(c))


def test_bf16_few_rows_and_no_workspace_are_rejected():
    """C.  60 rows: the bf16 storage problems have no kernel on the 32 x 320 tile (the entries need >= 8192 rows).  Without a
    workspace the backward's bias gradients have no path."""
    c = C(3, 20, 8, 8, bf=True, fam="cell bf16 64x320")
    with pytest.raises(RuntimeError):
        _bf_fwd(c)
    torch.cuda.synchronize()
    with _workspace(None):
        with pytest.raises(RuntimeError) as e:
            _bf_bwd(C(82, 100, 48, 160, bf=True, fam="cell bf16 64x320"))
        torch.cuda.synchronize()
    assert "need the split-K workspace" in str(e.value), str(e.value)

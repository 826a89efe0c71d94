"""Every dispatch path of the concat attention (gh_concat_att_fwd / gh_concat_att_bwd: att_fwd_impl / att_bwd_impl of
csrc/dense_ops.hip, the three kernels of csrc/concat_att_ops.hip and the GEMM plans of csrc/gemm_ops.hip around them) against
the float64 restatement `_concat64` of tests/util.py, and the paths only gh_get_backward reaches (att_rows_bwd_kernel, the
dw_in prologue of att_dpre_kernel, the claim-offset du, the gate-head epilogue on dright) against the module-by-module path.

Part 1 calls the C-ABI directly.  Every operand and output sits in a NaN-fenced allocation of its own and the stream
workspace is NaN-filled before each call.  u, t, e, weights, attended, de, dpre, du, dleft, dright start as NaN and must come
back finite; dw1 / dw2 start from non-zero values and are compared with dw0 + the float64 gradient.  Inputs are 0.2 * randn on
fixed seeds, masks are those of test_gpu_kernel_paths._masks.  Bound: TOL = 1e-4 of the float64 result's largest entry.
Masked weights are exactly 0, weights sum to 1 within 1e-5, dright is compared on every row, and `de` of a pair with one
live row (identically 0 in float64) is held to TOL of the size of its cancelling terms.

Bit-identical outputs of two calls: everything but dw1 and dw2 always, and dw1 / dw2 too while a workspace is registered.
Batch::flush sends a TN product with several K chunks through partial tiles in the workspace and a fixed-order reduce; a
single chunk is one atomic add per element onto dw (ordered by nothing but itself).  Only WITHOUT a workspace do several
chunks meet in dw through floating-point atomics (M >= 512 rows), so the no-workspace cases leave dw1 / dw2 out.

Shape -> path, derived from att_fwd_impl, Batch (bn = 320, nt_split_plan: K tiles of 16, ks = min(tiles / 4, 256 / blocks),
needs ks >= 2 and a workspace; finish per workgroup from ks >= 16) and the three launchers.  (b, l, xl, dr, ha, heads):

  forward, the t / e product
    few          (4, 5, 8, 8, 8, 3)         32 x 320 tile, fused EPI_ATT epilogue (K = dr < 128: no split)
    big          (82, 100, 8, 8, 8, 3)      M = 8200 >= 8192: 64 x 320 tile (129 row tiles >= 96 blocks: no split)
    split_wave   (4, 5, 8, 128, 8, 3)       8 K tiles -> ks = 2, wave-per-row finish applies tanh / W2
    split_wg     (4, 5, 8, 1024, 8, 3)      64 K tiles -> ks = 16, workgroup-per-row finish
    nosplit      split_wave, no workspace   one launch, fused epilogue
    generic_ha   (4, 5, 8, 8, 6, 3)         ha % 4 != 0: generic kernel with EPI_ATT, for u's product too (forward only)
    generic_u    few, u one float off       fast_ok rule 10 (and rule 7 for u's own product)
    generic_w2   few, w2 one float off      fast_ok rule 10; u's product stays fast
    stored       (4, 5, 8, 8, 324, 3)       ha > 320: EPI_STORE in two column blocks + launch_att_finish
    stored_split (4, 5, 8, 128, 324, 3)     the same through the split-K plan (its finish writes e first, att_finish again)
    stored_big   (82, 100, 8, 8, 324, 3)    no workspace, M >= 8192: stored + att_finish on the 64-row tile
    parts2       (82, 100, 8, 8, 324, 3)    workspace: per-block partials of e, summed by att_softmax_fwd (n_parts = 2)
    parts3       (82, 100, 8, 8, 644, 3)    n_parts = 3; e comes back as the sum
    no_left      (4, 5, 0, 8, 8, 3)         u by memset
  forward, att_softmax_fwd_kernel<2|5|8>
    heads1..8    (4, 5, 8, 8, 8, h)         <2> 1, 2; <5> 3..5; <8> 6..8
    trip*        l = 32 / 33 at 2 heads, 24 / 25 at 5, 16 / 17 at 8: one trip of RB * 4 rows and one row more
    l1, l3, l65  l = 65: the lane loop of the softmax wraps
    dr4, dr512, dr516   one float4 column; one full column block; a second block that owns one column
    lds64k       (2, 496, 8, 4, 4, 8)       exactly 64 KB of dynamic LDS; l = 497 is refused by the host check
    compact*     rows per pair 1, l, 0, l // 2 through goff / rowg of g_plan; the 0-row pair's attended is NaN
    all_masked   pair 2 of (4, 5, 8, 8, 8, 3) has no live row: its weights and attended are NaN (forward only)
  backward (public entry: always the per-pair att_softmax_bwd_kernel<2|5|8>)
    every case above that has a backward; w256 (512, 3, 8, 4, 4, 3): the 256-thread launch
    l1, l8, l9, trip16/17, trip33: rows against two rows per wave and trip (8 waves: 16 rows)
    dr512 / dr516: register path / column loop; *_nogw: g_w == NULL
    lds_optin    (2, 5, 8, 2052, 4, 8)      65 984 B of dynamic LDS: the attribute opt-in
  backward, att_dpre_kernel (S4 float4 columns x RL row lanes)
    ha4 (S4 1, RL 256: lds64k, w256), ha300 (75 x 3), ha512 (128 x 2), ha516 (two slabs of 65 x 3, 61 threads idle),
    ha1024 (two slabs of 128 x 2); rows11/12/13 at ha = 300 around RB * RL = 12; ha = 1028 and ha % 4 != 0 are refused
    dw2: workspace partials + launch_reduce_wave; the no-workspace cases take the TN product (generic kernel at 3 heads:
    nosplit, stored_big; fast kernel at 8: ha300_nows)
  backward, the GEMMs: dright += dpre W1r on the 32-row tile (ha < 128), through the split plan (ha >= 128) and on the
    64-row tile (big, parts*); dleft; both halves of dw1 (the left half contracts over b: below 4 pairs -- lds64k, lds_optin --
    fast_ok rule 1 sends it to the generic kernel); no_left.

What a run itself verifies of a path: the forward's fast / generic launch counts (gh_gemm_path_counters) and whether the
workspace was written (split plans, e partials).  Template instances, chunk counts and slab shapes are not observable from
outside: for those the evidence is the mutation check listed in DESIGN.md 4.21."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_gpu_kernel_paths import _masks
from tests.util import (DEV, TOL, _WS_MODE, _concat64, _Fenced, _ops, _poison, _rel, _same, _workspace, _ws_written,
                        bits_equal, g_plan, rel_close)

pytestmark = pytest.mark.gpu

FAM = "concat_att"
KINDS = ("full", "prefix", "holes", "mod4")
OUT_FWD = ("u", "t", "e", "weights", "attended")
OUT_BWD = ("de", "dpre", "du", "dleft", "dright", "dw1", "dw2")


# ----------------------------------------------------------------------------- the cases
def S(label, b, l, xl, dr, ha, heads, **kw):
    """fwd: (fast, generic) launches of the forward and whether it writes the workspace; bwd: run the backward too."""
    d = dict(label=label, b=b, l=l, xl=xl, dr=dr, ha=ha, heads=heads, ws="default", mis=None, gw=True, rows=None,
             all_masked=False, bwd=True, fwd=(2 if xl else 1, 0), wsw=False, seed=len(label) * 7919 + b * 31 + l * 17 + dr + ha + heads)
    d.update(kw)
    return d


GEMM_SPECS = [
    S("few", 4, 5, 8, 8, 8, 3),
    S("big", 82, 100, 8, 8, 8, 3),
    S("split_wave", 4, 5, 8, 128, 8, 3, wsw=True),
    S("split_wg", 4, 5, 8, 1024, 8, 3, wsw=True),
    S("nosplit", 4, 5, 8, 128, 8, 3, ws="none"),
    S("generic_ha", 4, 5, 8, 8, 6, 3, fwd=(0, 2), bwd=False),
    S("generic_u", 4, 5, 8, 8, 8, 3, mis="u", fwd=(0, 2), bwd=False),
    S("generic_w2", 4, 5, 8, 8, 8, 3, mis="w2", fwd=(1, 1), bwd=False),
    S("stored", 4, 5, 8, 8, 324, 3),
    S("stored_split", 4, 5, 8, 128, 324, 3, wsw=True),
    S("stored_big", 82, 100, 8, 8, 324, 3, ws="none"),
    S("parts2", 82, 100, 8, 8, 324, 3, wsw=True),
    S("parts3", 82, 100, 8, 8, 644, 3, wsw=True),
    S("no_left", 4, 5, 0, 8, 8, 3),
    S("no_left_nogw", 4, 5, 0, 8, 8, 3, gw=False),
]
SOFTMAX_SPECS = [S(f"heads{h}", 4, 5, 8, 8, 8, h) for h in range(1, 9)] + [
    S("trip32", 4, 32, 8, 8, 8, 2), S("trip33", 4, 33, 8, 8, 8, 2),
    S("trip24", 4, 24, 8, 8, 8, 5), S("trip25", 4, 25, 8, 8, 8, 5),
    S("trip16", 4, 16, 8, 8, 8, 8), S("trip17", 4, 17, 8, 8, 8, 8),
    S("l1", 4, 1, 8, 8, 8, 5), S("l3", 4, 3, 8, 8, 8, 3), S("l65", 4, 65, 8, 8, 8, 3),
    S("l8", 4, 8, 8, 8, 8, 5), S("l9", 4, 9, 8, 8, 8, 5),
    S("dr4", 4, 5, 8, 4, 8, 3),
    S("dr512", 4, 5, 8, 512, 8, 3, wsw=True), S("dr516", 4, 5, 8, 516, 8, 3, wsw=True),
    S("dr512_nogw", 4, 9, 8, 512, 8, 6, wsw=True, gw=False), S("dr516_nogw", 4, 9, 8, 516, 8, 6, wsw=True, gw=False),
    S("lds64k", 2, 496, 8, 4, 4, 8),
    S("compact", 4, 7, 8, 8, 8, 3, rows=(1, 7, 0, 3)),
    S("compact_wide", 4, 9, 8, 516, 8, 6, rows=(1, 9, 0, 4), wsw=True),
    S("all_masked", 4, 5, 8, 8, 8, 3, all_masked=True, bwd=False),
]
BWD_SPECS = [
    S("w256", 512, 3, 8, 4, 4, 3),
    S("lds_optin", 2, 5, 8, 2052, 4, 8, wsw=True),
    S("ha300", 4, 5, 8, 8, 300, 3), S("ha512", 4, 5, 8, 8, 512, 3), S("ha516", 4, 5, 8, 8, 516, 3),
    S("ha1024", 4, 5, 8, 8, 1024, 3),
    S("rows11", 4, 11, 8, 8, 300, 3), S("rows12", 4, 12, 8, 8, 300, 3), S("rows13", 4, 13, 8, 8, 300, 3),
    S("ha300_nows", 4, 5, 8, 8, 300, 8, ws="none"),
]
SPECS = {s["label"]: s for s in GEMM_SPECS + SOFTMAX_SPECS + BWD_SPECS}
assert len(SPECS) == len(GEMM_SPECS) + len(SOFTMAX_SPECS) + len(BWD_SPECS)


def all_specs():
    return list(SPECS.values())


def make_case(spec):
    """Inputs of a case on the CPU (fp32) -- no reference, no device.  mask_padded (b, l) is what decides which rows are
    live: the mask kinds, rows beyond a pair's count in the compact layout, the one all-masked pair."""
    b, l, xl, dr, ha, heads = (spec[k] for k in ("b", "l", "xl", "dr", "ha", "heads"))
    gen = torch.Generator().manual_seed(spec["seed"])
    rn = lambda *shape: 0.2 * torch.randn(shape, generator=gen)
    c = SimpleNamespace(spec=spec, left=rn(b, xl) if xl else None, right=rn(b, l, dr), w1=rn(ha, xl + dr), w2=rn(heads, ha),
                        g_att=rn(b, dr, heads), g_w=rn(b, l, heads) if spec["gw"] else None, dw1_0=rn(ha, xl + dr),
                        dw2_0=rn(heads, ha), rows=spec["rows"], sel=None, plan=None)
    if c.rows is None:
        mask = _masks(b, l, KINDS)
        if spec["all_masked"]:
            mask[2] = 0
    else:
        mask = torch.zeros((b, l))
        for g, n in enumerate(c.rows):
            if n > 0:
                mask[g, :n] = _masks(1, n, (KINDS[g % 4],))[0]
        c.plan = g_plan(np.asarray(c.rows), l)
        c.m_real = int(c.plan["goff"][b])
        c.sel = torch.from_numpy(c.plan["src"][:c.m_real].astype(np.int64))
    c.mask_padded = mask
    c.dead_pairs = [g for g in range(b) if float(mask[g].sum()) == 0]
    # pairs with ONE live row: de = w (dw - sum_l w dw) = 1 * (dw - dw) is identically 0; its cancelling terms are |dw|
    c.single = {}
    for g in range(b):
        if float(mask[g].sum()) == 1:
            row = int(mask[g].argmax())
            dw = c.right[g, row].double() @ c.g_att[g].double()
            if c.g_w is not None:
                dw = dw + c.g_w[g, row].double()
            c.single[g] = float(dw.abs().max())
    c.de_floor = min(c.single.values()) if c.single else None
    return c


@functools.lru_cache(maxsize=None)
def _case(label):
    return make_case(SPECS[label])


@functools.lru_cache(maxsize=None)
def _reference(label):
    """float64 values of every saved tensor and output (all pairs), and -- from autograd over the pairs that have a live
    row -- every gradient, zeros on the rows of a pair without one; computed once per case."""
    c = _case(label)
    spec = c.spec
    d = lambda x: None if x is None else x.double()
    u, t, e, w, att = _concat64(d(c.left), d(c.right), c.mask_padded, d(c.w1), d(c.w2))
    ref = dict(u=u, t=t, e=e, weights=w, attended=att)
    if not spec["bwd"]:
        return ref
    live = torch.tensor([g for g in range(spec["b"]) if g not in c.dead_pairs])
    left = d(c.left)[live].requires_grad_(True) if c.left is not None else None
    right, w1, w2 = d(c.right)[live].requires_grad_(True), d(c.w1).requires_grad_(True), d(c.w2).requires_grad_(True)
    u2, t2, e2, w_2, att2 = _concat64(left, right, c.mask_padded[live], w1, w2)
    t2.retain_grad()
    e2.retain_grad()
    loss = (att2 * d(c.g_att)[live]).sum()
    if c.g_w is not None:
        loss = loss + (w_2 * d(c.g_w)[live]).sum()
    loss.backward()

    def full(x):
        out = torch.zeros((spec["b"],) + tuple(x.shape[1:]), dtype=torch.float64)
        out[live] = x
        return out
    dpre = t2.grad * (1.0 - t2.detach() ** 2)            # through the tanh: the gradient of the pre-activation
    ref.update(de=full(e2.grad), dpre=full(dpre), du=full(dpre.sum(1)), dright=full(right.grad),
               dleft=full(left.grad) if left is not None else None, dw1=d(c.dw1_0) + w1.grad, dw2=d(c.dw2_0) + w2.grad)
    return ref


def _rows(c, x):
    """(b, l, ...) of the reference -> the layout the device holds: (b, l, ...) or the compact rows."""
    return x if c.sel is None else x.reshape((-1,) + tuple(x.shape[2:]))[c.sel]


# ----------------------------------------------------------------------------- device runs
def _fwd_once(c, what):
    _lib, _ = _ops()
    sp = c.spec
    b, l, xl, dr, ha, heads = (sp[k] for k in ("b", "l", "xl", "dr", "ha", "heads"))
    f = _Fenced()
    m = b * l if c.sel is None else c.m_real
    dv = SimpleNamespace(f=f, m=m)
    dv.left = f.put("left", c.left) if c.left is not None else None
    dv.right = f.put("right", _rows(c, c.right) if c.sel is not None else c.right)
    dv.mask = f.put("mask", _rows(c, c.mask_padded) if c.sel is not None else c.mask_padded)
    dv.w1, dv.w2 = f.put("w1", c.w1), f.put("w2", c.w2, mis=sp["mis"] == "w2")
    dv.goff = torch.from_numpy(c.plan["goff"]).to(DEV) if c.plan else None
    dv.rowg = torch.from_numpy(c.plan["rowg"]).to(DEV) if c.plan else None
    dv.u = f.put("u", shape=(b, ha), mis=sp["mis"] == "u")
    dv.t, dv.e = f.put("t", shape=(m, ha)), f.put("e", shape=(m, heads))
    dv.weights = f.put("weights", shape=(m, heads) if c.sel is not None else (b, l, heads))
    dv.attended = f.put("attended", shape=(b, dr, heads))
    _poison()
    _lib.gemm_path_counters(reset=True)
    _lib.call("gh_concat_att_fwd", _lib.ptr(dv.left), _lib.ptr(dv.right), _lib.ptr(dv.mask), _lib.ptr(dv.goff), _lib.ptr(dv.rowg),
              m if c.plan else 0, b, l, xl, dr, ha, heads, _lib.ptr(dv.w1), _lib.ptr(dv.w2), _lib.ptr(dv.u), _lib.ptr(dv.t),
              _lib.ptr(dv.e), _lib.ptr(dv.weights), _lib.ptr(dv.attended), _lib.stream())
    torch.cuda.synchronize()
    dv.cnt = _lib.gemm_path_counters()
    f.check(what + " forward")
    dv.wsw = _ws_written()[0]
    return dv


def _bwd_once(c, dv, what, phase="both", prev=None):
    """phase: both | first (dw1 == NULL) | second (dright == NULL, on the buffers `prev` of a first call)."""
    _lib, _ = _ops()
    sp = c.spec
    b, l, xl, dr, ha, heads = (sp[k] for k in ("b", "l", "xl", "dr", "ha", "heads"))
    f = _Fenced()
    o = SimpleNamespace(f=f)
    w1t = f.put("w1t", c.w1.t().contiguous())
    g_att = f.put("g_att", c.g_att)
    g_w = f.put("g_w", _rows(c, c.g_w) if c.sel is not None else c.g_w) if c.g_w is not None else None
    if prev is None:
        o.de, o.dpre, o.du = f.put("de", shape=(dv.m, heads)), f.put("dpre", shape=(dv.m, ha)), f.put("du", shape=(b, ha))
        o.dleft = f.put("dleft", shape=(b, xl)) if xl else None
        o.dright = f.put("dright", shape=tuple(dv.right.shape))
        o.dw2 = f.put("dw2", c.dw2_0)
    else:
        o.de, o.dpre, o.du, o.dleft, o.dright, o.dw2 = prev.de, prev.dpre, prev.du, prev.dleft, prev.dright, prev.dw2
    o.dw1 = f.put("dw1", c.dw1_0)
    _poison()
    _lib.gemm_path_counters(reset=True)
    _lib.call("gh_concat_att_bwd", _lib.ptr(dv.left), _lib.ptr(dv.right), _lib.ptr(dv.goff), dv.m if c.plan else 0, b, l, xl, dr, ha,
              heads, _lib.ptr(w1t), _lib.ptr(dv.w2), _lib.ptr(dv.t), _lib.ptr(dv.weights), _lib.ptr(g_att), _lib.ptr(g_w),
              _lib.ptr(o.de), _lib.ptr(o.dpre), _lib.ptr(o.du), _lib.ptr(o.dleft), None if phase == "second" else _lib.ptr(o.dright),
              None if phase == "first" else _lib.ptr(o.dw1), _lib.ptr(o.dw2), _lib.stream())
    torch.cuda.synchronize()
    o.cnt = _lib.gemm_path_counters()
    f.check(what + " backward")
    if prev is not None:
        prev.f.check(what + " backward, the first call's buffers")
    dv.f.check(what + " backward, the forward's buffers")
    return o


# ----------------------------------------------------------------------------- checks
def _rel_nan(got, want, what):
    """_rel where the float64 result is finite; NaN exactly where it is NaN."""
    g, w = got.detach().double().cpu(), want.detach().double()
    nan = torch.isnan(w)
    assert torch.equal(torch.isnan(g), nan), f"{what}: NaN where float64 is finite, or finite where it is NaN"
    _rel(torch.where(nan, torch.zeros_like(g), g), torch.where(nan, torch.zeros_like(w), w), what, FAM)


def _check_fwd(c, dv, ref, what):
    sp = c.spec
    _rel(dv.u, ref["u"], f"{what} u", FAM)
    _rel(dv.t.view(_rows(c, ref["t"]).shape), _rows(c, ref["t"]), f"{what} t", FAM)
    _rel(dv.e.view(_rows(c, ref["e"]).shape), _rows(c, ref["e"]), f"{what} e", FAM)
    _rel_nan(dv.weights, _rows(c, ref["weights"]), f"{what} weights")
    _rel_nan(dv.attended, ref["attended"], f"{what} attended")
    mask, w = dv.mask, dv.weights
    alive = [g for g in range(sp["b"]) if g not in c.dead_pairs]
    if c.sel is None:
        assert bool((w[alive][mask[alive] == 0] == 0.0).all()), f"{what}: a masked weight is not exactly 0"
        sums = w[alive].double().sum(1)
    else:                                                # (a pair without rows has no weights at all)
        assert bool((w[mask == 0] == 0.0).all()), f"{what}: a masked weight is not exactly 0"
        rowg = dv.rowg[:dv.m].long()
        sums = torch.zeros((sp["b"], sp["heads"]), device=DEV, dtype=torch.float64).index_add_(0, rowg, w.double())[alive]
    assert bool(((sums - 1.0).abs() <= 1e-5).all()), f"{what}: weights do not sum to 1"
    want_fast, want_generic = sp["fwd"]
    assert dv.cnt["generic_large"] == 0 and (dv.cnt["fast"], dv.cnt["generic"]) == (want_fast, want_generic), \
        f"{what}: expected {want_fast} fast and {want_generic} generic launches, counted {dv.cnt}"
    want_ws = sp["wsw"] and _WS_MODE[0] == "default"
    assert dv.wsw == want_ws, f"{what}: the workspace {'was' if dv.wsw else 'was not'} written by the forward"


def _check_bwd(c, dv, o, ref, what, names=OUT_BWD):
    sp = c.spec
    for name in names:
        got, want = getattr(o, name), ref[name]
        if want is None:
            assert got is None
            continue
        if name in ("de", "dpre", "dright"):
            want = _rows(c, want)
            got = got.view(want.shape)
        _rel(got, want, f"{what} {name}", FAM, floor=c.de_floor if name == "de" else None)
    if "de" in names:
        for g, floor in c.single.items():            # a pair with one live row, next to pairs with more
            rows = (dv.rowg[:dv.m] == g) if c.sel is not None else None
            got = o.de[rows] if rows is not None else o.de.view(sp["b"], sp["l"], -1)[g]
            _rel(got, torch.zeros(got.shape, dtype=torch.float64), f"{what} de of the single-row pair {g}", FAM, floor=floor)
    # the generic kernel is the net for two products here: without a workspace dw2 = de^T t where `heads` rows are not
    # float4-shaped (heads % 4 != 0), and the left half of dw1 = du^T left where it contracts over b < 4 pairs (fast_ok rule 1)
    want_generic = (1 if _WS_MODE[0] == "none" and sp["heads"] % 4 and "dw2" in names else 0) + \
                   (1 if sp["xl"] and sp["b"] < 4 and "dw1" in names else 0)
    assert o.cnt["generic_large"] == 0 and o.cnt["generic"] == want_generic, \
        f"{what}: expected {want_generic} generic launches in the backward, counted {o.cnt}"


def _outs(dv, o=None, skip=()):
    xs = [getattr(dv, k) for k in OUT_FWD]
    if o is not None:
        xs += [None if k in skip else getattr(o, k) for k in OUT_BWD]
    return xs


class _mode:
    def __init__(self, ws):
        self.cm = _workspace(None) if ws == "none" else None

    def __enter__(self):
        if self.cm:
            self.cm.__enter__()

    def __exit__(self, *exc):
        if self.cm:
            self.cm.__exit__(*exc)
        return False


def _run_case(label, backward=True, identical=True):
    c, ref = _case(label), _reference(label)
    sp = c.spec
    what = f"concat_att {label} (b={sp['b']} l={sp['l']} xl={sp['xl']} dr={sp['dr']} ha={sp['ha']} heads={sp['heads']})"
    with _mode(sp["ws"]):
        runs = []
        for k in range(2 if identical else 1):
            dv = _fwd_once(c, what)
            o = _bwd_once(c, dv, what) if backward and sp["bwd"] else None
            if k == 0:
                _check_fwd(c, dv, ref, what)
                if o is not None:
                    _check_bwd(c, dv, o, ref, what)
            runs.append(_outs(dv, o, skip=("dw1", "dw2") if sp["ws"] == "none" else ()))
        if identical:
            _same(runs[0], runs[1], what)


# ----------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("label", [s["label"] for s in GEMM_SPECS])
def test_t_and_e_product_paths(label):
    _run_case(label, identical=SPECS[label]["b"] < 80)


@pytest.mark.parametrize("label", [s["label"] for s in SOFTMAX_SPECS])
def test_softmax_kernel_paths(label):
    _run_case(label)


@pytest.mark.parametrize("label", [s["label"] for s in BWD_SPECS])
def test_backward_paths(label):
    _run_case(label, identical=SPECS[label]["b"] < 80)


@pytest.mark.parametrize("label", ["few", "big", "split_wave", "split_wg", "stored", "stored_split", "parts2", "no_left"])
def test_fast_forward_paths_in_both_arithmetic_modes(label, arith_mode):
    c, ref = _case(label), _reference(label)
    what = f"concat_att {label} {arith_mode}"
    _check_fwd(c, _fwd_once(c, what), ref, what)


def test_forward_refuses_more_than_64k_of_lds_and_names_the_op():
    c = make_case(S("lds_over", 2, 497, 8, 4, 4, 8))
    with pytest.raises(RuntimeError, match=r"att_softmax_fwd: sequence 497 x heads 8 too large"):
        _fwd_once(c, "l = 497")
    torch.cuda.synchronize()


@pytest.mark.parametrize("ha", [6, 1028])
def test_backward_refuses_hidden_widths_the_forward_accepts(ha):
    """The forward takes ha % 4 != 0 (generic kernel, ha <= 320) and ha = 1028; att_dpre_kernel walks float4 columns of at
    most 256 per row, so the backward refuses both (include/get_hip.h says so)."""
    c = make_case(S(f"refused{ha}", 4, 5, 8, 8, ha, 3))
    dv = _fwd_once(c, f"ha = {ha}")
    with pytest.raises(RuntimeError, match=rf"att_dpre: attention hidden {ha} must be a multiple of 4 and <= 1024"):
        _bwd_once(c, dv, f"ha = {ha}")
    torch.cuda.synchronize()


@pytest.mark.parametrize("label", ["few", "ha300", "compact", "no_left"])
def test_two_phase_use_equals_one_call(label):
    """dw1 == NULL, then dright == NULL on the same buffers: together what one call gives (within TOL of float64, both), the
    first call leaves dw1 alone, the second leaves dright, dleft, dw2, de, dpre, du alone -- bit for bit."""
    c, ref = _case(label), _reference(label)
    what = f"concat_att {label} two-phase"
    dv = _fwd_once(c, what)
    one = _bwd_once(c, dv, what)
    _check_bwd(c, dv, one, ref, what + " (one call)")
    first = _bwd_once(c, dv, what, phase="first")
    bits_equal(first.dw1, c.dw1_0.to(DEV), what + ": dw1 after the dw1 == NULL call")
    _check_bwd(c, dv, first, ref, what + " (first call)", names=("de", "dpre", "du", "dleft", "dright", "dw2"))
    keep = {k: getattr(first, k).clone() for k in ("dright", "dleft", "dw2", "de", "dpre", "du") if getattr(first, k) is not None}
    second = _bwd_once(c, dv, what, phase="second", prev=first)
    for k, v in keep.items():
        bits_equal(getattr(second, k), v, f"{what}: {k} after the dright == NULL call")
    _rel(second.dw1, ref["dw1"], what + " dw1 (second call)", FAM)
    for k in OUT_BWD:
        if getattr(one, k) is not None:
            rel_close(getattr(second, k), getattr(one, k), TOL, f"{what}: {k} of the two calls against one call",
                      floor=c.de_floor if k == "de" else None)


# ----------------------------------------------------------------------------- 2. the paths only gh_get_backward reaches
def _cfg(**kw):
    from get_amd.synth import SynthConfig
    base = dict(batch=3, evd_counts=[2, 5, 1], emb_dim=32, hidden=32, vocab=200, n_article_src=20, n_claim_src=10, src_dim=16,
                len_right=38)
    base.update(kw)
    return SynthConfig(**base)


HEAD_SWEEP = [(1, 8), (2, 7), (4, 6), (6, 4), (7, 3), (8, 5)]


@pytest.mark.parametrize("native", [True, "compact"])
@pytest.mark.parametrize("heads", HEAD_SWEEP, ids=lambda h: f"w{h[0]}e{h[1]}")
def test_row_kernel_every_head_count(heads, native):
    """att_rows_bwd_kernel<CT> is instantiated for the exact head count: with these six configs and the golden ones both
    levels see every instance 1..8.  len_right = 38 is no multiple of 4, so a wave's run of rows crosses a pair boundary in
    the padded layout as well."""
    from tests.util import composite_vs_modules
    composite_vs_modules(_cfg(word_heads=heads[0], evd_heads=heads[1]), 900 + 10 * heads[0] + heads[1], native)


@pytest.mark.parametrize("native", [True, "compact"])
def test_row_kernel_evidence_level_over_512_columns(native):
    """hidden = 64, 8 word heads: Dre = 64 * 8 + 16 = 528 floats, two column ranges of 66 float4 (lanes 64, 65 live in the
    second chunk); the prologue of att_dpre adds the two partial dw."""
    from tests.util import composite_vs_modules
    composite_vs_modules(_cfg(hidden=64, word_heads=8), 931, native)


@pytest.mark.parametrize("native", [True, "compact"])
def test_row_kernel_word_level_over_512_columns_against_modules_and_oracle(native):
    """hidden = 516: the word level has two column ranges (65 + 64 float4, dw_ranges = 2), ha = 516 (wide-row finish with the
    claim row map, att_dpre in two slabs); the evidence level has Dre = 1048, three ranges.  Also against the oracle."""
    from tests.util import composite_vs_modules
    composite_vs_modules(_cfg(hidden=516, word_heads=2, evd_heads=2), 932, native, oracle=True)


@pytest.mark.parametrize("native", [True, "compact"])
def test_row_kernel_eight_and_five_heads_against_the_oracle(native):
    from tests.util import composite_vs_modules
    composite_vs_modules(_cfg(word_heads=8, evd_heads=5), 985, native, oracle=True)

"""Every dispatch path of the plain linear GEMMs (gh_linear_fwd / gh_linear_bwd of csrc/dense_ops.hip: the host planner `Batch` of
csrc/gemm_batch.hip with the NT, TN and generic MFMA kernels, the split-K finish and reduce kernels, the tiny-width kernels
and the column sums of csrc/stream_ops.hip) against float64 on the CPU, and gh_transpose / gh_transpose_batch /
gh_weights_refresh bit for bit.

The C-ABI entries are called directly.  Every operand and every output sits inside a larger NaN-filled allocation of its
own, at least 64 floats of NaN on either side, 16-byte aligned or -- in the misalignment cases -- exactly one float past
a 16-byte boundary.  The split-K / column-sum workspace is filled with NaN before every call.  So a row, a column or a
contraction element outside an operand that reaches a sum, and a partial tile that is summed without having been
written, come back as NaN; a store outside an output breaks a fence.  y and dx start as NaN and must come back finite;
dw and db start from non-zero values of the result's size and are compared with the float64 `dw0 + g^T x`, `db0 +
colsum(g)`.  Bound: 1e-4 of the float64 result's largest entry, on every written element.  gh_gemm_path_counters proves
which kernel family ran (fast / generic) and how many launches a call took; with the default workspace two calls into
separately prepared buffers must agree bit for bit wherever no floating-point atomic orders the sum.

Shapes are (m, k, n) of y[m][n] = x[m][k] w[n][k]^T + b.  The backward of a shape runs dX as an NT product with
(M, N, K) = (m, k, n) and dW as a TN product with output [n][k] contracted over m.  The plan named next to a shape is
the planner's (csrc/gemm_plan.h): tools/gemm_plan_sweep.cpp asserts each of them on the CPU (tests/test_gemm_plan_cpu.py);
launch_colsum3's were derived by reading it.  What a run itself
verifies of a plan: the kernel family and the launch count (path counters), and whether partial tiles and column-sum
partials were written to the workspace (its first float, and the first float of its column-sum tail, are no longer the
NaN they were filled with), which tells split from unsplit NT launches, the workspace from the atomic TN path and the
two column-sum kernels apart.  Chunk counts, tile shapes and the finish kernel's shape are not observable from outside:
for those the evidence is a mutation check on a scratch copy of the library (one change per path, the cases carrying
that label fail), listed in the commit that added this file.

Out of scope here, because gh_linear_* cannot reach them: the 64 x 160 narrow tile, the fused gate and attention
epilogues, dropout inside the loaders, two-segment problems and the bf16 storage tiles: tests/test_gpu_cell_paths.py reaches
them through the GGNN cell entries, at this file's bound and with this file's fences (the attention epilogues stay with the
attention path tests); GEMM modes 1 (bf16 operands) and 2 keep their own tests in tests/test_gpu_ops.py."""
import ctypes
import functools
import math
from types import SimpleNamespace

import pytest
import torch

from tests.util import DEV, _WS_MODE, _Fenced, _ops, _poison, _rel, _same, _workspace, _ws_written

pytestmark = pytest.mark.gpu

BLOCK = 320                      # columns per problem of a launch (Batch::bn)
MAX_PROBLEMS = 12                # problems per launch (GH_MAX_PROBLEMS)
# dW labels: tn = fast kernel, one K chunk, one atomic add per element onto dw; atomic = fast kernel, several chunks added
# with atomics (no or too small a workspace); ws = partial tiles in the workspace, reduce_partials_kernel
FAMILY = {"nt": "gemm NT", "split": "gemm NT split-K", "generic": "gemm generic", "ws": "gemm TN via workspace",
          "atomic": "gemm TN atomic", "tn": "gemm TN single chunk", "colsum": "column sums", "tiny": "tiny linear"}


# ----------------------------------------------------------------------------- inputs and the float64 reference
@functools.lru_cache(maxsize=None)
def _case(m, k, n):
    """x, g, b ~ randn, w ~ randn / sqrt(k) on a seed of the shape; dw0, db0 ~ randn of the results' rms; the float64
    results, computed once per shape."""
    gen = torch.Generator().manual_seed(1_000_003 * m + 1009 * k + n)
    x, w = torch.randn(m, k, generator=gen), torch.randn(n, k, generator=gen) / math.sqrt(k)
    b, g = torch.randn(n, generator=gen), torch.randn(m, n, generator=gen)
    x64, w64, b64, g64 = x.double(), w.double(), b.double(), g.double()
    y_nb = x64 @ w64.t()
    dw, db = g64.t() @ x64, g64.sum(0)
    dw0 = torch.randn(n, k, generator=gen) * dw.pow(2).mean().sqrt().float()
    db0 = torch.randn(n, generator=gen) * db.pow(2).mean().sqrt().float()
    return SimpleNamespace(m=m, k=k, n=n, x=x, w=w, wt=w.t().contiguous(), b=b, g=g, dw0=dw0, db0=db0, y=y_nb + b64,
                           y_nb=y_nb, dx=g64 @ w64, dw=dw0.double() + dw, db=db0.double() + db)


def _launches(width):
    """GEMM launches of one product whose output is `width` columns wide: 320-column problems, 12 per launch."""
    return -(-(-(-width // BLOCK)) // MAX_PROBLEMS)


def _check_counters(cnt, want_fast, want_generic, what):
    assert cnt["generic_large"] == 0, f"{what}: a large GEMM took the generic kernel ({cnt})"
    assert cnt["generic"] == want_generic and cnt["fast"] == want_fast, \
        f"{what}: expected {want_fast} fast and {want_generic} generic launches, counted {cnt}"


# ----------------------------------------------------------------------------- forward
def _fwd_once(c, bias, mis, what):
    _lib, _ = _ops()
    f = _Fenced()
    x, w = f.put("x", c.x, mis=mis == "x"), f.put("w", c.w, mis=mis == "w")
    b = f.put("bias", c.b, mis=mis == "bias") if bias else None
    y = f.put("y", shape=(c.m, c.n), mis=mis == "y")
    _poison()
    _lib.gemm_path_counters(reset=True)
    _lib.call("gh_linear_fwd", _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), c.m, c.k, c.n, _lib.stream())
    torch.cuda.synchronize()
    cnt = _lib.gemm_path_counters()
    f.check(what)
    return y, cnt, _ws_written()


def _fwd_case(m, k, n, label, bias=True, mis=None, identical=True):
    """label: tiny | nt | split | generic -- the kernel family of the launch(es), which names the error family too."""
    c = _case(m, k, n)
    what = f"fwd ({m}, {k}, {n}) {label}{'' if bias else ' no bias'}{f' {mis} misaligned' if mis else ''}"
    y, cnt, (tiles, _) = _fwd_once(c, bias, mis, what)
    assert tiles == (label == "split"), f"{what}: partial tiles {'were' if tiles else 'were not'} written to the workspace"
    _rel(y, c.y if bias else c.y_nb, f"{what} y", FAMILY[label])
    total = 0 if label == "tiny" else _launches(n)
    _check_counters(cnt, 0 if label == "generic" else total, total if label == "generic" else 0, what)
    if identical:
        _same((y,), (_fwd_once(c, bias, mis, what)[0],), what)
    return y


# ----------------------------------------------------------------------------- backward
def _bwd_once(c, outs, mis, with_w, what):
    _lib, _ = _ops()
    f = _Fenced()
    x, g = f.put("x", c.x, mis=mis == "x"), f.put("g", c.g, mis=mis == "g")
    wt = f.put("wt", c.wt, mis=mis == "wt")
    w = f.put("w", c.w) if with_w else None
    dx = f.put("dx", shape=(c.m, c.k), mis=mis == "dx") if "dx" in outs else None
    dw = f.put("dw", c.dw0, mis=mis == "dw") if "dw" in outs else None
    db = f.put("db", c.db0) if "db" in outs else None
    _poison()
    _lib.gemm_path_counters(reset=True)
    _lib.call("gh_linear_bwd", _lib.ptr(x), _lib.ptr(wt), _lib.ptr(w), _lib.ptr(g), c.m, c.k, c.n, _lib.ptr(dx), _lib.ptr(dw),
              _lib.ptr(db), _lib.stream())
    torch.cuda.synchronize()
    cnt = _lib.gemm_path_counters()
    f.check(what)
    return (dx, dw, db), cnt, _ws_written()


def _bwd_case(m, k, n, dxl=None, dwl=None, outs=("dx", "dw", "db"), mis=None, with_w=True, db_ws=None):
    """dxl: tiny | nt | split | generic, the dX product; dwl: tiny | tn | ws | atomic | generic | generic+, the dW product
    (FAMILY; generic+: the generic kernel with several K chunks, which adds them with atomics whatever the workspace);
    either is None where its output is not requested.  db_ws: whether the column sums take the workspace kernels;
    default: launch_colsum3's rule for the default workspace (n a multiple of 4, at most 1024 columns, g aligned).
    Two runs must agree bit for bit in every output that no floating-point atomic orders: dw unless several chunks are
    added atomically, db unless colsum_kernel adds more than one 256-row partial per column."""
    c = _case(m, k, n)
    what = (f"bwd ({m}, {k}, {n}) dx {dxl} dw {dwl}{'' if len(outs) == 3 else ' only ' + '+'.join(outs)}"
            f"{f' {mis} misaligned' if mis else ''}{'' if with_w else ' w NULL'}{'' if _WS_MODE[0] == 'default' else ' workspace ' + _WS_MODE[0]}")
    assert (dxl is not None) == ("dx" in outs) and (dwl is not None) == ("dw" in outs)
    tiny = n <= 8 and with_w
    assert all((label == "tiny") == tiny for label in (dxl, dwl) if label is not None)
    if db_ws is None:
        db_ws = not tiny and n % 4 == 0 and n <= 1024 and mis != "g" and _WS_MODE[0] == "default"
    got, cnt, (tiles, sums) = _bwd_once(c, outs, mis, with_w, what)
    dx, dw, db = got
    if dx is not None:
        _rel(dx, c.dx, f"{what} dx", FAMILY[dxl])
    if dw is not None:
        _rel(dw, c.dw, f"{what} dw", FAMILY[dwl.rstrip("+")])
    if db is not None:
        _rel(db, c.db, f"{what} db", FAMILY["tiny" if tiny else "colsum"])
    fast = generic = 0
    if not tiny:
        for label in (dxl, dwl):
            if label is not None and label.rstrip("+") == "generic":
                generic += _launches(k)
            elif label is not None:
                fast += _launches(k)
    _check_counters(cnt, fast, generic, what)
    assert tiles == (dxl == "split" or dwl == "ws"), f"{what}: partial tiles {'were' if tiles else 'were not'} written to the workspace"
    assert sums == (db is not None and db_ws), f"{what}: column-sum partials {'were' if sums else 'were not'} written to the workspace"
    again, _, _ = _bwd_once(c, outs, mis, with_w, what)
    db_one_add = tiny or db_ws or m <= 256
    _same((dx, None if dwl in ("atomic", "generic+") else dw, db if db_one_add else None), again, what)
    return got


# ============================================================================= A. forward
TINY_FWD = [(1, 1), (5, 63), (9, 130)]


@pytest.mark.parametrize("n", [1, 2, 8])
def test_fwd_tiny_kernel(n):
    """A1.  n <= 8: tiny_linear_fwd_kernel, one wave per row, four rows per workgroup: k below, at and above one 64-lane
    pass, a last workgroup of one row, with and without bias.  No GEMM launch."""
    for m, k in TINY_FWD:
        for bias in (True, False):
            _fwd_case(m, k, n, "tiny", bias=bias)


# (m, k, n), family of the launch, plan
FWD_FAST = [
    ((7, 20, 12), "nt"),            # A2  one 32 x 320 tile, few-row decode, K tail of one quad
    ((64, 4, 12), "nt"),            # A2  K = 4: a single quad
    ((33, 128, 16), "split"),       # A2  ks = 2, wave-per-row finish; the second row tile holds 1 row
    ((960, 300, 300), "split"),     # A3  ks = 4 (chunks of 5 K tiles, the last of 4), wave-per-row finish, 30 row tiles
    ((3, 960, 300), "split"),       # A3  ks = 15, one below the finish switch
    ((3, 1024, 300), "split"),      # A4  ks = 16 exactly: workgroup-per-row finish, 75 float4 columns = two column passes
    ((4, 2048, 772), "split"),      # A4  three problems of 320, 320 and 132 columns, ks = 32
    ((32, 3556, 300), "split"),     # A4  the head: ks = 45, wave quarters of 12, 12, 12 and 9, K % 16 = 4
    ((32, 4096, 768), "split"),     # A4  ks = 64, three problems of 320, 320 and 128 columns (80, 80 and 32 float4 columns)
    ((257, 68, 324), "nt"),         # A5  9 row tiles (XCD-dealt decode, padded grid), 1 row in the last; blocks of 320 and 4; K tail
    ((5, 8, 3844), "nt"),           # A6  13 column blocks, the last 4 wide: two launches
    ((8200, 20, 16), "nt"),         # A7  m >= 8192, 129 tiles of 64 rows = 0.17 rounds: the occupancy rule takes 257 tiles of 32 rows
    ((8200, 20, 960), "nt"),        # A7  three problems on the 64 x 320 tile (0.50 rounds), an 8-row M tail, a K tail
    ((2500, 32, 24), "nt"),         # (the B3 / B6 shape's forward: 79 row tiles, no split)
    ((260, 4, 1024), "nt"),         # (the B8 shape's forward: four problems, 9 row tiles)
]
FWD_GENERIC = [
    ((300, 22, 30), None),          # A8  k % 4 and n % 4
    ((50, 3, 12), None),            # A8  K < 4
    ((40, 16, 13), None),           # A8  n % 4
    ((40, 16, 12), "x"), ((40, 16, 12), "w"), ((40, 16, 12), "bias"), ((40, 16, 12), "y"),   # A8 each alone one float off
    ((8200, 6, 962), None),         # A8  generic on the 64-row configuration (0.67 rounds), four problems, the last 2 wide
    ((2500, 30, 22), None),         # (the B5 shape's forward)
]


def _ids(cases):
    return ["-".join(str(v) for v in c[0]) + (f"-{c[1]}" if c[1] else "") for c in cases]


@pytest.mark.parametrize("shape,label", FWD_FAST, ids=_ids(FWD_FAST))
def test_fwd_fast_paths(shape, label, arith_mode):
    """A2 - A7: the NT MFMA kernel, unsplit and split over K, in exact fp32 and in fp32x3p at the same bound."""
    _, ops = _ops()
    ops.bump_weight_epoch()
    _fwd_case(*shape, label)
    if shape == (257, 68, 324):
        _fwd_case(*shape, label, bias=False)          # B9: the bias-free forward


@pytest.mark.parametrize("shape,mis", FWD_GENERIC, ids=_ids(FWD_GENERIC))
def test_fwd_generic_kernel(shape, mis, arith_mode):
    """A8: K tails, K < 4, n % 4 != 0 and each operand alone misaligned send the launch to gemm_kernel<.., false>."""
    _, ops = _ops()
    ops.bump_weight_epoch()
    _fwd_case(*shape, "generic", mis=mis)
    if mis is not None:
        _fwd_case(*shape, "nt")                        # the same shape aligned is a fast launch


@pytest.mark.parametrize("ws", [None, 1], ids=["no-workspace", "1MiB"])
def test_fwd_split_plan_refused_for_lack_of_workspace(ws, arith_mode):
    """A9.  (32, 3556, 300) needs 45 partial tiles = 1.7 MB, (960, 300, 300) 4 = 4.6 MB: with no workspace or 1 MiB the
    plan is refused and one unsplit launch gives the same result."""
    _, ops = _ops()
    ops.bump_weight_epoch()
    with _workspace(ws):
        for shape in ((32, 3556, 300), (960, 300, 300)):
            _fwd_case(*shape, "nt")


# ============================================================================= B. backward
# A2 - A8's shapes with dx, dw and db: (m, k, n), dX family, dW family
BWD_OF_FWD = [
    ((7, 20, 12), "nt", "tn"),
    ((64, 4, 12), "nt", "tn"),              # dX 4 columns wide; dW [12][4]
    ((33, 128, 16), "nt", "tn"),
    ((960, 300, 300), "split", "ws"),           # B3  dW: 3 chunks of 320, 5 row tiles with the last 44 rows high.  B8: 75 float4 columns, 3 row lanes
    ((3, 960, 300), "split", "generic"),        # dX three problems, ks = 4; dW contraction of 3
    ((3, 1024, 300), "split", "generic"),       # B5  dW contraction below 4; dX four problems, the last 64 wide
    ((4, 2048, 772), "split", "tn"),        # dX seven problems, ks = 10; dW contraction of exactly 4, 13 row tiles x 7 problems
    ((32, 3556, 300), "split", "tn"),       # B4  dW 12 problems in one launch; dX 12 problems, the last 36 wide, ks = 4
    ((32, 4096, 768), "split", "tn"),       # dX and dW 13 problems each: two launches each
    ((257, 68, 324), "split", "tn"),        # dX ks = 5 over 9 row tiles (XCD-dealt decode with a split)
    ((5, 8, 3844), "split", "tn"),          # dX ks = 49, workgroup-per-row finish of 2 float4 columns; dW 61 row tiles; db 961 float4 columns: atomic
    ((8200, 20, 16), "nt", "ws"),               # dX 257 tiles of 32 rows; dW 24 chunks of 352
    ((8200, 20, 960), "nt", "ws"),              # dW 15 row tiles x 24 chunks
    ((300, 22, 30), "generic", "generic"),      # B5
    ((50, 3, 12), "generic", "generic"),        # dX 3 columns wide, dW [12][3]
    ((40, 16, 13), "generic", "generic"),
    ((8200, 6, 962), "generic", "generic+"),    # dW 16 row tiles x 24 chunks on atomics; db atomic
]
BWD_TN = [
    ((2500, 32, 24), "nt", "ws"),               # B3  9 chunks of 288: the reduce kernel's 8-wide loop plus one; the last chunk ends in a 4-row tile
    ((4000, 16, 12), "nt", "ws"),               # B3  16 chunks of 256
    ((8448, 12, 20), "nt", "ws"),               # B3  32 chunks of 272, the last of 16 rows; column sums at 128 rows per block
    ((5, 3844, 12), "nt", "tn"),            # B4  13 problems: two launches (dX too)
    ((2500, 30, 22), "generic", "generic+"),    # B5  generic with 9 chunks, atomics
    ((260, 4, 1024), "split", "tn"),        # B8  256 float4 columns, the last width of the workspace column sum; dX ks = 16
    ((260, 4, 1028), "split", "tn"),        # B8  257: the atomic colsum_kernel, two row blocks
]


def _ids3(cases):
    return ["-".join(str(v) for v in c[0]) for c in cases]


@pytest.mark.parametrize("shape,dxl,dwl", BWD_OF_FWD + BWD_TN, ids=_ids3(BWD_OF_FWD + BWD_TN))
def test_bwd_all_outputs(shape, dxl, dwl):
    """B (A2 - A8's shapes), B3, B4, B5, B8: dx, dw and db in one call, exact fp32."""
    _bwd_case(*shape, dxl, dwl)


@pytest.mark.parametrize("shape,dxl,dwl", BWD_OF_FWD + BWD_TN, ids=_ids3(BWD_OF_FWD + BWD_TN))
def test_bwd_dx_in_both_arithmetic_modes(shape, dxl, dwl, arith_mode):
    """The dX products of every backward shape alone (wt is the NT kernel's B operand), in exact fp32 and in fp32x3p."""
    _, ops = _ops()
    ops.bump_weight_epoch()
    _bwd_case(*shape, dxl, None, outs=("dx",))


@pytest.mark.parametrize("n", [1, 2, 8])
def test_bwd_tiny_kernel(n):
    """B1.  n <= 8 with w given: tiny_linear_bwd_kernel, a thread per column of x (k below, just above and at two 64-thread
    workgroups plus 2), eight rows in flight with a last group of 1, all outputs and each of dx, dw, db alone NULL."""
    for m, k in [(1, 1), (9, 65), (17, 130)]:
        for outs in (("dx", "dw", "db"), ("dw", "db"), ("dx", "db"), ("dx", "dw")):
            _bwd_case(m, k, n, "tiny" if "dx" in outs else None, "tiny" if "dw" in outs else None, outs=outs)


@pytest.mark.parametrize("n,label", [(2, "generic"), (4, "fast"), (8, "fast")])
def test_bwd_without_w_contracts_two_to_eight_on_the_mfma_kernels(n, label):
    """B2.  w == NULL with n <= 8 skips the tiny kernel.  n = 2: K < 4 for dX and I % 4 for dW, both generic; n = 4 and 8:
    fast kernels with a K tile one or two quads deep (dX) and a 4- or 8-row output (dW)."""
    generic = label == "generic"
    _bwd_case(40, 16, n, "generic" if generic else "nt", "generic" if generic else "tn", with_w=False)


@pytest.mark.parametrize("mis,dxl,dwl", [("x", "nt", "generic"), ("g", "generic", "generic"), ("dw", "nt", "generic"),
                                         ("wt", "generic", "tn"), ("dx", "generic", "tn")])
def test_bwd_misaligned_operand_takes_generic_kernel(mis, dxl, dwl):
    """B5.  (40, 16, 12) with one operand one float past a 16-byte boundary: the product that reads or writes it runs on
    the generic kernel, the other stays fast; a misaligned g also sends db to the atomic colsum_kernel (85 row lanes on
    the workspace path otherwise, B8)."""
    got = _bwd_case(40, 16, 12, dxl, dwl, mis=mis)
    aligned = _bwd_case(40, 16, 12, "nt", "tn")
    for name, a, b in zip(("dx", "dw", "db"), got, aligned):
        _rel(a, b.cpu(), f"bwd (40, 16, 12) {mis} misaligned vs aligned {name}", FAMILY["generic"])


def test_bwd_without_workspace_adds_chunks_atomically():
    """B6.  (2500, 32, 24) without a workspace: the fast TN kernel adds its 9 chunks into dw with fp32 atomics, db goes
    through colsum_kernel (10 row blocks)."""
    with _workspace(None):
        _bwd_case(2500, 32, 24, "nt", "atomic")


def test_bwd_with_a_small_workspace_adds_chunks_atomically():
    """B7.  (2560, 300, 300) with 1 MiB: ten chunks of 256 need 3.6 MB of partial tiles, so atomics; the dX split plan
    (4 x 3 MB) is refused too; the column-sum tail (64 KB) is too small for 160 row blocks."""
    with _workspace(1):
        _bwd_case(2560, 300, 300, "nt", "atomic", db_ws=False)          # db: 160 row blocks need 576 KB
        _bwd_case(32, 3556, 300, "nt", "tn", db_ws=True)                # A9's shapes: dX plan refused (1.8 MB, 4.6 MB); one dW chunk; db: 2 row blocks
        _bwd_case(960, 300, 300, "nt", "atomic", db_ws=False)           # ... three chunks (1.08 MB) added atomically; db: 60 row blocks need 216 KB


def test_bwd_column_sums():
    """B8.  launch_colsum3 alone (db only): 3 float4 columns x 85 row lanes with one idle thread, 75 x 3 with 31 idle
    threads, 256 x 1 (the last width of the workspace path), 257 (atomic kernel, two row blocks), 128 rows per block
    above 8192 rows, a width that is no multiple of 4."""
    for shape in ((40, 16, 12), (960, 300, 300), (260, 4, 1024), (260, 4, 1028), (8448, 12, 20), (300, 22, 30)):
        _bwd_case(*shape, outs=("db",))


@pytest.mark.parametrize("outs", [("dx",), ("dw",), ("db",)], ids=["dx", "dw", "db"])
def test_bwd_output_subsets(outs):
    """B9.  (257, 68, 324) with one output requested: the other products are not launched."""
    _bwd_case(257, 68, 324, "split" if outs == ("dx",) else None, "tn" if outs == ("dw",) else None, outs=outs)


# ============================================================================= C. transposes
def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _exact(got, want, what):
    assert bool(torch.isfinite(got).all()), f"{what}: not every element was written"
    assert torch.equal(_bits(got), _bits(want.to(DEV))), f"{what}: differs from torch"


def _matrix(rows, cols, seed):
    return torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed))


def _ptrs(ts):
    return ctypes.cast((ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts]), ctypes.c_void_p)


def _ints(vs):
    return ctypes.cast((ctypes.c_int * len(vs))(*vs), ctypes.c_void_p)


@pytest.mark.parametrize("rows,cols", [(1, 1), (2, 300), (33, 31), (64, 64), (300, 3556)])
def test_transpose(rows, cols):
    """gh_transpose: one element, two rows, one more and one fewer than a 32 x 32 tile, whole tiles, the head layer."""
    _lib, _ = _ops()
    src = _matrix(rows, cols, 7 * rows + cols)
    f = _Fenced()
    w, wt = f.put("w", src), f.put("wt", shape=(cols, rows))
    _lib.call("gh_transpose", _lib.ptr(w), _lib.ptr(wt), rows, cols, _lib.stream())
    torch.cuda.synchronize()
    f.check(f"transpose {rows} x {cols}")
    _exact(wt, src.t().contiguous(), f"transpose {rows} x {cols}")


# 33 matrices = two launches (32 + 1): float4-shaped ones (single tile, many tiles, a partial last tile in either direction),
# rows % 4 != 0, cols % 4 != 0, both, one element, and a float4-shaped one with a misaligned source (index 5)
BATCH_SHAPES = [(4, 4), (32, 32), (64, 96), (300, 300), (36, 100), (64, 64), (33, 31), (2, 300), (300, 2), (1, 1), (30, 64),
                (64, 30), (100, 36), (8, 260), (260, 8), (1, 64), (64, 1)]
BATCH_MISALIGNED = 5


def _batch():
    shapes = [BATCH_SHAPES[i % len(BATCH_SHAPES)] for i in range(33)]
    shapes[32] = (68, 132)            # the second launch's only matrix: 3 x 5 tiles, float4-shaped
    return shapes, [_matrix(r, c, 100 + i) for i, (r, c) in enumerate(shapes)]


def test_transpose_batch_of_33_matrices():
    """gh_transpose_batch with more matrices than one launch holds (32)."""
    _lib, _ = _ops()
    shapes, srcs = _batch()
    f = _Fenced()
    ws = [f.put(f"src{i}", s, mis=i == BATCH_MISALIGNED) for i, s in enumerate(srcs)]
    wts = [f.put(f"dst{i}", shape=(c, r)) for i, (r, c) in enumerate(shapes)]
    _lib.call("gh_transpose_batch", len(ws), _ptrs(ws), _ptrs(wts), _ints([r for r, _ in shapes]), _ints([c for _, c in shapes]),
              _lib.stream())
    torch.cuda.synchronize()
    f.check("transpose_batch")
    for i, (s, wt) in enumerate(zip(srcs, wts)):
        _exact(wt, s.t().contiguous(), f"transpose_batch matrix {i} {shapes[i]}")


@pytest.mark.parametrize("with_dst", [True, False], ids=["dst", "twins-only"])
def test_weights_refresh_with_bf16_twins(with_dst):
    """gh_weights_refresh: the fp32 transpose (or none: dst == NULL) and both bf16 twins, round to nearest even as torch
    rounds, on the float4 path and on the scalar path, 33 matrices."""
    _lib, _ = _ops()
    shapes, srcs = _batch()
    f = _Fenced()
    ws = [f.put(f"src{i}", s, mis=i == BATCH_MISALIGNED) for i, s in enumerate(srcs)]
    wts = [f.put(f"dst{i}", shape=(c, r)) for i, (r, c) in enumerate(shapes)] if with_dst else None
    w16 = [f.put(f"w16_{i}", shape=(r, c), dtype=torch.bfloat16) for i, (r, c) in enumerate(shapes)]
    t16 = [f.put(f"t16_{i}", shape=(c, r), dtype=torch.bfloat16) for i, (r, c) in enumerate(shapes)]
    _lib.call("gh_weights_refresh", len(ws), _ptrs(ws), _ptrs(wts) if with_dst else None, _ptrs(w16), _ptrs(t16),
              _ints([r for r, _ in shapes]), _ints([c for _, c in shapes]), _lib.stream())
    torch.cuda.synchronize()
    f.check("weights_refresh")
    for i, s in enumerate(srcs):
        what = f"weights_refresh matrix {i} {shapes[i]}"
        if with_dst:
            _exact(wts[i], s.t().contiguous(), f"{what} transpose")
        _exact(w16[i], s.to(torch.bfloat16), f"{what} bf16 twin")
        _exact(t16[i], s.t().contiguous().to(torch.bfloat16), f"{what} bf16 twin of the transpose")


def test_weights_refresh_of_no_matrix_writes_nothing():
    """n == 0: no launch, NULL arrays allowed; a destination stays NaN."""
    _lib, _ = _ops()
    f = _Fenced()
    wt = f.put("wt", shape=(4, 4))
    _lib.call("gh_weights_refresh", 0, None, None, None, None, None, None, _lib.stream())
    _lib.call("gh_transpose_batch", 0, None, _ptrs([wt]), None, None, _lib.stream())
    torch.cuda.synchronize()
    f.check("weights_refresh n = 0")
    assert bool(torch.isnan(wt).all())


@pytest.mark.parametrize("shape", [(5, 7), (8, 12)])
def test_weight_caches_serve_exact_copies_and_keep_their_addresses(shape):
    """ops.transposed and ops.bf16_twins over the kernels above: exact copies, a hit is the same object, an in-place update is
    seen, and a refresh rewrites the twins where they are (the kernels themselves: test_weights_refresh_with_bf16_twins)."""
    _, ops = _ops()
    ops.bump_weight_epoch()
    w = torch.nn.Parameter(torch.randn(shape, device="cuda"))
    wt = ops.transposed(w)
    _exact(wt, w.detach().t().contiguous(), "transposed")
    assert ops.transposed(w) is wt
    with torch.no_grad():
        w.add_(1)
    _exact(ops.transposed(w), w.detach().t().contiguous(), "transposed after an in-place update")
    w16, wt16 = ops.bf16_twins(w)
    _exact(w16, w.detach().to(torch.bfloat16), "bf16 twin")
    _exact(wt16, w.detach().t().contiguous().to(torch.bfloat16), "bf16 twin of the transpose")
    addresses = (w16.data_ptr(), wt16.data_ptr())
    with torch.no_grad():
        w.mul_(0.5)
    ops.refresh_transposes([w])
    again = ops.bf16_twins(w)
    assert (again[0].data_ptr(), again[1].data_ptr()) == addresses
    _exact(again[0], w.detach().to(torch.bfloat16), "bf16 twin after the refresh")
    _exact(again[1], w.detach().t().contiguous().to(torch.bfloat16), "bf16 twin of the transpose after the refresh")
    _exact(ops.transposed(w), w.detach().t().contiguous(), "transposed after the refresh")

"""Every path of the four recurrence entries (csrc/rnn_ops.hip: gh_lstm_seq_fwd, gh_lstm_seq_bwd, gh_gru_seq_fwd,
gh_gru_seq_bwd) against the per-step float64 restatement of tests/rnn_ref.py (lstm_steps64 / gru_steps64, checked on their own by
tests/test_rnn_cpu.py).  tests/test_gpu_rnn.py reaches these kernels through modules.LSTM / modules.GRU only, and
get_amd/ops/rnn.py always passes ldgx = G h, ldy = ldgy = dirs h, t_out >= t_in, a permutation for `order` and torch.empty
outputs; here the C-ABI entries are called directly with the arguments include/get_hip.h allows.

Buffers.  Every float operand, saved stream and output sits inside a NaN-filled allocation of its own (tests/util.py _Fenced);
outputs start as NaN; gx holds NaN at every t >= len and in every pitch gap, g_y likewise (the kernels guard those reads: a NaN
that reaches a result is a finding).  lens and order are plain int32 tensors.  After every call: the fences are intact; what the
header calls "not written" is still NaN (gates / c / an at t >= len, the gap columns of y, every row of a sequence that `order`
skips); what it calls exact zeros is == 0 (y and h_prev at t >= len and in rows [t_in, t_out), h_prev of the step that starts
from the zero state, the state of an empty sequence, dgates / dgx / da at t >= len); everything else is finite.  A second call
into separately prepared buffers is bit-identical in every output.

Forward: every stream from the original inputs.  Backward: the saved streams handed in are the float64 forward rounded to fp32,
not the kernel's own, so that a backward fault cannot hide behind a forward one; the reference gradients are autograd of the
restatement.  Chain: the forward's own saved streams go to the backward, then gh_linear_bwd (dx = NULL) forms dW_hh (and
db_hh for the GRU) from h_prev and dgates / da as get_amd/ops/rnn.py does -- the one place where the zero rows of h_prev and of
the gradient streams meet their consumer.

Bounds.  Per tensor tests.util.TOL (1e-4 of the float64 result's largest entry) through _rel, families lstm_fwd, lstm_bwd,
gru_fwd, gru_bwd; and elementwise 1e-5 + 1e-4 |want| through golden_ratio on every stream of every case -- admissible because
the restatement evaluated in fp32 on the CPU stays within half of it at every case here
(tests/test_rnn_cpu.py::test_fp32_evaluation_stays_within_half_the_elementwise_bound).  dW_hh and db_hh of the chain, sums over
n t_in rows, are held to TOL.

Cases: tests/rnn_ref.py (WIDTH_CASES, ARG_CASES, CHAIN_CASES); what each width reaches is derived from the RNN_* constants by
tests/test_rnn_paths_cpu.py.  Not covered: t_in beyond 7 (the drift over long sequences is test_gpu_rnn.py's bi_l70 and width
cases), n beyond 37, an `order` with repeated entries (two workgroups would own one row: undefined), more than one layer (a
module's matter), streams other than the current one."""
import pytest
import torch

from tests.rnn_ref import (ARG_CASES, BWD_STREAMS, CELLS, CHAIN_CASES, FWD_STREAMS, P, WIDTH_CASES, case_inputs, case_name,
                           case_reference)
from tests.util import DEV, NAN, WORST, _Fenced, _f64, _ops, _poison, _rel, _same, bits_equal, golden_ratio

pytestmark = pytest.mark.gpu

ATOL, RTOL = 1e-5, 1e-4
ELEM = {}                        # family -> worst elementwise fraction of ATOL + RTOL |want|


@pytest.fixture(params=list(CELLS))
def kind(request):
    return request.param


# ----------------------------------------------------------------------------- what a case looks like on the device
def _aux(kind):
    return "c" if kind == "lstm" else "an"


def _dead(lens, t):
    """(n, t) bool: the steps of each sequence at or beyond its clamped length."""
    return torch.arange(t)[None, :] >= lens[:, None]


def _first(lens, t, d):
    """(n, t) bool: the step of direction d that starts from the zero state."""
    at = (lens - 1) if d else torch.zeros_like(lens)
    return (torch.arange(t)[None, :] == at[:, None]) & (lens[:, None] > 0)


def _order(c, lens):
    """(the int32 order tensor or None, the rows no slot processes)."""
    if c.order == "none":
        return None, []
    if c.order == "identity":
        return torch.arange(c.n, dtype=torch.int32), []
    srt = torch.argsort(-lens, stable=True).to(torch.int32)
    skipped = []
    if c.order == "skip":
        skipped = [int(v) for v in srt[-2:]]
        srt[-2], srt[-1] = -1, c.n
    return srt, skipped


def _padded(src, ld, dead):
    """src (n, t, w) inside a (n, t, ld) NaN tensor, the dead rows NaN as well."""
    out = torch.full(src.shape[:2] + (ld,), NAN)
    out[:, :, :src.shape[2]] = src
    out[dead] = NAN
    return out


def _common(kind, c, f, w_mis=False):
    G, ref, inp = CELLS[kind].gates, case_reference(kind, c), case_inputs(kind, c)
    lens = ref["lens"]
    order, skipped = _order(c, lens)
    w = [f.put(f"w_hh{d}", inp["w"][d], mis=(w_mis and d == 0)) for d in range(c.dirs)] + [None] * (2 - c.dirs)
    return G, ref, inp, lens, (order.to(DEV) if order is not None else None), skipped, w, inp["lens"].to(DEV)


def _fwd_buffers(kind, c, w_mis=False):
    f = _Fenced()
    G, ref, inp, lens, order, skipped, w, dlens = _common(kind, c, f, w_mis)
    h, n, d = c.h, c.n, c.dirs
    ldgx, ldy = G * h + (3 if c.pitch else 0), d * h + (5 if c.pitch else 0)
    gx = [f.put(f"gx{k}", _padded(inp["gx"][k], ldgx, _dead(lens, c.t_in)), mis=c.mis) for k in range(d)] + [None] * (2 - d)
    b = ([f.put(f"b_hh{k}", inp["b"][k]) for k in range(d)] + [None] * (2 - d)) if kind == "gru" else None
    out = {"y": f.put("y", shape=(n, c.t_out, ldy), mis=c.mis), "h_n": f.put("h_n", shape=(d, n, h))}
    if kind == "lstm":
        out["c_n"] = f.put("c_n", shape=(d, n, h))
    for k, width in (("gates", G * h), (_aux(kind), h), ("h_prev", h)):
        out[k] = f.put(k, shape=(d, n, c.t_in, width)) if c.save else None
    return dict(f=f, gx=gx, w=w, b=b, lens=dlens, order=order, skipped=skipped, out=out, ldgx=ldgx, ldy=ldy)


def _fwd_call(kind, c, B, **over):
    """The entry with the case's arguments; `over` replaces scalar arguments by name (the refusals)."""
    _lib, _ = _ops()
    a = dict(ldgx=B["ldgx"], ldy=B["ldy"], n=c.n, t_in=c.t_in, t_out=c.t_out, h=c.h, dirs=c.dirs)
    a.update(over)
    o, p = B["out"], _lib.ptr
    head = [p(B["gx"][0]), p(B["gx"][1]), a["ldgx"], p(B["w"][0]), p(B["w"][1])]
    if kind == "gru":
        head += [p(B["b"][0]), p(B["b"][1])]
    tail = [p(B["lens"]), p(B["order"]), a["n"], a["t_in"], a["t_out"], a["h"], a["dirs"], p(o["y"]), a["ldy"], p(o["gates"]),
            p(o[_aux(kind)]), p(o["h_prev"]), p(o["h_n"])] + ([p(o["c_n"])] if kind == "lstm" else [])
    try:
        _lib.call(f"gh_{kind}_seq_fwd", *head, *tail, _lib.stream())
    finally:
        torch.cuda.synchronize()


def _bwd_buffers(kind, c, saved=None, w_mis=False):
    """saved: the forward's device streams (the chain); None: the float64 forward rounded to fp32."""
    f = _Fenced()
    G, ref, inp, lens, order, skipped, w, dlens = _common(kind, c, f, w_mis)
    h, n, d = c.h, c.n, c.dirs
    ldgy = d * h + (2 if c.pitch else 0)
    g_y = f.put("g_y", _padded(inp["g_y"][:, :, :d * h], ldgy, _dead(lens, c.t_out)), mis=c.mis) if c.gy else None
    g_hn = f.put("g_hn", inp["g_hn"][:d]) if c.ghn else None
    names = ("gates", _aux(kind)) + (("h_prev",) if kind == "gru" else ())
    sv = [saved[k] if saved is not None else f.put(k, ref[k].float()) for k in names]
    out = {k: f.put(k, shape=(d, n, c.t_in, G * h)) for k in BWD_STREAMS[kind]}
    return dict(f=f, w=w, lens=dlens, order=order, skipped=skipped, g_y=g_y, g_hn=g_hn, saved=sv, out=out, ldgy=ldgy)


def _bwd_call(kind, c, B, **over):
    _lib, _ = _ops()
    a = dict(ldgy=B["ldgy"], n=c.n, t_in=c.t_in, t_out=c.t_out, h=c.h, dirs=c.dirs)
    a.update(over)
    p = _lib.ptr
    try:
        _lib.call(f"gh_{kind}_seq_bwd", p(B["w"][0]), p(B["w"][1]), p(B["lens"]), p(B["order"]), a["n"], a["t_in"], a["t_out"], a["h"],
                  a["dirs"], p(B["g_y"]), a["ldgy"], p(B["g_hn"]), *[p(t) for t in B["saved"]],
                  *[p(B["out"][k]) for k in BWD_STREAMS[kind]], _lib.stream())
    finally:
        torch.cuda.synchronize()


# ----------------------------------------------------------------------------- what it must hold afterwards
def _check(got, want, zero, what, fam):
    """want: float64, NaN where nothing may be written; zero: where the header promises an exact zero."""
    got = _f64(got)
    assert got.shape == want.shape == zero.shape, (what, got.shape, want.shape, zero.shape)
    wn, gn = torch.isnan(want), torch.isnan(got)
    assert not bool((wn & ~gn).any()), f"{what}: {int((wn & ~gn).sum())} elements the header calls not written were written"
    assert not bool((gn & ~wn).any()), f"{what}: {int((gn & ~wn).sum())} elements were not written or are NaN"
    assert bool((got[zero] == 0).all()), f"{what}: {int((got[zero] != 0).sum())} of the promised exact zeros are not zero"
    live = ~wn
    if bool(live.any()):
        _rel(got[live], want[live], what, fam)
        ELEM[fam] = max(ELEM.get(fam, 0.0), golden_ratio(got[live], want[live], ATOL, RTOL, what))
        print(f"{what}: worst so far {fam}: {WORST[fam]:.3e} of the largest entry, {ELEM[fam]:.3f} of the elementwise bound")


def _fwd_expect(kind, c, B):
    """{stream: (want with NaN where not written, exact-zero mask)} in the shapes of the device buffers."""
    ref, (h, n, d) = case_reference(kind, c), (c.h, c.n, c.dirs)
    lens, skipped = ref["lens"], B["skipped"]
    y = torch.full((n, c.t_out, B["ldy"]), NAN, dtype=torch.float64)
    y[:, :, :d * h] = ref["y"]
    yz = torch.zeros_like(y, dtype=torch.bool)
    yz[:, :, :d * h] = _dead(lens, c.t_out)[:, :, None]
    exp = {"y": (y, yz)}
    empty = (lens == 0)[None, :, None].expand(d, n, h)
    for k in ("h_n", "c_n") if kind == "lstm" else ("h_n",):
        exp[k] = (ref[k].clone(), empty.clone())
    if c.save:
        dead = _dead(lens, c.t_in)
        for k in ("gates", _aux(kind)):
            exp[k] = (ref[k].clone(), torch.zeros_like(ref[k], dtype=torch.bool))
        hz = torch.stack([dead | _first(lens, c.t_in, k) for k in range(d)])[..., None].expand(d, n, c.t_in, h)
        exp["h_prev"] = (ref["h_prev"].clone(), hz.clone())
    for k, (want, zero) in exp.items():
        for r in skipped:
            if k == "y":
                want[r], zero[r] = NAN, False
            else:
                want[:, r], zero[:, r] = NAN, False
    return exp


def _bwd_expect(kind, c, B):
    ref, d = case_reference(kind, c), c.dirs
    dead = _dead(ref["lens"], c.t_in)[None, :, :, None]
    exp = {}
    for k in BWD_STREAMS[kind]:
        want = ref[k].clone()
        zero = dead.expand_as(want).clone() if (c.gy or c.ghn) else torch.ones_like(want, dtype=torch.bool)    # no gradient at all: all zeros
        for r in B["skipped"]:
            want[:, r], zero[:, r] = NAN, False
        exp[k] = (want, zero)
    return exp


def _fwd_case(kind, c):
    what, fam = f"{kind} fwd {case_name(c)}", f"{kind}_fwd"
    runs = []
    for _ in range(2):
        B = _fwd_buffers(kind, c)
        _fwd_call(kind, c, B)
        B["f"].check(what)
        runs.append(B)
    for k, (want, zero) in _fwd_expect(kind, c, runs[0]).items():
        _check(runs[0]["out"][k], want, zero, f"{what} {k}", fam)
    names = [k for k in FWD_STREAMS[kind] if runs[0]["out"][k] is not None]
    _same([runs[0]["out"][k] for k in names], [runs[1]["out"][k] for k in names], what)
    return runs[0]


def _bwd_case(kind, c, saved=None):
    what, fam = f"{kind} bwd {case_name(c)}", f"{kind}_bwd"
    runs = []
    for _ in range(2):
        B = _bwd_buffers(kind, c, saved)
        _bwd_call(kind, c, B)
        B["f"].check(what)
        runs.append(B)
    for k, (want, zero) in _bwd_expect(kind, c, runs[0]).items():
        _check(runs[0]["out"][k], want, zero, f"{what} {k}", fam)
    _same([runs[0]["out"][k] for k in BWD_STREAMS[kind]], [runs[1]["out"][k] for k in BWD_STREAMS[kind]], what)
    return runs[0]


def _rows_equal(a, b, names, n, skipped, what):
    """Every output of two runs bit for bit, but for the rows `skipped` of the first."""
    keep = [r for r in range(n) if r not in skipped]
    for k in names:
        if a[k] is None or b[k] is None:
            continue
        u, v = (a[k][keep], b[k][keep]) if k == "y" else (a[k][:, keep], b[k][:, keep])
        bits_equal(u, v, f"{what}: {k}")


BIT_EQUAL_TO_PLAIN = ("mis", "order-null", "order-identity", "order-skip", "inference")
FWD_CASES = WIDTH_CASES + [c for c in ARG_CASES if c.tag not in ("gy-null", "ghn-null", "both-null")]
BWD_CASES = WIDTH_CASES + [c for c in ARG_CASES if c.tag != "inference"]


@pytest.mark.parametrize("c", FWD_CASES, ids=case_name)
def test_forward(kind, c):
    """Section 3 of the file's cases, forward.  mis, the order variants and inference must also give the plain run's bits (the
    plain run: the same numbers, sorted order, aligned, unpitched, saving)."""
    got = _fwd_case(kind, c)
    if c.tag in BIT_EQUAL_TO_PLAIN:
        plain = _fwd_buffers(kind, P(c.h))
        _fwd_call(kind, P(c.h), plain)
        _rows_equal(got["out"], plain["out"], FWD_STREAMS[kind], c.n, got["skipped"], f"{kind} fwd {case_name(c)} against the plain run")
    if c.order == "skip":
        assert len(got["skipped"]) == 2


@pytest.mark.parametrize("h", [6, 300])
def test_saturated_gates_are_exactly_0_or_1(kind, h):
    """gx of +-100: every sigmoid gate exactly 0 or 1, the tanh gate exactly +-1 (the saturated case itself -- finite, inside
    both bounds -- is test_forward's and test_backward's).

    Before rnn_sigmoid sent denormal results to 0, every gate at -100 came back as an fp32 denormal (1.4e-45 .. 1.9e-42 over both
    cells at h = 6 and 300, about half of all sigmoid gates of the case: gfx950 keeps denormals and expf returns them), against
    the header's "exact 0 / 1"."""
    c = P(h, sat=True, tag="saturated")
    B = _fwd_buffers(kind, c)
    _fwd_call(kind, c, B)
    g = B["out"]["gates"].cpu()[:, ~_dead(case_reference(kind, c)["lens"], c.t_in)]
    sig = torch.ones(CELLS[kind].gates * h, dtype=torch.bool)
    sig[2 * h:3 * h] = False
    s, t = g[..., sig], g[..., ~sig]
    off = s[(s != 0) & (s != 1)]
    print(f"{kind} h{h} saturated: {off.numel()} of {s.numel()} sigmoid gates are neither 0 nor 1"
          + (f", in [{off.min().item():.3e}, {off.max().item():.3e}]" if off.numel() else "")
          + f"; {int((t.abs() != 1).sum())} of {t.numel()} tanh gates are not +-1")
    assert bool((t.abs() == 1).all()), "a saturated tanh gate is not exactly +-1"
    assert off.numel() == 0, "a saturated sigmoid gate is neither exactly 0 nor exactly 1"


@pytest.mark.parametrize("c", BWD_CASES, ids=case_name)
def test_backward(kind, c):
    """Section 3, backward, from the float64 forward rounded to fp32."""
    got = _bwd_case(kind, c)
    if c.tag in BIT_EQUAL_TO_PLAIN:
        plain = _bwd_buffers(kind, P(c.h))
        _bwd_call(kind, P(c.h), plain)
        _rows_equal(got["out"], plain["out"], BWD_STREAMS[kind], c.n, got["skipped"], f"{kind} bwd {case_name(c)} against the plain run")


@pytest.mark.parametrize("c", CHAIN_CASES, ids=case_name)
def test_chain_to_the_weight_gradient(kind, c):
    """forward -> backward on the forward's own saved streams -> gh_linear_bwd (dx = NULL) per direction, as ops/rnn.py chains
    them: dW_hh and, for the GRU, db_hh against float64 autograd of the restatement."""
    _lib, _ = _ops()
    G, ref = CELLS[kind].gates, case_reference(kind, c)
    fwd = _fwd_case(kind, c)
    bwd = _bwd_case(kind, c, saved=fwd["out"])
    dpre = bwd["out"]["dgates" if kind == "lstm" else "da"]
    f = _Fenced()
    dw = [f.put(f"dw{d}", torch.zeros(G * c.h, c.h)) for d in range(c.dirs)]
    db = [f.put(f"db{d}", torch.zeros(G * c.h)) if kind == "gru" else None for d in range(c.dirs)]
    _poison()
    for d in range(c.dirs):
        _lib.call("gh_linear_bwd", _lib.ptr(fwd["out"]["h_prev"][d]), None, None, _lib.ptr(dpre[d]), c.n * c.t_in, c.h, G * c.h, None,
                  _lib.ptr(dw[d]), _lib.ptr(db[d]), _lib.stream())
    torch.cuda.synchronize()
    f.check(f"{kind} chain {case_name(c)}")
    fwd["f"].check(f"{kind} chain {case_name(c)} (forward buffers)")
    bwd["f"].check(f"{kind} chain {case_name(c)} (backward buffers)")
    for d in range(c.dirs):
        _rel(dw[d], ref["dw"][d], f"{kind} chain {case_name(c)} dW_hh{d}", f"{kind}_bwd")
        if kind == "gru":
            _rel(db[d], ref["db"][d], f"{kind} chain {case_name(c)} db_hh{d}", f"{kind}_bwd")


# ----------------------------------------------------------------------------- refusals
def _all_nan(B, what):
    B["f"].check(what)
    for k, t in B["out"].items():
        assert t is None or bool(torch.isnan(t).all()), f"{what}: {k} was written"


FWD_REFUSALS = [("w-misaligned", {}, "w_hh must be 16-byte aligned"),
                ("saved-alone", {}, "saved together or not at all"),
                ("ldgx", {"ldgx": -1}, "a leading dimension is smaller than its row"),
                ("ldy", {"ldy": -1}, "a leading dimension is smaller than its row"),
                ("dirs3", {"dirs": 3}, "dirs=3 is neither 1 nor 2"),
                ("n0", {"n": 0}, "empty problem"),
                ("h1025", {"h": 1025}, "h=1025 exceeds the supported 1024"),
                ("t4097", {"t_in": 4097}, "t_in=4097 exceeds the supported 4096")]
BWD_REFUSALS = [r for r in FWD_REFUSALS if r[0] in ("w-misaligned", "dirs3", "n0", "h1025", "t4097")] + \
               [("ldgy", {"ldgy": -1}, "ldgy is smaller than dirs * h")]


@pytest.mark.parametrize("h", [6, 300])
@pytest.mark.parametrize("name,over,msg", FWD_REFUSALS, ids=[r[0] for r in FWD_REFUSALS])
def test_forward_refusals_write_nothing(kind, h, name, over, msg):
    """Each refusal names its reason and leaves every output and every fence NaN (a leading dimension of -1 stands for "one
    below the row")."""
    c = P(h)
    what = f"{kind} fwd refused {name} h{h}"
    B = _fwd_buffers(kind, c, w_mis=name == "w-misaligned")
    G = CELLS[kind].gates
    over = {k: ({"ldgx": G * h - 1, "ldy": c.dirs * h - 1}[k] if v == -1 else v) for k, v in over.items()}
    if name == "saved-alone":
        for drop in (("gates",), (_aux(kind),), ("h_prev",), ("gates", _aux(kind))):
            kept = dict(B["out"])
            B["out"] = {k: (None if k in drop else v) for k, v in kept.items()}
            with pytest.raises(RuntimeError) as e:
                _fwd_call(kind, c, B)
            assert msg in str(e.value), str(e.value)
            B["out"] = kept
    else:
        with pytest.raises(RuntimeError) as e:
            _fwd_call(kind, c, B, **over)
        assert msg in str(e.value), str(e.value)
    _all_nan(B, what)


@pytest.mark.parametrize("h", [6, 300])
@pytest.mark.parametrize("name,over,msg", BWD_REFUSALS, ids=[r[0] for r in BWD_REFUSALS])
def test_backward_refusals_write_nothing(kind, h, name, over, msg):
    c = P(h)
    B = _bwd_buffers(kind, c, w_mis=name == "w-misaligned")
    over = {k: (c.dirs * h - 1 if v == -1 else v) for k, v in over.items()}
    with pytest.raises(RuntimeError) as e:
        _bwd_call(kind, c, B, **over)
    assert msg in str(e.value), str(e.value)
    _all_nan(B, f"{kind} bwd refused {name} h{h}")

"""Every dispatch path of the query / tanh attention kernels (csrc/attention_ops.hip) and of the GAT / GCN-norm kernels
(csrc/encoder_ops.hip) against the float64 restatements of tests/util.py: float4 and scalar loads, every unit count per
lane, 1 to 4 bit words per adjacency row, the misaligned-operand fallback, the LDS opt-in above 64 KB.

The C-ABI entries are called directly wherever a kernel writes a buffer, into outputs this file fills with NaN first: an
element the header documents as written must come back finite and within 1e-4 of the float64 result's scale, an element
documented as not written must still be NaN, masked weights and the gradient rows of padded positions must be exactly
0, and two calls into separately NaN-filled buffers must be bit-identical.  Inputs are 0.2 * randn on fixed seeds."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.util import _gat_head64, _query64, _rel, _same, _tanh64

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def _ops():
    from get_amd import _lib, ops
    _lib.ensure_workspace(DEV)
    return _lib, ops


def _randn(gen, *shape):
    return 0.2 * torch.randn(shape, generator=gen)


def _dev(t):
    return t.float().contiguous().to(DEV)


def _off(t):
    """`t` on the device, placed one float into its allocation (4 bytes past a 16-byte boundary)."""
    buf = torch.empty(t.numel() + 1, device=DEV, dtype=torch.float32)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _place(t, misaligned):
    return _off(t) if misaligned else _dev(t)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def _masks(b, l, kinds):
    """kinds per sequence: full | prefix | holes (first row masked, the last row the only survivor of its wave: rows are
    dealt to the four waves round-robin) | mod4 (rows = 2 mod 4 masked, so one wave owns no row).  Never all-masked."""
    m = torch.ones((b, l))
    idx = torch.arange(l)
    for s in range(b):
        k = kinds[s % len(kinds)]
        if k == "prefix":
            m[s, max(1, (2 * l) // 3):] = 0
        elif k == "holes" and l > 1:
            m[s, 0] = 0
            m[s, (idx % 4 == (l - 1) % 4) & (idx != l - 1)] = 0
            if l > 8:
                m[s, 5] = 0
        elif k == "mod4":
            m[s, idx % 4 == 2] = 0
    assert bool((m.sum(1) > 0).all())
    return m


# ----------------------------------------------------------------------------- 2a. query attention
def _query_dev(q, right, mask, g_avg, g_w, mis=None):
    _lib, _ = _ops()
    b, l, d = right.shape
    qd, rd = _place(q, mis == "q"), _place(right, mis == "right")
    md, gad = _dev(mask), _dev(g_avg)
    gwd = _dev(g_w) if g_w is not None else None
    w, avg, dq, dr = _nan(b, l), _nan(b, d), _nan(b, d), _nan(b, l, d)
    _lib.call("gh_query_att_fwd", _lib.ptr(qd), _lib.ptr(rd), _lib.ptr(md), b, l, d, _lib.ptr(w), _lib.ptr(avg), _lib.stream())
    _lib.call("gh_query_att_bwd", _lib.ptr(qd), _lib.ptr(rd), _lib.ptr(w), _lib.ptr(gad), _lib.ptr(gwd), b, l, d, _lib.ptr(dq),
              _lib.ptr(dr), _lib.stream())
    torch.cuda.synchronize()
    return w, avg, dq, dr


def _query_ref(q, right, mask, g_avg, g_w):
    q64, r64 = q.double().requires_grad_(True), right.double().requires_grad_(True)
    avg, w = _query64(q64, r64, mask)
    loss = (avg * g_avg.double()).sum()
    if g_w is not None:
        loss = loss + (w * g_w.double()).sum()
    loss.backward()
    return w.detach(), avg.detach(), q64.grad, r64.grad


def _query_floor(q, right, mask, g_avg, g_w):
    """Size of the terms w_l dw_l right_l that cancel in dq when a sequence has one live row (l == 1), else None."""
    if right.shape[1] > 1:
        return None
    dw = (right.double() @ g_avg.double().unsqueeze(-1)).squeeze(-1) + (g_w.double() if g_w is not None else 0.0)
    return (dw.abs().unsqueeze(-1) * right.double().abs()).max().item()


def _query_check(got, want, mask, what, floor=None):
    w, avg, dq, dr = got
    for name, g, x in zip(("weights", "avg", "dq", "dright"), got, want):
        _rel(g, x, f"{what} {name}", "query_att", floor if name == "dq" else None)
    pad = (mask == 0).to(DEV)
    assert bool((w[pad] == 0.0).all()), f"{what}: a masked weight is not exactly 0"
    assert bool(((w.double().sum(1) - 1.0).abs() <= 1e-5).all()), f"{what}: weights do not sum to 1"
    assert bool((dr[pad] == 0.0).all()), f"{what}: dright of a padded row is not exactly 0"


def _query_case(d, l, seed, with_gw, b=4):
    gen = torch.Generator().manual_seed(seed)
    q, right = _randn(gen, b, d), _randn(gen, b, l, d)
    g_avg, g_w = _randn(gen, b, d), (_randn(gen, b, l) if with_gw else None)
    return q, right, _masks(b, l, ("full", "prefix", "holes", "mod4")), g_avg, g_w


# path (V, K) of GH_QATT_DISPATCH by width
QUERY_WIDTHS = [4, 256, 260, 512, 516, 1024, 1028, 2048, 1, 3, 254, 257, 2047]


@pytest.mark.parametrize("d", QUERY_WIDTHS)
def test_query_att_every_width_path(d):
    """<4,1> d 4, 256; <4,2> 260, 512; <4,4> 516, 1024; <4,8> 1028, 2048; <1,4> 1, 3, 254; <1,32> 257, 2047, each at
    l = 1, 3, 5, 67 (fewer rows than waves, a partial last round), one sequence per mask kind (b = 4), with g_w and with
    g_w == NULL."""
    for l in (1, 3, 5, 67):
        for with_gw in (True, False):
            case = _query_case(d, l, 1000 + d, with_gw)
            got = _query_dev(*case)
            what = f"query d={d} l={l} g_w={'yes' if with_gw else 'NULL'}"
            _query_check(got, _query_ref(*case), case[2], what, _query_floor(*case))
            _same(got, _query_dev(*case), what)


@pytest.mark.parametrize("d", [8, 260])
@pytest.mark.parametrize("mis", ["q", "right"])
def test_query_att_misaligned_operand_takes_scalar_path(d, mis):
    """q alone, or right alone, one float into its allocation: forward and backward fall back to the scalar kernels and
    give the aligned run's result (within the bound) and float64's."""
    for l in (3, 67):
        case = _query_case(d, l, 2000 + d, True)
        got, aligned, want = _query_dev(*case, mis=mis), _query_dev(*case), _query_ref(*case)
        what = f"query d={d} l={l} {mis} misaligned"
        _query_check(got, want, case[2], what)
        for name, g, a in zip(("weights", "avg", "dq", "dright"), got, aligned):
            _rel(g, a.cpu(), f"{what} vs aligned {name}", "query_att")


# ----------------------------------------------------------------------------- 2b. tanh attention
def _tanh_dev(pre, u, w2, mask, values, g_att, g_w, mis=None, dw2_init=None):
    _lib, _ = _ops()
    b, l, ha = pre.shape
    heads, dv = w2.shape[0], values.shape[2]
    pd, vd = _place(pre, mis == "pre"), _place(values, mis == "values")
    ud = _dev(u) if u is not None else None
    wd, md, gad = _dev(w2), _dev(mask), _dev(g_att)
    gwd = _dev(g_w) if g_w is not None else None
    t, w, att = _nan(b, l, ha), _nan(b, l, heads), _nan(b, heads, dv)
    _lib.call("gh_tanh_att_fwd", _lib.ptr(pd), _lib.ptr(ud), _lib.ptr(wd), _lib.ptr(md), _lib.ptr(vd), b, l, ha, heads, dv,
              _lib.ptr(t), _lib.ptr(w), _lib.ptr(att), _lib.stream())
    dpre, dvalues = _nan(b, l, ha), _nan(b, l, dv)
    du = _nan(b, ha) if u is not None else None
    dw2 = torch.zeros((heads, ha), device=DEV) if dw2_init is None else _dev(dw2_init)
    _lib.call("gh_tanh_att_bwd", _lib.ptr(t), _lib.ptr(wd), _lib.ptr(w), _lib.ptr(vd), _lib.ptr(gad), _lib.ptr(gwd), b, l, ha,
              heads, dv, _lib.ptr(dpre), _lib.ptr(du), _lib.ptr(dw2), _lib.ptr(dvalues), _lib.stream())
    torch.cuda.synchronize()
    return t, w, att, dpre, du, dw2, dvalues


def _tanh_ref(pre, u, w2, mask, values, g_att, g_w):
    p64, w64, v64 = (x.double().requires_grad_(True) for x in (pre, w2, values))
    u64 = u.double().requires_grad_(True) if u is not None else None
    att, w = _tanh64(p64, u64, w64, mask, v64)
    loss = (att * g_att.double()).sum()
    if g_w is not None:
        loss = loss + (w * g_w.double()).sum()
    loss.backward()
    t = torch.tanh(p64 if u64 is None else p64 + u64.unsqueeze(1)).detach()
    return t, w.detach(), att.detach(), p64.grad, (u64.grad if u64 is not None else None), w64.grad, v64.grad


TANH_NAMES = ("t", "weights", "attended", "dpre", "du", "dw2", "dvalues")


def _tanh_floors(pre, u, w2, mask, values, g_att, g_w):
    """At l == 1 the softmax has one element and dpre, du and dw2 are identically 0: the sizes of their cancelling terms
    w dw w2 (1 - t^2) and w dw t, bounded by max |dw| max |w2| and max |dw| (dw = g_w + g_att . values)."""
    if pre.shape[1] > 1:
        return {}
    dw = torch.einsum("bcv,blv->blc", g_att.double(), values.double()) + (g_w.double() if g_w is not None else 0.0)
    m = dw.abs().max().item()
    return {"dpre": m * w2.abs().max().item(), "du": m * w2.abs().max().item(), "dw2": m}


def _tanh_check(got, want, mask, what, dw2_init=None, floors=None):
    t, w, att, dpre, du, dw2, dvalues = got
    floors = floors or {}
    pad = (mask == 0).to(DEV)
    live = ~pad
    assert bool(torch.isnan(t[pad]).all()), f"{what}: a t row of a padded position was written"
    _rel(t[live], want[0][live.cpu()], f"{what} t", "tanh_att")
    for name, g, x in list(zip(TANH_NAMES, got, want))[1:]:
        if g is None:
            assert x is None
            continue
        if name == "dw2" and dw2_init is not None:
            x = x + dw2_init.double()
        _rel(g, x, f"{what} {name}", "tanh_att", floors.get(name))
    assert bool((w[pad] == 0.0).all()), f"{what}: a masked weight is not exactly 0"
    assert bool(((w.double().sum(1) - 1.0).abs() <= 1e-5).all()), f"{what}: weights do not sum to 1"
    assert bool((dpre[pad] == 0.0).all()) and bool((dvalues[pad] == 0.0).all()), \
        f"{what}: a gradient row of a padded position is not exactly 0"


def _tanh_case(ha, dv, heads, l, seed, with_u=True, with_gw=True, b=3):
    gen = torch.Generator().manual_seed(seed)
    pre, values, w2 = _randn(gen, b, l, ha), _randn(gen, b, l, dv), _randn(gen, heads, ha)
    u = _randn(gen, b, ha) if with_u else None
    g_att = _randn(gen, b, heads, dv)
    g_w = _randn(gen, b, l, heads) if with_gw else None
    return pre, u, w2, _masks(b, l, ("full", "prefix", "holes")), values, g_att, g_w


def _tanh_run(ha, dv, heads, l, with_u, with_gw, rerun=True, **kw):
    case = _tanh_case(ha, dv, heads, l, 3000 + 7 * ha + dv + 131 * heads + l, with_u, with_gw, **kw)
    got = _tanh_dev(*case)
    what = f"tanh ha={ha} dv={dv} heads={heads} l={l} u={'yes' if with_u else 'NULL'} g_w={'yes' if with_gw else 'NULL'}"
    _tanh_check(got, _tanh_ref(*case), case[3], what, floors=_tanh_floors(*case))
    if rerun:
        _same(got, _tanh_dev(*case), what)


TANH_HEADS = (1, 2, 4, 5, 8)
TANH_LENGTHS = (1, 3, 5, 70)
# float4 pairs, then scalar pairs (one and several 64-lane chunks, either width alone a multiple of 4)
TANH_PAIRS = [(4, 4), (8, 8), (256, 256), (260, 8), (8, 260), (516, 260),
              (7, 8), (8, 6), (64, 64), (65, 8), (8, 65), (130, 67)]
TANH_FULL_SWEEP = {(8, 8), (260, 8), (130, 67)}


@pytest.mark.parametrize("ha,dv", TANH_PAIRS)
def test_tanh_att_every_width_path(ha, dv):
    """Every (ha, dv) pair at 1, 2, 4, 5 and 8 heads: all of l = 1, 3, 5, 70 and all four u / g_w combinations at (8, 8),
    (260, 8) and (130, 67); elsewhere one l per head count (l = 3 at 5 heads, so l * heads is odd and the LDS split is
    padded) with u and g_w both given and both NULL."""
    k = TANH_PAIRS.index((ha, dv))
    for hi, heads in enumerate(TANH_HEADS):
        if (ha, dv) in TANH_FULL_SWEEP:
            for l in TANH_LENGTHS:
                for with_u in (True, False):
                    for with_gw in (True, False):
                        _tanh_run(ha, dv, heads, l, with_u, with_gw, rerun=with_u == with_gw)
        else:
            l = 3 if heads == 5 else TANH_LENGTHS[(k + hi) % 4]
            _tanh_run(ha, dv, heads, l, True, True)
            _tanh_run(ha, dv, heads, l, False, False)


@pytest.mark.parametrize("ha,dv", [(8, 8), (260, 8)])
@pytest.mark.parametrize("mis", ["values", "pre"])
def test_tanh_att_misaligned_operand_takes_scalar_path(ha, dv, mis):
    """values alone, or pre alone, one float into its allocation.  Misaligned values send the forward and the backward
    to the scalar kernels; the backward has no pre operand, so misaligned pre sends only the forward there."""
    for heads, l in ((2, 5), (5, 3), (8, 70)):
        case = _tanh_case(ha, dv, heads, l, 4000 + ha + heads)
        got, aligned = _tanh_dev(*case, mis=mis), _tanh_dev(*case)
        what = f"tanh ha={ha} dv={dv} heads={heads} l={l} {mis} misaligned"
        _tanh_check(got, _tanh_ref(*case), case[3], what)
        live = (case[3] != 0).to(DEV)
        for name, g, a in zip(TANH_NAMES, got, aligned):
            if name == "t":
                g, a = g[live], a[live]
            _rel(g, a.cpu(), f"{what} vs aligned {name}", "tanh_att")


@pytest.mark.parametrize("l,heads", [(1024, 8), (8192, 1)])
def test_tanh_att_at_the_length_limit(l, heads):
    """Full parity at l * heads == 8192, ha = dv = 8, b = 2."""
    _tanh_run(8, 8, heads, l, True, True, b=2)


@pytest.mark.parametrize("b", [1, 3, 9])
def test_tanh_att_dw2_second_stage(b):
    """sum_partials_kernel over 1, 3 and 9 sequences at heads * ha = 5 * 65 (no multiple of 64); at b = 9 dw2 starts from
    a non-zero value, which must be added to."""
    case = _tanh_case(65, 8, 5, 5, 5000 + b, b=b)
    init = _randn(torch.Generator().manual_seed(b), 5, 65) if b == 9 else None
    got = _tanh_dev(*case, dw2_init=init)
    _tanh_check(got, _tanh_ref(*case), case[3], f"tanh dw2 b={b}", dw2_init=init)
    _same(got, _tanh_dev(*case, dw2_init=init), f"tanh dw2 b={b}")


# ----------------------------------------------------------------------------- 2c. GAT layer
def _text_adj(n, r, seed, lengths=None):
    """ops.graph_build on random tokens with lengths {r, r/2, 1}: padding nodes, hence uniform rows."""
    _, ops = _ops()
    gen = torch.Generator().manual_seed(seed)
    if lengths is None:
        lengths = [(r, max(1, r // 2), 1)[g % 3] for g in range(n)]
    lengths = torch.tensor(lengths)
    tokens = torch.randint(2, 5000, (n, r), generator=gen)
    tokens[torch.arange(r)[None, :] >= lengths[:, None]] = 0
    packed, _, _ = ops.graph_build(tokens.to(DEV), lengths.to(DEV), 3)
    return packed


def _dense_adj(n, r, seed):
    """Asymmetric, density ~0.08, negative entries (the reference keeps adj > 0), rows and columns r/3 and r-1 zeroed,
    edges forced across the word boundary and between the first and last node where r allows."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn((n, r, r), generator=gen) * (torch.rand((n, r, r), generator=gen) < 0.08)
    for k in (r // 3, r - 1):
        a[:, k, :] = 0
        a[:, :, k] = 0
    for i, j in ((63, 64), (64, 63), (0, r - 1), (r - 1, 0)):      # forced after the zeroing: the only edges of node r-1
        if max(i, j) < r and i != j:
            a[:, i, j] = 0.5
    return a


def _keep_words(keep):
    """bool (n, r) -> int64 (n, words) bit rows, as PackedAdj.with_keep takes them."""
    n, r = keep.shape
    kw = np.zeros((n, (r + 63) // 64), np.uint64)
    k = keep.numpy()
    for j in range(r):
        kw[:, j // 64] |= k[:, j].astype(np.uint64) << np.uint64(j % 64)
    return torch.from_numpy(kw.view(np.int64)).to(DEV)


def _gat_heads(din, f, heads, seed):
    from get_amd import modules
    torch.manual_seed(seed)
    return [modules.GraphAttentionLayer(din, f, dropout=0.0, alpha=0.2).to(DEV) for _ in range(heads)]


def _gat_ref(x64, adj64, Ws, As, mode, r, att_masks=None, p=0.0):
    """Pre-activation of the layer in float64: elu / plain heads side by side, or the output mode's sum of heads / r."""
    kind = "elu" if mode == 1 else "plain"
    hs = [_gat_head64(x64, adj64, W, a, 0.2, att_masks[j] if att_masks is not None else None, p, kind)
          for j, (W, a) in enumerate(zip(Ws, As))]
    return sum(hs) / r if mode == 0 else torch.cat(hs, dim=2)


def _relu_decisions(out_dev, pre64, what):
    """The output mode's ReLU: the device's decision is taken only for entries whose float64 pre-activation lies within
    1e-5 of the largest one, at most 0.1 % of the outputs; any other disagreement fails."""
    dev_on = (out_dev.detach() > 0).cpu()
    ref_on = pre64.detach() > 0
    near = pre64.detach().abs() <= 1e-5 * pre64.detach().abs().max()
    differ = dev_on != ref_on
    assert not bool((differ & ~near).any()), f"{what}: {int((differ & ~near).sum())} ReLU decisions differ away from 0"
    taken = int((differ & near).sum())
    assert taken <= 1e-3 * differ.numel(), f"{what}: {taken} ReLU decisions taken from the device"
    return torch.where(near, dev_on, ref_on).double()


def _gat_run(heads_m, x, packed, adj64, mode, what, layer=0, p=0.0, seed=0, da_elementwise=False):
    _, ops = _ops()
    n, r = packed.n, packed.r
    for m in heads_m:
        m.W.grad = m.a.grad = None
    xd = _dev(x).requires_grad_(True)
    out = ops.gat_layer(xd, packed, heads_m, mode, layer, p, seed)
    gout = _randn(torch.Generator().manual_seed(17), *out.shape)
    (out * gout.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    x64 = x.double().requires_grad_(True)
    Ws = [m.W.detach().double().cpu().requires_grad_(True) for m in heads_m]
    As = [m.a.detach().double().cpu().requires_grad_(True) for m in heads_m]
    masks = torch.from_numpy(ops.gat_dropout_mask(seed, layer, len(heads_m), n, r, p)).double() if p > 0 else None
    y64 = _gat_ref(x64, adj64, Ws, As, mode, r, masks, p)
    if mode == 0:
        y64 = y64 * _relu_decisions(out, y64, what)
    (y64 * gout.double()).sum().backward()
    _rel(out, y64, f"{what} out", "gat")
    _rel(xd.grad, x64.grad, f"{what} dx", "gat")
    _rel(torch.cat([m.W.grad for m in heads_m], 1), torch.cat([w.grad for w in Ws], 1), f"{what} dW", "gat")
    da, da64 = torch.cat([m.a.grad for m in heads_m], 1), torch.cat([a.grad for a in As], 1)
    # r <= 2: every row's softmax has one element (or the row is uniform) and da is identically 0; its cancelling terms
    # P dP h with dP = dhp . h are bounded by f max |g| max |h|^2
    floor = None
    if r <= 2:
        hmax = max((x64.detach() @ w.detach()).abs().max().item() for w in Ws)
        floor = Ws[0].shape[1] * gout.abs().max().item() * hmax * hmax
    _rel(da, da64, f"{what} da", "gat", floor)
    if da_elementwise:
        err = (da.double().cpu() - da64).abs()
        assert bool((err <= 1e-5 + 1e-4 * da64.abs()).all()), f"{what} da elementwise: max err {err.max().item():.3e}"


GAT_SHAPES = [(1, 1, 4), (2, 3, 3), (63, 1, 4), (64, 3, 6), (65, 3, 130), (100, 8, 64), (128, 8, 4), (129, 1, 1024),
              (200, 8, 512), (256, 3, 65), (256, 8, 4)]


@pytest.mark.parametrize("r,heads,f", GAT_SHAPES)
def test_gat_layer_every_shape_path(r, heads, f):
    """1 to 4 bit words per row with the tail-word boundaries r = 63..65 and 128/129, up to 8 heads, head widths above 64
    off and on float4 up to the limit 1024, and the two shapes that need more than 64 KB of LDS ((256, 8, 4) forward,
    (200, 8, 512) backward), which must launch.  Output, elu and plain mode in evaluation mode, 3 graphs, on a
    graph_build adjacency with padding nodes (din 5) and on a dense mixed-sign one with isolated rows (din 8)."""
    _, ops = _ops()
    n = 3
    text = _text_adj(n, r, 60 + r)
    dense = _dense_adj(n, r, 70 + r)
    for kind, din, packed, adj64 in (("text", 5, text, text.to_dense().double().cpu()),
                                     ("dense", 8, ops.PackedAdj.from_dense(_dev(dense)), dense.double())):
        heads_m = _gat_heads(din, f, heads, 100 + r + f)
        x = _randn(torch.Generator().manual_seed(r + heads + f), n, r, din)
        for mode in (0, 1, 2):
            _gat_run(heads_m, x, packed, adj64, mode, f"gat r={r} heads={heads} f={f} {kind} mode={mode}")


@pytest.mark.parametrize("r", [65, 200])
def test_gat_layer_keep_set(r):
    """A keep-set refined adjacency: an edge survives where either end is kept (the dense mask keep_i | keep_j)."""
    _, ops = _ops()
    n, heads, f, din = 3, 3, 6, 5
    keep = torch.rand((n, r), generator=torch.Generator().manual_seed(r)) < 0.5
    kw = _keep_words(keep)
    kmask = (keep[:, :, None] | keep[:, None, :]).double()
    dense = _dense_adj(n, r, 80 + r)
    text = _text_adj(n, r, 90 + r)
    heads_m = _gat_heads(din, f, heads, 200 + r)
    x = _randn(torch.Generator().manual_seed(r), n, r, din)
    for kind, packed, adj64 in (("text", text.with_keep(kw), text.to_dense().double().cpu() * kmask),
                                ("dense", ops.PackedAdj.from_dense(_dev(dense)).with_keep(kw), dense.double() * kmask)):
        for mode in (0, 1):
            _gat_run(heads_m, x, packed, adj64, mode, f"gat keep r={r} {kind} mode={mode}")


@pytest.mark.parametrize("layer", [0, 1])
def test_gat_layer_training_mode_dropout(layer):
    """(130, 3, 6) with attention dropout, ops.gat_dropout_mask replayed into the float64 heads: the dropout key runs
    across the word boundaries of a row and, at layer = 1, from a non-zero layer offset."""
    n, r, heads, f, din = 3, 130, 3, 6, 5
    text = _text_adj(n, r, 300)
    heads_m = _gat_heads(din, f, heads, 301)
    x = _randn(torch.Generator().manual_seed(302), n, r, din)
    _gat_run(heads_m, x, text, text.to_dense().double().cpu(), 1, f"gat training layer={layer}", layer=layer, p=0.3,
             seed=123456789 + layer)


@pytest.mark.parametrize("n", [17, 33])
def test_gat_da_reduction_over_graphs(n):
    """gat_da_reduce_kernel's second and third round over the graphs (n > 16, n > 32), da elementwise at
    1e-5 + 1e-4 |want|."""
    r, heads, f, din = 12, 1, 3, 5
    text = _text_adj(n, r, 400 + n, lengths=[1 + (5 * g) % r for g in range(n)])
    heads_m = _gat_heads(din, f, heads, 401)
    x = _randn(torch.Generator().manual_seed(402), n, r, din)
    _gat_run(heads_m, x, text, text.to_dense().double().cpu(), 1, f"gat n={n}", da_elementwise=True)


@pytest.mark.parametrize("r,heads,f", [(65, 3, 130), (256, 8, 4)])
def test_gat_layer_direct_abi_writes_every_element(r, heads, f):
    """gh_gat_layer_fwd / _bwd into NaN-filled h, s, stats, hp, out, dh, da_part and dx (elu mode, dense adjacency): all
    written, within the bound; dw_cat and da start from non-zero values, which must be added to; two calls bit-identical."""
    _lib, ops = _ops()
    n, din, Fw = 3, 5, heads * f
    gen = torch.Generator().manual_seed(500 + r)
    dense = _dense_adj(n, r, 501 + r)
    packed = ops.PackedAdj.from_dense(_dev(dense))
    x, g = _randn(gen, n, r, din), _randn(gen, n * r, Fw)
    Ws = [torch.randn((din, f), generator=gen) * 0.5 for _ in range(heads)]
    As = [torch.randn((2 * f, 1), generator=gen) * 0.5 for _ in range(heads)]
    dw0, da0 = _randn(gen, din, Fw), _randn(gen, heads, 2 * f)
    w_cat = _dev(torch.cat(Ws, 1))
    w_lin = _dev(torch.cat(Ws, 1).t())
    a_cat = _dev(torch.cat([a.reshape(1, -1) for a in As], 0))
    xd, gd = _dev(x.reshape(n * r, din)), _dev(g)
    P = _lib.ptr

    def run():
        h, s, stats = _nan(n * r, Fw), _nan(n * r, heads, 2), _nan(n * r, heads, 2)
        hp, out = _nan(n * r, Fw), _nan(n * r, Fw)
        _lib.call("gh_gat_layer_fwd", P(packed.bits), P(packed.vals), None, P(xd), P(w_lin), P(a_cat), n, r, din, heads, f,
                  0.2, 1, 0, 0.0, 0, P(h), P(s), P(stats), P(hp), P(out), _lib.stream())
        dh, da_part, dx = _nan(n * r, Fw), _nan(n, heads, 2 * f), _nan(n * r, din)
        dw, da = _dev(dw0), _dev(da0)
        _lib.call("gh_gat_layer_bwd", P(packed.bits), P(packed.vals), None, P(xd), P(w_cat), P(a_cat), n, r, din, heads, f,
                  0.2, 1, 0, 0.0, 0, P(h), P(s), P(stats), P(hp), P(out), P(gd), P(dh), P(da_part), P(dx), P(dw), P(da),
                  _lib.stream())
        torch.cuda.synchronize()
        return h, s, stats, hp, out, dh, da_part, dx, dw, da

    got = run()
    h, s, stats, hp, out, dh, da_part, dx, dw, da = got
    what = f"gat abi r={r} heads={heads} f={f}"
    for name, t in zip(("h", "s", "stats", "hp", "out", "dh", "da_part", "dx", "dw_cat", "da"), got):
        assert bool(torch.isfinite(t).all()), f"{what}: {int((~torch.isfinite(t)).sum())} elements of {name} not written"
    x64 = x.double().requires_grad_(True)
    W64 = [w.double().requires_grad_(True) for w in Ws]
    A64 = [a.double().requires_grad_(True) for a in As]
    h64 = x64 @ torch.cat(W64, 1)                 # the projection as a node of its own: dh is its gradient
    h64.retain_grad()
    eye = torch.eye(f, dtype=torch.float64)
    hp64 = torch.cat([_gat_head64(h64[..., j * f:(j + 1) * f], dense.double(), eye, A64[j], 0.2, None, 0.0, "plain")
                      for j in range(heads)], dim=2)
    y64 = F.elu(hp64)
    (y64 * g.double().view(n, r, Fw)).sum().backward()
    s64 = torch.stack([torch.cat([h64[..., j * f:(j + 1) * f] @ A64[j][:f], h64[..., j * f:(j + 1) * f] @ A64[j][f:]], -1)
                       for j in range(heads)], dim=2)
    _rel(h.view(n, r, Fw), h64, f"{what} h", "gat")
    _rel(s.view(n, r, heads, 2), s64, f"{what} s", "gat")
    _rel(dh.view(n, r, Fw), h64.grad, f"{what} dh", "gat")
    _rel(hp.view(n, r, Fw), hp64, f"{what} hp", "gat")
    _rel(out.view(n, r, Fw), y64, f"{what} out", "gat")
    _rel(dx.view(n, r, din), x64.grad, f"{what} dx", "gat")
    _rel(dw, torch.cat([w.grad for w in W64], 1) + dw0.double(), f"{what} dw_cat", "gat")
    _rel(da, torch.cat([a.grad.reshape(1, -1) for a in A64], 0) + da0.double(), f"{what} da", "gat")
    _rel(da_part.sum(0), torch.cat([a.grad.reshape(1, -1) for a in A64], 0), f"{what} da_part", "gat")
    _same(got, run(), what)


# ----------------------------------------------------------------------------- 2d. GCN normalisation
@pytest.mark.parametrize("r", [64, 65, 129, 256])
def test_gcn_norm_row_scales(r):
    """gh_gcn_norm in normalised mode (dinv) and weighted mode (vals), with and without a keep-set, into a NaN-filled
    scale: rowsum^-1/2 of the refined adjacency's float64 row sums (times dinv in normalised mode, whose result is the
    new dinv), 0 where the sum is 0, within 2e-6 relative."""
    _lib, ops = _ops()
    n = 3
    text = _text_adj(n, r, 600 + r)
    vals = _dense_adj(n, r, 601 + r).abs()
    weighted = ops.PackedAdj.from_dense(_dev(vals))
    keep = torch.rand((n, r), generator=torch.Generator().manual_seed(r)) < 0.5
    kw = _keep_words(keep)
    kmask = (keep[:, :, None] | keep[:, None, :]).double()
    for kind, base, dense64 in (("dinv", text, text.to_dense().double().cpu()), ("vals", weighted, vals.float().double())):
        for adj, a64 in ((base, dense64), (base.with_keep(kw), dense64 * kmask)):
            scale = _nan(n, r)
            _lib.call("gh_gcn_norm", _lib.ptr(adj.bits), _lib.ptr(adj.dinv) if adj.vals is None else None, _lib.ptr(adj.vals),
                      _lib.ptr(adj.keep), n, r, _lib.ptr(scale), _lib.stream())
            torch.cuda.synchronize()
            rows = a64.sum(-1)
            want = torch.where(rows > 0, rows.clamp_min(1e-300).pow(-0.5), torch.zeros_like(rows))
            if kind == "dinv":
                want = want * text.dinv.double().cpu()
            got = scale.double().cpu()
            what = f"gcn_norm r={r} {kind} keep={'yes' if adj.keep is not None else 'no'}"
            assert bool(torch.isfinite(got).all()), f"{what}: elements not written"
            err = (got - want).abs().max().item()
            print(f"{what}: max err {err:.3e} over scale {want.abs().max().item():.3e}")
            assert err <= 2e-6 * max(1.0, want.abs().max().item()), f"{what}: max err {err:.3e}"
            assert bool((got[rows == 0] == 0.0).all()), f"{what}: a row without entries has a non-zero scale"

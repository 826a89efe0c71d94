"""Every path of the BERT entries of csrc/bert_ops.hip (gh_bert_attention_fwd / _bwd, gh_act_fwd / _bwd, gh_bert_embed_fwd),
called through the C-ABI on NaN-fenced buffers and compared with the float64 restatement of tests/bert_ref.py.

Attention.  q, k and v are the three column blocks of ONE [rows][3 W + 4] buffer (W = heads * dh, so ld > W; the four spare
columns hold NaN on the way in and must hold NaN on the way out), dq, dk and dv the three blocks of another, `out` has
ld = W + 4.  lse and delta start as NaN.  Geometries (b, heads, lq = lk, dh):
    (2, 3, 5, 6)      no width a multiple of 4: single-float staging, one query tile, one key slab
    (2, 3, 70, 8)     five query tiles / key slabs, keys cross 64 (two score chunks in the query-tiled backward), float4 staging
    (1, 1, 1, 4)      one query, one key
    (2, 2, 35, 64)    BERT's head width: four column tiles, one per wave
    (1, 16, 17, 20)   the most heads; 20 columns = a full tile and a 4-column one, two query tiles
    (1, 1, 33, 80)    dh > 64: five column tiles, so wave 0 owns two accumulators (the t = 1 tiles of store_acc, in all three kernels)
each with bias NULL and with a bias whose LAST batch is fully masked (-10000 on every key; the other batch, where there is
one, has -10000 on its last keys and -1 on key 0), and with p in {0, 0.1, 0.5} under the mask ops.dropout_mask_reference
predicts.  Scores offset by +-96 (the first column of every head of q at +-96 / scale against ones in k) overflow resp.
underflow a softmax that does not subtract the maximum.

Bounds.  Everything is held to TOL = 1e-4 of the float64 result's largest entry, except the fully masked batch.  There every
score is a sum next to -10000, where fp32's grid is 2^-10: the rounded sum is off by up to 2^-11, a probability -- a ratio of
two such exponentials -- by the factor e^(+-2^-10), and the backward's recomputed one by a further e^(+-2^-11) from the rounding
of lse.  That is the arithmetic the entry is specified to do (the reference's own), not an error of the kernel, so for that batch
the bound is TOL of the largest entry PLUS the first-order propagation of EPS = 2^-9 (2^-10 + 2^-11, rounded up to a power of
two) through the float64 formulas, elementwise, with kf = keep / (1 - p) and Pd = P kf: out EPS (Pd |v|), dv EPS (Pd^T |gO|), and
from dS = P (kf dP - delta), delta = sum_j Pd dP, with E = P (|kf dP - delta| + sum_j Pd |dP|) (a dropped entry still carries
-P delta): dq EPS scale (E |k|), dk EPS scale (E^T |q|).

The keep pattern itself is read back with v = I at dh = lk = 20 (out = the dropped probabilities) and must equal
dropout_mask_reference bit for bit.  Refused calls (lk = 1025, dh = 513, heads = 17, NULL q, ld < W) return non-zero with a
message and leave every output NaN."""
import ctypes
import math

import pytest
import torch

from tests import bert_ref
from tests.util import DEV, NAN, TOL, _Fenced, _ops, _poison, bits_equal, rel_close

pytestmark = pytest.mark.gpu

GEOMS = [(2, 3, 5, 6), (2, 3, 70, 8), (1, 1, 1, 4), (2, 2, 35, 64), (1, 16, 17, 20), (1, 1, 33, 80)]
EPS = 2.0 ** -9
SEED = 20211


def _inputs(b, heads, lq, lk, dh, bias_mode, offset, scale):
    g = torch.Generator().manual_seed(1000 * lq + 10 * dh + heads + (7 if bias_mode else 0))
    w = heads * dh
    q, k, v, go = (torch.randn(b, n, w, generator=g) for n in (lq, lk, lk, lq))
    if offset:
        q.view(b, lq, heads, dh)[..., 0] = offset / scale
        k.view(b, lk, heads, dh)[..., 0] = 1.0
    bias = None
    if bias_mode:
        bias = torch.zeros(b, lk)
        bias[-1] = -10000.0                      # the last batch: fully masked
        if b > 1:
            bias[0, lk - 1 - lk // 4:] = -10000.0
            bias[0, 0] = -1.0
    return q, k, v, go, bias


def _keep(b, heads, lq, lk, p):
    from get_amd import ops
    if p == 0:
        return None
    return torch.from_numpy(ops.dropout_mask_reference(SEED, b * heads * lq, lk, p)).reshape(b, heads, lq, lk)


class _Att:
    """One forward + backward of the two attention entries on fenced buffers."""

    def __init__(self, b, heads, lq, lk, dh, q, k, v, go, bias, scale, p, runs=1):
        _lib, _ = _ops()
        w = heads * dh
        self.F = F = _Fenced()
        self.w = w
        if lq == lk:      # the three column blocks of one [rows][3 W + 4] buffer
            ld = 3 * w + 4
            host = torch.full((b * lq, ld), NAN)
            host[:, :w], host[:, w:2 * w], host[:, 2 * w:3 * w] = q.reshape(-1, w), k.reshape(-1, w), v.reshape(-1, w)
            self.qkv = F.put("qkv", host)
            qs, ks, vs = (self.qkv[:, i * w:(i + 1) * w] for i in range(3))
            self.dqkv = F.put("dqkv", shape=(b * lq, ld))
            dqs, dks, dvs = (self.dqkv[:, i * w:(i + 1) * w] for i in range(3))
            ldq = ldk = ld
        else:
            ldq, ldk = w + 4, 2 * w + 4
            hq, hkv = torch.full((b * lq, ldq), NAN), torch.full((b * lk, ldk), NAN)
            hq[:, :w], hkv[:, :w], hkv[:, w:2 * w] = q.reshape(-1, w), k.reshape(-1, w), v.reshape(-1, w)
            self.qkv, self.kv = F.put("q", hq), F.put("kv", hkv)
            qs, ks, vs = self.qkv[:, :w], self.kv[:, :w], self.kv[:, w:2 * w]
            self.dqkv, self.dkv = F.put("dq", shape=(b * lq, ldq)), F.put("dkv", shape=(b * lk, ldk))
            dqs, dks, dvs = self.dqkv[:, :w], self.dkv[:, :w], self.dkv[:, w:2 * w]
        ldo = w + 4
        hgo = torch.full((b * lq, ldo), NAN)
        hgo[:, :w] = go.reshape(-1, w)
        gob = F.put("g_out", hgo)
        biasb = F.put("bias", bias) if bias is not None else None
        self.outb = F.put("out", shape=(b * lq, ldo))
        self.lse, self.delta = F.put("lse", shape=(b, heads, lq)), F.put("delta", shape=(b, heads, lq))
        bp = biasb.data_ptr() if biasb is not None else None
        _poison()
        _lib.call("gh_bert_attention_fwd", qs.data_ptr(), ks.data_ptr(), vs.data_ptr(), ldq, ldk, ldk, bp, b, heads, lq, lk, dh, scale,
                  p, SEED, self.outb.data_ptr(), ldo, self.lse.data_ptr(), _lib.stream())
        self.out = self.outb[:, :w].clone().view(b, lq, w)
        self.grads = []
        for _ in range(runs):
            self.delta.fill_(NAN)
            self.dqkv.fill_(NAN)
            if lq != lk:
                self.dkv.fill_(NAN)
            _lib.call("gh_bert_attention_bwd", qs.data_ptr(), ks.data_ptr(), vs.data_ptr(), ldq, ldk, ldk, bp, self.outb.data_ptr(), ldo,
                      self.lse.data_ptr(), gob.data_ptr(), ldo, b, heads, lq, lk, dh, scale, p, SEED, self.delta.data_ptr(),
                      dqs.data_ptr(), ldq, dks.data_ptr(), ldk, dvs.data_ptr(), ldk, _lib.stream())
            self.grads.append((dqs.clone().view(b, lq, w), dks.clone().view(b, lk, w), dvs.clone().view(b, lk, w), self.delta.clone()))
        torch.cuda.synchronize()
        # the spare columns of the strided outputs were never written, nor was anything around any buffer
        assert bool(torch.isnan(self.outb[:, w:]).all()) and bool(torch.isnan(self.dqkv[:, (3 * w if lq == lk else w):]).all())
        if lq != lk:
            assert bool(torch.isnan(self.dkv[:, 2 * w:]).all())
        F.check(f"bert_attention b={b} heads={heads} lq={lq} lk={lk} dh={dh} p={p}")


def _reference(b, heads, lq, lk, dh, q, k, v, go, bias, scale, p):
    """float64: out, lse, delta, (dq, dk, dv) and, per batch, the EPS propagation terms of the module docstring."""
    keep = _keep(b, heads, lq, lk, p)
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    b64 = bias.double() if bias is not None else None
    out, lse = bert_ref.attention(q64, k64, v64, b64, heads, scale, keep, p)
    (out * go.double()).sum().backward()
    split = lambda t, n: t.detach().double().reshape(b, n, heads, dh).permute(0, 2, 1, 3)
    merge = lambda t, n: t.permute(0, 2, 1, 3).reshape(b, n, heads * dh)
    qh, kh, vh, gh = split(q, lq), split(k, lk), split(v, lk), split(go, lq)
    s = scale * (qh @ kh.transpose(-1, -2)) + (0 if b64 is None else b64[:, None, None, :])
    pr = torch.softmax(s, -1)
    kf = 1.0 if keep is None else keep.double() / (1.0 - p)
    pe = pr * kf
    dpe = gh @ vh.transpose(-1, -2)
    delta = (pe * dpe).sum(-1)
    e = pr * ((kf * dpe - delta[..., None]).abs() + (pe * dpe.abs()).sum(-1, keepdim=True))
    prop = dict(out=merge(pe @ vh.abs(), lq), dv=merge(pe.transpose(-1, -2) @ gh.abs(), lk),
                dq=scale * merge(e @ kh.abs(), lq), dk=scale * merge(e.transpose(-1, -2) @ qh.abs(), lk))
    assert float((delta - (gh * split(out, lq)).sum(-1)).abs().max()) <= 1e-9 * (1 + float(delta.abs().max()))
    # a softmax over ONE key has a zero Jacobian: dq and dk are identically 0 in float64, the terms that cancel are of the size
    # of dP (rel_close's `floor`, used only where the float64 result is 0)
    size = scale * float(dpe.abs().max())
    prop["floor"] = dict(dq=size * float(k.abs().max()), dk=size * float(q.abs().max()), out=None, dv=None)
    return out.detach(), lse.detach(), delta, dict(dq=q64.grad, dk=k64.grad, dv=v64.grad), prop


def _check(got, want, what, masked_batch=None, prop=None, floor=None):
    """TOL of the largest entry; the fully masked batch (index masked_batch) at TOL of the largest entry + EPS * prop."""
    if masked_batch is None:
        rel_close(got, want, TOL, what, floor=floor, fam="bert")
        return
    live = [i for i in range(want.shape[0]) if i != masked_batch]
    if live:
        rel_close(got[live], want[live], TOL, what + " (unmasked batches)", fam="bert")
    g, w_ = got[masked_batch].double().cpu(), want[masked_batch]
    assert bool(torch.isfinite(g).all()), what
    bound = TOL * (float(want.abs().max()) + 1e-12) + EPS * prop[masked_batch]
    worst = float(((g - w_).abs() / bound).max())
    print(f"{what} (fully masked batch): {worst:.3f} of the bound")
    assert worst <= 1.0, f"{what} (fully masked batch): {worst:.2f} x bound"


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("bias_mode", [0, 1], ids=["nobias", "masked"])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "b%dh%dl%dd%d" % g)
def test_attention_matches_float64(geom, bias_mode, p):
    b, heads, l, dh = geom
    scale = 1.0 / math.sqrt(dh)
    q, k, v, go, bias = _inputs(b, heads, l, l, dh, bias_mode, 0.0, scale)
    run = _Att(b, heads, l, l, dh, q, k, v, go, bias, scale, p, runs=2)
    out, lse, delta, grads, prop = _reference(b, heads, l, l, dh, q, k, v, go, bias, scale, p)
    mb = b - 1 if bias_mode else None
    what = f"bert_attention {geom} bias={bias_mode} p={p}: "
    _check(run.out, out, what + "out", mb, prop["out"])
    dq, dk, dv, dl = run.grads[0]
    _check(dq, grads["dq"], what + "dq", mb, prop["dq"], prop["floor"]["dq"])
    _check(dk, grads["dk"], what + "dk", mb, prop["dk"], prop["floor"]["dk"])
    _check(dv, grads["dv"], what + "dv", mb, prop["dv"])
    # lse: absolute, on the grid of its own magnitude (2^-10 next to -10000, a few ulp of O(1) elsewhere)
    err = (run.lse.double().cpu() - lse).abs()
    assert bool((err <= 1e-5 + 2.0 ** -22 * lse.abs()).all()), what + f"lse off by {float(err.max()):.3e}"
    live = [i for i in range(b) if i != mb]      # (the masked batch's delta carries the EPS error of its `out`: covered through dq, dk)
    if live:
        rel_close(dl[live], delta[live], TOL, what + "delta", fam="bert")
    for a, c in zip(run.grads[0], run.grads[1]):
        bits_equal(a, c, what + "two backward calls")


@pytest.mark.parametrize("offset", [96.0, -96.0], ids=["pos96", "neg96"])
@pytest.mark.parametrize("geom", [(2, 3, 5, 6), (2, 3, 70, 8)], ids=lambda g: "b%dh%dl%dd%d" % g)
def test_attention_subtracts_the_maximum(geom, offset):
    """Every scaled score sits near +-96 with an O(1) spread: exp overflows (+) or underflows to an all-zero row (-) in a softmax
    without max-subtraction, and in a backward that does not recompute through lse."""
    b, heads, l, dh = geom
    scale = 1.0 / math.sqrt(dh)
    q, k, v, go, bias = _inputs(b, heads, l, l, dh, 0, offset, scale)
    run = _Att(b, heads, l, l, dh, q, k, v, go, bias, scale, 0.1)
    out, lse, _, grads, _ = _reference(b, heads, l, l, dh, q, k, v, go, bias, scale, 0.1)
    assert float(lse.abs().min()) > 80.0
    what = f"bert_attention {geom} offset {offset}: "
    rel_close(run.out, out, TOL, what + "out", fam="bert")
    rel_close(run.lse, lse, TOL, what + "lse", fam="bert")
    for name, got in zip(("dq", "dk", "dv"), run.grads[0]):
        rel_close(got, grads[name], TOL, what + name, fam="bert")


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_realised_keep_pattern_is_the_predicted_one(p):
    """v = I per head at dh = lk = 20: out is the dropped probability tile itself, so out != 0 is the kernel's keep pattern."""
    b, heads, lq, lk, dh = 2, 3, 17, 20, 20
    scale = 1.0 / math.sqrt(dh)
    q, k, v, go, _ = _inputs(b, heads, lq, lk, dh, 0, 0.0, scale)
    v = torch.eye(lk, dh).repeat(b, 1, heads).contiguous()
    run = _Att(b, heads, lq, lk, dh, q, k, v, go, None, scale, p)
    probs = run.out.view(b, lq, heads, dh).permute(0, 2, 1, 3).cpu()
    keep = _keep(b, heads, lq, lk, p)
    assert torch.equal(probs != 0, keep), "the realised keep pattern differs from dropout_mask_reference"
    assert 0.5 * p < 1.0 - float(keep.double().mean()) < 1.5 * p
    out, _, _, grads, _ = _reference(b, heads, lq, lk, dh, q, k, v, go, None, scale, p)
    rel_close(run.out, out, TOL, f"keep pattern p={p}: out", fam="bert")
    for name, got in zip(("dq", "dk", "dv"), run.grads[0]):
        rel_close(got, grads[name], TOL, f"keep pattern p={p}: {name}", fam="bert")
    # p == 0 keeps everything: the same call without dropout has no exact zero
    assert bool((_Att(b, heads, lq, lk, dh, q, k, v, go, None, scale, 0.0).out != 0).all())


def test_attention_refusals_write_nothing():
    _lib, _ = _ops()
    F = _Fenced()
    buf = F.put("in", torch.randn(64, 64))
    outs = [F.put(n, shape=(64, 64)) for n in ("out", "lse", "delta", "dq", "dk", "dv")]
    o, lse, dl, dq, dk, dv = (t.data_ptr() for t in outs)
    x = buf.data_ptr()
    st = _lib.stream()

    def fwd(q=x, ld=16, heads=2, lq=4, lk=4, dh=8, p=0.0):
        _lib.call("gh_bert_attention_fwd", q, x, x, ld, ld, ld, None, 1, heads, lq, lk, dh, 0.5, p, 1, o, ld, lse, st)

    def bwd(q=x, ld=16, heads=2, lq=4, lk=4, dh=8, p=0.0):
        _lib.call("gh_bert_attention_bwd", q, x, x, ld, ld, ld, None, x, ld, x, x, ld, 1, heads, lq, lk, dh, 0.5, p, 1, dl, dq, ld, dk, ld,
                  dv, ld, st)

    for call in (fwd, bwd):
        for kw, msg in ((dict(lk=1025), "lk=1025 exceeds"), (dict(lq=1025), "lq=1025 exceeds"), (dict(dh=513, ld=1026), "dh=513 exceeds"),
                        (dict(heads=17, ld=136), "heads=17 exceeds"), (dict(q=None), "NULL"), (dict(ld=15), "leading dimension"),
                        (dict(p=1.0), "dropout"), (dict(lk=0), "empty")):
            with pytest.raises(RuntimeError, match=msg):
                call(**kw)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in outs), "a refused call wrote to an output"
    F.check("bert_attention refusals")
    fwd()          # the same arguments without the fault are served
    bwd()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0].view(-1)[:64]).all()) and bool(torch.isfinite(outs[3].view(-1)[:64]).all())


def test_attention_at_the_length_limit():
    """lq = lk = 1024 (the [16][1028] score tile, beyond 64 KB of dynamic LDS), one head: against float64."""
    b, heads, l, dh = 1, 1, 1024, 8
    scale = 1.0 / math.sqrt(dh)
    q, k, v, go, bias = _inputs(b, heads, l, l, dh, 0, 0.0, scale)
    run = _Att(b, heads, l, l, dh, q, k, v, go, bias, scale, 0.1)
    out, _, _, grads, _ = _reference(b, heads, l, l, dh, q, k, v, go, bias, scale, 0.1)
    rel_close(run.out, out, TOL, "bert_attention l=1024: out", fam="bert")
    for name, got in zip(("dq", "dk", "dv"), run.grads[0]):
        rel_close(got, grads[name], TOL, "bert_attention l=1024: " + name, fam="bert")


# ----------------------------------------------------------------------------- activations
@pytest.mark.parametrize("mis", [False, True], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("n", [1, 3, 40, 3072])
@pytest.mark.parametrize("mode", [0, 1], ids=["gelu", "tanh"])
def test_activations_match_float64(mode, n, mis):
    _lib, _ = _ops()
    rows = 3
    g = torch.Generator().manual_seed(40 + n)
    x = (torch.rand(rows, n, generator=g) * 20.0 - 10.0)
    x.view(-1)[::5] = 0.0
    x.view(-1)[1::7] *= 0.05                                  # the curved part of both functions
    go = torch.randn(rows, n, generator=g)
    F = _Fenced()
    xb, gb = F.put("x", x, mis=mis), F.put("g", go, mis=mis)
    yb, dxb = F.put("y", shape=(rows, n), mis=mis), F.put("dx", shape=(rows, n), mis=mis)
    _lib.call("gh_act_fwd", xb.data_ptr(), yb.data_ptr(), rows, n, mode, _lib.stream())
    _lib.call("gh_act_bwd", xb.data_ptr(), gb.data_ptr(), dxb.data_ptr(), rows, n, mode, _lib.stream())
    torch.cuda.synchronize()
    F.check(f"act mode={mode} n={n}")
    x64 = x.double().requires_grad_(True)
    y64 = bert_ref.gelu(x64) if mode == 0 else torch.tanh(x64)
    (y64 * go.double()).sum().backward()
    rel_close(yb, y64.detach(), TOL, f"act_fwd mode={mode} n={n}", fam="bert")
    rel_close(dxb, x64.grad, TOL, f"act_bwd mode={mode} n={n}", fam="bert")
    zero = x == 0
    assert bool((yb.cpu()[zero] == 0).all()), "act(0) is exactly 0"
    for bad in (dict(mode=2), dict(rows=0)):
        with pytest.raises(RuntimeError, match="act_fwd"):
            _lib.call("gh_act_fwd", xb.data_ptr(), yb.data_ptr(), bad.get("rows", rows), n, bad.get("mode", mode), _lib.stream())


# ----------------------------------------------------------------------------- embedding sum + LayerNorm
def _clamp_events(reset):
    _lib, _ = _ops()
    buf = (ctypes.c_int64 * 4)()
    _lib.call("gh_clamp_events", ctypes.cast(buf, ctypes.c_void_p), 1 if reset else 0)
    return list(buf)


@pytest.mark.parametrize("explicit", [False, True], ids=["null_ids", "explicit_ids"])
@pytest.mark.parametrize("d", [18, 24, 200])
def test_embed_matches_float64(d, explicit):
    _lib, _ = _ops()
    b, l, vocab, npos, ntype, eps = 3, 7, 11, 9, 2, 1e-12
    g = torch.Generator().manual_seed(d)
    word, pos, typ = (torch.randn(n, d, generator=g) for n in (vocab, npos, ntype))
    gamma, beta = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    ids = torch.randint(0, vocab, (b, l), generator=g, dtype=torch.int32)
    pos_ids = torch.randint(0, npos, (b, l), generator=g, dtype=torch.int32) if explicit else None
    type_ids = torch.randint(0, ntype, (b, l), generator=g, dtype=torch.int32) if explicit else None
    bad = 0
    if explicit:      # ids outside their tables: clamped to the nearest row and counted, one count per id
        ids[0, 1], ids[2, 3], pos_ids[1, 1], type_ids[2, 6] = -3, vocab + 2, npos, -1
        bad = 4
    F = _Fenced()
    tabs = [F.put(n, t) for n, t in (("word", word), ("pos", pos), ("type", typ), ("gamma", gamma), ("beta", beta))]
    idb = ids.to(DEV)      # (read-only int32 operands: the fences are for what the entry writes and for float reads)
    pb = pos_ids.to(DEV) if explicit else None
    tb = type_ids.to(DEV) if explicit else None
    outs = [F.put(n, shape=s) for n, s in (("sum", (b * l, d)), ("y", (b * l, d)), ("mean", (b * l,)), ("rstd", (b * l,)))]
    _clamp_events(True)
    _lib.call("gh_bert_embed_fwd", tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), idb.data_ptr(),
              pb.data_ptr() if explicit else None, tb.data_ptr() if explicit else None, tabs[3].data_ptr(), tabs[4].data_ptr(), eps,
              b * l, l, d, vocab, npos, ntype, *(t.data_ptr() for t in outs), _lib.stream())
    assert _clamp_events(True) == [0, 0, 0, bad]
    F.check(f"bert_embed d={d}")
    p64 = {"embeddings.word_embeddings.weight": word.double(), "embeddings.position_embeddings.weight": pos.double(),
           "embeddings.token_type_embeddings.weight": typ.double(), "embeddings.LayerNorm.weight": gamma.double(),
           "embeddings.LayerNorm.bias": beta.double()}
    clamp = lambda t, n: None if t is None else t.long().clamp(0, n - 1)
    s64, y64 = bert_ref.embed(p64, clamp(ids, vocab), clamp(pos_ids, npos), clamp(type_ids, ntype), eps)
    what = f"bert_embed d={d} explicit={explicit}: "
    rel_close(outs[0], s64.reshape(b * l, d), TOL, what + "sum", fam="bert")
    rel_close(outs[1], y64.reshape(b * l, d), TOL, what + "y", fam="bert")
    mu = s64.mean(-1).reshape(-1)
    rel_close(outs[2], mu, TOL, what + "mean", floor=1.0, fam="bert")
    rel_close(outs[3], 1.0 / torch.sqrt(((s64.reshape(b * l, d) - mu[:, None]) ** 2).mean(-1) + eps), TOL, what + "rstd", fam="bert")
    for kw, msg in ((dict(d=2049), "d=2049 exceeds"), (dict(word=None), "NULL"), (dict(rows=0), "bad sizes")):
        with pytest.raises(RuntimeError, match=msg):
            _lib.call("gh_bert_embed_fwd", kw.get("word", tabs[0].data_ptr()), tabs[1].data_ptr(), tabs[2].data_ptr(), idb.data_ptr(), None,
                      None, tabs[3].data_ptr(), tabs[4].data_ptr(), eps, kw.get("rows", b * l), l, kw.get("d", d), vocab, npos, ntype,
                      *(t.data_ptr() for t in outs), _lib.stream())


def test_bert_embed_op_forward_and_backward():
    """ops.bert_embed end to end (gh_add_layernorm_bwd on the saved sum + three table gradients) against float64, twice
    bit-identical; the word table's padding row 0 receives nothing."""
    _, ops = _ops()
    b, l, vocab, npos, d = 4, 9, 13, 12, 18
    g = torch.Generator().manual_seed(77)
    tabs = [torch.randn(n, d, generator=g) for n in (vocab, npos, 2)]
    gamma, beta = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    ids = torch.randint(0, vocab, (b, l), generator=g)
    ids[:, -2:] = 0
    types = torch.randint(0, 2, (b, l), generator=g)
    go = torch.randn(b, l, d, generator=g)
    runs = []
    for _ in range(2):
        ps = [t.clone().to(DEV).requires_grad_(True) for t in tabs + [gamma, beta]]
        y = ops.bert_embed(ps[0], ps[1], ps[2], ids.to(DEV), None, types.to(DEV), ps[3], ps[4], 1e-12)
        (y * go.to(DEV)).sum().backward()
        runs.append([y.detach()] + [t.grad for t in ps])
    names = ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight", "LayerNorm.weight", "LayerNorm.bias")
    p64 = {"embeddings." + n: t.double().requires_grad_(True) for n, t in zip(names, tabs + [gamma, beta])}
    _, y64 = bert_ref.embed(p64, ids, None, types, 1e-12)
    (y64 * go.double()).sum().backward()
    rel_close(runs[0][0], y64.detach(), TOL, "ops.bert_embed y", fam="bert")
    for got, n in zip(runs[0][1:], names):
        rel_close(got, p64["embeddings." + n].grad, TOL, "ops.bert_embed grad " + n, fam="bert")
    assert float(runs[0][1][0].abs().max()) == 0.0
    for a, c in zip(runs[0], runs[1]):
        bits_equal(a, c, "ops.bert_embed twice")

"""The embedding family on the GPU (csrc/embed_ops.hip, get_amd/ops/embed, modules.Embedding): the table gradient against
float64 bit for bit on small integers, against the order restatement of tests/embed_ref.py bit for bit on floats and within
the derived fp32 bound of float64, reproducibility, padding and out-of-range ids, the module, the GGNN cell with a trainable
table and the whole model with embedding_freeze=False, also under a FlatTrainer.

Shapes: C = ops.EMBED_CHUNK sorted positions make a chunk, so m runs over 1, C-1, C, C+1 and 3C+5 (a run over four chunks); D
over the scalar path (1, 7, 50) and the float4 path (128, 300, 768).  A workgroup has at most 256 threads, so a row wider than
1024 floats takes a second pass over the chunk: D = 1200 covers that once."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import cases
from oracle import get_oracle as O
from oracle.assemble import assemble_inputs, reference_kargs
from oracle.cases_model import MODEL_CASES
from tests import embed_ref
from tests.util import DEV, NAN, _Fenced, build_model, to_dev

pytestmark = pytest.mark.gpu

C = embed_ref.EMBED_CHUNK
MS = [1, C - 1, C, C + 1, 3 * C + 5]
DS = [1, 7, 50, 128, 300, 768]
PATTERNS = ["equal", "distinct", "zipf", "run_ends_on_edge", "run_starts_on_last_row", "first_and_last_id"]


def _lib_ops():
    from get_amd import _lib, ops
    assert ops.EMBED_CHUNK == C
    # (a registered workspace changes how the few-row GEMMs of the cell split their sums: register it before the first forward,
    #  not in the middle of a comparison of two passes)
    _lib.ensure_workspace(DEV)
    return _lib, ops


def _vocab(m):
    return 2 * m + 9


def _ids(pattern, m, vocab, rng):
    """m ids in [0, vocab) whose SORTED order has the named feature; the rows are then shuffled."""
    if pattern == "equal":
        s = np.full(m, vocab // 2)
    elif pattern == "distinct":
        s = rng.permutation(vocab)[:m]
    elif pattern == "zipf":
        s = np.minimum(rng.zipf(1.4, m) - 1, vocab - 1)
    elif pattern == "run_ends_on_edge":          # id 1 on positions 0 .. C-6, id 2 on C-5 .. C-1, id 3 on C .. C+2, then distinct ones
        s = np.concatenate([np.full(C - 5, 1), np.full(5, 2), np.full(3, 3), 4 + np.arange(m)])[:m]
    elif pattern == "run_starts_on_last_row":    # id 1 on positions 0 .. C-2, id 2 from C-1 on into the next chunk (and the third)
        s = np.concatenate([np.full(C - 1, 1), np.full(C + 9, 2), 3 + np.arange(m)])[:m]
    else:
        s = rng.integers(0, vocab, m)
        s[0] = 0
        s[-1] = vocab - 1 if m > 1 else 0
    return rng.permutation(s.astype(np.int64))


def _prior(vocab, d):
    """A table whose every entry tells its place: small integers in [-8, 8]."""
    t, j = np.arange(vocab)[:, None], np.arange(d)[None, :]
    return ((t * 7 + j * 3) % 17 - 8).astype(np.float32)


def _bwd(dx, ids, g0, padding_idx=-1, ldx=None, ids_dtype=torch.int64, what=""):
    """gh_embed_bwd through the C-ABI on fenced operands and a NaN-filled workspace of exactly the documented size."""
    _lib, ops = _lib_ops()
    m, d = dx.shape
    vocab = g0.shape[0]
    sid, perm = ops.embed_plan(torch.from_numpy(ids).to(ids_dtype).to(DEV), vocab)
    assert sid.dtype == perm.dtype == torch.int32 and sid.is_cuda
    F = _Fenced()
    ld = d if ldx is None else ldx
    rows = F.put("dx", torch.full((m, ld), NAN))            # (the columns beyond d stay NaN: nobody may read them)
    rows[:, :d] = torch.from_numpy(dx).to(DEV)
    table = F.put("dtable", torch.from_numpy(g0))
    ws = F.put("workspace", shape=(2 * ((m + C - 1) // C) * d,))
    _lib.call("gh_embed_bwd", rows.data_ptr(), ld, _lib.ptr(sid), _lib.ptr(perm), m, d, vocab, padding_idx, _lib.ptr(table), _lib.ptr(ws),
              ws.numel(), _lib.stream())
    torch.cuda.synchronize()
    F.check(what)
    return table.cpu().numpy()


def _clamp_events(reset):
    _lib, _ = _lib_ops()
    buf = (ctypes.c_int64 * 4)()
    _lib.call("gh_clamp_events", ctypes.cast(buf, ctypes.c_void_p), 1 if reset else 0)
    return list(buf)


def _int_case(m, d, pattern, seed):
    rng = np.random.default_rng(seed)
    vocab = _vocab(m)
    ids = _ids(pattern, m, vocab, rng)
    dx = rng.integers(-8, 9, (m, d)).astype(np.float32)
    return ids, dx, _prior(vocab, d)


# ---------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("m", MS)
def test_small_integers_equal_float64_bit_for_bit(m, d):
    for pi, pattern in enumerate(PATTERNS):
        what = f"m={m} d={d} {pattern}"
        ids, dx, g0 = _int_case(m, d, pattern, 100 * m + d + pi)
        got = _bwd(dx, ids, g0, what=what)
        want = embed_ref.embed_bwd_f64(dx, ids, g0)
        assert np.array_equal(got.astype(np.float64), want), what
        untouched = np.setdiff1d(np.arange(g0.shape[0]), ids)
        assert untouched.size and np.array_equal(got[untouched], g0[untouched]), what
        if pattern == "first_and_last_id" and m > 1:
            assert (ids == 0).any() and (ids == g0.shape[0] - 1).any()


@pytest.mark.parametrize("m,d,ldx", [(3 * C + 5, 50, 57), (3 * C + 5, 128, 132), (C + 1, 1200, 1204)])
def test_leading_dimension_and_column_loop(m, d, ldx):
    """dx as a row view with a leading dimension (scalar and float4 path), and a row wider than one pass of the workgroup."""
    for pattern in ("equal", "zipf", "run_starts_on_last_row"):
        ids, dx, g0 = _int_case(m, d, pattern, 7 * m + d)
        got = _bwd(dx, ids, g0, ldx=ldx, what=f"m={m} d={d} ldx={ldx} {pattern}")
        assert np.array_equal(got.astype(np.float64), embed_ref.embed_bwd_f64(dx, ids, g0)), pattern


def test_int32_ids_and_the_python_front_give_the_same_table():
    _lib, ops = _lib_ops()
    ids, dx, g0 = _int_case(3 * C + 5, 300, "zipf", 5)
    want = embed_ref.embed_bwd_f64(dx, ids, g0)
    assert np.array_equal(_bwd(dx, ids, g0, ids_dtype=torch.int32).astype(np.float64), want)
    for dtype in (torch.int32, torch.int64):
        idt = torch.from_numpy(ids).to(dtype).to(DEV)
        table = torch.from_numpy(g0).to(DEV)
        big = torch.full((dx.shape[0], 304), NAN, device=DEV)
        big[:, :300] = torch.from_numpy(dx).to(DEV)
        out = ops.embedding_backward(big[:, :300], ops.embed_plan(idt, g0.shape[0]), table)        # a row view, read in place
        assert out is table and np.array_equal(table.cpu().numpy().astype(np.float64), want)
    empty = torch.from_numpy(g0).to(DEV)
    ops.embedding_backward(torch.empty((0, 300), device=DEV), ops.embed_plan(torch.empty((0,), dtype=torch.int64, device=DEV), g0.shape[0]), empty)
    assert np.array_equal(empty.cpu().numpy(), g0)
    with pytest.raises(RuntimeError, match="workspace"):
        sid, perm = ops.embed_plan(torch.from_numpy(ids).to(DEV), g0.shape[0])
        t = torch.from_numpy(g0).to(DEV)
        ws = torch.empty((2 * 4 * 300 - 1,), device=DEV)
        _lib.call("gh_embed_bwd", _lib.ptr(torch.from_numpy(dx).to(DEV)), 300, _lib.ptr(sid), _lib.ptr(perm), dx.shape[0], 300, g0.shape[0], -1,
                  _lib.ptr(t), _lib.ptr(ws), ws.numel(), _lib.stream())


# ---------------------------------------------------------------- 2. order
FLOAT_CASES = [(1, 7, "equal"), (C - 1, 50, "zipf"), (C, 128, "run_ends_on_edge"), (C + 1, 1, "equal"), (C + 1, 300, "run_starts_on_last_row"),
               (3 * C + 5, 300, "equal"), (3 * C + 5, 768, "zipf"), (3 * C + 5, 7, "first_and_last_id"), (3 * C + 5, 128, "distinct")]


def _float_case(m, d, pattern):
    rng = np.random.default_rng(31 * m + d)
    vocab = _vocab(m)
    return _ids(pattern, m, vocab, rng), rng.standard_normal((m, d)).astype(np.float32), rng.standard_normal((vocab, d)).astype(np.float32)


def _check_floats(got, dx, ids, g0, what, padding_idx=-1):
    want = embed_ref.embed_bwd_ordered(dx, ids, g0, padding_idx)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"{what}: not the bits of the order restatement"
    err = np.abs(got.astype(np.float64) - embed_ref.embed_bwd_f64(dx, ids, g0, padding_idx))
    bound = embed_ref.embed_bwd_bound(dx, ids, g0, padding_idx)
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    print(f"{what}: worst |err| / bound = {float(ratio.max()):.3f}")
    assert (err <= bound).all(), what


@pytest.mark.parametrize("m,d,pattern", FLOAT_CASES)
def test_floats_equal_the_order_restatement_bit_for_bit(m, d, pattern):
    ids, dx, g0 = _float_case(m, d, pattern)
    _check_floats(_bwd(dx, ids, g0, what=f"m={m} d={d} {pattern}"), dx, ids, g0, f"m={m} d={d} {pattern}")


# ---------------------------------------------------------------- 3. reproducible
def test_three_calls_give_the_same_bits():
    for m, d, pattern in [(3 * C + 5, 300, "zipf"), (3 * C + 5, 50, "equal")]:
        ids, dx, g0 = _float_case(m, d, pattern)
        runs = [_bwd(dx, ids, g0) for _ in range(3)]
        assert np.array_equal(runs[0].view(np.int32), runs[1].view(np.int32)) and np.array_equal(runs[0].view(np.int32), runs[2].view(np.int32))


# ---------------------------------------------------------------- 4. padding_idx, ids outside the table
def test_padding_row_is_left_alone():
    for m, d in [(C + 1, 50), (3 * C + 5, 128)]:
        ids, dx, g0 = _int_case(m, d, "zipf", 3 * m + d)
        pad = int(np.bincount(ids).argmax())                     # the heaviest id: its run crosses chunk edges at the larger m
        before = _clamp_events(reset=True)
        got = _bwd(dx, ids, g0, padding_idx=pad)
        assert _clamp_events(reset=True)[3] == 0, "the padding id is not an out-of-range id"
        assert np.array_equal(got[pad], g0[pad])
        assert np.array_equal(got.astype(np.float64), embed_ref.embed_bwd_f64(dx, ids, g0, padding_idx=pad))
        assert not np.array_equal(got, _bwd(dx, ids, g0)), "the padding id named no row: the case is vacuous"
        del before


def test_ids_outside_the_table_add_nothing_and_are_counted():
    m, d = 3 * C + 5, 300
    ids, dx, g0 = _int_case(m, d, "zipf", 77)
    vocab = g0.shape[0]
    rng = np.random.default_rng(8)
    bad = rng.permutation(m)[:C + 40]                            # more than a chunk of them on either end of the sorted order
    ids[bad[:C // 2 + 20]] = -1
    ids[bad[C // 2 + 20:]] = vocab
    ids[bad[0]] = -5
    ids[bad[-1]] = 2 ** 40 + 3                                   # would wrap into the table as an int32
    _clamp_events(reset=True)
    got = _bwd(dx, ids, g0, what="ids outside the table")
    events = _clamp_events(reset=True)
    assert events[3] == bad.size and events[:3] == [0, 0, 0], events
    assert np.array_equal(got.astype(np.float64), embed_ref.embed_bwd_f64(dx, ids, g0))
    untouched = np.setdiff1d(np.arange(vocab), ids)
    assert np.array_equal(got[untouched], g0[untouched])
    fl_ids, fl_dx, fl_g0 = ids.copy(), np.random.default_rng(9).standard_normal((m, d)).astype(np.float32), g0 * 0.37
    _check_floats(_bwd(fl_dx, fl_ids, fl_g0, padding_idx=3), fl_dx, fl_ids, fl_g0.astype(np.float32), "floats, bad ids and padding", padding_idx=3)
    _clamp_events(reset=True)


# ---------------------------------------------------------------- 5. module
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("padding_idx", [None, 4])
def test_module_forward_and_backward(dtype, padding_idx):
    from get_amd import modules
    rng = np.random.default_rng(12)
    vocab, d, B, L = 61, 300, 5, 3 * C // 5 + 1                  # 5 x 77 = 385 lookups: four chunks
    table = rng.standard_normal((vocab, d)).astype(np.float32)
    emb = modules.Embedding.from_pretrained(torch.from_numpy(table), freeze=False, padding_idx=padding_idx).to(DEV)
    ids = np.minimum(rng.zipf(1.3, (B, L)) - 1, vocab - 1)
    out = emb(torch.from_numpy(ids).to(dtype).to(DEV))
    assert out.shape == (B, L, d) and out.dtype == torch.float32
    assert np.array_equal(out.detach().cpu().numpy().view(np.int32), table[ids].view(np.int32))
    w = rng.standard_normal((B, L, d)).astype(np.float32)
    (out * torch.from_numpy(w).to(DEV)).sum().backward()
    pad = -1 if padding_idx is None else padding_idx
    _check_floats(emb.weight.grad.cpu().numpy(), w.reshape(-1, d), ids.reshape(-1), np.zeros_like(table), f"module {dtype}", padding_idx=pad)
    if padding_idx is not None:
        assert (ids == padding_idx).any() and not emb.weight.grad[padding_idx].any()
    odd = modules.Embedding(9, 7).to(DEV)                        # a width without a float4 path, ids of rank 3 and rank 0
    i3 = torch.from_numpy(rng.integers(0, 9, (2, 3, 4))).to(dtype).to(DEV)
    assert torch.equal(odd(i3), odd.weight.detach()[i3.long()]) and odd(i3[0, 0, 0]).shape == (7,)
    assert odd(i3[:0]).shape == (0, 3, 4, 7)


def test_frozen_module_launches_no_backward(monkeypatch):
    from get_amd import modules, ops
    emb = modules.Embedding.from_pretrained(torch.randn(20, 16), freeze=True).to(DEV)
    calls = []
    real = ops.embed.call
    monkeypatch.setattr(ops.embed, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    ids = torch.randint(0, 20, (4, 6), device=DEV)
    out = emb(ids)
    assert not out.requires_grad
    w = torch.randn(4, 6, 16, device=DEV, requires_grad=True)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    assert calls == ["gh_embed_fwd"] and emb.weight.grad is None
    assert torch.equal(w.grad, out)


def test_direct_accumulation_allocates_no_table():
    """Under a trainer the table gradient is added straight into weight.grad: the backward may allocate the sort, the plan and
    the workspace of a few rows, never a (V, D) tensor.  V x D = 8 MB here, the lookups' rows 64 KB."""
    from get_amd import modules
    vocab, d = 8192, 256
    emb = modules.Embedding(vocab, d).to(DEV)
    ids = torch.randint(0, vocab, (64,), device=DEV)
    ids[:20] = 5
    w = torch.randn(64, d, device=DEV)
    (emb(ids) * w).sum().backward()                              # plain autograd: one zeroed table comes back
    plain = emb.weight.grad.clone()
    emb.weight.grad = torch.zeros_like(emb.weight)
    emb.weight._gh_direct_grad = True                            # what dist.FlatTrainer sets on the views of its bucket
    loss = (emb(ids) * w).sum()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss.backward()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert extra < vocab * d * 4 // 4, f"the direct backward allocated {extra} bytes; the table has {vocab * d * 4}"
    assert torch.equal(emb.weight.grad, plain)
    (emb(ids) * w).sum().backward()                              # and it accumulates: g + g
    assert torch.equal(emb.weight.grad, plain + plain)


# ---------------------------------------------------------------- 6. cell
@pytest.mark.parametrize("layout", ["padded", "compact"])
def test_ggnn_cell_trainable_table_is_deterministic(layout):
    from get_amd import modules
    _, ops = _lib_ops()
    rng = np.random.default_rng(77)
    n, r, d, h, vocab = 5, 30, 48, 64, 50
    toks, lens, ids, adj = cases.graphs(rng, n, r, 3, O.convert_text, vocab=vocab)
    emb = rng.standard_normal((vocab, d)).astype(np.float32)
    p = cases.cell_params(rng, d, h)
    mod = modules.GGNN(d, h)
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, strict=True)
    mod = mod.to(DEV).train(False)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    padj, node_ids, n_nodes = ops.graph_build(T(toks), T(lens), 3)
    assert np.array_equal(node_ids.cpu().numpy(), ids)
    real = np.arange(r)[None, :] < n_nodes.cpu().numpy()[:, None]                # the padding nodes take no part in either layout's loss
    gw = rng.standard_normal((n, r, h)).astype(np.float32) * real[:, :, None]
    embo = torch.from_numpy(emb).requires_grad_(True)
    oo = O.ggnn_cell(torch.from_numpy(adj).float(), embo[torch.from_numpy(ids)], {k: torch.from_numpy(v) for k, v in p.items()})
    (oo * torch.from_numpy(gw)).sum().backward()
    grads = []
    for _ in range(2):
        e = modules.Embedding.from_pretrained(torch.from_numpy(emb), freeze=False).to(DEV)
        if layout == "padded":
            out = mod.forward_ids(padj, e, node_ids)
        else:
            plan = ops.RaggedPlan(n_nodes, node_ids, int(real.sum()))
            out = plan.to_padded(mod.forward_ids(padj, e, node_ids, plan=plan))
        (out * T(gw)).sum().backward()
        grads.append(e.weight.grad.clone())
    err = float((grads[0].cpu() - embo.grad).abs().max())
    assert err <= 1e-3 * float(embo.grad.abs().max()) + 1e-6, err
    assert torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32)), "two backward passes differ in the table gradient"


# ---------------------------------------------------------------- 7. model
def _small_batch():
    from get_amd.synth import make_raw_batch
    cfg, seed = MODEL_CASES["small"]
    inp = assemble_inputs(make_raw_batch(cfg, seed), cfg, O.convert_text)
    return cfg, seed, inp


def _model_backward(model, inp):
    """One eval-mode forward and backward of the loss; returns the peak of allocated bytes above the level right before backward."""
    from get_amd import fused
    kargs = to_dev(reference_kargs(inp, torch, output_ranking=False))
    query = torch.from_numpy(inp["query"]).to(DEV)
    assert fused.ENABLED and not fused.eligible(model, query, kargs), "a trainable table takes the module-by-module path"
    phi = model(query, torch.from_numpy(inp["document"]).to(DEV), **kargs)
    loss = torch.nn.functional.cross_entropy(phi, torch.from_numpy(inp["labels"]).to(DEV))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss.backward()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_model_with_a_trainable_table_vs_oracle_and_under_a_flat_trainer():
    from get_amd.dist import FlatTrainer
    from get_amd.synth import make_embeddings, make_state_dict
    _, ops = _lib_ops()
    cfg, seed, inp = _small_batch()
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    emb, art, _ = make_embeddings(cfg, seed)
    p = {k: T(v).requires_grad_(True) for k, v in make_state_dict(cfg, seed).items()}
    p["embedding.weight"], p["article_source_embs.weight"] = T(emb).requires_grad_(True), T(art)
    phi_o, _, _ = O.model_forward(p, cfg.__dict__, T(inp["query"]), T(inp["document"]), T(inp["query_adj"]), T(inp["doc_ids"]),
                                  T(inp["doc_adj"]), T(inp["query_lens"]), inp["evd_counts"], T(inp["doc_sources"]), T(inp["query_sources"]))
    O.cross_entropy(phi_o, T(inp["labels"])).backward()
    want = p["embedding.weight"].grad
    # one run first: the first backward on a stream registers its split-K workspace (256 MB, and the few-row GEMMs split their sums
    # once it is there), which belongs neither in a comparison of two runs nor in a peak
    warm = build_model(cfg, seed)
    warm.embedding.weight.requires_grad_(True)
    _model_backward(warm, inp)
    del warm
    plain, peaks = [], []
    for _ in range(2):
        model = build_model(cfg, seed)
        model.embedding.weight.requires_grad_(True)
        assert type(model.embedding).__name__ == "Embedding" and type(model.embedding).__module__ == "get_amd.modules"
        peaks.append(_model_backward(model, inp))
        plain.append(model.embedding.weight.grad.clone())
    err = float((plain[0].cpu() - want).abs().max())
    assert err <= 1e-3 * float(want.abs().max()) + 1e-6, err
    assert float(want.abs().max()) > 0
    assert torch.equal(plain[0].view(torch.int32), plain[1].view(torch.int32)), "two runs differ in the table gradient"
    # under a FlatTrainer the table's slice of the flat bucket receives the same bits, and no (V, D) temporary exists
    model = build_model(cfg, seed)
    model.embedding.weight.requires_grad_(True)
    trainer = FlatTrainer(model, lr=1e-4, weight_decay=1e-3)
    ops.bump_weight_epoch()
    assert "embedding.weight" in trainer.live_names and ops.weights._direct(model.embedding.weight)
    trainer.zero_grad()
    peak_direct = _model_backward(model, inp)
    view = trainer._views[trainer.live_names.index("embedding.weight")]
    assert view.data_ptr() == model.embedding.weight.grad.data_ptr()
    assert torch.equal(view.view(torch.int32), plain[0].view(torch.int32)), "the flat bucket's table slice differs from plain autograd"
    table_bytes = emb.size * 4
    print(f"backward peak above its start: plain autograd {peaks[0]} B, FlatTrainer {peak_direct} B, table {table_bytes} B")
    assert peaks[0] - peak_direct >= table_bytes

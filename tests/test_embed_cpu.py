"""CPU-side checks of the embedding family: the order restatement of tests/embed_ref.py against float64 within the derived
bound, the header / binding / Makefile agreement, and modules.Embedding as the drop-in of torch.nn.Embedding in the models."""
import os
import re

import numpy as np
import pytest
import torch

from tests import embed_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ids(rng, m, vocab, kind):
    if kind == "one":
        return np.full(m, int(rng.integers(0, vocab)), np.int64)
    if kind == "heavy":          # 60 % of the rows name one id
        ids = rng.integers(0, vocab, m)
        ids[rng.random(m) < 0.6] = int(rng.integers(0, vocab))
        return ids.astype(np.int64)
    return rng.integers(0, vocab, m).astype(np.int64)


# (m, d, vocab, id pattern): below, at and above one chunk; a run over four chunks; a heavy hitter among others
RESTATEMENT_CASES = [(1, 5, 4, "any"), (127, 9, 7, "any"), (128, 9, 8, "any"), (129, 300, 12, "any"), (389, 3, 300, "one"),
                     (700, 40, 50, "heavy")]


@pytest.mark.parametrize("m,d,vocab,kind", RESTATEMENT_CASES)
def test_order_restatement_is_within_the_fp32_bound_of_float64(m, d, vocab, kind):
    rng = np.random.default_rng(1000 + m)
    ids = _ids(rng, m, vocab, kind)
    dx = rng.standard_normal((m, d)).astype(np.float32)
    g0 = rng.standard_normal((vocab, d)).astype(np.float32)
    got = embed_ref.embed_bwd_ordered(dx, ids, g0)
    want = embed_ref.embed_bwd_f64(dx, ids, g0)
    bound = embed_ref.embed_bwd_bound(dx, ids, g0)
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / bound).max())
    print(f"m={m} d={d} vocab={vocab} {kind}: worst |err| / bound = {worst:.3f}")
    assert (err <= bound).all(), worst
    untouched = np.setdiff1d(np.arange(vocab), ids)
    assert np.array_equal(got[untouched], g0[untouched])
    # a dropped row is far outside the bound: the bound can tell a wrong sum from a rounded one
    if m > 1:
        short = embed_ref.embed_bwd_f64(dx[1:], ids[1:], g0)
        assert (np.abs(short - want) > bound).any()


def test_restatement_skips_padding_and_ids_outside_the_table():
    rng = np.random.default_rng(5)
    ids = np.array([3, -1, 0, 7, 3, 8, 2, 2, 0], np.int64)         # vocab 8: -1 and 8 are outside, 2 is the padding id
    dx = rng.integers(-8, 9, (ids.size, 6)).astype(np.float32)
    g0 = rng.integers(-8, 9, (8, 6)).astype(np.float32)
    got = embed_ref.embed_bwd_ordered(dx, ids, g0, padding_idx=2)
    want = g0.copy()
    for i, t in enumerate(ids):
        if t in (0, 3, 7):
            want[t] += dx[i]
    assert np.array_equal(got, want)
    assert np.array_equal(got, embed_ref.embed_bwd_f64(dx, ids, g0, padding_idx=2).astype(np.float32))


def test_header_binding_and_makefile_agree():
    from get_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "get_hip.h")).read()
    chunk = int(re.search(r"#define\s+GH_EMBED_CHUNK\s+(\d+)", header).group(1))
    assert chunk == ops.EMBED_CHUNK == embed_ref.EMBED_CHUNK
    assert re.search(r"#define\s+GH_ABI_VERSION\s+10\b", header) and _lib.ABI_VERSION == 10      # the exports are additive
    for name in ("gh_embed_fwd", "gh_embed_bwd"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared"
        assert name in _lib.SIGNATURES, f"{name} is not bound"
    assert "[3] = reserved" not in header                # slot 3 of gh_clamp_events is documented
    makefile = open(os.path.join(ROOT, "get_amd", "csrc", "Makefile")).read()
    src = re.search(r"^SRC\s*:=(.*)$", makefile, flags=re.M).group(1).split()
    assert "embed_ops.hip" in src and os.path.exists(os.path.join(ROOT, "get_amd", "csrc", "embed_ops.hip"))
    assert ops.embed.embed_workspace_floats(129, 7) == 2 * 2 * 7 and ops.embed.embed_workspace_floats(128, 7) == 2 * 7


def test_ops_refuse_cpu_tensors():
    from get_amd import ops
    w = torch.zeros(4, 3, requires_grad=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.embedding(w, torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.embed_plan(torch.zeros(2, dtype=torch.int64), 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.embedding_backward(torch.zeros(2, 3), (torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)), torch.zeros(4, 3))


@pytest.mark.parametrize("padding_idx", [None, 2, -1])
def test_module_on_cpu_is_torch_embedding(padding_idx):
    from get_amd import modules
    g = torch.Generator().manual_seed(3)
    table = torch.randn(9, 5, generator=g)
    ours = modules.Embedding.from_pretrained(table.clone(), freeze=False, padding_idx=padding_idx)
    ref = torch.nn.Embedding.from_pretrained(table.clone(), freeze=False, padding_idx=padding_idx)
    assert isinstance(ours, torch.nn.Embedding) and type(ours) is modules.Embedding
    assert set(ours.state_dict()) == {"weight"} and ours.padding_idx == ref.padding_idx
    ids = torch.tensor([[0, 2, 8, 2], [8, 8, 1, 0]])
    w = torch.randn(2, 4, 5, generator=g)
    a, b = ours(ids), ref(ids)
    assert torch.equal(a, b)
    (a * w).sum().backward()
    (b * w).sum().backward()
    assert torch.equal(ours.weight.grad, ref.weight.grad)
    frozen = modules.Embedding.from_pretrained(table.clone())
    assert not frozen.weight.requires_grad and not frozen(ids).requires_grad
    fresh = modules.Embedding(9, 5, padding_idx=padding_idx)
    assert tuple(fresh.weight.shape) == (9, 5) and fresh.weight.requires_grad
    ref.load_state_dict(ours.state_dict(), strict=True)          # the state dicts are interchangeable


@pytest.mark.parametrize("kwargs", [dict(max_norm=1.0), dict(scale_grad_by_freq=True), dict(sparse=True)])
def test_module_refuses_what_the_kernels_do_not_do(kwargs):
    from get_amd import modules
    with pytest.raises(ValueError, match="not supported"):
        modules.Embedding(6, 4, **kwargs)
    with pytest.raises(ValueError, match="not supported"):
        modules.Embedding.from_pretrained(torch.zeros(6, 4), **kwargs)


@pytest.mark.parametrize("freeze", [True, False])
def test_models_build_with_both_embedding_freeze_values(freeze):
    from get_amd import modules
    from get_amd.synth import make_embeddings
    from oracle.cases_model import MODEL_CASES
    cfg, seed = MODEL_CASES["small"]
    emb, art, clm = make_embeddings(cfg, seed)

    def keys(embedding_class):
        """state_dict keys and shapes of both models with the two factories returning `embedding_class` layers"""
        params = cfg.model_params(emb, art, clm)
        params["embedding_freeze"] = freeze
        get = modules.Graph_basedSemantiStructure(params)
        bidaf = modules.BiDAF(dict(embedding=emb, embedding_freeze=freeze, word_dim=emb.shape[1], hidden_size=8, dropout=0.2))
        tables = [get.embedding, bidaf.word_emb] + [getattr(get, n) for n in ("claim_source_embs", "article_source_embs") if hasattr(get, n)]
        assert len(tables) >= 3 and all(type(t) is embedding_class for t in tables)
        assert get.embedding.weight.requires_grad == (not freeze) == bidaf.word_emb.weight.requires_grad
        assert all(t.weight.requires_grad for t in tables[2:])                       # the source tables always train
        return [{k: tuple(v.shape) for k, v in m.state_dict().items()} for m in (get, bidaf)]

    ours = keys(modules.Embedding)
    # the same models with torch's own class in the factories: the keys and shapes must not have moved
    G = modules.Graph_basedSemantiStructure
    saved = G._make_default_embedding_layer, G._make_entity_embedding_layer
    try:
        G._make_default_embedding_layer = staticmethod(
            lambda p: (p.__setitem__("embedding_input_dim", p["embedding"].shape[0]), p.__setitem__("embedding_output_dim", p["embedding"].shape[1]),
                       torch.nn.Embedding.from_pretrained(torch.Tensor(p["embedding"]), freeze=p["embedding_freeze"]))[2])
        G._make_entity_embedding_layer = staticmethod(lambda m, freeze: torch.nn.Embedding.from_pretrained(torch.Tensor(m), freeze=freeze))
        theirs = keys(torch.nn.Embedding)
    finally:
        G._make_default_embedding_layer, G._make_entity_embedding_layer = (staticmethod(f) for f in saved)
    assert ours == theirs

"""CPU-side checks of the BiDAF drop-in (Models/BiDAF/bidaf_model.py): the float64 restatement the GPU tests compare the
kernels with (tests/bidaf_ref.py) reproduces the reference's goldens on its own, install() serves the reference's import
path, the constructor builds the reference's state_dict (keys, order, shapes) and draws what the reference draws from a
seed, the model's seeded construction is untouched, and the new ops refuse CPU tensors."""
import os
import zlib

import numpy as np
import pytest
import torch

from tests.bidaf_ref import att_flow64, bidaf64, highway64
from tests.util import golden_ratio, load_golden, run_in_fresh_interpreter

CASES = ["v50_h12", "v60_h16", "v80_h20", "short_query"]
KEYS = (["word_emb.weight"]
        + [f"highway_{kind}{i}.0.linear.{p}" for i in range(2) for kind in ("linear", "gate") for p in ("weight", "bias")]
        + [f"context_LSTM.rnn.{p}_l0{s}" for s in ("", "_reverse") for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        + [f"att_weight_{n}.linear.{p}" for n in ("c", "q", "cq") for p in ("weight", "bias")]
        + [f"modeling_LSTM1.rnn.{p}_l0{s}" for s in ("", "_reverse") for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        + ["last_linear.weight", "last_linear.bias"])


def _archive(golden_dir):
    return load_golden(golden_dir, "g15_bidaf.npz", "bidaf_contract.json")


def params_of(z, name):
    key = f"{name}::param::"
    return {k[len(key):]: torch.from_numpy(z[k].astype(np.float32)) for k in z if k.startswith(key)}


def model_params(z, contract, name):
    """The params dict of a golden case, as the reference's driver would hand it over."""
    return dict(contract[name]["params"], embedding=z[f"{name}::param::word_emb.weight"].astype(np.float32))


def test_bidaf_golden_archive_is_complete(golden_dir):
    z, meta, contract = _archive(golden_dir)
    assert meta["cases"] == CASES and set(contract) == set(CASES)
    shapes = {"v50_h12": (50, 20, 12, 5, 7, 11), "v60_h16": (60, 24, 16, 19, 9, 37), "v80_h20": (80, 32, 20, 6, 33, 70)}
    frozen = set()
    for name in CASES:
        c = contract[name]
        assert [k for k, _ in c["state_dict"]] == KEYS, name
        assert set(c["params"]) == {"embedding_freeze", "word_dim", "hidden_size", "dropout", "embedding_input_dim",
                                    "embedding_output_dim"}
        B, L = z[name + "::query"].shape
        R = z[name + "::document"].shape[1]
        ql, cl = z[name + "::q_lens"], z[name + "::c_lens"]
        assert B >= 2 and cl.max() == R >= 2 and ql.min() >= 1 and cl.min() >= 1 and len(set(ql)) > 1 and len(set(cl)) > 1
        if name in shapes:
            assert (c["embedding_shape"][0], c["params"]["word_dim"], c["params"]["hidden_size"], B, L, R) == shapes[name]
            assert ql.max() == L
        for side, lens in (("q", ql), ("d", cl)):
            new, rest = z[f"{name}::{side}_new_indices"], z[f"{name}::{side}_restoring_indices"]
            assert (new[rest] == np.arange(B)).all() and (np.diff(lens[new]) <= 0).all()
        assert z[name + "::logits"].shape == (B, 1) == z[name + "::g_logits"].shape
        trainable = [k for k in KEYS if k != "word_emb.weight" or not c["params"]["embedding_freeze"]]
        assert {k[len(name) + 8:] for k in z if k.startswith(name + "::grad::")} == set(trainable)
        if c["params"]["embedding_freeze"]:
            frozen.add(name)
        for k in KEYS:
            if "bias" in k:
                assert (z[f"{name}::param::{k}"] != 0).all(), k
    assert 0 < len(frozen) < len(CASES)                                    # embedding_freeze both ways
    assert z["short_query::q_lens"].max() < z["short_query::query"].shape[1]
    assert os.path.getsize(os.path.join(golden_dir, "g15_bidaf.npz")) < 1024 * 1024


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_reproduces_the_bidaf_goldens(golden_dir, name):
    """tests/bidaf_ref.py alone, in float64 on the archive's inputs and parameters: logits within 1e-4 + 1e-4 |want| and every
    gradient within 1e-5 + 1e-4 |want| of the reference's fp32 results; the three attention bias gradients vanish."""
    z, _, contract = _archive(golden_dir)
    p64 = {k: v.double().requires_grad_(True) for k, v in params_of(z, name).items()}
    logits = bidaf64(p64, torch.from_numpy(z[name + "::query"]), torch.from_numpy(z[name + "::document"]), z[name + "::q_lens"],
                     z[name + "::c_lens"])
    (logits * torch.from_numpy(z[name + "::g_logits"]).double()).sum().backward()
    worst = golden_ratio(logits, z[name + "::logits"], 1e-4, 1e-4, f"{name}::logits")
    for k in KEYS:
        if f"{name}::grad::{k}" in z:
            worst = max(worst, golden_ratio(p64[k].grad, z[f"{name}::grad::{k}"], 1e-5, 1e-4, f"{name}::grad::{k}"))
    print(f"{name}: worst ratio of the bound {worst:.3f}")
    for n in ("c", "q", "cq"):
        assert float(p64[f"att_weight_{n}.linear.bias"].grad.abs().max()) <= 1e-12


def test_closed_form_is_the_reference_loop():
    """The q_len loop, the expands, both bmm and the cat of bidaf_model.py:72-104 written out with torch ops (B >= 2 and
    c_len >= 2, where the reference's squeezes are harmless) against the closed form of tests/bidaf_ref.py."""
    g = torch.Generator().manual_seed(5)
    c, q = torch.randn(3, 7, 6, generator=g, dtype=torch.float64), torch.randn(3, 4, 6, generator=g, dtype=torch.float64)
    w = [torch.randn(6, generator=g, dtype=torch.float64) for _ in range(3)]
    bias = torch.randn(3, generator=g, dtype=torch.float64)
    cq = torch.stack([(c * q[:, i:i + 1]) @ w[2] + bias[2] for i in range(4)], dim=-1)
    s = ((c @ w[0] + bias[0]).unsqueeze(2).expand(-1, -1, 4) + (q @ w[1] + bias[1]).unsqueeze(1).expand(-1, 7, -1) + cq)
    a = torch.softmax(s, dim=2)
    c2q = torch.bmm(a, q)
    b = torch.softmax(torch.max(s, dim=2)[0], dim=1).unsqueeze(1)
    q2c = torch.bmm(b, c).squeeze(1).unsqueeze(1).expand(-1, 7, -1)
    want = torch.cat([c, c2q, c * c2q, c * q2c], dim=-1)
    got, am = att_flow64(c, q, w[0], w[1], w[2], bias.sum())
    assert float((got - want).abs().max()) <= 1e-13 and torch.equal(am, torch.max(s, dim=2)[1])
    x, h, gp = (torch.randn(5, 3, generator=g, dtype=torch.float64) for _ in range(3))
    gate = torch.sigmoid(gp)
    assert torch.equal(highway64(x, h, gp), gate * torch.relu(h) + (1 - gate) * x)


def test_install_serves_the_bidaf_import_path(tmp_path):
    run_in_fresh_interpreter(tmp_path, "from Models.BiDAF.bidaf_model import BiDAF\n"
                             "assert BiDAF is M.BiDAF and BiDAF.__module__ == 'get_amd.modules'\n"
                             "from Models.BiDAF.wrapper import LSTM\n"
                             "from Models.BiDAF import bidaf_model as bm\nassert bm.LSTM is LSTM", packages=("Models", "Models/BiDAF"))


def test_bidaf_state_dict_matches_the_reference_contract(golden_dir):
    from get_amd import modules
    z, _, contract = _archive(golden_dir)
    for name in CASES:
        params = model_params(z, contract, name)
        del params["embedding_input_dim"], params["embedding_output_dim"]
        m = modules.BiDAF(params)
        V, D = contract[name]["embedding_shape"]
        assert params["embedding_input_dim"] == V and params["embedding_output_dim"] == D      # written back
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == contract[name]["state_dict"], name
        assert m.word_emb.weight.requires_grad == (not params["embedding_freeze"])
        m.load_state_dict(params_of(z, name), strict=True)
        assert m.context_LSTM.dropout.p == m.modeling_LSTM1.dropout.p == m.dropout.p == 0.2
        assert isinstance(m.highway_linear0[1], torch.nn.ReLU) and isinstance(m.highway_gate1[1], torch.nn.Sigmoid)
    # without a matrix: the two dims are read
    m = modules.BiDAF(dict(embedding=None, embedding_input_dim=9, embedding_output_dim=6, embedding_freeze=False, word_dim=6,
                           hidden_size=4, dropout=0.0))
    assert m.word_emb.weight.shape == (9, 6) and m.last_seeds == [None, None, None]


@pytest.mark.parametrize("name", ["v50_h12", "short_query"])
def test_seeded_construction_draws_what_the_reference_draws(golden_dir, name):
    """The generator seeds torch with crc32(case) before it builds the reference's model; the same seed here gives the same
    weights (rounded to float16, as the archive stores them; the archive's biases are re-seeded and not compared)."""
    from get_amd import modules
    z, _, contract = _archive(golden_dir)
    torch.manual_seed(zlib.crc32(name.encode()))
    m = modules.BiDAF(model_params(z, contract, name))
    for k, v in m.state_dict().items():
        if "bias" not in k:
            assert np.array_equal(v.numpy().astype(np.float16), z[f"{name}::param::{k}"]), k


def test_the_models_seeded_construction_is_unchanged(golden_dir):
    """Building a BiDAF first leaves what a seed gives Graph_basedSemantiStructure as it was."""
    from get_amd import modules
    from get_amd.synth import make_embeddings
    from oracle.cases_model import MODEL_CASES
    z, _, contract = _archive(golden_dir)
    cfg, seed = MODEL_CASES["small"]
    emb, art, clm = make_embeddings(cfg, seed)

    def build():
        torch.manual_seed(7)
        return {k: v.clone() for k, v in modules.Graph_basedSemantiStructure(cfg.model_params(emb, art, clm)).state_dict().items()}
    before = build()
    modules.BiDAF(model_params(z, contract, "v50_h12"))
    after = build()
    assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)


def test_bidaf_ops_refuse_cpu_tensors(golden_dir):
    from get_amd import modules, ops
    c, q, w, b = torch.zeros(2, 5, 4), torch.zeros(2, 3, 4), torch.zeros(4), torch.zeros(1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.att_flow(c, q, w, w, w, b, b, b)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.highway(c, c, c)
    z, _, contract = _archive(golden_dir)
    m = modules.BiDAF(model_params(z, contract, "short_query")).eval()
    idx = np.arange(4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.from_numpy(z["short_query::query"]), torch.from_numpy(z["short_query::document"]),
          query_lens_indices=(idx, idx, z["short_query::q_lens"]), doc_lens_indices=(idx, idx, z["short_query::c_lens"]))

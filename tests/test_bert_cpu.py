"""CPU-side checks of the BERT encoder drop-in (get_amd/bert.py): the float64 restatement the GPU tests compare the kernels
with (tests/bert_ref.py) reproduces the reference's goldens on its own, BertModel builds the reference's state_dict for both
configurations of tests/golden/bert_contract.json, BertConfig round-trips a config.json, BertModule loads a directory written
the way the reference's checkpoints are (``bert.`` prefix, ``gamma`` / ``beta``) and refuses a model name without any network
call, every unsupported use raises, install(bert=True) serves ``matchzoo.modules.BertModule``, and the C-ABI declares the new entries
at an unchanged ABI version."""
import json
import os
import re
import socket

import numpy as np
import pytest
import torch

from tests import bert_ref
from tests.util import ROOT, load_golden, rel_close, run_in_fresh_interpreter

CASES = {"h24_l2_L70": "h24", "h18_l1_L5": "h18", "h24_L1": "h24", "bertmodule_cat": "h24", "mask_half": "h24"}
ENTRIES = ("gh_bert_attention_fwd", "gh_bert_attention_bwd", "gh_act_fwd", "gh_act_bwd", "gh_bert_embed_fwd")


def _archive(golden_dir):
    return load_golden(golden_dir, "g21_bert.npz", "bert_contract.json")


def case_inputs(z, name):
    """(ids, token types or None, mask or None) of a golden case as torch tensors; bertmodule_cat: cat((x, y), -1)."""
    key = name + "::"
    if key + "x" in z:
        return torch.cat((torch.from_numpy(z[key + "x"]), torch.from_numpy(z[key + "y"])), -1), None, None
    return tuple(torch.from_numpy(z[key + k]) for k in ("input_ids", "token_type_ids", "attention_mask"))


def case_params(z, name, dtype=torch.float32):
    pre = name + "::param::"
    return {k[len(pre):]: torch.from_numpy(z[k]).to(dtype) for k in z if k.startswith(pre)}


def want64(z, name, k):
    """The reference's float64 result of `k`: its fp32 result plus the stored residual."""
    return torch.from_numpy(z[f"{name}::{k}"]).double() + torch.from_numpy(z[f"{name}::resid::{k}"]).double()


def test_bert_golden_archive_is_complete(golden_dir):
    z, meta, contract = _archive(golden_dir)
    assert meta["cases"] == CASES and set(contract) == {"h24", "h18"}
    for name, conf in CASES.items():
        key = name + "::"
        have = {k[len(key):] for k in z if k.startswith(key)}
        assert {"sequence_output", "pooled_output", "g_seq", "g_pooled"} <= have, name
        params = {k[len("param::"):] for k in have if k.startswith("param::")}
        assert params == {k for k, _ in contract[conf]["state_dict"]}
        for k in params:
            assert "grad::" + k in have and "resid::grad::" + k in have, (name, k)
    ids, types, mask = case_inputs(z, "h24_l2_L70")
    assert ids.shape == (2, 70) and len(types.unique()) == 2 and bool((mask[1, 41:] == 0).all()) and bool((mask[0] == 1).all())
    ids, _, mask = case_inputs(z, "h18_l1_L5")
    assert ids.shape == (3, 5) and float(mask[2].sum()) == 0 and float(mask[0].sum()) == 1 and bool((mask[1] == 1).all())
    assert case_inputs(z, "h24_L1")[0].shape == (2, 1)
    assert z["bertmodule_cat::x"].shape == (2, 7) and z["bertmodule_cat::y"].shape == (2, 30)
    mask = case_inputs(z, "mask_half")[2]
    assert bool((mask == 0.5).any()) and bool(((mask > 0.5) & (mask < 1)).any())
    for k in z:
        if k != "meta":
            assert np.isfinite(z[k]).all(), k
    assert os.path.getsize(os.path.join(golden_dir, "g21_bert.npz")) < 1 << 20


@pytest.mark.parametrize("name", list(CASES))
def test_float64_restatement_reproduces_the_bert_goldens(golden_dir, name):
    """tests/bert_ref.py alone, in float64 on the archive's inputs and parameters, against the reference's float64 outputs and
    parameter gradients: largest error over largest entry <= 1e-9."""
    z, meta, contract = _archive(golden_dir)
    p64 = {k: v.requires_grad_(True) for k, v in case_params(z, name, torch.float64).items()}
    ids, types, mask = case_inputs(z, name)
    seq, pooled, _ = bert_ref.model(p64, contract[CASES[name]]["config"], ids, types, mask)
    g_seq, g_pooled = (torch.from_numpy(z[f"{name}::{k}"]).double() for k in ("g_seq", "g_pooled"))
    ((seq * g_seq).sum() + (pooled * g_pooled).sum()).backward()
    rel_close(seq, want64(z, name, "sequence_output"), 1e-9, name + " sequence_output")
    rel_close(pooled, want64(z, name, "pooled_output"), 1e-9, name + " pooled_output")
    for k, t in p64.items():
        want = want64(z, name, "grad::" + k)
        if k.endswith("self.key.bias"):      # a shift of a row's scores leaves its softmax alone: O(1) terms cancel to zero
            assert float(t.grad.abs().max()) <= 1e-9 and float(want.abs().max()) <= 1e-9, k
        else:
            rel_close(t.grad, want, 1e-9, f"{name} grad::{k}")


def test_restatement_attends_by_raw_scores_under_a_full_mask():
    """A row whose keys all carry the bias -10000 is the softmax of its raw scores: the bias cancels, nothing is zero."""
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(2, 5, 6, generator=g).double() for _ in range(3))
    bias = torch.zeros(2, 5).double()
    bias[1] = -10000.0
    out, lse = bert_ref.attention(q, k, v, bias, 3, 0.5)
    free, lse0 = bert_ref.attention(q, k, v, None, 3, 0.5)
    assert float((out - free).abs().max()) <= 1e-10 and float((lse[0] - lse0[0]).abs().max()) <= 1e-12
    assert float((lse[1] - lse0[1] + 10000.0).abs().max()) <= 1e-9
    keep = torch.ones(2, 3, 5, 5, dtype=torch.bool)
    keep[0, 1, 2, :] = False
    dropped, _ = bert_ref.attention(q, k, v, bias, 3, 0.5, keep, 0.5)
    assert float(dropped[0, 2, 2:4].abs().max()) == 0 and float((dropped[1] - 2 * out[1]).abs().max()) <= 1e-12


def test_bert_state_dicts_match_the_reference_contract(golden_dir):
    from get_amd.bert import BertConfig, BertModel
    _, _, contract = _archive(golden_dir)
    for conf, c in contract.items():
        assert c["class"] == "BertModel"
        cfg = BertConfig.from_dict(c["config"])
        m = BertModel(cfg)
        got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert got == c["state_dict"], conf
        assert len(got) == 5 + 16 * cfg.num_hidden_layers + 2
    keys = [k for k, _ in contract["h18"]["state_dict"]]
    assert keys[:5] == ["embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight",
                        "embeddings.token_type_embeddings.weight", "embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"]
    assert keys[5] == "encoder.layer.0.attention.self.query.weight" and keys[-2:] == ["pooler.dense.weight", "pooler.dense.bias"]


def test_random_init_follows_init_weights():
    from get_amd.bert import BertConfig, BertModel
    torch.manual_seed(5)
    m = BertModel(BertConfig(200, hidden_size=64, num_hidden_layers=1, num_attention_heads=4, intermediate_size=128,
                             initializer_range=0.05))
    sd = m.state_dict()
    for k, v in sd.items():
        if "LayerNorm.weight" in k:
            assert bool((v == 1).all()), k
        elif k.endswith("bias"):
            assert bool((v == 0).all()), k
        else:
            assert 0.04 < float(v.std()) < 0.06 and abs(float(v.mean())) < 0.01, k
    assert float(sd["embeddings.word_embeddings.weight"][0].abs().max()) > 0      # (the padding row is drawn too, as upstream)


def test_bert_config_round_trips_a_config_json(tmp_path):
    from get_amd.bert import BertConfig
    cfg = BertConfig(99, hidden_size=32, num_hidden_layers=3, num_attention_heads=4, intermediate_size=64, hidden_act="relu",
                     hidden_dropout_prob=0.2, attention_probs_dropout_prob=0.3, max_position_embeddings=40, type_vocab_size=3,
                     initializer_range=0.1, layer_norm_eps=1e-6, output_hidden_states=True)
    assert cfg.vocab_size == 99 and cfg.output_hidden_states and not cfg.output_attentions
    cfg.save_pretrained(str(tmp_path))
    path = os.path.join(str(tmp_path), "config.json")
    assert json.load(open(path))["intermediate_size"] == 64
    for back in (BertConfig.from_json_file(path), BertConfig(path)):
        assert back == cfg and back.to_dict() == cfg.to_dict()
    assert BertConfig(vocab_size=7).vocab_size == 7 and BertConfig().hidden_size == 768
    with pytest.raises(ValueError, match="first argument"):
        BertConfig(1.5)
    with pytest.raises(TypeError, match="unknown arguments"):
        BertConfig(10, hidden=3)


def _checkpoint_dir(tmp_path, z, contract, name="h18_l1_L5"):
    """A directory as the reference's from_pretrained reads it, with the keys an upstream BertForPreTraining checkpoint has:
    a `bert.` prefix, LayerNorm `gamma` / `beta`, and a head the encoder does not own."""
    d = os.path.join(str(tmp_path), "ckpt")
    os.makedirs(d)
    with open(os.path.join(d, "config.json"), "w") as fh:
        json.dump(contract[CASES[name]]["config"], fh)
    state = {}
    for k, v in case_params(z, name).items():
        k = k.replace("LayerNorm.weight", "LayerNorm.gamma").replace("LayerNorm.bias", "LayerNorm.beta")
        state["bert." + k] = v
    state["cls.seq_relationship.weight"] = torch.zeros(2, 18)
    torch.save(state, os.path.join(d, "pytorch_model.bin"))
    return d


def test_bertmodule_loads_a_checkpoint_directory(tmp_path, golden_dir):
    from get_amd import modules
    from get_amd.bert import BertModel
    z, _, contract = _archive(golden_dir)
    d = _checkpoint_dir(tmp_path, z, contract)
    m = modules.BertModule(d)
    assert isinstance(m.bert, BertModel) and not m.bert.training and m.bert.config.hidden_size == 18
    want = case_params(z, "h18_l1_L5")
    got = m.bert.state_dict()
    assert list(got) == [k for k, _ in contract["h18"]["state_dict"]]
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    assert [k for k, _ in m.state_dict().items()] == ["bert." + k for k in got]
    # the model's own save / load round trip
    out = os.path.join(str(tmp_path), "saved")
    os.makedirs(out)
    m.bert.save_pretrained(out)
    again = BertModel.from_pretrained(out)
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in got.items()) and again.config == m.bert.config
    # a key the file lacks keeps its initialisation, loudly
    state = torch.load(os.path.join(d, "pytorch_model.bin"), weights_only=True)
    del state["bert.pooler.dense.bias"]
    torch.save(state, os.path.join(d, "pytorch_model.bin"))
    with pytest.warns(UserWarning, match="pooler.dense.bias"):
        modules.BertModule(d)
    os.remove(os.path.join(d, "pytorch_model.bin"))
    with pytest.raises(ValueError, match="pytorch_model.bin"):
        modules.BertModule(d)


def test_checkpoint_keys_are_renamed_by_the_two_rules():
    from get_amd.bert import BertConfig, BertModule, checkpoint_key
    assert checkpoint_key("bert.embeddings.LayerNorm.gamma") == "embeddings.LayerNorm.weight"
    assert checkpoint_key("encoder.layer.3.output.LayerNorm.beta") == "encoder.layer.3.output.LayerNorm.bias"
    assert checkpoint_key("bert.pooler.dense.weight") == "pooler.dense.weight"
    assert checkpoint_key("cls.predictions.bias") == "cls.predictions.bias" and checkpoint_key("gamma") == "weight"
    # a config builds a model for training; a directory gives one in eval mode (test_bertmodule_loads_a_checkpoint_directory)
    assert BertModule(BertConfig(20, hidden_size=8, num_hidden_layers=1, num_attention_heads=2, intermediate_size=8)).bert.training


def test_bertmodule_refuses_a_model_name_without_any_network_call(monkeypatch):
    from get_amd import modules

    def no_network(*a, **k):
        raise AssertionError("a network call was attempted")
    monkeypatch.setattr(socket, "socket", no_network)
    monkeypatch.setattr(socket, "create_connection", no_network)
    monkeypatch.setattr(socket, "getaddrinfo", no_network)
    for mode in ("bert-base-uncased", "bert-large-cased"):
        with pytest.raises(ValueError, match="Nothing is ever downloaded"):
            modules.BertModule(mode)
    with pytest.raises(ValueError, match="Nothing is ever downloaded"):
        modules.BertModule()
    with pytest.raises(ValueError, match="Nothing is ever downloaded"):
        modules.BertModel.from_pretrained("bert-base-uncased")


def test_unsupported_uses_raise():
    from get_amd.bert import BertConfig, BertModel, BertModule
    small = dict(hidden_size=8, num_hidden_layers=1, num_attention_heads=2, intermediate_size=8, max_position_embeddings=6)
    m = BertModel(BertConfig(20, **small))
    ids = torch.ones(2, 4, dtype=torch.long)
    with pytest.raises(ValueError, match="head_mask"):
        m(ids, head_mask=torch.ones(2))
    with pytest.raises(ValueError, match="output_attentions"):
        BertModel(BertConfig(20, output_attentions=True, **small))
    m.config.output_attentions = True          # set after construction: refused in forward
    with pytest.raises(ValueError, match="output_attentions"):
        m(ids)
    m.config.output_attentions = False
    for act in ("swish", "tanh"):
        with pytest.raises(ValueError, match="hidden_act"):
            BertModel(BertConfig(20, hidden_act=act, **small))
    BertModel(BertConfig(20, hidden_act="relu", **small))
    with pytest.raises(ValueError, match="max_position_embeddings"):
        m(torch.ones(2, 7, dtype=torch.long))
    with pytest.raises(ValueError, match="not divisible by num_attention_heads"):
        BertModel(BertConfig(20, hidden_size=9, num_hidden_layers=1, num_attention_heads=2, intermediate_size=8))
    with pytest.raises(ValueError, match="BertConfig"):
        BertModel({"hidden_size": 8})
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(ids)
    with pytest.raises(RuntimeError, match="no CPU path"):
        BertModule(BertConfig(20, **small))(ids, ids[:, :2])


def test_bert_ops_refuse_cpu_tensors():
    from get_amd import ops
    x = torch.zeros(2, 3, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.bert_attention(x, x, x, None, 2, 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.gelu(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.tanh_act(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.bert_embed(torch.zeros(5, 8), torch.zeros(4, 8), torch.zeros(2, 8), torch.zeros(2, 3, dtype=torch.long), None, None,
                       torch.ones(8), torch.zeros(8))


def test_install_serves_bertmodule(tmp_path):
    """install(bert=True): a plain install() keeps raising ImportError for BertModule (tests/test_match_cpu.py pins that)."""
    run_in_fresh_interpreter(tmp_path, r"""
try:
    from matchzoo.modules import BertModule
except ImportError:
    pass
else:
    raise AssertionError('a plain install() serves what it served before')
M = get_amd.install(bert=True)
from matchzoo.modules import BertModule, Attention
import get_amd.bert
assert BertModule is M.BertModule is get_amd.bert.BertModule and Attention is M.Attention
assert 'pytorch_transformers' not in sys.modules, 'pytorch_transformers must not be shimmed'
try:
    BertModule('bert-base-uncased')
except ValueError as e:
    assert 'directory' in str(e)
else:
    raise AssertionError('a model name must be refused')
""", packages=("matchzoo",))


def test_header_declares_the_bert_entries_at_abi_10():
    from get_amd import _lib
    src = open(os.path.join(ROOT, "include", "get_hip.h")).read()
    assert re.search(r"#define\s+GH_ABI_VERSION\s+10\b", src) and _lib.ABI_VERSION == 10
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, plain, flags=re.S)
        assert m, name + " is not declared in include/get_hip.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name]), name
    assert re.search(r"#define\s+GH_ACT_GELU\s+0\b", src) and re.search(r"#define\s+GH_ACT_TANH\s+1\b", src)
    for name in ENTRIES[:2]:      # each declaration cites the reference lines it replaces
        doc = src[:src.index("int " + name)]
        assert ":203-228" in doc[doc.rindex("/*"):], name
    mk = open(os.path.join(ROOT, "get_amd", "csrc", "Makefile")).read()
    assert "bert_ops.hip" in mk

"""CPU-side checks of the BERT task heads (get_amd/bert.py: the five head blocks and the seven task models): the float64
restatement the GPU tests compare the kernels with (tests/heads_ref.py) reproduces the reference's goldens on its own and
torch's cross_entropy with its edge cases; every class builds the reference's state_dict (tests/golden/bert_heads_contract.json);
the decoder stays tied to the word table through load_state_dict, from_pretrained and the optimiser's bucket; from_pretrained
reads prefixed and bare checkpoints with `gamma` / `beta` names, warns about a missing head and refuses a model name; and the
dispatch thresholds the GPU path tests use are the kernel file's constants.

Two tests here run no code of the feature itself -- num_labels through a config.json (BertConfig carried arbitrary fields before)
and the restated loss against torch's -- and are kept because the feature leans on both; the file imports tests/heads_ref.py, so
without the feature it fails as a whole."""
import json
import math
import os
import re
import socket
import warnings

import numpy as np
import pytest
import torch

from tests import heads_ref
from tests.util import ROOT, load_golden, rel_close

ENTRIES = ("gh_softmax_xent_fwd", "gh_softmax_xent_bwd", "gh_clamp_events_n")
CLASSES = ("BertForPreTraining", "BertForMaskedLM", "BertForNextSentencePrediction", "BertForSequenceClassification",
           "BertForMultipleChoice", "BertForTokenClassification", "BertForQuestionAnswering")
CASES = {"pretraining": "pretraining_h18", "mlm_labels": "mlm_v131", "mlm_plain": "mlm_v131", "nsp": "nsp_h18",
         "seqcls_n1": "seqcls_h18_n1", "seqcls_n2": "seqcls_h24_n2", "seqcls_n5": "seqcls_h18_n5", "choice": "choice_h18",
         "tokcls_mask": "tokcls_h18_n5", "tokcls_plain": "tokcls_h18_n5", "qa": "qa_h18"}
CANCELS = {"qa": ("qa_outputs.bias", "bert.encoder.layer.0.output.LayerNorm.bias"), "choice": ("classifier.bias",)}
TIED = ["bert.embeddings.word_embeddings.weight", "cls.predictions.decoder.weight"]


def archive(golden_dir):
    return load_golden(golden_dir, "g23_bert_heads.npz", "bert_heads_contract.json")


def case_inputs(z, name):
    """The forward's keyword arguments of a golden case as torch tensors."""
    pre = name + "::input::"
    return {k[len(pre):]: torch.from_numpy(z[k]) for k in z if k.startswith(pre)}


def pset_params(z, pset, dtype=torch.float32):
    """The parameters of a parameter set by named_parameters name (a tied weight once, under the word table's name)."""
    pre = f"pset::{pset}::param::"
    return {k[len(pre):]: torch.from_numpy(z[k]).to(dtype) for k in z if k.startswith(pre)}


def state_of(params, contract_entry):
    """`params` under every state_dict key of the contract: an alias holds the tensor of the key that is stored."""
    out = dict(params)
    for group in contract_entry["aliases"]:
        have = [k for k in group if k in params]
        for k in group:
            out[k] = params[have[0]]
    return out


def case_outputs(z, name):
    n = len([k for k in z if k.startswith(name + "::out::")])
    return [z[f"{name}::out::{i}"] for i in range(n)]


def as_stored(t):
    """A result as the archive holds it: a scalar (the loss) is stored as one element."""
    return t.reshape(1) if t.dim() == 0 else t


def want64(z, name, k):
    return torch.from_numpy(z[f"{name}::{k}"]).double() + torch.from_numpy(z[f"{name}::resid::{k}"]).double()


def has_labels(inputs):
    return any(k.endswith("labels") or k.endswith("label") or k.endswith("positions") for k in inputs)


def objective(z, meta, name, out, dtype):
    """What the generator differentiated: gs * loss with labels, else sum_i sum(out_i * g_i)."""
    if has_labels(case_inputs(z, name)):
        return out[0] * meta["scales"][CASES[name]]["loss_or_upstream_gradients"]
    return sum((t * torch.from_numpy(z[f"{name}::g::{i}"]).to(dtype).to(t.device)).sum() for i, t in enumerate(out))


def small_config(**fields):
    from get_amd.bert import BertConfig
    return BertConfig(20, hidden_size=8, num_hidden_layers=1, num_attention_heads=2, intermediate_size=8, max_position_embeddings=6,
                      **fields)


# ----------------------------------------------------------------------------- the archive and the restatement
def test_heads_golden_archive_is_complete(golden_dir):
    z, meta, contract = archive(golden_dir)
    assert meta["cases"] == CASES and set(contract) == set(CASES.values())
    assert {contract[p]["class"] for p in contract} == set(CLASSES)
    assert {contract[p]["config"]["num_labels"] for p in contract if "seqcls" in p} == {1, 2, 5}
    assert contract["mlm_v131"]["config"]["vocab_size"] == 131 and contract["seqcls_h24_n2"]["config"]["hidden_size"] == 24
    for name, pset in CASES.items():
        params = set(pset_params(z, pset))
        keys = {k for k, _ in contract[pset]["state_dict"]}
        assert params <= keys and keys - params <= {"cls.predictions.decoder.weight"}, name
        have = {k[len(name) + 2:] for k in z if k.startswith(name + "::")}
        grads = {k[len("grad::"):] for k in have if k.startswith("grad::")}
        assert params - grads <= {"bert.pooler.dense.weight", "bert.pooler.dense.bias"}, (name, params - grads)
        for k in grads:
            assert "resid::grad::" + k in have
        assert "out::0" in have and "resid::out::0" in have
    for pset in ("pretraining_h18", "mlm_v131"):
        assert contract[pset]["aliases"] == [TIED]
    for pset in set(CASES.values()) - {"pretraining_h18", "mlm_v131"}:
        assert contract[pset]["aliases"] == []
    lab = z["pretraining::input::masked_lm_labels"]
    assert (lab[1] == -1).all() and (lab[0] == -1).any() and (lab[0] != -1).any() and (z["pretraining::input::next_sentence_label"] == -1).sum() == 1
    assert "mlm_plain::input::masked_lm_labels" not in z and (z["mlm_labels::input::masked_lm_labels"] == -1).any()
    assert z["choice::input::input_ids"].shape == (2, 3, 6)
    mask = z["tokcls_mask::input::attention_mask"]
    assert (mask[0] == 1).all() and (mask[1, 5:] == 0).all() and "tokcls_plain::input::attention_mask" not in z
    sp, ep = z["qa::input::start_positions"], z["qa::input::end_positions"]
    assert sp.shape == (3, 1) and (sp > 10).any() and (ep < 0).any()
    for k in z:
        if k != "meta":
            assert np.isfinite(z[k]).all(), k
    # no larger than the largest archive committed before it
    assert os.path.getsize(os.path.join(golden_dir, "g23_bert_heads.npz")) <= os.path.getsize(os.path.join(golden_dir, "g17_match.npz")) < 1 << 20


@pytest.mark.parametrize("name", list(CASES))
def test_float64_restatement_reproduces_the_heads_goldens(golden_dir, name):
    """tests/heads_ref.py alone, in float64 on the archive's inputs and parameters, against the reference's float64 outputs and
    parameter gradients: largest error over largest entry <= 1e-9."""
    z, meta, contract = archive(golden_dir)
    c = contract[CASES[name]]
    p64 = {k: v.requires_grad_(True) for k, v in pset_params(z, CASES[name], torch.float64).items()}
    out = heads_ref.task_model(c["class"], state_of(p64, c), c["config"], case_inputs(z, name))
    assert len(out) == len(case_outputs(z, name))
    for i, t in enumerate(out):
        rel_close(as_stored(t), want64(z, name, f"out::{i}"), 1e-9, f"{name} out::{i}")
    objective(z, meta, name, out, torch.float64).backward()
    for k, t in p64.items():
        if f"{name}::grad::{k}" not in z:
            assert t.grad is None, k
            continue
        want = want64(z, name, "grad::" + k)
        # a shift of a row's scores leaves its softmax alone, so O(1) terms cancel to zero: the key bias everywhere, and where the
        # softmax runs over the positions or the choices the head's bias and the last LayerNorm's
        if k.endswith("self.key.bias") or k in CANCELS.get(name, ()):
            assert float(t.grad.abs().max()) <= 1e-9 and float(want.abs().max()) <= 1e-9, k
        else:
            rel_close(t.grad, want, 1e-9, f"{name} grad::{k}")


def test_restated_loss_is_torchs_with_the_edge_cases_pinned():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(9, 7, generator=g).double().requires_grad_(True)
    for ignore, y in ((-100, [0, 3, -100, 6, 2, -100, 1, 1, 5]), (-1, [-1, 3, 0, 6, 2, 4, 1, 1, -1]), (7, [7, 3, 0, 6, 2, 7, 1, 1, 5])):
        y = torch.tensor(y)
        loss, lse, n = heads_ref.xent(x, y, ignore)
        want = torch.nn.functional.cross_entropy(x, y, ignore_index=ignore)
        assert abs(float((loss - want).detach())) <= 1e-14 and n == 7
        gx, = torch.autograd.grad(want * 0.3, x)
        assert float((heads_ref.xent_grad(x.detach(), y, lse.detach(), n, 0.3, ignore) - gx).abs().max()) <= 1e-15
    # every row ignored: NaN loss (0 / 0), zero gradient -- torch's own answer
    y = torch.full((9,), -100)
    loss, lse, n = heads_ref.xent(x, y)
    want = torch.nn.functional.cross_entropy(x, y)
    assert n == 0 and math.isnan(float(loss)) and math.isnan(float(want))
    assert float(torch.autograd.grad(want, x)[0].abs().max()) == 0
    assert float(heads_ref.xent_grad(x.detach(), y, lse.detach(), n, 1.0).abs().max()) == 0
    # c = 1: loss 0, gradient 0
    x1 = torch.randn(4, 1, generator=g).double().requires_grad_(True)
    y1 = torch.zeros(4, dtype=torch.long)
    loss, lse, n = heads_ref.xent(x1, y1)
    want = torch.nn.functional.cross_entropy(x1, y1)
    assert float(loss) == 0 == float(want) and float(torch.autograd.grad(want, x1)[0].abs().max()) == 0
    assert float(heads_ref.xent_grad(x1.detach(), y1, lse.detach(), n, 1.0).abs().max()) == 0
    # a label outside [0, c) that is not the ignore index: torch raises, the restatement drops the row
    y = torch.tensor([0, 3, 9, 6, 2, -100, 1, -2, 5])
    with pytest.raises((IndexError, RuntimeError)):
        torch.nn.functional.cross_entropy(x, y)
    ok = torch.tensor([0, 3, -100, 6, 2, -100, 1, -100, 5])
    assert float(heads_ref.xent(x, y)[0]) == float(heads_ref.xent(x, ok)[0]) and heads_ref.xent(x, y)[2] == 6


# ----------------------------------------------------------------------------- the classes on the CPU
def test_every_class_builds_the_contracts_state_dict(golden_dir):
    from get_amd import bert, modules
    _, _, contract = archive(golden_dir)
    for pset, c in contract.items():
        cls = getattr(bert, c["class"])
        assert getattr(modules, c["class"]) is cls
        m = cls(bert.BertConfig.from_dict(c["config"]))
        sd = m.state_dict()
        assert [[k, list(v.shape)] for k, v in sd.items()] == c["state_dict"], pset
        groups = {}
        for k, v in sd.items():
            groups.setdefault(v.data_ptr(), []).append(k)
        assert sorted(sorted(g) for g in groups.values() if len(g) > 1) == c["aliases"], pset
        assert m.config.num_labels == c["config"]["num_labels"]
    for name in ("BertPredictionHeadTransform", "BertLMPredictionHead", "BertOnlyMLMHead", "BertOnlyNSPHead", "BertPreTrainingHeads"):
        block = getattr(bert, name)(small_config())
        assert getattr(modules, name) is type(block) and len(block.state_dict()) > 0
    assert list(bert.BertLMPredictionHead(small_config()).state_dict()) == [
        "bias", "transform.dense.weight", "transform.dense.bias", "transform.LayerNorm.weight", "transform.LayerNorm.bias", "decoder.weight"]


def test_num_labels_round_trips_through_a_config_json(tmp_path):
    from get_amd.bert import BertConfig
    cfg = small_config(num_labels=5)
    cfg.save_pretrained(str(tmp_path))
    assert BertConfig.from_json_file(os.path.join(str(tmp_path), "config.json")).num_labels == 5
    assert json.load(open(os.path.join(str(tmp_path), "config.json")))["num_labels"] == 5


def test_head_initialisation_follows_init_weights():
    from get_amd.bert import BertForPreTraining, BertForTokenClassification
    torch.manual_seed(3)
    from get_amd.bert import BertConfig
    cfg = BertConfig(300, hidden_size=64, num_hidden_layers=1, num_attention_heads=4, intermediate_size=64, initializer_range=0.05,
                     num_labels=40)
    for m in (BertForPreTraining(cfg), BertForTokenClassification(cfg)):
        for k, v in m.state_dict().items():
            if k.startswith("bert."):
                continue
            if "LayerNorm.weight" in k:
                assert bool((v == 1).all()), k
            elif k.endswith("bias"):
                assert bool((v == 0).all()), k
            else:
                assert 0.04 < float(v.std()) < 0.06, k


def test_the_decoder_is_the_word_table(tmp_path, golden_dir):
    from get_amd.bert import BertConfig, BertForMaskedLM, BertForPreTraining
    z, _, contract = archive(golden_dir)
    for cls, pset in ((BertForMaskedLM, "mlm_v131"), (BertForPreTraining, "pretraining_h18")):
        c = contract[pset]
        m = cls(BertConfig.from_dict(c["config"]))
        tied = lambda mod: mod.cls.predictions.decoder.weight is mod.bert.embeddings.word_embeddings.weight
        assert tied(m)
        names = [k for k, _ in m.named_parameters()]
        assert TIED[0] in names and TIED[1] not in names and len(names) == len(set(names)) == len(c["state_dict"]) - 1
        sd = m.state_dict()
        assert sd[TIED[0]].data_ptr() == sd[TIED[1]].data_ptr()
        params = pset_params(z, pset)
        m.load_state_dict(state_of(params, c), strict=True)
        assert tied(m) and torch.equal(m.cls.predictions.decoder.weight, params[TIED[0]])
        # a state_dict whose two entries differ (an untied checkpoint): the tie holds, the later key's values win
        loose = state_of(params, c)
        loose[TIED[1]] = loose[TIED[1]] + 1.0
        m.load_state_dict(loose)
        assert tied(m)
        assert tied(m.to(torch.float64)) and tied(m.float())
        d = os.path.join(str(tmp_path), pset)
        os.makedirs(d)
        m.load_state_dict(state_of(params, c))
        m.save_pretrained(d)
        again = cls.from_pretrained(d)
        assert tied(again) and not again.training and again.config == m.config
        for k, v in m.state_dict().items():
            assert torch.equal(v, again.state_dict()[k]), k


def _write_checkpoint(d, config, state):
    os.makedirs(d)
    with open(os.path.join(d, "config.json"), "w") as fh:
        json.dump(config, fh)
    torch.save(state, os.path.join(d, "pytorch_model.bin"))
    return d


def test_from_pretrained_reads_prefixed_and_bare_checkpoints(tmp_path, golden_dir):
    from get_amd.bert import BertForMaskedLM, BertForSequenceClassification, BertModel
    z, _, contract = archive(golden_dir)
    c = contract["mlm_v131"]
    params = pset_params(z, "mlm_v131")
    tf_name = lambda k: k.replace("LayerNorm.weight", "LayerNorm.gamma").replace("LayerNorm.bias", "LayerNorm.beta")
    # a task model's own checkpoint, TensorFlow-era names, the tied key absent
    d = _write_checkpoint(os.path.join(str(tmp_path), "prefixed"), c["config"], {tf_name(k): v for k, v in params.items()})
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = BertForMaskedLM.from_pretrained(d)
    assert not m.training and m.cls.predictions.decoder.weight is m.bert.embeddings.word_embeddings.weight
    for k, v in state_of(params, c).items():
        assert torch.equal(m.state_dict()[k], v), k
    # the encoder of that checkpoint still loads into a bare BertModel, and into another task model with a warning for its head
    assert torch.equal(BertModel.from_pretrained(d).state_dict()["pooler.dense.weight"], params["bert.pooler.dense.weight"])
    with pytest.warns(UserWarning, match="classifier.weight"):
        s = BertForSequenceClassification.from_pretrained(d)
    assert torch.equal(s.bert.encoder.layer[0].output.dense.weight, params["bert.encoder.layer.0.output.dense.weight"])
    # a bare BertModel checkpoint fills the encoder alone: the head keeps its initialisation, loudly
    bare = {tf_name(k[len("bert."):]): v for k, v in params.items() if k.startswith("bert.")}
    d2 = _write_checkpoint(os.path.join(str(tmp_path), "bare"), c["config"], bare)
    with pytest.warns(UserWarning, match="cls.predictions.transform.dense.weight") as rec:
        m2 = BertForMaskedLM.from_pretrained(d2)
    assert "decoder.weight" not in str(rec[0].message) and "bert." not in str(rec[0].message)
    assert torch.equal(m2.bert.embeddings.LayerNorm.weight, params["bert.embeddings.LayerNorm.weight"])
    assert m2.cls.predictions.decoder.weight is m2.bert.embeddings.word_embeddings.weight
    assert torch.equal(m2.cls.predictions.decoder.weight, params[TIED[0]])
    os.remove(os.path.join(d2, "pytorch_model.bin"))
    with pytest.raises(ValueError, match="pytorch_model.bin"):
        BertForMaskedLM.from_pretrained(d2)


def test_task_models_refuse_a_model_name_without_any_network_call(monkeypatch):
    from get_amd import bert

    def no_network(*a, **k):
        raise AssertionError("a network call was attempted")
    monkeypatch.setattr(socket, "socket", no_network)
    monkeypatch.setattr(socket, "create_connection", no_network)
    monkeypatch.setattr(socket, "getaddrinfo", no_network)
    for cls in bert.TASK_MODELS:
        with pytest.raises(ValueError, match="Nothing is ever downloaded"):
            cls.from_pretrained("bert-base-uncased")
    assert [c.__name__ for c in bert.TASK_MODELS] == list(CLASSES)


def test_adamw_holds_the_tied_tensor_once():
    from get_amd.bert import BertForMaskedLM
    from get_amd.optim import AdamW
    m = BertForMaskedLM(small_config())
    opt = AdamW(m.parameters(), lr=1e-3)
    held = [p for group in opt.param_groups for p in group["params"]]
    word = m.bert.embeddings.word_embeddings.weight
    assert sum(p is word for p in held) == 1 and len(held) == len({id(p) for p in held}) == len(list(m.named_parameters()))
    assert m.cls.predictions.decoder.weight is word


def test_unsupported_uses_of_the_task_models_raise():
    from get_amd import bert
    ids = torch.ones(2, 4, dtype=torch.long)
    for cls in bert.TASK_MODELS:
        m = cls(small_config())
        x = ids.view(1, 2, 4) if cls is bert.BertForMultipleChoice else ids
        with pytest.raises(ValueError, match="head_mask"):
            m(x, head_mask=torch.ones(2))
        with pytest.raises(RuntimeError, match="no CPU path"):
            m(x)
        with pytest.raises(ValueError, match="output_attentions"):
            cls(small_config(output_attentions=True))
        with pytest.raises(ValueError, match="BertConfig"):
            cls({"hidden_size": 8})
    from get_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.softmax_cross_entropy(torch.zeros(2, 3), torch.zeros(2, dtype=torch.long))


# ----------------------------------------------------------------------------- the kernel file and the C-ABI
def test_path_thresholds_are_the_kernel_files_constants():
    """tests/test_gpu_loss_paths.py places its widths around these two; the header's prose names them too."""
    from tests import test_gpu_loss_paths as paths
    src = open(os.path.join(ROOT, "get_amd", "csrc", "loss_ops.hip")).read()
    const = lambda name: int(re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, src).group(1))
    assert const("XENT_LANE_MAX_C") == paths.LANE_MAX_C and const("XENT_WAVE_MAX_C") == paths.WAVE_MAX_C
    assert const("XENT_THREADS") == 256
    assert "c <= XENT_LANE_MAX_C" in src and "c <= XENT_WAVE_MAX_C" in src
    for t in (paths.LANE_MAX_C, paths.WAVE_MAX_C):
        assert {t - 1, t, t + 1} <= set(paths.WIDTHS)
    header = open(os.path.join(ROOT, "include", "get_hip.h")).read()
    assert f"<= {paths.LANE_MAX_C} one lane per row, <= {paths.WAVE_MAX_C} one wave per row" in header


def test_header_declares_the_loss_entries_at_abi_10():
    from get_amd import _lib
    src = open(os.path.join(ROOT, "include", "get_hip.h")).read()
    assert re.search(r"#define\s+GH_ABI_VERSION\s+10\b", src) and _lib.ABI_VERSION == 10
    plain = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, plain, flags=re.S)
        assert m, name + " is not declared in include/get_hip.h"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name]), name
    doc = src[:src.index("int gh_softmax_xent_fwd")]
    assert "modeling_bert.py" in doc[doc.rindex("/*"):] and ":1142" in doc[doc.rindex("/*"):]
    assert re.search(r"#define\s+GH_CLAMP_SLOTS\s+5\b", src)
    assert "loss_ops.hip" in open(os.path.join(ROOT, "get_amd", "csrc", "Makefile")).read()

"""The BERT encoder drop-in (get_amd/bert.py: BertModel, BertModule) on the GPU against the reference's golden vectors
(tests/golden/g21_bert.npz, captured by tools/make_bert_golden.py) and, in training mode, against the float64 restatement of
tests/bert_ref.py fed the dropout masks ops.dropout_mask_reference predicts.

Bounds, elementwise against the reference's fp32 result: outputs 1e-4 + 1e-4 |want|, parameter gradients 1e-5 + 1e-4 |want| (the
multi-head attention family's; the generator holds the reference's own fp32-vs-float64 error to a tenth of them, rescaling a
case's upstream gradients or weights where it has to -- the scales are in the archive's meta).  The training-mode case is held
to the same two bounds against float64."""
import pytest
import torch

from tests import bert_ref
from tests.test_bert_cpu import CASES, case_inputs, case_params
from tests.util import DEV, bits_equal, golden_ratio, load_golden

pytestmark = pytest.mark.gpu

OUT_TOL, GRAD_TOL = (1e-4, 1e-4), (1e-5, 1e-4)


def _archive(golden_dir):
    return load_golden(golden_dir, "g21_bert.npz", "bert_contract.json")


def _build(z, contract, name, **config_changes):
    from get_amd.bert import BertConfig, BertModel
    conf = dict(contract[CASES[name]]["config"], **config_changes)
    m = BertModel(BertConfig.from_dict(conf))
    m.load_state_dict(case_params(z, name), strict=True)
    return m.to(DEV).eval()


def _forward(m, z, name, int32=False):
    ids, types, mask = (t.to(DEV) if t is not None else None for t in case_inputs(z, name))
    if int32:
        ids, types = ids.int(), (types.int() if types is not None else None)
    return m(ids, token_type_ids=types, attention_mask=mask)


def _backward(m, z, name, seq, pooled):
    m.zero_grad(set_to_none=True)
    g_seq, g_pooled = (torch.from_numpy(z[f"{name}::{k}"]).to(DEV) for k in ("g_seq", "g_pooled"))
    ((seq * g_seq).sum() + (pooled * g_pooled).sum()).backward()
    torch.cuda.synchronize()
    return {k: p.grad.clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("name", list(CASES))
def test_golden_case_through_the_drop_in(golden_dir, name):
    """Outputs and every parameter gradient of every golden case; two backward passes give the same bits."""
    from get_amd import modules
    z, meta, contract = _archive(golden_dir)
    m = _build(z, contract, name)
    if name == "bertmodule_cat":      # through BertModule.forward(x, y), as the case was captured
        wrapper = modules.BertModule(m.config)
        wrapper.bert = m
        seq, pooled = wrapper(torch.from_numpy(z[name + "::x"]).to(DEV), torch.from_numpy(z[name + "::y"]).to(DEV))
    else:
        seq, pooled = _forward(m, z, name)
    worst = golden_ratio(seq, z[name + "::sequence_output"], *OUT_TOL, name + " sequence_output")
    worst = max(worst, golden_ratio(pooled, z[name + "::pooled_output"], *OUT_TOL, name + " pooled_output"))
    grads = _backward(m, z, name, seq, pooled)
    assert set(grads) == {k for k, _ in contract[CASES[name]]["state_dict"]}
    for k, g in grads.items():
        worst = max(worst, golden_ratio(g, z[f"{name}::grad::{k}"], *GRAD_TOL, f"{name} grad::{k}"))
    print(f"{name}: worst ratio of the bound {worst:.3f}")
    seq2, pooled2 = (wrapper(torch.from_numpy(z[name + "::x"]).to(DEV), torch.from_numpy(z[name + "::y"]).to(DEV))
                     if name == "bertmodule_cat" else _forward(m, z, name))
    bits_equal(seq, seq2, name + ": two forward passes")
    again = _backward(m, z, name, seq2, pooled2)
    for k, g in grads.items():
        bits_equal(g, again[k], f"{name} grad::{k}: two backward passes")


def test_training_mode_without_dropout_is_eval_bit_for_bit(golden_dir):
    z, _, contract = _archive(golden_dir)
    name = "h24_l2_L70"
    m = _build(z, contract, name, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    seq, pooled = _forward(m, z, name)
    grads = _backward(m, z, name, seq, pooled)
    m.train()
    seq_t, pooled_t = _forward(m, z, name)
    assert m.last_dropout_seeds == []
    bits_equal(seq, seq_t, "train(p=0) vs eval: sequence_output")
    bits_equal(pooled, pooled_t, "train(p=0) vs eval: pooled_output")
    for k, g in _backward(m, z, name, seq_t, pooled_t).items():
        bits_equal(grads[k], g, f"train(p=0) vs eval: grad::{k}")


def test_int32_ids_give_the_same_bits(golden_dir):
    z, _, contract = _archive(golden_dir)
    name = "h18_l1_L5"
    m = _build(z, contract, name)
    seq, pooled = _forward(m, z, name)
    grads = _backward(m, z, name, seq, pooled)
    seq32, pooled32 = _forward(m, z, name, int32=True)
    bits_equal(seq, seq32, "int32 ids: sequence_output")
    bits_equal(pooled, pooled32, "int32 ids: pooled_output")
    for k, g in _backward(m, z, name, seq32, pooled32).items():
        bits_equal(grads[k], g, f"int32 ids: grad::{k}")


def test_hidden_states_are_returned_when_configured(golden_dir):
    z, _, contract = _archive(golden_dir)
    name = "mask_half"
    m = _build(z, contract, name, output_hidden_states=True)
    seq, pooled, hidden = _forward(m, z, name)
    assert len(hidden) == m.config.num_hidden_layers + 1 and hidden[-1] is seq
    p64 = case_params(z, name, torch.float64)
    ids, types, mask = case_inputs(z, name)
    _, _, want = bert_ref.model(p64, contract[CASES[name]]["config"], ids, types, mask)
    for i, (got, w) in enumerate(zip(hidden, want)):
        golden_ratio(got, w, *OUT_TOL, f"hidden state {i}")


def test_relu_as_the_hidden_activation(golden_dir):
    """hidden_act = "relu" (the other activation the model accepts) against the float64 restatement, forward and backward."""
    z, _, contract = _archive(golden_dir)
    name = "mask_half"
    m = _build(z, contract, name, hidden_act="relu")
    seq, pooled = _forward(m, z, name)
    grads = _backward(m, z, name, seq, pooled)
    p64 = {k: v.requires_grad_(True) for k, v in case_params(z, name, torch.float64).items()}
    ids, types, mask = case_inputs(z, name)
    seq64, pooled64, _ = bert_ref.model(p64, m.config.to_dict(), ids, types, mask)
    g_seq, g_pooled = (torch.from_numpy(z[f"{name}::{k}"]).double() for k in ("g_seq", "g_pooled"))
    ((seq64 * g_seq).sum() + (pooled64 * g_pooled).sum()).backward()
    golden_ratio(seq, seq64, *OUT_TOL, "relu: sequence_output")
    golden_ratio(pooled, pooled64, *OUT_TOL, "relu: pooled_output")
    assert float((seq.detach().double().cpu() - torch.from_numpy(z[name + "::sequence_output"]).double()).abs().max()) > 1e-2
    for k, g in grads.items():
        golden_ratio(g, p64[k].grad, *GRAD_TOL, f"relu: grad::{k}")


def test_training_mode_dropout_follows_the_predicted_masks(golden_dir):
    """hidden_dropout_prob = attention_probs_dropout_prob = 0.1 under torch.manual_seed: the seeds are the next draws of
    ops.new_dropout_seed() in forward order (embeddings; per layer the attention probabilities, the attention output, the layer
    output), and the result is the float64 restatement's under the masks those seeds predict."""
    from get_amd import ops
    z, _, contract = _archive(golden_dir)
    name, p = "mask_half", 0.1
    m = _build(z, contract, name, hidden_dropout_prob=p, attention_probs_dropout_prob=p).train()
    cfg = m.config
    torch.manual_seed(4242)
    seq, pooled = _forward(m, z, name)
    seeds = list(m.last_dropout_seeds)
    torch.manual_seed(4242)
    assert seeds == [ops.new_dropout_seed() for _ in range(1 + 3 * cfg.num_hidden_layers)]
    grads = _backward(m, z, name, seq, pooled)

    ids, types, mask = case_inputs(z, name)
    b, l = ids.shape
    h, heads = cfg.hidden_size, cfg.num_attention_heads
    rows = lambda seed: torch.from_numpy(ops.dropout_mask_reference(seed, b * l, h, p)).reshape(b, l, h)
    att = lambda seed: torch.from_numpy(ops.dropout_mask_reference(seed, b * heads * l, l, p)).reshape(b, heads, l, l)
    masks = {"emb": rows(seeds[0]),
             "layers": [{"att": att(seeds[1 + 3 * n]), "att_out": rows(seeds[2 + 3 * n]), "out": rows(seeds[3 + 3 * n])}
                        for n in range(cfg.num_hidden_layers)]}
    assert all(0.03 < 1.0 - float(t.double().mean()) < 0.25 for t in [masks["emb"]] + [x for d in masks["layers"] for x in d.values()])
    p64 = {k: v.requires_grad_(True) for k, v in case_params(z, name, torch.float64).items()}
    seq64, pooled64, _ = bert_ref.model(p64, cfg.to_dict(), ids, types, mask, masks=masks)
    g_seq, g_pooled = (torch.from_numpy(z[f"{name}::{k}"]).double() for k in ("g_seq", "g_pooled"))
    ((seq64 * g_seq).sum() + (pooled64 * g_pooled).sum()).backward()
    golden_ratio(seq, seq64, *OUT_TOL, "training mode: sequence_output")
    golden_ratio(pooled, pooled64, *OUT_TOL, "training mode: pooled_output")
    assert float((seq.detach().double().cpu() - torch.from_numpy(z[name + "::sequence_output"]).double()).abs().max()) > 1e-2      # dropout acted
    for k, g in grads.items():
        golden_ratio(g, p64[k].grad, *GRAD_TOL, f"training mode: grad::{k}")
    # a second pass under the same seed reproduces the first bit for bit
    torch.manual_seed(4242)
    seq2, pooled2 = _forward(m, z, name)
    bits_equal(seq, seq2, "training mode under one seed, twice")
    for k, g in _backward(m, z, name, seq2, pooled2).items():
        bits_equal(grads[k], g, f"training mode under one seed, twice: grad::{k}")

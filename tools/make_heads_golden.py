"""Golden vectors of the BERT task models (pytorch_transformers/modeling_bert.py:634-1148: BertForPreTraining, BertForMaskedLM,
BertForNextSentencePrediction, BertForSequenceClassification, BertForMultipleChoice, BertForTokenClassification,
BertForQuestionAnswering), captured from the upstream reference in the build container -- never on the GPU machine, and no
test reads the reference.

Imports the reference's ``pytorch_transformers.modeling_bert`` at run time only (``oracle/_refshim.py``), runs every case in fp32
on the CPU, in eval mode, with seeded weights and inputs, and writes

    tests/golden/g23_bert_heads.npz         every case below
    tests/golden/bert_heads_contract.json   per parameter set: class, config, state_dict keys / shapes and which keys alias

Configurations: ``h24`` = tools/make_bert_golden.py's (vocab 50, hidden 24, 2 layers, 3 heads, intermediate 40, 80 positions);
``v131`` = vocab_size 131 (a prime above 128, no multiple of 4), hidden 24, 1 layer, 3 heads, intermediate 40, 16 positions;
``h18`` = make_bert_golden.py's h18 (vocab 50, hidden 18, 1 layer, 3 heads, intermediate 30, 16 positions), with num_labels 1, 2
and 5 where the head reads it.

Cases (CASES): each names its class, its configuration and its parameter set; cases of one parameter set share one draw of
the parameters, stored once (``pset::<set>::param::<name>``).
  pretraining        h18   B=3 L=9; some masked_lm_labels at -1, sequence 1 entirely at -1, one next_sentence_label at -1
  mlm_labels         v131  B=2 L=11; labels with -1 among them        mlm_plain   the same parameters without labels
  nsp                h18   B=4 L=6
  seqcls_n1          h18, num_labels 1 (MSE regression, float labels)
  seqcls_n2          h24, num_labels 2                                seqcls_n5   h18, num_labels 5
  choice             h18   B=2, 3 choices, L=6
  tokcls_mask        h18, num_labels 5, B=3 L=8, a mask that drops a suffix of sequences 1 and 2
  tokcls_plain       the same parameters without a mask
  qa                 h18   B=3 L=10; start position 1 beyond L, end position 2 negative, positions of shape (B, 1)

Every parameter is drawn, the biases and LayerNorm vectors included (as make_bert_golden.py draws them).  Per case
``<case>::``: the forward's keyword arguments (``input::<name>``), the returned tuple (``out::<i>``; the loss first where the
case passes labels), the gradient of every parameter (``grad::<name>``, a tied weight once, under the word table's name) of
gs * loss -- or, without labels, of sum_i sum(out_i * g_i) with the seeded ``g::<i>`` -- and the float64 results as fp32
residuals (``resid::<key>``), which tests/test_bert_heads_cpu.py holds the float64 restatement of tests/heads_ref.py to.

The reference's own fp32 result must lie within one tenth of the tolerance the GPU test applies (tests/test_gpu_bert_heads.py:
outputs and loss 1e-4 + 1e-4 |want|, gradients 1e-5 + 1e-4 |want|); a case that misses takes the next smaller gradient scale gs,
then the next smaller weight scale.  The test's tolerance is never loosened.  The scales used are in ``meta``.

    python tools/make_heads_golden.py
"""
import json
import os
import zlib

import numpy as np
import torch

from golden_common import OUT, _refshim, margin, to_numpy, write_contract, write_npz

H24 = dict(vocab_size_or_config_json_file=50, hidden_size=24, num_hidden_layers=2, num_attention_heads=3, intermediate_size=40,
           max_position_embeddings=80)
H18 = dict(vocab_size_or_config_json_file=50, hidden_size=18, num_hidden_layers=1, num_attention_heads=3, intermediate_size=30,
           max_position_embeddings=16)
V131 = dict(vocab_size_or_config_json_file=131, hidden_size=24, num_hidden_layers=1, num_attention_heads=3, intermediate_size=40,
            max_position_embeddings=16)
# parameter set -> (class, config)
PSETS = {
    "pretraining_h18": ("BertForPreTraining", H18),
    "mlm_v131": ("BertForMaskedLM", V131),
    "nsp_h18": ("BertForNextSentencePrediction", H18),
    "seqcls_h18_n1": ("BertForSequenceClassification", dict(H18, num_labels=1)),
    "seqcls_h24_n2": ("BertForSequenceClassification", dict(H24, num_labels=2)),
    "seqcls_h18_n5": ("BertForSequenceClassification", dict(H18, num_labels=5)),
    "choice_h18": ("BertForMultipleChoice", H18),
    "tokcls_h18_n5": ("BertForTokenClassification", dict(H18, num_labels=5)),
    "qa_h18": ("BertForQuestionAnswering", dict(H18, num_labels=2)),
}
CASES = {
    "pretraining": "pretraining_h18", "mlm_labels": "mlm_v131", "mlm_plain": "mlm_v131", "nsp": "nsp_h18",
    "seqcls_n1": "seqcls_h18_n1", "seqcls_n2": "seqcls_h24_n2", "seqcls_n5": "seqcls_h18_n5", "choice": "choice_h18",
    "tokcls_mask": "tokcls_h18_n5", "tokcls_plain": "tokcls_h18_n5", "qa": "qa_h18",
}
WEIGHT_SCALES = (0.2, 0.1, 0.05, 0.02)
GRAD_SCALES = (1.0, 0.25, 0.0625)
TOL_OUT, TOL_GRAD = (1e-4, 1e-4), (1e-5, 1e-4)


def make_inputs(name, vocab, g):
    """The forward's keyword arguments of one case (int64 ids and labels, float32 masks)."""
    ids = lambda *shape: torch.randint(1, vocab, shape, generator=g)
    types = lambda *shape: torch.randint(0, 2, shape, generator=g)
    if name == "pretraining":
        x = ids(3, 9)
        labels = torch.where(torch.rand(3, 9, generator=g) < 0.4, x, torch.full_like(x, -1))
        labels[0, 0], labels[0, 1], labels[2, 8] = x[0, 0], -1, x[2, 8]
        labels[1, :] = -1
        return dict(input_ids=x, token_type_ids=types(3, 9), attention_mask=torch.ones(3, 9), masked_lm_labels=labels,
                    next_sentence_label=torch.tensor([1, -1, 0]))
    if name in ("mlm_labels", "mlm_plain"):
        x = ids(2, 11)
        mask = torch.ones(2, 11)
        mask[1, 8:] = 0.0
        out = dict(input_ids=x, token_type_ids=types(2, 11), attention_mask=mask)
        if name == "mlm_labels":
            labels = torch.where(torch.rand(2, 11, generator=g) < 0.5, x, torch.full_like(x, -1))
            labels[0, 2], labels[1, 3], labels[1, 8:] = x[0, 2], -1, -1
            out["masked_lm_labels"] = labels
        return out
    if name == "nsp":
        return dict(input_ids=ids(4, 6), token_type_ids=types(4, 6), next_sentence_label=torch.tensor([0, 1, 1, 0]))
    if name == "seqcls_n1":
        return dict(input_ids=ids(4, 7), token_type_ids=types(4, 7), labels=torch.randn(4, generator=g))
    if name == "seqcls_n2":
        return dict(input_ids=ids(4, 12), token_type_ids=types(4, 12), labels=torch.tensor([1, 0, 0, 1]))
    if name == "seqcls_n5":
        return dict(input_ids=ids(5, 7), labels=torch.tensor([4, 0, 2, 2, 3]))
    if name == "choice":
        mask = torch.ones(2, 3, 6)
        mask[1, 2, 4:] = 0.0
        return dict(input_ids=ids(2, 3, 6), token_type_ids=types(2, 3, 6), attention_mask=mask, labels=torch.tensor([2, 0]))
    if name in ("tokcls_mask", "tokcls_plain"):
        out = dict(input_ids=ids(3, 8), token_type_ids=types(3, 8), labels=torch.randint(0, 5, (3, 8), generator=g))
        if name == "tokcls_mask":
            mask = torch.ones(3, 8)
            mask[1, 5:] = 0.0
            mask[2, 2:] = 0.0
            out["attention_mask"] = mask
        return out
    if name == "qa":
        return dict(input_ids=ids(3, 10), token_type_ids=types(3, 10), start_positions=torch.tensor([[2], [13], [0]]),
                    end_positions=torch.tensor([[5], [9], [-3]]))
    raise ValueError(name)


def has_labels(inputs):
    return any(k.endswith("labels") or k.endswith("label") or k.endswith("positions") for k in inputs)


def build(ref, pset, dtype, w):
    cls, conf = PSETS[pset]
    cfg = ref.BertConfig(initializer_range=w, **conf)
    torch.manual_seed(zlib.crc32(pset.encode()))
    m = getattr(ref, cls)(cfg)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "LayerNorm" in k:
                p.copy_(torch.randn(p.shape) * 0.1 + (1.0 if k.endswith("weight") else 0.0))
            elif k.endswith("bias"):
                p.copy_(torch.randn(p.shape) * w)
    return m.to(dtype).eval(), cfg


def run(ref, name, dtype, w, gs):
    m, cfg = build(ref, CASES[name], dtype, w)
    assert not hasattr(m, "cls") or not hasattr(m.cls, "predictions") or \
        m.cls.predictions.decoder.weight is m.bert.embeddings.word_embeddings.weight
    g = torch.Generator().manual_seed(23 + len(name))
    inputs = make_inputs(name, cfg.vocab_size, g)
    res = {"input::" + k: v for k, v in inputs.items()}
    # (the reference clamps the question-answering positions in place: it gets clones; regression labels follow the dtype)
    given = {k: (v.to(dtype) if k == "labels" and v.is_floating_point() else v.clone()) for k, v in inputs.items()}
    out = m(**given)
    for i, t in enumerate(out):
        res[f"out::{i}"] = t
    if has_labels(inputs):
        (out[0] * gs).backward()
    else:
        total = 0
        for i, t in enumerate(out):
            res[f"g::{i}"] = torch.randn(t.shape, generator=g) * gs
            total = total + (t * res[f"g::{i}"].to(dtype)).sum()
        total.backward()
    for k, p in m.named_parameters():
        res["param::" + k] = p
        if p.grad is not None:      # (the pooler of a model whose head reads the sequence output alone has none)
            res["grad::" + k] = p.grad
    return m, cfg, to_numpy(res)


def checked(k):
    return k.startswith("out::") or k.startswith("grad::")


def margin_of(r32, r64):
    def bound(k, want):
        atol, rtol = TOL_OUT if k.startswith("out::") else TOL_GRAD
        return atol + rtol * np.abs(want)
    return margin(r32, r64, [k for k in r32 if checked(k)], bound)


def main():
    _refshim.install()
    from pytorch_transformers import modeling_bert as ref
    torch.set_num_threads(1)
    store, contract, scales = {}, {}, {}
    for pset in PSETS:
        names = [n for n, s in CASES.items() if s == pset]
        for w, gs in ((w, gs) for w in WEIGHT_SCALES for gs in GRAD_SCALES):      # one pair of scales for the whole parameter set
            runs = {n: (run(ref, n, torch.float32, w, gs), run(ref, n, torch.float64, w, gs)) for n in names}
            worst = max(margin_of(r32[2], r64[2]) for r32, r64 in runs.values())
            if worst <= 1.0:
                break
        assert worst <= 1.0, (pset, worst)
        scales[pset] = {"weights": w, "loss_or_upstream_gradients": gs}
        print(f"{pset}: weight scale {w}, gradient scale {gs}, fp32 reference at {worst:.3f} of a tenth of the bound")
        m, cfg, _ = runs[names[0]][0]
        sd = m.state_dict()
        by_ptr = {}
        for k, v in sd.items():
            by_ptr.setdefault(v.data_ptr(), []).append(k)
        contract[pset] = {"class": PSETS[pset][0], "config": {k: v for k, v in cfg.to_dict().items() if k != "initializer_range"},
                          "state_dict": [[k, list(v.shape)] for k, v in sd.items()],
                          "aliases": sorted(sorted(ks) for ks in by_ptr.values() if len(ks) > 1)}
        for n in names:
            (_, _, r32), (_, _, r64) = runs[n]
            for k, v in r32.items():
                if k.startswith("param::"):
                    store[f"pset::{pset}::{k}"] = v
                    continue
                store[f"{n}::{k}"] = v
                if checked(k):
                    store[f"{n}::resid::{k}"] = (r64[k].astype(np.float64) - v.astype(np.float64)).astype(np.float32)
    meta = {"cases": CASES, "scales": scales}
    store["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    write_npz(os.path.join(OUT, "g23_bert_heads.npz"), store)
    write_contract(os.path.join(OUT, "bert_heads_contract.json"), contract)
    for f in ("g23_bert_heads.npz", "bert_heads_contract.json"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()

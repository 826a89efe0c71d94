"""Golden vectors of the BERT encoder (BertModel as matchzoo's BertModule wraps it), captured from the upstream reference in
the build container -- never on the GPU machine, and no test reads the reference.

Imports the reference's ``pytorch_transformers.modeling_bert`` at run time only (``oracle/_refshim.py`` puts the tree on the
path behind its meta-path stub for the third-party roots that are absent here: boto3, botocore, sacremoses, tensorflow), runs
every case in fp32 on the CPU, in eval mode, with seeded weights and inputs, and writes

    tests/golden/g21_bert.npz           every case below
    tests/golden/bert_contract.json     class, config and state_dict key / shape list of both configurations

Configurations: ``h24`` = BertConfig(50, hidden_size=24, num_hidden_layers=2, num_attention_heads=3 (dh = 8), intermediate_size=40,
max_position_embeddings=80); ``h18`` = BertConfig(50, hidden_size=18, num_hidden_layers=1, num_attention_heads=3 (dh = 6: no width
is a multiple of 4), intermediate_size=30, max_position_embeddings=16).

Cases:
  h24_l2_L70       h24, B=2, L=70: keys cross 64, five query tiles; sequence 1 has suffix padding; mixed token types
  h18_l1_L5        h18, B=3, L=5: sequence 2 is entirely padding (under the additive mask its softmax runs over the raw scores, not
                   zeros), sequence 0 has one real token
  h24_L1           h24, B=2, L=1
  bertmodule_cat   h24 through the reference's BertModule.forward(x, y) with x (2,7), y (2,30): no mask, no token types
  mask_half        h24, B=2, L=12 with a non-binary float mask: entries of 0.5 (bias -5000: no weight) and of 0.9999 (bias -1.0002:
                   a weight e^-1 times smaller), which only the rule (1 - mask) * -10000 reproduces

Every parameter is drawn, the biases and LayerNorm vectors included: weights and biases normal(0, w), LayerNorm weight 1 +
normal(0, 0.1), LayerNorm bias normal(0, 0.1).  Per case ``<case>::``: ``input_ids``, ``token_type_ids`` and ``attention_mask``
(where the case passes them; ``x`` and ``y`` for bertmodule_cat), every parameter (``param::<name>``), ``sequence_output``,
``pooled_output``, the seeded upstream gradients ``g_seq`` / ``g_pooled`` of the loss sum(sequence_output * g_seq) +
sum(pooled_output * g_pooled), and the gradient of every parameter (``grad::<name>``).  These are the reference's fp32
results; its float64 results ride along as fp32 residuals (``resid::<key>`` = float64 result - fp32 result, so the sum of the
two in float64 is the float64 result to ~1e-13 of its scale), which is what tests/test_bert_cpu.py holds the float64
restatement of tests/bert_ref.py to.

Every case also runs in float64, and the reference's own fp32 result must lie within one tenth of the tolerance the GPU test
applies (tests/test_gpu_bert.py), so the fixture never eats the test's margin.  A case that misses its tenth takes the next
smaller scale of its upstream gradients (GRAD_SCALES), then the next smaller weight scale w (WEIGHT_SCALES); the test's
tolerance is never loosened.  The scales used are in ``meta``.

    python tools/make_bert_golden.py
"""
import json
import os
import zlib

import numpy as np
import torch

from golden_common import OUT, _refshim, load_reference, margin, to_numpy, write_contract, write_npz

CONFIGS = {
    "h24": dict(vocab_size_or_config_json_file=50, hidden_size=24, num_hidden_layers=2, num_attention_heads=3, intermediate_size=40,
                max_position_embeddings=80),
    "h18": dict(vocab_size_or_config_json_file=50, hidden_size=18, num_hidden_layers=1, num_attention_heads=3, intermediate_size=30,
                max_position_embeddings=16),
}
CASES = {
    "h24_l2_L70": dict(config="h24", b=2, l=70),
    "h18_l1_L5": dict(config="h18", b=3, l=5),
    "h24_L1": dict(config="h24", b=2, l=1),
    "bertmodule_cat": dict(config="h24", b=2, l=37, split=7),
    "mask_half": dict(config="h24", b=2, l=12),
}
WEIGHT_SCALES = (0.2, 0.1, 0.05, 0.02)
GRAD_SCALES = (1.0, 0.25, 0.0625)      # of the upstream gradients: the gradients' errors shrink with them, the bound's atol does not
# h18_l1_L5: the upstream gradient of the all-padding sequence.  Every score of it sits next to -10000, on fp32's grid of 2^-10
# there, so its probabilities carry a relative error of up to 2^-11 in fp32 -- the reference's own -- whatever the weights
# are: 50 times the tenth's rtol.  Scaled by 2^-10 its share of every gradient's error stays below the tenth's atol; the
# sequence's outputs are compared at the full bound.
PAD_GRAD_SCALE = 2.0 ** -10
# the GPU test's tolerances (elementwise atol + rtol |want|)
TOL_OUT, TOL_GRAD = (1e-4, 1e-4), (1e-5, 1e-4)
OUTPUTS = ("sequence_output", "pooled_output")


def make_inputs(name, spec, vocab, g):
    """The forward's keyword arguments of one case (int64 ids, float32 mask)."""
    b, l = spec["b"], spec["l"]
    ids = torch.randint(1, vocab, (b, l), generator=g)
    if name == "bertmodule_cat":
        return {"input_ids": ids}
    types = torch.randint(0, 2, (b, l), generator=g)
    mask = torch.ones((b, l), dtype=torch.float32)
    if name == "h24_l2_L70":
        mask[1, 41:] = 0.0                     # suffix padding
    elif name == "h18_l1_L5":
        mask[0, 1:] = 0.0                      # one real token
        mask[2, :] = 0.0                       # entirely padding
    elif name == "mask_half":
        mask[0, 3:5] = 0.5
        mask[0, 6] = 0.9999
        mask[1, 1] = 0.9999
        mask[1, 2] = 0.5
        mask[1, 8:] = 0.0
    ids[mask == 0] = 0
    return {"input_ids": ids, "token_type_ids": types, "attention_mask": mask}


def run(ref, bert_module, name, spec, dtype, w, gs):
    cfg = ref.BertConfig(initializer_range=w, **CONFIGS[spec["config"]])
    torch.manual_seed(zlib.crc32(name.encode()))
    m = ref.BertModel(cfg)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "LayerNorm" in k:
                p.copy_(torch.randn(p.shape) * 0.1 + (1.0 if k.endswith("weight") else 0.0))
            elif k.endswith("bias"):
                p.copy_(torch.randn(p.shape) * w)
    m = m.to(dtype).eval()
    g = torch.Generator().manual_seed(21 + len(name))
    inputs = make_inputs(name, spec, cfg.vocab_size, g)
    res = dict(inputs)
    if name == "bertmodule_cat":
        wrapper = bert_module.BertModule.__new__(bert_module.BertModule)      # (its constructor downloads a pretrained model)
        torch.nn.Module.__init__(wrapper)
        wrapper.bert = m
        res = {"x": inputs["input_ids"][:, :spec["split"]], "y": inputs["input_ids"][:, spec["split"]:]}
        seq, pooled = wrapper(res["x"], res["y"])
    else:
        seq, pooled = m(**inputs)
    g_seq, g_pooled = torch.randn(seq.shape, generator=g) * gs, torch.randn(pooled.shape, generator=g) * gs
    if name == "h18_l1_L5":
        g_seq[2] *= PAD_GRAD_SCALE
        g_pooled[2] *= PAD_GRAD_SCALE
    ((seq * g_seq.to(dtype)).sum() + (pooled * g_pooled.to(dtype)).sum()).backward()
    res.update(sequence_output=seq, pooled_output=pooled, g_seq=g_seq, g_pooled=g_pooled)
    for k, p in m.named_parameters():
        res["param::" + k] = p
        res["grad::" + k] = p.grad
    return m, cfg, to_numpy(res)


def margin_of(r32, r64):
    """The reference's fp32 result against its float64 one, as a fraction of a tenth of the GPU test's tolerance."""
    def bound(k, want):
        atol, rtol = TOL_OUT if k in OUTPUTS else TOL_GRAD
        return atol + rtol * np.abs(want)
    return margin(r32, r64, [k for k in r32 if k in OUTPUTS or k.startswith("grad::")], bound)


def main():
    _refshim.install()
    from pytorch_transformers import modeling_bert as ref
    bert_module = load_reference("matchzoo/modules/bert_module.py", "ref_bert_module")
    torch.set_num_threads(1)
    store, contract, scales = {}, {}, {}
    for name, spec in CASES.items():
        for w, gs in ((w, gs) for w in WEIGHT_SCALES for gs in GRAD_SCALES):
            m, cfg, r32 = run(ref, bert_module, name, spec, torch.float32, w, gs)
            _, _, r64 = run(ref, bert_module, name, spec, torch.float64, w, gs)
            worst = margin_of(r32, r64)
            if worst <= 1.0:
                break
        assert worst <= 1.0, (name, worst)
        scales[name] = {"weights": w, "upstream_gradients": gs}
        print(f"{name}: weight scale {w}, upstream gradient scale {gs}, fp32 reference at {worst:.3f} of a tenth of the bound")
        if spec["config"] not in contract:
            conf = {k: v for k, v in cfg.to_dict().items() if k != "initializer_range"}
            contract[spec["config"]] = {"class": "BertModel", "config": conf,
                                        "state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()]}
        for k, v in r32.items():
            store[f"{name}::{k}"] = v
            if k in OUTPUTS or k.startswith("grad::"):
                store[f"{name}::resid::{k}"] = (r64[k].astype(np.float64) - v.astype(np.float64)).astype(np.float32)
    meta = {"cases": {n: s["config"] for n, s in CASES.items()}, "scales": scales, "pad_grad_scale": PAD_GRAD_SCALE,
            "split": {n: s["split"] for n, s in CASES.items() if "split" in s}}
    store["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    write_npz(os.path.join(OUT, "g21_bert.npz"), store)
    write_contract(os.path.join(OUT, "bert_contract.json"), contract)
    for f in ("g21_bert.npz", "bert_contract.json"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()

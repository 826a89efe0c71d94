#!/usr/bin/env python
"""Forward and backward of the BERT self-attention entry (ops.bert_attention: gh_bert_attention_fwd / _bwd, the probabilities
never in HBM) and of one BERT-base encoder layer (get_amd.bert.BertLayer: H = 768, 12 heads, intermediate 3072) at B = 32,
L in {128, 512}.  For the attention alone ops.mha_sdpa (gh_mha_sdpa_fwd / _bwd, which writes the [b][heads][lq][lk] weights and
needs a `ds` scratch of the same size) runs at the same shape on the same q, k, v: before the BERT entry it was the only
attention here such a layer could have run on.  The two do not compute the same thing (mha_sdpa has no temperature, bias or
dropout), so no outputs are compared; the BERT entry's correctness is tests/test_gpu_bert_paths.py's.

Timing: warm-up of every implementation, then BLOCKS timed blocks of REPS calls each per implementation and direction, the
implementations alternating block by block, device events around each block; reported are the median block time per call and
the spread (max - min over median).  The backward is timed as autograd's backward of a forward that ran before the events.
Saved state is computed from the shapes: 2 b heads lq floats (lse + delta) against 2 b heads lq lk (weights + ds).

    python tools/bert_bench.py [--blocks 7] [--json PATH]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from get_amd import ops  # noqa: E402
from get_amd.bert import BertConfig, BertLayer  # noqa: E402

B, HEADS, DH, HIDDEN, INTER = 32, 12, 64, 768, 3072
LENGTHS = (128, 512)
REPS = 5


def timed(blocks, impls):
    """impls: {tag: (setup, run)}; setup() -> state outside the events, run(state) inside.  Median ms per call and spread."""
    times = {k: [] for k in impls}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(blocks):
        for tag, (setup, run) in impls.items():
            total = 0.0
            for _ in range(REPS):
                state = setup()
                e0.record()
                run(state)
                e1.record()
                torch.cuda.synchronize()
                total += e0.elapsed_time(e1)
            times[tag].append(total / REPS)
    med = {k: statistics.median(v) for k, v in times.items()}
    return med, {k: (max(v) - min(v)) / med[k] for k, v in times.items()}


def attention_rows(l, p, blocks, dev):
    w = HEADS * DH
    torch.manual_seed(3)
    qkv = torch.randn(B, l, 3 * w, device=dev)      # the three column blocks of one buffer, as a fused projection leaves them
    q, k, v = (qkv[:, :, i * w:(i + 1) * w].detach().requires_grad_(True) for i in range(3))
    lens = l - (torch.arange(B, device=dev) * 7) % (l // 2)
    pad = torch.arange(l, device=dev)[None, :] >= lens[:, None]                      # (B, L) True = padding
    bias = pad.float() * -10000.0
    mask3 = pad[:, None, :].expand(B, l, l).contiguous()
    gout = torch.randn(B, l, w, device=dev)
    scale = 1.0 / math.sqrt(DH)
    fwd = {"bert": lambda: ops.bert_attention(q, k, v, bias, HEADS, scale, p, 11),
           "mha_sdpa": lambda: ops.mha_sdpa(q, k, v, mask3, HEADS)[0]}

    def bwd(out):
        for t in (q, k, v):
            t.grad = None
        out.backward(gout)

    for f in fwd.values():      # warm-up
        for _ in range(2):
            bwd(f())
    torch.cuda.synchronize()
    f_med, f_spread = timed(blocks, {k: ((lambda: None), (lambda _, f=f: f())) for k, f in fwd.items()})
    b_med, b_spread = timed(blocks, {k: (f, bwd) for k, f in fwd.items()})
    floats = B * HEADS * l
    return dict(what="attention", b=B, heads=HEADS, l=l, dh=DH, drop_p=p,
                bert_fwd_ms=f_med["bert"], bert_bwd_ms=b_med["bert"], mha_sdpa_fwd_ms=f_med["mha_sdpa"], mha_sdpa_bwd_ms=b_med["mha_sdpa"],
                spread=dict(bert_fwd=f_spread["bert"], bert_bwd=b_spread["bert"], mha_sdpa_fwd=f_spread["mha_sdpa"],
                            mha_sdpa_bwd=b_spread["mha_sdpa"]),
                mha_sdpa_over_bert=(f_med["mha_sdpa"] + b_med["mha_sdpa"]) / (f_med["bert"] + b_med["bert"]),
                bert_saved_bytes=2 * floats * 4, mha_sdpa_saved_bytes=2 * floats * l * 4,
                attention_flops_fwd=4 * B * HEADS * l * l * DH)


def layer_row(l, train, blocks, dev):
    torch.manual_seed(5)
    cfg = BertConfig(30522, hidden_size=HIDDEN, num_attention_heads=HEADS, intermediate_size=INTER, num_hidden_layers=1)
    layer = BertLayer(cfg).to(dev).train(train)
    x = torch.randn(B, l, HIDDEN, device=dev, requires_grad=True)
    lens = l - (torch.arange(B, device=dev) * 7) % (l // 2)
    bias = (torch.arange(l, device=dev)[None, :] >= lens[:, None]).float() * -10000.0
    gout = torch.randn(B, l, HIDDEN, device=dev)

    def bwd(out):
        x.grad = None
        layer.zero_grad(set_to_none=True)
        out.backward(gout)

    for _ in range(2):
        bwd(layer(x, bias))
    torch.cuda.synchronize()
    f_med, f_spread = timed(blocks, {"layer": ((lambda: None), (lambda _: layer(x, bias)))})
    b_med, b_spread = timed(blocks, {"layer": ((lambda: layer(x, bias)), bwd)})
    return dict(what="bert_base_layer", b=B, l=l, hidden=HIDDEN, heads=HEADS, intermediate=INTER, training=train,
                fwd_ms=f_med["layer"], bwd_ms=b_med["layer"], spread=dict(fwd=f_spread["layer"], bwd=b_spread["layer"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bert_bench: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda:0")
    results = []
    for l in LENGTHS:
        for p in (0.0, 0.1):
            results.append(attention_rows(l, p, args.blocks, dev))
            print(json.dumps(results[-1]), flush=True)
        for train in (False, True):
            results.append(layer_row(l, train, args.blocks, dev))
            print(json.dumps(results[-1]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()

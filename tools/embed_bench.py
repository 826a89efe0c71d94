"""Time the embedding table gradient (ops.embed_plan + ops.embedding_backward: csrc/embed_ops.hip) against the two ways torch
offers on the same device, in the same process.

A tool, not a test.  The table gradient of V = 20 000 words of width D = 300 from two sets of lookups:

    headline   the real node rows of the B = 32 x 30 evidence batch of synth.make_raw_batch after the graph build (the ids the
               first evidence cell gathers): ~62 000 rows, Zipf-distributed words
    one_id     the same number of rows, all naming one word: a single run over every chunk

Three versions, each from a given (m, D) row-gradient tensor to a (V, D) table gradient that starts from zeros:

    hip        torch.zeros + the stable sort of the ids (embed_plan) + gh_embed_bwd; also timed without the sort and the
               zero fill (`hip_kernels`: what a trainer's direct accumulation with a plan in hand would pay)
    index_add  torch.zeros + index_add_, what the GGNN cell did before
    aten       torch.ops.aten.embedding_dense_backward, what nn.Embedding's autograd runs

Timing: HIP events around one call on the current stream, after a warm-up; the versions alternate inside every round, --runs
rounds (>= 20); the median and the spread (min .. max) per version, in microseconds.  The result of each version is compared
with the float64 sum: the largest error over the largest entry.

    python tools/embed_bench.py [--runs 30] [--warmup 5] [--out FILE]

Prints one JSON line per shape.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

V, D = 20000, 300


def headline_ids(dev):
    """The node ids of the real rows of the bench batch's evidence graphs, in row order."""
    from get_amd import ops
    from get_amd.synth import SynthConfig, make_raw_batch
    cfg = SynthConfig(vocab=V, emb_dim=D)
    raw = make_raw_batch(cfg, 0)
    _, node_ids, n_nodes = ops.graph_build(torch.from_numpy(raw["evd_tokens"]).to(dev), torch.from_numpy(raw["evd_len"]).to(dev), cfg.window)
    real = torch.arange(node_ids.shape[1], device=dev)[None, :] < n_nodes[:, None]
    return node_ids[real].contiguous()


def event_times(fns, runs, warmup):
    """{name: [microseconds per call]}: the versions alternate inside a round, one pair of events per call."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3)
    return times


def bench_shape(name, ids, runs, warmup):
    from get_amd import ops
    dev = ids.device
    m = ids.numel()
    gen = torch.Generator(device="cpu").manual_seed(1)
    dx = torch.randn(m, D, generator=gen).to(dev)
    ids64 = ids.long()
    plan = ops.embed_plan(ids, V)
    acc = torch.zeros(V, D, device=dev)

    def hip():
        return ops.embedding_backward(dx, ops.embed_plan(ids, V), torch.zeros(V, D, device=dev))

    def hip_kernels():
        return ops.embedding_backward(dx, plan, acc)

    def index_add():
        return torch.zeros(V, D, device=dev).index_add_(0, ids64, dx)

    def aten():
        return torch.ops.aten.embedding_dense_backward(dx, ids64, V, -1, False)

    fns = {"hip": hip, "hip_kernels": hip_kernels, "index_add": index_add, "aten": aten}
    exact = torch.zeros(V, D, dtype=torch.float64, device=dev).index_add_(0, ids64, dx.double())
    scale = float(exact.abs().max())
    err = {k: float((fns[k]().double() - exact).abs().max()) / scale for k in ("hip", "index_add", "aten")}
    twice = torch.equal(hip(), hip())
    t = event_times(fns, runs, warmup)
    row = {"shape": name, "rows": m, "distinct_ids": int(torch.unique(ids).numel()), "V": V, "D": D, "runs": runs,
           "hip_bit_identical_twice": twice, "err_over_scale": {k: float("%.3g" % v) for k, v in err.items()}}
    for k, v in t.items():
        row[k + "_us"] = {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
    for k in ("index_add", "aten"):
        row[f"{k}_over_hip"] = round(float(np.median(t[k]) / np.median(t["hip"])), 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("embed_bench: no ROCm device; times are only taken on the GPU")
    if args.runs < 20:
        sys.exit("embed_bench: at least 20 runs per version")
    dev = torch.device("cuda:0")
    ids = headline_ids(dev)
    shapes = {"headline": ids, "one_id": torch.full_like(ids, 17)}
    lines = [json.dumps(bench_shape(k, v, args.runs, args.warmup)) for k, v in shapes.items()]
    for line in lines:
        print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

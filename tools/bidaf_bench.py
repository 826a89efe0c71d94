"""Time the attention-flow layer of the BiDAF drop-in (ops.att_flow: csrc/bidaf_ops.hip) against the reference's formulation
written with torch ops on the same device, alone and inside the whole model.

A tool, not a test.  Forward + backward at the project's shape:

    layer    c 960 x 100 x 600, q 960 x 30 x 600
    model    B = 960, L = 30, R = 100, D = 300, H = 300 (lengths: documents all 100, queries uniform in [5, 30])

The baseline of the layer is bidaf_model.py:72-104 as written there: the q_len loop of a 1-wide linear over c * q_i, the stack,
the two expand adds, two softmaxes, two bmm, the tiled expand and the four-way cat -- same weights, same GPU.  The baseline of
the model is the same drop-in with ops.att_flow and ops.highway swapped for those torch ops (the LSTMs and the projections stay
on the HIP kernels in both), so the difference is the two new kernels' alone.  Timing: a host clock around work that ends in
a device synchronise, after a warm-up; windows of at least --window seconds, the two versions alternated for --rounds rounds;
the median time per iteration and the spread (min .. max over the windows) are reported, with the largest relative
difference between the two versions' outputs and gradients.

    python tools/bidaf_bench.py [--rounds 5] [--window 1.0] [--out FILE]

Prints one JSON line per shape.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

B, L, R, D, H = 960, 30, 100, 300, 300


def loop_att_flow(c, q, w_c, w_q, w_cq, b_c, b_q, b_cq, out=None):
    c_len, q_len = c.size(1), q.size(1)
    cq = torch.stack([F.linear(c * q.select(1, i).unsqueeze(1), w_cq, b_cq).squeeze(-1) for i in range(q_len)], dim=-1)
    s = F.linear(c, w_c, b_c).expand(-1, -1, q_len) + F.linear(q, w_q, b_q).permute(0, 2, 1).expand(-1, c_len, -1) + cq
    a = F.softmax(s, dim=2)
    c2q = torch.bmm(a, q)
    b = F.softmax(torch.max(s, dim=2)[0], dim=1).unsqueeze(1)
    q2c = torch.bmm(b, c).squeeze(1).unsqueeze(1).expand(-1, c_len, -1)
    return torch.cat([c, c2q, c * c2q, c * q2c], dim=-1)


def torch_highway(x, h_pre, g_pre):
    g = torch.sigmoid(g_pre)
    return g * torch.relu(h_pre) + (1 - g) * x


def timed(fns, rounds, window):
    for fn in fns.values():      # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for tag, fn in fns.items():
            n, t0 = 0, time.perf_counter()
            while True:
                fn()
                n += 1
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if dt >= window:
                    break
            times[tag].append(1e3 * dt / n)
    return {k + "_ms": {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in times.items()}


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bidaf_bench: needs a GPU; a CPU run says nothing about the MI355X")
    from get_amd import modules, ops
    from get_amd.synth import make_tokens
    dev = torch.device("cuda:0")
    lines = []

    # ---- the layer alone
    torch.manual_seed(3)
    d = 2 * H
    c = torch.randn(B, R, d, device=dev, requires_grad=True)
    q = torch.randn(B, L, d, device=dev, requires_grad=True)
    w = [(torch.randn(1, d, device=dev) / d ** 0.5).requires_grad_(True) for _ in range(3)]
    bias = [torch.zeros(1, device=dev, requires_grad=True) for _ in range(3)]
    gx = torch.randn(B, R, 4 * d, device=dev)
    leaves = [c, q] + w

    def layer(fn):
        def run():
            for t in leaves + bias:
                t.grad = None
            x = fn(c, q, w[0], w[1], w[2], bias[0], bias[1], bias[2])
            x.backward(gx)
            return x
        return run
    fns = {"hip": layer(ops.att_flow), "loop": layer(loop_att_flow)}
    x1 = fns["hip"]().detach()
    g1 = [t.grad.clone() for t in leaves]
    x2 = fns["loop"]().detach()
    diff = max([rel(x1, x2)] + [rel(u, t.grad) for u, t in zip(g1, leaves)])
    line = {"shape": "layer", "B": B, "lc": R, "lq": L, "d": d, "rounds": args.rounds, "window_s": args.window, "max_rel_diff": diff}
    line.update(timed(fns, args.rounds, args.window))
    line["hip_over_loop"] = line["hip_ms"]["median"] / line["loop_ms"]["median"]
    print(json.dumps(line), flush=True)
    lines.append(line)
    del c, q, gx, x1, x2, g1, fns
    torch.cuda.empty_cache()

    # ---- the whole model
    rng = np.random.default_rng(7)
    query, q_lens = make_tokens(rng, B, L, 1000, 5, L)
    document, c_lens = make_tokens(rng, B, R, 1000, R, R)
    torch.manual_seed(3)
    m = modules.BiDAF(dict(embedding=None, embedding_input_dim=1000, embedding_output_dim=D, embedding_freeze=False, word_dim=D,
                           hidden_size=H, dropout=0.2)).to(dev).eval()
    idx = []
    for lens in (q_lens, c_lens):
        lens = torch.from_numpy(np.asarray(lens)).long()
        new = torch.sort(lens, descending=True, stable=True)[1]
        idx.append((new.to(dev), torch.argsort(new).to(dev), lens))
    qd, dd = torch.from_numpy(np.asarray(query)).to(dev), torch.from_numpy(np.asarray(document)).to(dev)
    g_logits = torch.randn(B, 1, device=dev)
    hip_ops = ops.att_flow, ops.highway

    def model(att, hw):
        def run():
            ops.att_flow, ops.highway = att, hw
            try:
                m.zero_grad(set_to_none=True)
                out = m(qd, dd, query_lens_indices=idx[0], doc_lens_indices=idx[1])
                (out * g_logits).sum().backward()
            finally:
                ops.att_flow, ops.highway = hip_ops
            return out
        return run
    fns = {"hip": model(*hip_ops), "loop": model(loop_att_flow, torch_highway)}
    o1 = fns["hip"]().detach()
    g1 = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    o2 = fns["loop"]().detach()
    diff = max([rel(o1, o2)] + [rel(g1[k], p.grad) for k, p in m.named_parameters() if k in g1 and not k.endswith("linear.bias")])
    line = {"shape": "model", "B": B, "L": L, "R": R, "D": D, "H": H, "rounds": args.rounds, "window_s": args.window,
            "max_rel_diff": diff}
    line.update(timed(fns, args.rounds, args.window))
    line["hip_over_loop"] = line["hip_ms"]["median"] / line["loop_ms"]["median"]
    print(json.dumps(line), flush=True)
    lines.append(line)
    if args.out:
        with open(args.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

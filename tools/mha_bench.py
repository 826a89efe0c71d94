#!/usr/bin/env python
"""Forward + backward of modules.MultiHeadAttentionOriginal (HIP: three ops.linear, ops.mha_sdpa on their outputs in place,
ops.linear, ops.add_layernorm) against a plain-torch fp32 restatement of the same module on the same GPU -- our own
composition of torch ops (nn.Linear, the per-head permute copies, two bmm, masked_fill / softmax / masked_fill, nn.LayerNorm),
not the reference.  Both run on the same seeded inputs and parameters; their outputs are compared first.

Timing: warm-up of both, then BLOCKS timed blocks of REPS steps each per implementation, the two alternating block by block;
reported are the median block time per step, the spread (max - min over median) of each, and the ratio of the medians.

    python tools/mha_bench.py [--blocks 9] [--json PATH]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from get_amd import modules  # noqa: E402

SHAPES = [dict(name="word", b=960, l=100, d_model=300, n_head=5, d=60, reps=5),
          dict(name="evidence_wide", b=32, l=30, d_model=1628, n_head=4, d=407, reps=20)]


class TorchMHA(nn.Module):
    """The same module on torch ops alone (fp32)."""

    def __init__(self, n_head, d_model, d_k, d_v):
        super().__init__()
        self.n_head, self.d_k, self.d_v = n_head, d_k, d_v
        self.w_qs = nn.Linear(d_model, n_head * d_k)
        self.w_ks = nn.Linear(d_model, n_head * d_k)
        self.w_vs = nn.Linear(d_model, n_head * d_v)
        self.layer_norm = nn.LayerNorm(d_model)
        self.fc = nn.Linear(n_head * d_v, d_model)

    def forward(self, q, k, v, mask):
        h, dk, dv = self.n_head, self.d_k, self.d_v
        b, lq, _ = q.shape
        lk = k.shape[1]
        split = lambda x, l, d: x.view(b, l, h, d).permute(2, 0, 1, 3).contiguous().view(-1, l, d)
        qh, kh, vh = split(self.w_qs(q), lq, dk), split(self.w_ks(k), lk, dk), split(self.w_vs(v), lk, dv)
        mh = mask.repeat(h, 1, 1)
        attn = torch.bmm(qh, kh.transpose(1, 2)).masked_fill(mh, float("-inf"))
        attn = F.softmax(attn, dim=-1).masked_fill(mh, 0)
        out = torch.bmm(attn, vh).view(h, b, lq, dv).permute(1, 2, 0, 3).contiguous().view(b, lq, -1)
        return self.layer_norm(self.fc(out) + q), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mha_bench: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda:0")
    results = []
    for s in SHAPES:
        torch.manual_seed(7)
        hip = modules.MultiHeadAttentionOriginal(s["n_head"], s["d_model"], s["d"], s["d"]).to(dev)
        ref = TorchMHA(s["n_head"], s["d_model"], s["d"], s["d"]).to(dev)
        ref.load_state_dict(hip.state_dict())
        b, l = s["b"], s["l"]
        q = torch.randn(b, l, s["d_model"], device=dev, requires_grad=True)
        kv = torch.randn(b, l, s["d_model"], device=dev, requires_grad=True)
        lens = l - (torch.arange(b, device=dev) * 7) % (l // 2)
        mask = (torch.arange(l, device=dev)[None, None, :] >= lens[:, None, None]).expand(b, l, l).contiguous()
        gout = torch.randn(b, l, s["d_model"], device=dev)

        def step(m):
            for t in (q, kv):
                t.grad = None
            m.zero_grad(set_to_none=True)
            out, _ = m(q, kv, kv, mask)
            (out * gout).sum().backward()
            return out

        o_hip, o_ref = step(hip).detach(), step(ref).detach()
        diff = ((o_hip - o_ref).abs().max() / o_ref.abs().max()).item()
        for _ in range(3):
            step(hip), step(ref)
        torch.cuda.synchronize()
        times = {"hip": [], "torch": []}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.blocks):
            for tag, m in (("hip", hip), ("torch", ref)):
                e0.record()
                for _ in range(s["reps"]):
                    step(m)
                e1.record()
                torch.cuda.synchronize()
                times[tag].append(e0.elapsed_time(e1) / s["reps"])
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
        r = dict(shape={k: v for k, v in s.items() if k != "reps"}, out_rel_diff=diff, hip_ms=med["hip"], torch_ms=med["torch"],
                 hip_spread=spread["hip"], torch_spread=spread["torch"], torch_over_hip=med["torch"] / med["hip"],
                 blocks=args.blocks, reps=s["reps"])
        results.append(r)
        print(json.dumps(r), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()

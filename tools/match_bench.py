"""Time the soft-alignment kernels of the matchzoo/modules drop-ins (ops.soft_align: csrc/match_ops.hip) against the
reference's own statements executed by torch on the same device, in the same process.

A tool, not a test.  Forward + backward at the project's shape, B = 960, L1 = 30, L2 = 100, D = 600:

    bidir    BidirectionalAttention: v1 960 x 30 x 600, v2 960 x 100 x 600, both masks from ragged lengths
    match    MatchModule(600): the same two sequences

The baseline of ``bidir`` is matchzoo/modules/attention.py:50-63 as written there (bmm, two masked_fill + softmax, two bmm, two
masked_fill_).  The baseline of ``match`` is the same drop-in with ops.soft_align swapped for :99-105 (bmm, masked_fill,
softmax, bmm, the four-way cat) -- the two projections, the ReLU and their gradients stay on the HIP kernels in both, so the
difference is the new kernel's alone.  Timing: a host clock around work that ends in a device synchronise, after a warm-up;
windows of at least --window seconds, the two versions alternated for --rounds rounds; the median time per iteration and
the spread (min .. max over the windows) are reported, with the largest relative difference between the two versions'
outputs and gradients.

    python tools/match_bench.py [--rounds 5] [--window 1.0] [--batch 960] [--out FILE]

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

L1, L2, D = 30, 100, 600


def torch_bidir(v1, v1_mask, v2, v2_mask):
    s = v1.bmm(v2.transpose(2, 1).contiguous())
    v2_v1 = F.softmax(s.masked_fill(v1_mask.unsqueeze(2), -1e-7), dim=1)
    v1_v2 = F.softmax(s.masked_fill(v2_mask.unsqueeze(1), -1e-7), dim=2)
    a1 = v1_v2.bmm(v2)
    a2 = v2_v1.transpose(1, 2).bmm(v1)
    a1.masked_fill_(v1_mask.unsqueeze(2), 0)
    a2.masked_fill_(v2_mask.unsqueeze(2), 0)
    return a1, a2


def torch_soft_align(q, k, v, key_fill, row_zero=None, fill=-1e-7, fuse=False, out=None):
    """MatchModule's statements behind the signature of ops.soft_align (fuse only)."""
    assert fuse and row_zero is None and out is None
    a = F.softmax(q.bmm(k.transpose(2, 1).contiguous()).masked_fill(key_fill.unsqueeze(1), fill), dim=2)
    o = a.bmm(v)
    return torch.cat([q, o, q - o, q * o], dim=2), a


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
    ap.add_argument("--batch", type=int, default=960)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("match_bench: needs a GPU; a CPU run says nothing about the MI355X")
    from get_amd import modules, ops
    dev = torch.device("cuda:0")
    B = args.batch
    lines = []
    g = torch.Generator().manual_seed(3)
    v1 = (0.5 * torch.randn(B, L1, D, generator=g)).to(dev).requires_grad_(True)
    v2 = (0.5 * torch.randn(B, L2, D, generator=g)).to(dev).requires_grad_(True)
    len1, len2 = torch.randint(5, L1 + 1, (B,), generator=g), torch.randint(20, L2 + 1, (B,), generator=g)
    m1 = (torch.arange(L1)[None, :] >= len1[:, None]).to(dev)
    m2 = (torch.arange(L2)[None, :] >= len2[:, None]).to(dev)
    leaves = [v1, v2]

    def finish(name, fns, params, extra):
        fns["hip"]()
        r1 = [t.clone() for t in extra["last"]] + [t.grad.clone() for t in leaves + params]
        fns["torch"]()
        r2 = list(extra["last"]) + [t.grad for t in leaves + params]
        line = {"shape": name, "B": B, "L1": L1, "L2": L2, "D": D, "rounds": args.rounds, "window_s": args.window,
                "max_rel_diff": max(rel(a, b) for a, b in zip(r1, r2))}
        line.update(timed(fns, args.rounds, args.window))
        line["hip_over_torch"] = line["hip_ms"]["median"] / line["torch_ms"]["median"]
        print(json.dumps(line), flush=True)
        lines.append(line)

    # ---- BidirectionalAttention
    g1, g2 = torch.randn(B, L1, D, generator=g).to(dev), torch.randn(B, L2, D, generator=g).to(dev)
    bidir = modules.BidirectionalAttention()
    state = {"last": None}

    def run_bidir(fn):
        def run():
            for t in leaves:
                t.grad = None
            a1, a2 = fn(v1, m1, v2, m2)
            torch.autograd.backward([a1, a2], [g1, g2])
            state["last"] = (a1.detach(), a2.detach())
        return run
    finish("bidir", {"hip": run_bidir(bidir), "torch": run_bidir(torch_bidir)}, [], state)
    del g1, g2
    torch.cuda.empty_cache()

    # ---- MatchModule
    torch.manual_seed(3)
    mm = modules.MatchModule(D).to(dev).eval()
    gm = torch.randn(B, L1, 2 * D, generator=g).to(dev)
    params = list(mm.parameters())
    hip_align = ops.soft_align

    def run_match(align):
        def run():
            ops.soft_align = align
            try:
                for t in leaves + params:
                    t.grad = None
                y = mm(v1, v2, m2)
                y.backward(gm)
            finally:
                ops.soft_align = hip_align
            state["last"] = (y.detach(),)
        return run
    finish("match", {"hip": run_match(hip_align), "torch": run_match(torch_soft_align)}, params, state)
    if args.out:
        with open(args.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()

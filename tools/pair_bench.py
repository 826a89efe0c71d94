"""Time the pairwise helpers (ops.pair: csrc/pair_ops.hip) against the reference's own formulations executed by torch on the
same device -- for the histogram, by numpy on the host, where the reference runs it.

A tool, not a test.  Forward + backward (the histogram has no backward):

    pair_l2       64 x 30 x 300 against 64 x 100 x 300    torch_utils.py:311-329: two squared norms, bmm, sqrt(|.| + 1e-10)
    pair_l1       the same operands                       torch_utils.py:332-348: norm(x - y, p=1) over a (B,L,R,D) difference
    window_mean   64 x 100 x 300, window 5, with a mask   torch_utils.py:351-376: pad, cumsum, slice subtraction, divide, mask
    match_hist    B = 64, Lq = 30, Ld = 100, D = 300, 30 bins   matching_histogram.py:44-60 pair by pair over the batch

Without --op this is a driver that never touches the GPU itself: it runs every op in a process of its own under a time limit
and starts nothing further after one that fails, is killed or runs out of time.  With --op it measures that op: a host clock
around work that ends in a device synchronise, after a warm-up; windows of at least --window seconds, the two versions
alternated for --rounds rounds; the median time per iteration and the spread are reported, with the largest relative difference
between the two versions' results and, for pair_l1, the peak device memory of one iteration of either version
(torch.cuda.max_memory_allocated over what the operands already hold).

    python tools/pair_bench.py [--rounds 5] [--window 0.5] [--timeout 120] [--out FILE]

Prints one JSON line per op.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS = ["pair_l2", "pair_l1", "window_mean", "match_hist"]
B, L, R, D, W, BINS = 64, 30, 100, 300, 5, 30


def torch_l2(a, b):
    import torch
    sa, sb = (a * a).sum(dim=-1), (b * b).sum(dim=-1)
    return torch.sqrt(torch.abs(sa.unsqueeze(-1) - 2 * torch.bmm(a, b.permute(0, 2, 1)) + sb.unsqueeze(1)) + 1e-10)


def torch_l1(a, b):
    import torch
    return torch.norm(a.unsqueeze(2) - b.unsqueeze(1), p=1, dim=-1)


def torch_context(doc, mask, c):
    import torch
    import torch.nn.functional as F
    left = c // 2
    ret = torch.cumsum(F.pad(doc, (0, 0, left, c - left - 1)), dim=1)
    ret[:, c:] = ret[:, c:] - ret[:, :-c]
    return ret[:, c - 1:] / c * mask.unsqueeze(-1).float()


def host_hist(table, ids_left, ids_right, len_right, bins):
    out = []
    for left, right, n in zip(ids_left, ids_right, len_right):
        hist = np.ones((len(left), bins), dtype=np.float32)
        mm = table[left].dot(np.transpose(table[right[:n]]))
        for (i, j), value in np.ndenumerate(mm):
            hist[i][int((value + 1.) / 2. * (bins - 1.))] += 1.0
        out.append(np.log(hist))
    return np.asarray(out)


def timed(fns, rounds, window, sync):
    for fn in fns.values():
        fn()
    sync()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for tag, fn in fns.items():
            n, t0 = 0, time.perf_counter()
            while True:
                fn()
                n += 1
                sync()
                dt = time.perf_counter() - t0
                if dt >= window:
                    break
            times[tag].append(1e3 * dt / n)
    return {k + "_ms": {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))} for k, v in times.items()}


def measure(op, rounds, window):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pair_bench: needs a GPU; a CPU run says nothing about the MI355X")
    from get_amd import ops, pairwise
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    line = {"op": op, "B": B, "rounds": rounds, "window_s": window}
    rel = lambda u, v: float((u - v).abs().max() / v.abs().max().clamp_min(1e-30))
    last = {}

    def fwd_bwd(fn, leaves, gu, tag):
        def run():
            for t in leaves:
                t.grad = None
            out = fn(*leaves)
            out.backward(gu)
            last[tag] = [out.detach()] + [t.grad for t in leaves]
        return run

    def peak(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 2 ** 20

    if op in ("pair_l2", "pair_l1"):
        a = torch.randn(B, L, D, generator=g).to(dev).requires_grad_(True)
        b = torch.randn(B, R, D, generator=g).to(dev).requires_grad_(True)
        gu = torch.randn(B, L, R, generator=g).to(dev)
        hip, ref = (ops.pair.pair_l2, torch_l2) if op == "pair_l2" else (ops.pair.pair_l1, torch_l1)
        fns = {"hip": fwd_bwd(lambda x, y: hip(x, y), [a, b], gu, "hip"), "torch": fwd_bwd(ref, [a, b], gu, "torch")}
        line.update(L=L, R=R, D=D)
    elif op == "window_mean":
        x = torch.randn(B, R, D, generator=g).to(dev).requires_grad_(True)
        mask = (torch.arange(R)[None, :] < torch.randint(20, R + 1, (B,), generator=g)[:, None]).to(dev)
        gu = torch.randn(B, R, D, generator=g).to(dev)
        fns = {"hip": fwd_bwd(lambda t: ops.pair.window_mean(t, W, W // 2, W - W // 2 - 1, mask), [x], gu, "hip"),
               "torch": fwd_bwd(lambda t: torch_context(t, mask, W), [x], gu, "torch")}
        line.update(L=R, D=D, window=W)
    else:
        V = 5000
        table = torch.randn(V, D, generator=g).double().numpy()
        ids_left = torch.randint(0, V, (B, L), generator=g)
        ids_right = torch.randint(0, V, (B, R), generator=g)
        len_right = torch.randint(20, R + 1, (B,), generator=g)
        unit = pairwise.MatchingHistogram(BINS, table, True, "LCH")
        il, ir, ln = ids_left.to(dev), ids_right.to(dev), len_right.to(dev)
        norm = table / np.sqrt((table * table).sum(axis=1))[:, None]
        hl, hr, hn = ids_left.numpy(), ids_right.numpy(), len_right.numpy()

        def run_hip():
            last["hip"] = [unit.transform_batch(il, ir, ln)]

        def run_host():
            last["torch"] = [torch.from_numpy(host_hist(norm, hl, hr, hn, BINS))]
        fns = {"hip": run_hip, "torch": run_host}
        line.update(Lq=L, Ld=R, D=D, bins=BINS, baseline="host loop (numpy)")
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    if op == "match_hist":      # fp32 on the device against float64 on the host: a pair on a bin edge may fall either way
        diff = (last["hip"][0].cpu().double().exp() - last["torch"][0].double().exp()).abs()
        line["rows_with_a_moved_pair"] = int((diff.sum(2) > 0.5).sum())
    else:
        line["max_rel_diff"] = max(rel(u, v) for u, v in zip(last["hip"], last["torch"]))
    if op == "pair_l1":
        line["hip_peak_mib"], line["torch_peak_mib"] = peak(fns["hip"]), peak(fns["torch"])
    line.update(timed(fns, rounds, window, torch.cuda.synchronize))
    line["hip_over_torch"] = line["hip_ms"]["median"] / line["torch_ms"]["median"]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", choices=OPS, default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--timeout", type=int, default=120, help="seconds every op's process may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.op is not None:
        print(json.dumps(measure(args.op, args.rounds, args.window)), flush=True)
        return
    lines = []
    for op in OPS:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--op", op, "--rounds", str(args.rounds),
               "--window", str(args.window)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode != 0:
            sys.stderr.write(res.stderr[-4000:])
            raise SystemExit(f"pair_bench: {op} ended with status {res.returncode}; nothing further is started")
        lines.append(res.stdout.strip().splitlines()[-1])
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

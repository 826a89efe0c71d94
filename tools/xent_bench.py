"""Time forward + backward of ops.softmax_cross_entropy (csrc/loss_ops.hip) against torch.nn.functional.cross_entropy on the
same GPU, at the shapes the BERT task models meet: the masked-LM loss (16384, 30522), token classification (16384, 9), a
sequence-classification head (32, 2) and the question-answering layout (32, 384) read at element stride 2 out of a (32, 384, 2)
tensor.  The baseline is torch's own kernels (log_softmax + nll_loss and their backward), at ignore_index = -1 with 15 % of the
rows kept at the masked-LM shape (and that shape again with every row kept) and every row kept elsewhere.

A tool, not a test.  Without --variant this is a driver that never touches the GPU itself: it runs every (variant, shape) in a
process of its own under a time limit (the widest holds 2 GB of logits, their gradient and, for torch, the saved log-softmax)
and starts nothing further after one that fails, is killed or runs out of time.  With --variant and --shape it measures that
one: a host clock around work that ends in a device synchronise, after a warm-up; windows of at least --window seconds,
--rounds rounds; the median time per forward + backward and the spread.

Each line carries the milliseconds, the peak device memory above the logits themselves, and the algorithmic minimum traffic --
two reads and one write of the logits, 12 B per element -- as a rate and as a fraction of 6.29 TB/s, the float4 copy rate measured
on the MI355X, and beside it the bytes the HIP kernels really move (the backward does not read the rows it only zeroes: 8 B per
element plus 4 B per element of a kept row) as a fraction of that rate.

    python tools/xent_bench.py [--rounds 5] [--window 0.5] [--timeout 300] [--out FILE]

Prints one JSON line per variant and shape.
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

VARIANTS = ["hip", "torch"]
SHAPES = {"mlm_16384x30522": (16384, 30522, 1), "mlm_16384x30522_all_kept": (16384, 30522, 1), "tokens_16384x9": (16384, 9, 1),
          "head_32x2": (32, 2, 1), "qa_32x384_cs2": (32, 384, 2)}
COPY_RATE = 6.29e12          # bytes per second, float4 copy


def timed(fn, rounds, window, sync):
    fn()
    sync()
    times = []
    for _ in range(rounds):
        n, t0 = 0, time.perf_counter()
        while True:
            fn()
            n += 1
            sync()
            dt = time.perf_counter() - t0
            if dt >= window:
                break
        times.append(1e3 * dt / n)
    return {"median": float(np.median(times)), "min": float(min(times)), "max": float(max(times))}


def measure(variant, shape, rounds, window):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("xent_bench: needs a GPU; a CPU run says nothing about the MI355X")
    from get_amd import ops
    dev = torch.device("cuda:0")
    rows, c, cs = SHAPES[shape]
    g = torch.Generator(device=dev).manual_seed(11)
    store = torch.randn((rows, c, cs) if cs > 1 else (rows, c), generator=g, device=dev).requires_grad_(True)
    logits = store[..., 0] if cs > 1 else store
    labels = torch.randint(0, c, (rows,), generator=g, device=dev)
    if shape == "mlm_16384x30522":
        labels[torch.rand(rows, generator=g, device=dev) >= 0.15] = -1
    fn = ops.softmax_cross_entropy if variant == "hip" else torch.nn.functional.cross_entropy

    def step():
        store.grad = None
        fn(logits, labels, ignore_index=-1).backward()

    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t = timed(step, rounds, window, torch.cuda.synchronize)
    peak = torch.cuda.max_memory_allocated() - base
    nbytes = 12 * rows * c
    rate = nbytes / (t["median"] * 1e-3)
    # what the HIP kernels really move: the forward reads every row, the backward reads the kept rows and writes every row
    kept = float((labels != -1).double().mean())
    moved = int((8 + 4 * kept) * rows * c)
    return {"variant": variant, "shape": shape, "rows": rows, "c": c, "cs": cs, "rounds": rounds, "window_s": window, "ms": t,
            "min_bytes": nbytes, "tb_per_s": rate / 1e12, "of_copy_rate": rate / COPY_RATE, "peak_bytes_above_logits": int(peak),
            "kept_rows": kept, "hip_moved_bytes": moved, "hip_moved_of_copy_rate": moved / (t["median"] * 1e-3) / COPY_RATE}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=VARIANTS, default=None)
    ap.add_argument("--shape", choices=list(SHAPES), default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds every measurement's process may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.variant is not None:
        if args.shape is None:
            raise SystemExit("xent_bench: --variant needs --shape")
        print(json.dumps(measure(args.variant, args.shape, args.rounds, args.window)), flush=True)
        return
    lines = []
    for shape in SHAPES:
        for variant in VARIANTS:
            cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--variant", variant, "--shape",
                   shape, "--rounds", str(args.rounds), "--window", str(args.window)]
            res = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(res.stdout)
            sys.stdout.flush()
            if res.returncode != 0:
                sys.stderr.write(res.stderr[-4000:])
                raise SystemExit(f"xent_bench: {variant} at {shape} ended with status {res.returncode}; nothing further is started")
            lines.append(res.stdout.strip().splitlines()[-1])
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

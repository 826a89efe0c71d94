"""Time one optimiser step with gradient clipping on a BERT-base-sized set of parameters (the state_dict shapes of BertConfig's
defaults: 199 tensors, about 110 M elements): get_amd.optim.AdamW (csrc/optim_ops.hip: the norm in two launches, the update in
one) against torch's own torch.optim.AdamW after torch.nn.utils.clip_grad_norm_ in its per-parameter, foreach and fused forms.
That baseline is torch's code, not the reference's AdamW, whose step issues about eight elementwise launches per parameter.

A tool, not a test.  Without --variant this is a driver that never touches the GPU itself: it runs every variant in a process of
its own under a time limit (each holds parameters, gradients and two moments, 1.8 GB) and starts nothing further after one that
fails, is killed or runs out of time.  With --variant it measures that one: a host clock around work that ends in a device
synchronise, after a warm-up; windows of at least --window seconds, --rounds rounds; the median time per step and the spread.

For the HIP variant the line also carries the update alone and the norm alone, with the bytes they move -- 28 B per element for
the update (p, m, v read and written, g read), 4 B per element for the norm -- and that rate as a fraction of 6.29 TB/s, the
float4 copy rate measured on the MI355X, which is the ceiling of a streaming kernel there.

    python tools/optim_bench.py [--rounds 5] [--window 0.5] [--timeout 300] [--out FILE]

Prints one JSON line per variant.
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

VARIANTS = ["hip", "torch_loop", "torch_foreach", "torch_fused"]
COPY_RATE = 6.29e12          # bytes per second, float4 copy
MAX_NORM = 1.0


def bert_base_shapes():
    import torch
    from get_amd.bert import BertConfig, BertModel
    with torch.device("meta"):
        model = BertModel(BertConfig())
    return [(k, tuple(p.shape)) for k, p in model.named_parameters()]


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


def measure(variant, rounds, window):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench: needs a GPU; a CPU run says nothing about the MI355X")
    from get_amd import ops, optim
    dev = torch.device("cuda:0")
    shapes = bert_base_shapes()
    g = torch.Generator(device=dev).manual_seed(7)
    params = [torch.nn.Parameter(torch.randn(s, generator=g, device=dev) * 0.02) for _, s in shapes]
    grads = [torch.randn(s, generator=g, device=dev) * 0.01 for _, s in shapes]
    no_decay = [("bias" in k or "LayerNorm" in k) for k, _ in shapes]
    groups = [dict(params=[p for p, nd in zip(params, no_decay) if not nd], weight_decay=0.01),
              dict(params=[p for p, nd in zip(params, no_decay) if nd], weight_decay=0.0)]
    elements = sum(p.numel() for p in params)
    line = {"variant": variant, "tensors": len(params), "elements": elements, "rounds": rounds, "window_s": window, "max_norm": MAX_NORM}
    sync = torch.cuda.synchronize
    if variant == "hip":
        opt = optim.AdamW(groups, lr=5e-5, max_grad_norm=MAX_NORM)
        opt._matrices = []          # the transposes the next forward consumes are not part of what the torch variants do either
        for p, gr in zip(params, grads):
            p.grad.copy_(gr)
        del grads
        line["bucket_elements"] = n = opt.flat_p.numel()
        line["step_ms"] = timed(opt.step, rounds, window, sync)
        fs = opt._flat_step
        hypers = [(5e-5, (0.9, 0.999), 1e-6, 0.01, True, 10)] * len(params)
        table = fs.table.upload(hypers)
        upd = timed(lambda: ops.adamw_step_flat(fs.p, fs.g, fs.m, fs.v, fs.block_seg, table), rounds, window, sync)
        nrm = timed(lambda: ops.grad_norm_flat(fs.g, 1.0, fs.partials, fs.norm), rounds, window, sync)
        for tag, t, per in (("update", upd, 28), ("norm", nrm, 4)):
            rate = per * n / (t["median"] * 1e-3)
            line[tag] = {"ms": t, "bytes": per * n, "tb_per_s": rate / 1e12, "of_copy_rate": rate / COPY_RATE}
        line["step_bytes"] = 32 * n
        line["step_of_copy_rate"] = 32 * n / (line["step_ms"]["median"] * 1e-3) / COPY_RATE
    else:
        kw = {"torch_loop": dict(foreach=False), "torch_foreach": dict(foreach=True), "torch_fused": dict(fused=True)}[variant]
        opt = torch.optim.AdamW(groups, lr=5e-5, eps=1e-6, **kw)
        for p, gr in zip(params, grads):
            p.grad = gr
        clip_kw = dict(foreach=False) if variant == "torch_loop" else {}

        def step():
            torch.nn.utils.clip_grad_norm_(params, MAX_NORM, **clip_kw)
            opt.step()
        line["step_ms"] = timed(step, rounds, window, sync)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=VARIANTS, default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds every variant's process may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.variant is not None:
        print(json.dumps(measure(args.variant, args.rounds, args.window)), flush=True)
        return
    lines = []
    for variant in VARIANTS:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--variant", variant, "--rounds",
               str(args.rounds), "--window", str(args.window)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(res.stdout)
        sys.stdout.flush()
        if res.returncode != 0:
            sys.stderr.write(res.stderr[-4000:])
            raise SystemExit(f"optim_bench: {variant} ended with status {res.returncode}; nothing further is started")
        lines.append(res.stdout.strip().splitlines()[-1])
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

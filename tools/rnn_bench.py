"""Time a sequence-encoder drop-in (get_amd.modules.LSTM / GRU: HIP recurrence kernels) against torch's own nn.LSTM / nn.GRU on
packed sequences.

A tool, not a test.  Forward + backward of one bidirectional layer at the project's two shapes, lengths drawn by
get_amd/synth.py's make_tokens (evidence side: every length 100; claim side: uniform in [5, 30]):

    evidence   960 x 100, D = H = 300
    claim       32 x  30, D = H = 300

The baseline is the reference's forward (Models/BiDAF/wrapper.py:256-276 / :306-327) written with torch's module: the sorted
gather, pack_padded_sequence, nn.LSTM / nn.GRU (MIOpen), pad_packed_sequence, the restoring gather -- same weights, same GPU;
neither applies dropout.  Timing: a host clock around work that ends in a device synchronise, after a warm-up of every shape;
windows of at least --window seconds, the two versions alternated in the same call for --rounds rounds; the median time per
iteration and the spread (min .. max over the windows) are reported.  The outputs and gradients of the two are compared at the
timed shape (largest error over largest entry), before anything is timed.  After the windows, the pieces of the drop-in's
step are timed on their own with device events (median of --piece-iters launches): the two gx GEMMs, the forward recurrence
(saving for the backward), the backward recurrence, the two dW_hh (GRU: and db_hh) GEMMs.

    python tools/rnn_bench.py --cell lstm|gru [--rounds 5] [--window 1.0] [--out FILE]

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
import torch.nn as nn  # noqa: E402

SHAPES = {"evidence": dict(B=960, L=100, min_len=100), "claim": dict(B=32, L=30, min_len=5)}
D = H = 300
GATES = {"lstm": 4, "gru": 3}


def baseline_forward(rnn, x, lens_sorted_cpu, new, restoring, max_len):
    packed = nn.utils.rnn.pack_padded_sequence(x[new], lens_sorted_cpu, batch_first=True)
    out, h = rnn(packed)
    if isinstance(h, tuple):      # nn.LSTM: (h_n, c_n)
        h = h[0]
    y = nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=max_len)[0][restoring]
    return y, h.permute(1, 0, 2).contiguous().view(-1, h.size(0) * h.size(2))[restoring]


def pieces(cell, m, x, lens, order, T, gy, iters, ops, _lib, call, ptr, stream):
    """Device-event times (us, median over `iters`) of the four pieces of one bidirectional layer's forward + backward."""
    r, dev, G = m.rnn, x.device, GATES[cell]
    n, t_in, h = x.shape[0], x.shape[1], r.hidden_size
    ws = [r.weight_hh_l0.detach(), r.weight_hh_l0_reverse.detach()]
    bs = [r.bias_hh_l0.detach(), r.bias_hh_l0_reverse.detach()]
    new = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
    # `aux`: the LSTM's saved c, the GRU's saved a_n; `dpre`: the LSTM's dgates, the GRU's gradient of a
    y, hn, gates, aux, hprev = new(n, T, 2 * h), new(2, n, h), new(2, n, t_in, G * h), new(2, n, t_in, h), new(2, n, t_in, h)
    cn, dgx, dpre = torch.empty_like(hn), torch.empty_like(gates), torch.empty_like(gates)
    dw, db = torch.zeros(G * h, h, device=dev), torch.zeros(G * h, device=dev)
    _lib.ensure_workspace(dev)
    gx = []

    def gx_gemms():
        if cell == "lstm":
            gx[:] = [ops.linear(x, r.weight_ih_l0, r.bias_ih_l0 + r.bias_hh_l0),
                     ops.linear(x, r.weight_ih_l0_reverse, r.bias_ih_l0_reverse + r.bias_hh_l0_reverse)]
        else:
            gx[:] = [ops.linear(x, r.weight_ih_l0, r.bias_ih_l0), ops.linear(x, r.weight_ih_l0_reverse, r.bias_ih_l0_reverse)]

    def fwd():
        if cell == "lstm":
            call("gh_lstm_seq_fwd", ptr(gx[0]), ptr(gx[1]), G * h, ptr(ws[0]), ptr(ws[1]), ptr(lens), ptr(order), n, t_in, T, h, 2, ptr(y),
                 2 * h, ptr(gates), ptr(aux), ptr(hprev), ptr(hn), ptr(cn), stream())
        else:
            call("gh_gru_seq_fwd", ptr(gx[0]), ptr(gx[1]), G * h, ptr(ws[0]), ptr(ws[1]), ptr(bs[0]), ptr(bs[1]), ptr(lens), ptr(order), n,
                 t_in, T, h, 2, ptr(y), 2 * h, ptr(gates), ptr(aux), ptr(hprev), ptr(hn), stream())

    def bwd():
        if cell == "lstm":
            call("gh_lstm_seq_bwd", ptr(ws[0]), ptr(ws[1]), ptr(lens), ptr(order), n, t_in, T, h, 2, ptr(gy), 2 * h, None, ptr(gates),
                 ptr(aux), ptr(dpre), stream())
        else:
            call("gh_gru_seq_bwd", ptr(ws[0]), ptr(ws[1]), ptr(lens), ptr(order), n, t_in, T, h, 2, ptr(gy), 2 * h, None, ptr(gates),
                 ptr(aux), ptr(hprev), ptr(dgx), ptr(dpre), stream())

    def wgrad():
        for d in range(2):
            call("gh_linear_bwd", ptr(hprev[d]), None, None, ptr(dpre[d]), n * t_in, h, G * h, None, ptr(dw),
                 ptr(db) if cell == "gru" else None, stream())

    out = {}
    with torch.no_grad():
        for tag, fn in (("gx_gemms", gx_gemms), ("fwd_recurrence", fwd), ("bwd_recurrence", bwd), ("dw_hh_gemms", wgrad)):
            fn()
            torch.cuda.synchronize()
            ts = []
            for _ in range(iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(1e3 * e0.elapsed_time(e1))
            out[tag] = float(np.median(ts))
    out["fwd_per_step"] = out["fwd_recurrence"] / t_in
    out["bwd_per_step"] = out["bwd_recurrence"] / t_in
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", choices=sorted(GATES), required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--piece-iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rnn_bench: needs a GPU; a CPU run says nothing about the MI355X")
    from get_amd import _lib, modules, ops
    from get_amd._lib import call, ptr, stream
    from get_amd.synth import make_tokens
    dev = torch.device("cuda:0")
    drop_in, torch_rnn = {"lstm": (modules.LSTM, nn.LSTM), "gru": (modules.GRU, nn.GRU)}[args.cell]
    lines = []
    for name, s in SHAPES.items():
        B, L = s["B"], s["L"]
        rng = np.random.default_rng(7)
        _, lens_np = make_tokens(rng, B, L, 1000, s["min_len"], L)
        lens_cpu = torch.from_numpy(lens_np).long()
        new = torch.sort(lens_cpu, descending=True, stable=True)[1].to(dev)
        restoring = torch.argsort(new)
        torch.manual_seed(3)
        m = drop_in(D, H, bidirectional=True).to(dev).eval()
        ref = torch_rnn(D, H, bidirectional=True, batch_first=True).to(dev)      # (training mode: MIOpen's backward needs it; no dropout)
        ref.load_state_dict(m.rnn.state_dict())
        x = torch.randn(B, L, D, device=dev, requires_grad=True)
        gy, gh = torch.randn(B, L, 2 * H, device=dev), torch.randn(B, 2 * H, device=dev)
        lens_dev = lens_cpu.to(dev)
        lens_sorted_cpu = lens_cpu[new.cpu()]      # (the reference copies the sorted lengths to the host on every call; the baseline does not)

        def run_hip():
            m.zero_grad(set_to_none=True)
            x.grad = None
            y, h = m((x, lens_dev, new, restoring), max_len=L)
            ((y * gy).sum() + (h * gh).sum()).backward()
            return y, h

        def run_ref():
            ref.zero_grad(set_to_none=True)
            x.grad = None
            y, h = baseline_forward(ref, x, lens_sorted_cpu, new, restoring, L)
            ((y * gy).sum() + (h * gh).sum()).backward()
            return y, h

        def rel(a, b):
            return float((a - b).abs().max() / b.abs().max())

        y1, h1 = run_hip()
        g1 = {"x": x.grad.clone(), **{k: p.grad.clone() for k, p in m.rnn.named_parameters()}}
        y2, h2 = run_ref()
        g2 = {"x": x.grad.clone(), **{k: p.grad.clone() for k, p in ref.named_parameters()}}
        diff = {"y": rel(y1, y2), "h": rel(h1, h2), **{"grad " + k: rel(g1[k], g2[k]) for k in g1}}
        for fn in (run_hip, run_ref):      # warm-up
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {"hip": [], "torch": []}
        for _ in range(args.rounds):
            for tag, fn in (("hip", run_hip), ("torch", run_ref)):
                n, t0 = 0, time.perf_counter()
                while True:
                    fn()
                    n += 1
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if dt >= args.window:
                        break
                times[tag].append(1e3 * dt / n)
        line = {"cell": args.cell, "shape": name, "B": B, "L": L, "D": D, "H": H, "mean_len": float(lens_np.mean()), "rounds": args.rounds,
                "window_s": args.window, "max_rel_diff": max(diff.values()), "rel_diff": diff}
        for tag, ts in times.items():
            line[tag + "_ms"] = {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}
        line["hip_over_torch"] = line["hip_ms"]["median"] / line["torch_ms"]["median"]
        line["pieces_us"] = pieces(args.cell, m, x.detach(), lens_dev.int(), new.int(), L, gy, args.piece_iters, ops, _lib, call, ptr, stream)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

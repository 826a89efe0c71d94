"""Time the ranking metrics of a batch of query groups two ways, on the same scores and labels, in one process.

A tool, not a test.  Two shapes: --shape get, 2000 groups of 0..30 items (the GET-style evaluation), and --shape long, 64 groups
of 1024 items (a ranking dataset at the group limit).  Scores are 2 randn rounded to a quarter, labels integers 0..3; the
metrics are AP, MAP, MRR and precision / DCG / NDCG at k = 1, 3, 10.

    a  host_loop   what the reference's evaluation does with its classes: per group, sort on the host and loop per metric -- here
                   the float64 restatement tests/rank_ref.group_metrics, which computes all twelve values of a group from ONE
                   sort (the reference's classes sort once per metric, AveragePrecision once per item), so this arm is timed in
                   its favour; scores and labels start on the host
    b  one_launch  get_amd.ranking.ranking_metrics on device-resident scores and labels with host offsets: one gh_rank_metrics
                   launch, one read-back, the float64 means on the host

Every arm ends with its values on the host; after a warm-up of both, the arms are alternated for --rounds rounds and the median
wall time is reported with the spread.  The kernel's own time is taken with device events around --kernel-reps back-to-back
launches into preallocated outputs.

    python tools/rank_bench.py [--shape get|long] [--rounds 7] [--kernel-reps 200] [--out FILE]

Prints one JSON line.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

KS = [1, 3, 10]


def make_batch(shape, seed=0):
    g = np.random.default_rng(seed)
    lengths = g.integers(0, 31, 2000) if shape == "get" else np.full(64, 1024)
    offsets = np.zeros(len(lengths) + 1, np.int32)
    offsets[1:] = np.cumsum(lengths)
    n = int(offsets[-1])
    return np.round(8 * g.standard_normal(n)) / 4, g.integers(0, 4, n).astype(np.float64), offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["get", "long"], default="get")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--out")
    args = ap.parse_args()
    from get_amd import _lib, ranking as K
    from tests import rank_ref as R
    dev = torch.device("cuda:0")
    scores, labels, offsets = make_batch(args.shape)
    d_scores, d_labels = torch.from_numpy(scores).to(dev), torch.from_numpy(labels).to(dev)
    metrics = [K.AveragePrecision(), K.MeanAveragePrecision(), K.MeanReciprocalRank()] + \
        [cls(k) for cls in (K.Precision, K.DiscountedCumulativeGain, K.NormalizedDiscountedCumulativeGain) for k in KS]

    def host_loop():
        return R.batch_metrics(labels, scores, offsets, KS, 0.)[2].mean(axis=0)

    def one_launch():
        return K.ranking_metrics(metrics, d_scores, d_labels, offsets)

    arms = {"host_loop": host_loop, "one_launch": one_launch}
    want, got = host_loop(), one_launch()
    worst = max(abs(got[m] - float(m._pick(want[None, :], KS)[0])) for m in metrics)
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    # the launch alone (memset of the two counters + kernel), device events around back-to-back calls
    n, g, nk = len(scores), len(offsets) - 1, len(KS)
    off_dev = torch.from_numpy(offsets).to(dev)
    rank = torch.empty(n, device=dev, dtype=torch.int32)
    gi = torch.empty((g, 3 + nk), device=dev, dtype=torch.int32)
    gd = torch.empty((g, 3 + 3 * nk), device=dev, dtype=torch.float64)
    nan_count = torch.empty(2, device=dev, dtype=torch.int32)
    ks_host = (ctypes.c_int32 * nk)(*KS)

    def launch():
        _lib.call("gh_rank_metrics", _lib.ptr(d_scores), 1, _lib.ptr(d_labels), _lib.ptr(off_dev), offsets.ctypes.data, n, g, 0.0,
                  ctypes.cast(ks_host, ctypes.c_void_p), nk, _lib.ptr(rank), _lib.ptr(gi), _lib.ptr(gd), _lib.ptr(nan_count), _lib.stream())

    launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.kernel_reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    res = {"shape": args.shape, "groups": g, "items": n, "rounds": args.rounds, "max_abs_diff_of_the_means": worst,
           "kernel_us_per_call": e0.elapsed_time(e1) * 1e3 / args.kernel_reps}
    for name, t in times.items():
        res[name + "_ms"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
    res["speedup"] = res["host_loop_ms"]["median"] / res["one_launch_ms"]["median"]
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

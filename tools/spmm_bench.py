#!/usr/bin/env python
"""Aggregation (spmm) micro-benchmark: Zipf word graphs vs near-diagonal graphs, padded and node-compact layouts, the bf16
pipeline's kernels, and a plain device copy of the same bytes for reference.  Phase ticks need the tool build (bench.py --measure-build)."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from get_amd import _lib, ops  # noqa: E402
from get_amd.synth import make_tokens  # noqa: E402

dev = "cuda:0"
n, r, h = 960, 100, 300
rng = np.random.default_rng(0)


def timeit(fn, reps=20):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


x = torch.randn(n, r, h, device=dev)
y = torch.empty_like(x)
for name, toks in (("zipf", make_tokens(rng, n, r, 20000, r, r)[0]),
                   ("distinct", (np.arange(n * r).reshape(n, r) % 19000 + 2).astype(np.int32))):
    lens = np.full((n,), r, np.int32)
    adj, _, n_nodes = ops.graph_build(torch.from_numpy(toks).to(dev), torch.from_numpy(lens).to(dev), 3)
    nnz = float(torch.count_nonzero(adj.to_dense())) / n
    deg = adj.to_dense().ne(0).sum(-1).max().item()
    ms = timeit(lambda: _lib.call("gh_spmm", *adj._args(), None, 0, x.data_ptr(), y.data_ptr(), n, r, h, 0, 0, _lib.stream()))
    print(f"{name:9s} nnz/graph {nnz:7.1f} max degree {deg:3d}: {ms*1e3:7.1f} us  {2*n*r*h*4/ms/1e6:7.1f} GB/s")
    # node-compact layout (what the training step runs): the real nodes of all graphs back to back
    goff = torch.zeros(n + 1, device=dev, dtype=torch.int32)
    goff[1:] = torch.cumsum(n_nodes, 0).to(torch.int32)
    m_real = int(goff[-1])
    real = (torch.arange(r, device=dev)[None, :] < n_nodes[:, None])
    xc = x[real].contiguous()
    yc = torch.empty_like(xc)
    msc = timeit(lambda: _lib.call("gh_spmm", *adj._args(), goff.data_ptr(), m_real, xc.data_ptr(), yc.data_ptr(), n, r, h, 0, 0, _lib.stream()))
    # reference: the padded launch on an input whose padding rows are zero
    xz = torch.where(real[..., None], x, torch.zeros_like(x))
    _lib.call("gh_spmm", *adj._args(), None, 0, xz.data_ptr(), y.data_ptr(), n, r, h, 0, 0, _lib.stream())
    err = float((y[real] - yc).abs().max())
    dense = (adj.to_dense().double() @ xz.double())[real]
    err64 = float((dense - yc.double()).abs().max())
    print(f"{name:9s} compact m_real {m_real} ({m_real / n:.1f} rows/graph): {msc*1e3:7.1f} us  {2*m_real*h*4/msc/1e6:7.1f} GB/s  "
          f"|compact - padded| {err:.2e}  |compact - dense f64| {err64:.2e}")
PHASES = ["issue", "rowwords+scan", "barrier1", "listbuild", "slabwait", "barrier2", "aggregate"]


def phase_ticks(run):
    """Tool build only: per-phase s_memtime ticks of the edge-list kernel, thread 0 of every workgroup that ran."""
    L = _lib.load()
    L.gh_debug_spmm_phases.argtypes = [ctypes.c_void_p, ctypes.c_int]
    buf = (ctypes.c_uint * (8192 * 8))()
    L.gh_debug_spmm_phases(None, 1)
    run()
    torch.cuda.synchronize()
    L.gh_debug_spmm_phases(buf, 1)
    a = np.frombuffer(buf, dtype=np.uint32).reshape(8192, 8)[:, :7].astype(np.float64)
    a = a[a.sum(1) > 0]                     # workgroups that ran (one per graph and chunk of slabs)
    return (f"{a.shape[0]} workgroups, s_memtime ticks (~0.5 ns; with several slabs per workgroup the slab phases hold the LAST slab), "
            "mean / p90: " + ", ".join(f"{nm} {a[:, i].mean():.2f}/{np.percentile(a[:, i], 90):.2f}" for i, nm in enumerate(PHASES))
            + f"  total {a.sum(1).mean():.2f}")


def compact(toks, n_graphs, window):
    """graph_build + the node-compact row offsets of its graphs"""
    adj, _, n_nodes = ops.graph_build(torch.from_numpy(toks).to(dev), torch.from_numpy(np.full((n_graphs,), toks.shape[1], np.int32)).to(dev), window)
    goff = torch.zeros(n_graphs + 1, device=dev, dtype=torch.int32)
    goff[1:] = torch.cumsum(n_nodes, 0).to(torch.int32)
    return adj, goff, int(goff[-1])


try:
    print("phases, thread 0 of each of " + phase_ticks(lambda: _lib.call("gh_spmm", *adj._args(), goff.data_ptr(), m_real, xc.data_ptr(),
                                                                            yc.data_ptr(), n, r, h, 0, 0, _lib.stream())))
except Exception as e:
    print("no phase instrumentation:", e)
# the bf16 storage pipeline's aggregation at the configs[4] shape (h = 768, window 5, node-compact): the matrix-pipe kernel (R <= 128);
# its edge-list kernel -- the one with phase ticks -- runs for graphs of more than 128 nodes (R = 200)
try:
    h16 = 768
    adj16, goff16, m16 = compact(make_tokens(rng, n, r, 20000, r, r)[0], n, 5)
    x16 = torch.randn(m16, h16, device=dev).to(torch.bfloat16)
    y16 = torch.empty_like(x16)
    nnz16 = float(torch.count_nonzero(adj16.to_dense())) / n
    for acc in (0, 1):
        ms16 = timeit(lambda: _lib.call("gh_spmm_bf16", *adj16._args(), goff16.data_ptr(), m16, x16.data_ptr(), y16.data_ptr(), n, r, h16, 0, acc, _lib.stream()))
        print(f"bf16 h=768 window 5 compact m_real {m16} nnz/graph {nnz16:.1f} accumulate {acc}: {ms16*1e3:7.1f} us  {(2 + acc)*m16*h16*2/ms16/1e6:7.1f} GB/s")
    n2, r2 = 640, 200
    adj2, goff2, m2 = compact(make_tokens(rng, n2, r2, 20000, r2, r2)[0], n2, 5)
    x2 = torch.randn(m2, h16, device=dev).to(torch.bfloat16)
    y2 = torch.empty_like(x2)
    run2 = lambda: _lib.call("gh_spmm_bf16", *adj2._args(), goff2.data_ptr(), m2, x2.data_ptr(), y2.data_ptr(), n2, r2, h16, 0, 0, _lib.stream())  # noqa: E731
    ms2 = timeit(run2)
    print(f"bf16 h=768 window 5 R=200 (edge-list kernel) compact m_real {m2}: {ms2*1e3:7.1f} us  {2*m2*h16*2/ms2/1e6:7.1f} GB/s")
    print("bf16 R=200 phases, thread 0 of each of " + phase_ticks(run2))
except Exception as e:
    print("bf16 section failed:", e)
ms = timeit(lambda: y.copy_(x))
print(f"copy      {ms*1e3:7.1f} us  {2*n*r*h*4/ms/1e6:7.1f} GB/s")

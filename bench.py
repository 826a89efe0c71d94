#!/usr/bin/env python
"""GET hot-path benchmark: claim-evidence pairs/s, forward + backward (+ gradient all-reduce + Adam),
on synthetic Snopes-shaped batches (BASELINE.json configs[1]: B=32 claims x 30 evidences, L=30, R=100,
D=H=300, 5 word heads / 2 evidence heads, window 3, gsl_rate 0.6, fp32).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus 1 --steps 20 --warmup 5 --full              # + every side measurement (see below)
    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR  # + the last timed step's results as DIR/*.npy
    python bench.py --gpus N ...          # RANK unset: re-executes itself under torch.distributed.run, one rank per GPU
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = graph build from token ids + full model forward + cross-entropy + backward + one flat
gradient all-reduce (N>1) + fused Adam, with the batch already resident in HBM.  Rank 0 prints ONE
JSON line.  Weak scaling: every rank runs its own B=32 batch (claims are independent; the only
exchange is the gradient all-reduce).

A plain run sets up, runs --warmup W steps, times exactly --steps K steps as one block, optionally
writes the outputs of the last timed step (--dump-outputs) and prints the line.  --full adds what the
headline figure does not need: the repeated-block statistics with the live roofline of the dominant
kernel, the per-kernel table, the phase split, the strong-scaling leg, the side regimes, the realistic
series, the other BASELINE configs, the parity slice against the CPU oracle, the CPU baseline and the
box's copy / BLAS ceilings (each still switched off by its --no-* option).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from get_amd.synth import SynthConfig, make_embeddings, make_raw_batch  # noqa: E402

PEAK_F32_MFMA_TFLOPS = 157.3     # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, dense, spec
PEAK_BF16_MFMA_TFLOPS = 2500.0   # same guide: dense bf16 MFMA (the opt-in --gemm-mode bf16 prices gemm_big against this)
PEAK_HBM_GBPS = 8000.0           # HBM3E spec (6.3 TB/s achievable)


def flops_per_pair(cfg: SynthConfig, nnz_per_graph: float, real_nodes: float = None) -> dict:
    """Minimal-formulation FLOPs per claim-evidence pair (SURVEY.md 8(d) formulas as functions).
    `fwd_bwd`: every layer on all R padded node rows (the reference's shape of the work).
    `executed`: what the node-compact layout actually runs -- the first cell's forward and the scorer on R rows,
    everything else on the `real_nodes` (mean unique tokens per evidence) rows that can influence a result."""
    R, D, H, hw = cfg.len_right, cfg.emb_dim, cfg.hidden, cfg.word_heads

    def cell(rows, din, dout, agg):
        return 2 * rows * din * dout + 12 * rows * dout * dout + agg * dout

    def att(rows):
        return 2 * H * H + 2 * rows * H * H + 2 * rows * H * hw + 2 * rows * H * hw

    agg = 2 * nnz_per_graph
    fwd = cell(R, D, H, agg) + cell(R, H, 1, agg) + cell(R, H, H, agg) + att(R)
    out = {"fwd": fwd, "fwd_bwd": 3 * fwd - 2 * R * D * H}
    if real_nodes is not None:
        n = real_nodes
        fwd_x = cell(R, D, H, agg) + cell(R, H, 1, agg) + cell(n, H, H, agg) + att(n)
        bwd_x = 2 * (cell(n, D, H, agg) + cell(n, H, H, agg) + att(n)) - 2 * n * D * H
        out["executed"] = fwd_x + bwd_x
    return out


def build_workload(batch=32, n_evd=30, seed=20240229, device="cuda:0", cfg: SynthConfig = None, lr=1e-4, compact=None,
                   n_batches=1, evd_dist="fixed", model_seed=None, claim_shard=None):
    """Model (random init, reference init scheme), `n_batches` distinct seeded synthetic batches resident on `device`
    (seed, seed + 1000, ...; the step loop rotates through them so that no per-batch cost hides behind one reused
    batch), and `oracle_slice(k)`: CPU-oracle results of the first k claims of batch 0.
    evd_dist: "fixed" (cfg.n_evd per claim; <= 0 = U[1,30]) or "snopes" (empirical histogram, mean 6.9).
    model_seed: seed of the embeddings and the parameter init (default: `seed`); data-parallel ranks pass the SAME
    model_seed and different data seeds, so that replicas are identical by construction.
    claim_shard(counts) -> claim indices: this rank's shard of a GLOBAL batch of cfg.batch claims (strong scaling: every
    rank generates the same global batch from `seed` and keeps its shard, dist.shard_claims)."""
    from get_amd import modules
    from get_amd.batch import NativeBatch
    from get_amd.synth import snopes_evidence_counts
    cfg = cfg or SynthConfig(batch=batch, n_evd=n_evd)
    model_seed = seed if model_seed is None else model_seed
    emb, art, clm = make_embeddings(cfg, model_seed)
    torch.manual_seed(model_seed)
    model = modules.Graph_basedSemantiStructure(cfg.model_params(emb, art, clm)).to(device)
    raws, batches = [], []
    for i in range(max(1, n_batches)):
        c = cfg
        if evd_dist == "snopes":
            counts = snopes_evidence_counts(np.random.default_rng(seed + 1000 * i + 17), cfg.batch)
            c = SynthConfig(**{**cfg.__dict__, "evd_counts": [int(x) for x in counts]})
        raw = make_raw_batch(c, seed + 1000 * i)
        if claim_shard is not None:
            raw = subset_raw(raw, claim_shard(raw["evd_counts"]))
        raws.append(raw)
        batches.append(NativeBatch(raw["claim_tokens"], raw["claim_len"], raw["evd_tokens"], raw["evd_len"], raw["evd_counts"],
                                   raw["doc_sources"], raw["query_sources"], raw["labels"], window=cfg.window,
                                   n_max=cfg.fixed_num_evidences, device=device, compact=compact))
    raw, b0 = raws[0], batches[0]
    if claim_shard is not None:
        cfg = SynthConfig(**{**cfg.__dict__, "batch": b0.b, "evd_counts": None})
    query, document, kargs = b0.inputs()
    nnz = float(torch.count_nonzero(kargs["docs_adj"].to_dense()).item()) / max(b0.b1, 1)

    def oracle_slice(k: int, return_aux=False):
        from oracle import get_oracle as O
        from oracle.assemble import assemble_inputs
        sub_cfg = SynthConfig(**{**cfg.__dict__, "batch": k, "evd_counts": [int(c) for c in raw["evd_counts"][:k]]})
        nb1 = int(raw["evd_counts"][:k].sum())
        sub = dict(claim_tokens=raw["claim_tokens"][:k], claim_len=raw["claim_len"][:k],
                   evd_tokens=raw["evd_tokens"][:nb1], evd_len=raw["evd_len"][:nb1],
                   evd_counts=raw["evd_counts"][:k], doc_sources=raw["doc_sources"][:k],
                   query_sources=raw["query_sources"][:k], labels=raw["labels"][:k])
        inp = assemble_inputs(sub, sub_cfg, O.convert_text)
        p = {kk: v.detach().cpu().clone() for kk, v in model.state_dict().items()}
        T = torch.from_numpy
        res = O.model_forward(p, sub_cfg.__dict__, T(inp["query"]), T(inp["document"]), T(inp["query_adj"]),
                              T(inp["doc_ids"]), T(inp["doc_adj"]), T(inp["query_lens"]), inp["evd_counts"],
                              T(inp["doc_sources"]), T(inp["query_sources"]), return_aux=return_aux)
        out = dict(phi=res[0].detach(), word_w=res[1].detach(), inp=inp, params=p, cfg=sub_cfg)
        if return_aux:
            out["keep"] = res[3]["keep"]
        return out

    return dict(cfg=cfg, model=model, raw=raw, raws=raws, batches=batches, oracle_slice=oracle_slice, nnz_per_graph=nnz,
                query=query, document=document, kargs=kargs, labels=b0.labels, make_inputs=b0.inputs,
                compact=b0.compact, b1=sum(b.b1 for b in batches) / len(batches), b1_each=[b.b1 for b in batches],
                m_real=sum(b.m_real for b in batches) / len(batches))


def subset_raw(raw: dict, claims) -> dict:
    """The claims `claims` (ascending indices) of a raw batch, evidences kept claim-major."""
    cl = np.asarray(list(claims), dtype=np.int64)
    counts = raw["evd_counts"]
    offs = np.concatenate([[0], np.cumsum(counts)])
    rows = np.concatenate([np.arange(offs[c], offs[c + 1]) for c in cl]) if len(cl) else np.zeros((0,), np.int64)
    return dict(claim_tokens=raw["claim_tokens"][cl], claim_len=raw["claim_len"][cl], evd_tokens=raw["evd_tokens"][rows],
                evd_len=raw["evd_len"][rows], evd_counts=counts[cl], doc_sources=raw["doc_sources"][cl],
                query_sources=raw["query_sources"][cl], labels=raw["labels"][cl])


class ReferenceApiBatch:
    """What the UNCHANGED fitter holds on the device before its de-padding loop (char_man_fitter_query_repr1.py:92-107,
    196-223): padded (B,n,R) node ids, dense float64 (B,n,R,R) evidence adjacency and (B,L,L) claim adjacency
    (handlers/mz_sampler.py:146-160), counts, sources.  inputs() runs the compatibility shim
    (batch.kargs_from_reference_tensors: one mask gather instead of the per-claim loop); the model then packs the dense
    adjacency on the device (PackedAdj.from_dense) and derives the node-compact plan from the ids (fused._plan_from_dense)."""

    def __init__(self, nb):
        from get_amd import ops
        b, n, r = nb.b, nb.n_max, nb.evd_tokens.shape[1]
        qa, q_ids, q_n = ops.graph_build(nb.claim_tokens, nb.claim_len, nb.window)
        da, d_ids, d_n = ops.graph_build(nb.evd_tokens, nb.evd_len, nb.window)
        dev = nb.device
        self.query = q_ids.long()
        self.query_lens = q_n.long()
        self.query_adj = qa.to_dense().double()
        self.doc_ids = torch.zeros((b * n, r), device=dev, dtype=torch.int64)
        self.doc_ids.index_copy_(0, nb._slot, d_ids.long())
        self.doc_ids = self.doc_ids.view(b, n, r)
        adj = torch.zeros((b * n, r, r), device=dev, dtype=torch.float64)
        adj.index_copy_(0, nb._slot, da.to_dense().double())
        self.docs_adj = adj.view(b, n, r, r)
        self.counts, self.doc_sources, self.query_sources, self.labels = nb.counts, nb.doc_sources, nb.query_sources, nb.labels
        self.b, self.b1, self.n_max = b, nb.b1, n
        self.bytes_handed_over = sum(t.numel() * t.element_size() for t in
                                     (self.query, self.query_adj, self.doc_ids, self.docs_adj, self.counts, self.doc_sources))

        self._pending = None

    def tensors(self):
        return (self.query_lens, self.doc_ids, self.docs_adj, self.query_adj, self.counts, self.doc_sources, self.query_sources)

    def start(self, stream):
        """Launch the de-padding on `stream` now (get_amd.batch.ReferenceDepad); inputs() then only waits for its counters."""
        from get_amd.batch import ReferenceDepad
        self._pending = ReferenceDepad(*self.tensors(), n_max=self.n_max, stream=stream)

    def inputs(self):
        from get_amd.batch import kargs_from_reference_tensors
        if self._pending is not None:
            dep, self._pending = self._pending, None
            return self.query, self.doc_ids, dep.kargs()
        kargs = kargs_from_reference_tensors(*self.tensors(), n_max=self.n_max)
        return self.query, self.doc_ids, kargs


class HostReferenceBatches:
    """The unchanged fitter's hand-over starting in HOST memory: per batch the numpy arrays its training loop
    slices (char_man_fitter_query_repr1.py:85-107): padded ids, the dense float64 (B,n,R,R) evidence adjacency (76.8 MB at the
    headline shape), the claim adjacency, counts, sources, labels.  Two schedules:
      inline   -- exactly the fitter's: `torch.from_numpy(a).cuda()` for every array at the start of the step (torch_utils.py:24-27:
                  pageable memory, synchronous copies on the compute stream), then the de-padding shim
                  (batch.kargs_from_reference_tensors) and its read-back;
      prefetch -- what INTEGRATION.md recommends for a fitter that keeps its dense tensors: the arrays live in PINNED memory, the copies
                  and gh_ref_depad of batch i + 1 run on a side stream while step i runs (batch.ReferenceDepad)."""

    FIELDS = ("query", "query_lens", "query_adj", "doc_ids", "docs_adj", "counts", "doc_sources", "query_sources", "labels")

    def __init__(self, ref_batches, device, prefetch):
        self.device, self.do_prefetch = torch.device(device), prefetch
        self.meta = [(rb.b, rb.b1, rb.n_max) for rb in ref_batches]
        self.host = []
        for rb in ref_batches:
            arrs = {}
            for f in self.FIELDS:
                t = getattr(rb, f).detach().cpu().contiguous()
                arrs[f] = t.pin_memory() if prefetch else torch.from_numpy(t.numpy().copy())      # pageable: a plain numpy array, as the sampler's
            self.host.append(arrs)
        self.bytes_per_step = sum(t.numel() * t.element_size() for t in self.host[0].values())
        self.i = 0
        self.side = torch.cuda.Stream(device=self.device) if prefetch else None
        self.ready = None
        if prefetch:
            self._start()

    class _Batch:
        def __init__(self, dev, meta, pending=None):
            self.__dict__.update(dev)
            self.b, self.b1, self.n_max = meta
            self._pending = pending

        def inputs(self):
            from get_amd.batch import kargs_from_reference_tensors
            if self._pending is not None:
                return self.query, self.doc_ids, self._pending.kargs()
            return self.query, self.doc_ids, kargs_from_reference_tensors(self.query_lens, self.doc_ids, self.docs_adj, self.query_adj, self.counts,
                                                                          self.doc_sources, self.query_sources, n_max=self.n_max)

    def _start(self):
        from get_amd.batch import ReferenceDepad
        j = self.i % len(self.host)
        self.i += 1
        with torch.cuda.stream(self.side):
            dev = {f: t.to(self.device, non_blocking=True) for f, t in self.host[j].items()}
            dep = ReferenceDepad(dev["query_lens"], dev["doc_ids"], dev["docs_adj"], dev["query_adj"], dev["counts"], dev["doc_sources"],
                                 dev["query_sources"], n_max=self.meta[j][2], stream=self.side)
        self.ready = (self._Batch(dev, self.meta[j], dep), self.side.record_event())

    def take(self):
        if not self.do_prefetch:      # the fitter's own loop: every array through .cuda() now, on the compute stream
            j = self.i % len(self.host)
            self.i += 1
            return self._Batch({f: t.cuda(self.device) for f, t in self.host[j].items()}, self.meta[j])
        b, ev = self.ready
        main = torch.cuda.current_stream(self.device)
        main.wait_event(ev)
        for f in self.FIELDS:
            getattr(b, f).record_stream(main)
        self.ready = None
        return b

    def prefetch(self):
        if self.do_prefetch:
            self._start()


class StreamedBatches:
    """A fresh NativeBatch per step from HOST arrays: H2D of the token ids / counts / sources (one packed pinned buffer),
    the device graph build that counts the nodes and the 4-byte m_real read-back (get_amd/batch.py), built ONE batch
    ahead on a side stream while the previous step's launches run (take() ... issue the step ... prefetch())."""

    def __init__(self, raws, cfg, device, compact):
        self.raws, self.cfg, self.device, self.compact = raws, cfg, torch.device(device), compact
        self.stream = torch.cuda.Stream(device=self.device)
        self.i = 0
        self.ready = None
        self._prepare()

    def _prepare(self):
        from get_amd.batch import NativeBatch
        raw = self.raws[self.i % len(self.raws)]
        self.i += 1
        # (no wait on the caller's stream: the next batch depends on nothing the step computes -- ordering the loader stream
        #  behind the step made the 4-byte read-back below wait for the WHOLE step, so the host could never run ahead)
        with torch.cuda.stream(self.stream):
            nb = NativeBatch(raw["claim_tokens"], raw["claim_len"], raw["evd_tokens"], raw["evd_len"], raw["evd_counts"],
                             raw["doc_sources"], raw["query_sources"], raw["labels"], window=self.cfg.window,
                             n_max=self.cfg.fixed_num_evidences, device=self.device, compact=self.compact, pinned=True)
        self.ready = (nb, self.stream.record_event())

    def take(self):
        """The batch prepared during the previous step (the current stream waits for its copies / graph build)."""
        nb, ev = self.ready
        main = torch.cuda.current_stream(self.device)
        main.wait_event(ev)
        for t in nb.device_tensors():          # allocated on the side stream, consumed on the caller's
            t.record_stream(main)
        self.ready = None
        return nb

    def prefetch(self):
        """Call AFTER the step's launches are issued: the host then blocks on the next batch's 4-byte read-back while the
        device is busy with the step."""
        self._prepare()


def box_reference(device):
    """Measured ceilings of THIS box, next to the datasheet peaks: a plain device copy (HBM read +
    write bytes per second) and the vendor BLAS fp32 GEMM rate at 8192^3 (torch.mm -> hipBLASLt/rocBLAS)."""
    x = torch.empty(256 << 20, device=device, dtype=torch.float32)      # 1 GiB
    y = torch.empty_like(x)
    a = torch.randn(8192, 8192, device=device)
    b = torch.randn(8192, 8192, device=device)
    c = torch.empty(8192, 8192, device=device)

    def timed(fn, reps):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e-3

    t_copy = timed(lambda: y.copy_(x), 10)
    t_mm = timed(lambda: torch.mm(a, b, out=c), 5)
    return {"copy_gbps": 2.0 * x.numel() * 4 / t_copy / 1e9, "blas_sgemm_8192_tflops": 2.0 * 8192 ** 3 / t_mm / 1e12}


def _oracle_train_step_fn(wl, claims, train):
    """One oracle step on the first `claims` claims of batch 0: forward (+dropout when `train`), CE, backward and --
    in training mode -- one Adam(lr 1e-4, weight_decay 1e-3) update, as declare_fitter.py:58-61."""
    from oracle import get_oracle as O
    s = wl["oracle_slice"](claims)
    inp, cfg = s["inp"], s["cfg"]
    T = torch.from_numpy
    state = {"p": {k: v.clone().requires_grad_(v.is_floating_point() and k != "embedding.weight") for k, v in s["params"].items()},
             "adam": {}}
    pairs = int(inp["evd_counts"].sum())

    def one():
        p = state["p"]
        for v in p.values():
            v.grad = None
        phi, _, _ = O.model_forward(p, cfg.__dict__, T(inp["query"]), T(inp["document"]), T(inp["query_adj"]),
                                    T(inp["doc_ids"]), T(inp["doc_adj"]), T(inp["query_lens"]), inp["evd_counts"],
                                    T(inp["doc_sources"]), T(inp["query_sources"]), drop_p=0.2 if train else 0.0)
        O.cross_entropy(phi, T(inp["labels"])).backward()
        if train:
            with torch.no_grad():
                new = O.adam_step({k: v.detach() for k, v in p.items()}, {k: v.grad for k, v in p.items()}, state["adam"])
            state["p"] = {k: v.clone().requires_grad_(p[k].requires_grad) for k, v in new.items()}

    return one, pairs


def cpu_baseline(wl, threads=None, budget_s=60.0):
    """SURVEY.md 8(d) / BASELINE.md 3: the CPU oracle (a port of the reference's PyTorch path) on the FULL batch, training
    mode (dropout on) + Adam, 2 warm-up + 5 timed steps.  Threads: `threads`, i.e. the pool size the probe found fastest
    -- handing torch all os.cpu_count() = 256 hardware threads of the GPU box makes this workload 100x SLOWER (141 s per
    step measured, against ~1.5 s at 16 threads), and the default bench run has to finish within minutes; both numbers
    are stated in the output.  If one step exceeds budget_s / 7 the step counts are cut (and reported)."""
    cores = os.cpu_count() or 1
    use = int(threads) if threads else cores
    torch.set_num_threads(use)
    one, pairs = _oracle_train_step_fn(wl, wl["cfg"].batch, train=True)
    t0 = time.time()
    one()
    t1 = time.time() - t0
    warm, timed = (2, 5) if 7 * t1 <= budget_s else (1, max(1, int(budget_s / max(t1, 1e-3)) - 1))
    for _ in range(warm - 1):
        one()
    t0 = time.time()
    for _ in range(timed):
        one()
    dt = time.time() - t0
    return {"value": pairs * timed / dt, "unit": "pairs/s", "cores": use, "host_cpu_count": cores, "kind": "port",
            "s_per_step": dt / timed,
            "sample": f"oracle fwd+bwd+Adam, training mode (dropout 0.2), the full batch of {wl['cfg'].batch} claims = {pairs} pairs, "
                      f"{warm} warm-up + {timed} timed steps in {dt:.1f} s, torch CPU with {use} intra-op threads (fastest pool "
                      f"size of the probe) on a host with os.cpu_count() = {cores}"}


def cpu_baseline_probe(wl, budget_s=8.0, claims=2):
    """Second figure: the same oracle on a 2-claim sample in evaluation mode at the best torch pool size of a 8..128 probe
    (torch's intra-op pool thrashes when handed every hardware thread of a 2-socket host for matrices this small)."""
    cores = os.cpu_count() or 1
    one, pairs = _oracle_train_step_fn(wl, claims, train=False)
    torch.set_num_threads(min(8, cores))
    one()
    best_threads, best_dt = None, None
    for th in [t for t in (8, 16, 32, 64, 128) if t <= cores] or [cores]:
        torch.set_num_threads(th)
        one()
        t0 = time.time()
        one()
        d = time.time() - t0
        if best_dt is None or d < best_dt:
            best_threads, best_dt = th, d
        if d > 4.0:
            break
    torch.set_num_threads(best_threads)
    t0 = time.time()
    n = 0
    while True:
        one()
        n += 1
        if time.time() - t0 >= budget_s or n >= 200:
            break
    dt = time.time() - t0
    return {"value": pairs * n / dt, "unit": "pairs/s", "cores": best_threads, "host_cpu_count": cores, "kind": "port",
            "sample": f"oracle fwd+bwd (evaluation mode, no optimiser) on the first {claims} claims = {pairs} pairs, {n} repeats "
                      f"in {dt:.1f} s, best torch pool size of a 8..128 probe"}


MIN_TIMED_SECONDS = 2.0        # the K-step block is repeated until the timed region is at least this long
MAX_TIMED_BLOCKS = 64
MIN_TIMED_BLOCKS = 5           # a median over fewer blocks is a mean in disguise
SETTLE_REL = 0.02              # untimed settle blocks until two consecutive ones agree within this ...
MAX_SETTLE_BLOCKS = 12         # ... or this many have run (the leg is then flagged `unsettled`)
UNSTABLE_SPREAD = 0.10         # blocks further than this from the median are outliers; a leg with more than one (or > 10 % of its blocks) is flagged, not trusted


def make_step(args, wl, trainer, source="resident"):
    """One training step over the next batch.  source: "resident" (rotating resident NativeBatches -- the headline),
    "reference" (ReferenceApiBatch: dense float64 hand-over, padded layout) or "streamed" (StreamedBatches: a fresh
    NativeBatch per step, H2D + read-back included).  Returns (step_fn, pairs_fn) -- pairs_fn() = pairs of the steps
    issued since its last call."""
    from get_amd import ops
    model = wl["model"]
    state = {"i": 0, "pairs": 0}
    batches = wl["ref_batches"] if source in ("reference", "reference_sync") else wl["batches"]
    streamed = wl.get("streamed") if source == "streamed" else wl.get("host_ref") if source == "reference_host" else None
    # "reference": the dense hand-over of batch i+1 is de-padded on a side stream while step i runs (batch.prefetch_reference's
    # schedule); "reference_sync": de-padding and its read-back at the start of every step (kargs_from_reference_tensors)
    ref_side = torch.cuda.Stream(device=batches[0].docs_adj.device) if source == "reference" else None
    if ref_side is not None:
        batches[0].start(ref_side)

    def step():
        if streamed is not None:
            b = streamed.take()
        else:
            b = batches[state["i"] % len(batches)]
        state["i"] += 1
        state["pairs"] += b.b1
        if args.forward_only:
            with torch.no_grad():
                query, document, kargs = b.inputs()
                phi = model(query, document, **kargs)
                state["phi"] = phi
                return phi.sum()
        trainer.zero_grad()
        query, document, kargs = b.inputs()
        phi = model(query, document, **kargs)
        state["phi"] = phi                             # (a reference, no device work: what --dump-outputs writes)
        loss = ops.cross_entropy(phi, b.labels)        # losses.py:29-32, loss + gradient in one launch
        if source in ("reference", "reference_sync", "reference_host"):
            loss.backward()                            # what the unchanged fitter calls
        else:
            ops.backward(loss)                         # = loss.backward() without autograd's root fill + scale launches
        trainer.step()
        if streamed is not None:
            streamed.prefetch()
        if ref_side is not None:
            batches[state["i"] % len(batches)].start(ref_side)
        return loss

    def pairs():
        p, state["pairs"] = state["pairs"], 0
        return p

    step.state = state
    return step, pairs


def measure(args, wl, trainer, world, device, dist, steps, warmup, profile=True, source="resident",
            min_seconds=MIN_TIMED_SECONDS):
    """W warm-up steps, then UNTIMED settle blocks of K steps until two consecutive blocks agree within SETTLE_REL (at most
    MAX_SETTLE_BLOCKS: a fresh model / batch source still pays allocator, workspace and pinned-buffer warm-up in its first
    blocks, and a cold block averaged into two or three warm ones is what made round 3's side legs print 91 K beside a
    6.17 ms step), then blocks of EXACTLY K timed steps, each bracketed by barrier + synchronize on both sides and reduced
    with MAX over the ranks.  The number of timed blocks comes from the LAST (warm) settle block, identically on every rank
    (its duration is already the MAX over ranks): enough for `min_seconds`, never fewer than MIN_TIMED_BLOCKS.
    Returns a dict: the per-block seconds, the pairs this rank processed per block, the settle blocks, the last loss, the
    dominant-kernel profile row and the step fn."""
    from get_amd import _lib
    step, pairs_fn = make_step(args, wl, trainer, source)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def rank_max(x):
        if world == 1:
            return x
        t = torch.tensor([x], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def block(hook=None):
        barrier()
        t0 = time.perf_counter()
        out = None
        for i in range(steps):
            if hook is not None:
                hook(i)
            out = step()
        barrier()
        return rank_max(time.perf_counter() - t0), out

    for _ in range(warmup):
        step()
    settle = []
    while len(settle) < MAX_SETTLE_BLOCKS:
        dt, _ = block()
        settle.append(dt)
        if len(settle) >= 2 and abs(settle[-1] - settle[-2]) <= SETTLE_REL * min(settle[-1], settle[-2]):
            break
    pairs_fn()
    unsettled = not (len(settle) >= 2 and abs(settle[-1] - settle[-2]) <= SETTLE_REL * min(settle[-1], settle[-2]))
    warm_dt = min(settle[-2:]) if len(settle) >= 2 else settle[-1]
    n_blocks = int(min(MAX_TIMED_BLOCKS, max(MIN_TIMED_BLOCKS, np.ceil(min_seconds / max(warm_dt, 1e-6)))))
    prof_dom = None
    # live roofline of the dominant kernel: HIP events around each of its launches in the FIRST `prof_steps` timed steps
    # of the first block (an event pair between two kernels costs ~10 us of dispatch overlap: 0.4 % of those steps)
    prof_steps = min(steps, max(1, PROFILE_TIMED_STEPS)) if profile else 0
    if profile:
        _lib.profile_enable(True, only=[DOMINANT])
        _lib.profile_collect()
    blocks, block_pairs = [], []
    loss = None
    for b in range(n_blocks):
        hook = None
        if profile and b == 0:
            hook = lambda i: _lib.profile_enable(False) if i == prof_steps else None      # host-side switch, no device work
        dt, loss = block(hook)
        blocks.append(dt)
        block_pairs.append(pairs_fn())
        if b == 0 and profile:
            prof_dom = _lib.profile_collect()[DOMINANT]
            prof_dom["steps"] = prof_steps
            _lib.profile_enable(False)
    return {"blocks_s": blocks, "block_pairs": block_pairs, "settle_s": settle, "unsettled": unsettled, "loss": loss,
            "prof_dom": prof_dom, "step": step}


def time_steps(args, wl, trainer, world, device, dist, steps, warmup):
    """The headline protocol: `warmup` steps, then ONE block of exactly `steps` timed steps, bracketed by barrier +
    synchronize on both sides and reduced with MAX over the ranks.  Returns the seconds of the block, the pairs this rank
    processed in it, the last loss and the step fn (step.state["phi"]: the logits of the last step)."""
    step, pairs_fn = make_step(args, wl, trainer)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(warmup):
        step()
    barrier()
    pairs_fn()
    loss = None
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    return {"seconds": dt, "pairs": pairs_fn(), "loss": loss, "step": step}


DUMP_MAX_ELEMENTS = 2 << 20       # per array: larger outputs are written as a fixed, seeded sample of this many elements


def dump_outputs(path, step, trainer, loss, forward_only):
    """--dump-outputs: what the timed path handed its caller in the LAST timed step, as float32 / float64 .npy files --
    logits.npy (the model's output), and for a training step loss.npy, params.npy (the parameters after the Adam update:
    the trainer's flat fp32 buffer) and grads.npy (the flat gradient the update consumed).  An array above
    DUMP_MAX_ELEMENTS is replaced by a seeded sample of that many elements (NAME.npy) and its flat indices
    (NAME_index.npy); with the same arguments the inputs, and so the sample, are the same in every run."""
    os.makedirs(path, exist_ok=True)
    torch.cuda.synchronize()
    arrays = {"logits": step.state["phi"]}
    if not forward_only:
        arrays.update(loss=loss, params=trainer.flat_p, grads=trainer.flat_g)
    written = {}
    for name, t in arrays.items():
        if t is None:
            continue
        a = t.detach().float().reshape(-1).cpu().numpy()
        shape = tuple(t.shape)
        if a.size > DUMP_MAX_ELEMENTS:
            idx = np.sort(np.random.default_rng(SEED).choice(a.size, DUMP_MAX_ELEMENTS, replace=False))
            np.save(os.path.join(path, f"{name}_index.npy"), idx.astype(np.float64))
            a = a[idx]
        else:
            a = a.reshape(shape)
        np.save(os.path.join(path, f"{name}.npy"), a)
        written[name] = list(a.shape)
    return written


def phase_split(wl, trainer, steps=5):
    """fwd / bwd / all-reduce / optimiser milliseconds per step: HIP events on the compute stream between the phases of
    `steps` extra, untimed steps (the events serialise the overlapped early all-reduce, so this is a breakdown, not the
    step time)."""
    from get_amd import ops
    model, batches = wl["model"], wl["batches"]
    ev = lambda: torch.cuda.Event(enable_timing=True)
    acc = np.zeros(5)
    for i in range(steps):
        b = batches[i % len(batches)]
        e = [ev() for _ in range(6)]
        trainer.zero_grad()
        e[0].record()
        query, document, kargs = b.inputs()
        e[1].record()
        loss = ops.cross_entropy(model(query, document, **kargs), b.labels)
        e[2].record()
        ops.backward(loss)
        e[3].record()
        trainer.allreduce()
        e[4].record()
        trainer.t += 1
        ops.adam_step_flat(trainer.flat_p, trainer.flat_g, trainer.flat_m, trainer.flat_v, trainer.t, lr=trainer.lr,
                           betas=trainer.betas, eps=trainer.eps, weight_decay=trainer.weight_decay,
                           grad_scale=1.0 / trainer.world)
        ops.refresh_transposes(trainer._matrices)
        e[5].record()
        torch.cuda.synchronize()
        acc += np.array([e[j].elapsed_time(e[j + 1]) for j in range(5)])
    acc /= steps
    return {"graph_build_ms": acc[0], "forward_ms": acc[1], "backward_ms": acc[2], "allreduce_ms": acc[3],
            "optimizer_ms": acc[4], "note": f"HIP events between the phases of {steps} extra untimed steps"}


def parity_check(wl, k=4):
    """Evaluation-mode logits and GSL keep-sets of the first k claims of batch 0 against the CPU oracle."""
    model = wl["model"]
    was = model.training
    model.train(False)
    try:
        with torch.no_grad():
            q, d_, k_ = wl["batches"][0].inputs()
            phi_gpu = model(q, d_, **k_)[:k].cpu()
            keep_words = model.ggnn_with_gsl.last_keep.cpu().numpy().astype(np.uint64)      # (B1, W) bit words
        par = wl["oracle_slice"](k, return_aux=True)
        n_pairs = par["keep"].shape[0]
        r = par["keep"].shape[1]
        bits = ((keep_words[:n_pairs, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool)
        keep_gpu = bits.reshape(n_pairs, -1)[:, :r]
        real = par["inp"]["doc_ids"][:n_pairs] > 0
        mism = int(((keep_gpu != par["keep"].numpy()) & real).any(axis=1).sum())
        return {"max_abs_logit_diff_vs_cpu_oracle": float((phi_gpu - par["phi"]).abs().max()), "claims_checked": k,
                "graphs_checked": n_pairs, "graphs_with_real_node_keep_set_mismatch": mism}
    finally:
        model.train(was)


DOMINANT = "gemm_big"
SEED = 20240229                   # data / model seed of every workload (rank r adds r to the data seed)
# Largest |logit - CPU oracle| the bf16 storage pipeline may show on the configs[4] bench batch (asserted at full size, evaluation and
# training mode, by tests/test_gpu_fullsize_grads.py::test_config4_bf16_storage_at_the_bench_batch_vs_oracle; measured 1.6e-3 - 1.8e-3).
# The configs[4] bf16 leg reports itself as FAILED when its own oracle slice exceeds it.
BF16_BENCH_LOGIT_BOUND = 5e-3
STRONG_GLOBAL_BATCH = 256         # BASELINE configs[3]

# The BASELINE configs the headline invocation does not run as its main workload, printed beside it (`other_configs`) so that
# the `python bench.py --gpus 1 --full` line carries a timing of each: (name, SynthConfig overrides, gemm mode, steps per block)
OTHER_CONFIGS = [
    ("configs[2] PolitiFact-shaped: B=64 x 10 evidences, L_right=200, fp32",
     dict(batch=64, n_evd=10, len_right=200), "fp32", 10),
    ("configs[4] h=768, 8 word heads, gnn_window=5, gsl_rate=0.8, B=32 x 30, fp32",
     dict(batch=32, n_evd=30, hidden=768, emb_dim=768, word_heads=8, window=5, gsl_rate=0.8), "fp32", 4),
    ("configs[4] h=768, 8 word heads, gnn_window=5, gsl_rate=0.8, B=32 x 30, bf16 storage in the cells",
     dict(batch=32, n_evd=30, hidden=768, emb_dim=768, word_heads=8, window=5, gsl_rate=0.8), "bf16", 10),
]


def other_config_seed(i: int) -> int:
    """Seed of OTHER_CONFIGS[i]'s workload (tests/test_gpu_fullsize_grads.py rebuilds the configs[4] bf16 batch from it)."""
    return SEED + 7 * (i + 1)


def other_config_leg(args, name, overrides, mode, steps, device, dist, seed):
    """One BASELINE config as a side leg of the headline run: its own model, trainer and resident batches, the same step and
    the same measure() protocol (settle blocks, >= MIN_TIMED_BLOCKS timed blocks, median), the live roofline of the dominant
    kernel (HIP events around its launches in the first timed steps) and an evaluation-mode logit slice against the CPU oracle."""
    from get_amd import _lib, ops
    from get_amd.dist import FlatTrainer
    cfg = SynthConfig(**overrides)
    _lib.set_gemm_mode(mode)
    ops.bump_weight_epoch()
    try:
        wl = build_workload(seed=seed, device=device, cfg=cfg, n_batches=2)
        # parity of the leg on the INITIAL weights -- the state tests/test_gpu_fullsize_grads.py asserts its bounds on (the slice
        # after the timed training steps is reported beside it: bf16 noise moves GSL keep decisions of tie-range nodes, which
        # moves logits in discrete steps, so that number has no asserted bound)
        parity0 = parity_check(wl, k=2) if mode == "bf16" else None
        wl["model"].train(True)
        tr = FlatTrainer(wl["model"], lr=1e-4, weight_decay=1e-3)
        ops.bump_weight_epoch()
        m = measure(args, wl, tr, 1, device, dist, steps, 3, profile=True, min_seconds=1.0)
        s = summarize_blocks(m, steps, m["block_pairs"])
        leg = {"workload": name, "gemm_mode": mode, **leg_summary(s), "pairs_per_step": wl["b1"],
               "layout_rows": wl["m_real"], "mode": "train (dropout on)"}
        pd = m["prof_dom"]
        if pd and pd["launches"] > 0 and pd["ms"] > 0:
            peak = PEAK_BF16_MFMA_TFLOPS if mode == "bf16" else PEAK_F32_MFMA_TFLOPS
            rate = pd["work"] / (pd["ms"] * 1e-3) / 1e12
            leg["roofline"] = {"kernel": DOMINANT, "bound": "mfma", "achieved": rate, "peak": peak, "unit": "TFLOP/s",
                               "frac": rate / peak, "traffic": None, "avg_launch_ms": pd["ms"] / pd["launches"],
                               "launches_per_step": pd["launches"] / pd["steps"],
                               "measured": f"HIP events around every {DOMINANT} launch of the first {pd['steps']} timed steps"}
        leg["parity"] = parity_check(wl, k=2)
        if mode == "bf16":
            leg["parity"] = dict(parity0, after_the_timed_training_steps=leg["parity"])
            # bf16 storage inside the cells is not the 1e-4 fp32 contract: its asserted bound at THIS batch is BF16_BENCH_LOGIT_BOUND
            # (tests/test_gpu_fullsize_grads.py checks logits, weights, scores, keep-sets and every gradient of the full batch)
            d = leg["parity"]["max_abs_logit_diff_vs_cpu_oracle"]
            leg["parity"]["bound"] = BF16_BENCH_LOGIT_BOUND
            leg["parity"]["within_bound"] = bool(d <= BF16_BENCH_LOGIT_BOUND)
            leg["parity"]["bound_asserted_by"] = "tests/test_gpu_fullsize_grads.py::test_config4_bf16_storage_at_the_bench_batch_vs_oracle"
            if not leg["parity"]["within_bound"]:
                leg["failed"] = f"logits differ from the CPU oracle by {d:.2e} > {BF16_BENCH_LOGIT_BOUND:.0e}: the timing of this leg is not a valid number"
                leg["value"] = None
        fl = flops_per_pair(cfg, wl["nnz_per_graph"], wl["m_real"] / max(wl["b1"], 1) if wl["compact"] else None)
        fl_run = fl.get("executed", fl["fwd_bwd"])
        leg["path_tflops"] = fl_run * s["value"] / 1e12
        del wl, tr, m
        return leg
    finally:
        ops.bump_weight_epoch()
        _lib.set_gemm_mode("fp32")
        torch.cuda.empty_cache()
PROFILE_TIMED_STEPS = 5           # timed steps whose dominant-kernel launches carry HIP events


def _free_port():
    import socket
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    return port


def spawn_ranks(n_gpus: int) -> int:
    """`python bench.py --gpus N` with RANK unset: run this very command line under torch.distributed.run, one rank per
    GPU of this node (RCCL needs one device per rank: fewer visible GPUs than ranks is an error, not a silent 1-rank run)."""
    import subprocess
    have = torch.cuda.device_count()
    # (GET_AMD_BENCH_BACKEND=gloo: rehearsal of the launch / barrier / reduction path with ranks sharing devices)
    if have < n_gpus and os.environ.get("GET_AMD_BENCH_BACKEND", "nccl") == "nccl":
        sys.stderr.write(f"bench.py: --gpus {n_gpus} needs {n_gpus} visible GPUs, this node shows {have}; RCCL runs one rank per "
                         f"device, so the {n_gpus}-rank measurement cannot be taken here (no line printed).\n")
        return 3
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def summarize_blocks(m, steps, world_pairs_per_block):
    """value = median over the blocks of (pairs / seconds); ms_per_step = median block seconds / steps; spread over the
    blocks; `unstable` when the blocks spread more than UNSTABLE_SPREAD (such a leg is a warm-up artefact, not a rate)."""
    secs = np.asarray(m["blocks_s"], dtype=np.float64)
    rates = np.asarray(world_pairs_per_block, dtype=np.float64) / secs
    med = float(np.median(rates))
    spread = float((rates.max() - rates.min()) / med) if med > 0 else None
    timed = {"blocks": int(len(secs)), "steps_per_block": int(steps), "seconds_total": float(secs.sum()),
             "pairs_per_s_min": float(rates.min()), "pairs_per_s_median": med, "pairs_per_s_max": float(rates.max()),
             "spread_rel": spread, "settle_blocks_untimed": int(len(m.get("settle_s", []))),
             "settle_block_ms_per_step": [round(1e3 * float(x) / steps, 4) for x in m.get("settle_s", [])],
             "note": f"after the warm-up steps, untimed {steps}-step settle blocks run until two consecutive ones agree within "
                     f"{SETTLE_REL:.0%} (<= {MAX_SETTLE_BLOCKS}); then the {steps}-step block (barrier + synchronize on both sides, "
                     f"MAX over ranks) is timed >= {MIN_TIMED_BLOCKS} times and until >= {MIN_TIMED_SECONDS:g} s; value = median block"}
    # one hiccup block (a host-side stall: 1 of 8 blocks at 2/3 of the rate on one box) must neither move the median nor condemn the
    # leg; several deviating blocks do.  Both spreads are printed.
    if med > 0:
        dev = np.abs(rates - med) / med
        out_n = int((dev > UNSTABLE_SPREAD).sum())
        timed["outlier_blocks"] = out_n
        if out_n:
            inl = rates[dev <= UNSTABLE_SPREAD]
            timed["spread_rel_without_outliers"] = float((inl.max() - inl.min()) / med) if len(inl) else None
        # `unstable` as in round 4 -- ANY spread beyond UNSTABLE_SPREAD -- and beside it `unstable_without_outliers` (several deviating
        # blocks, or a single one among fewer than 8): the first says "look at the blocks", the second "do not trust the median"
        if spread is not None and spread > UNSTABLE_SPREAD:
            timed["unstable"] = True
        if out_n > max(1, len(rates) // 10) or (out_n >= 1 and len(rates) < 8):
            timed["unstable_without_outliers"] = True
    if m.get("unsettled"):
        timed["unsettled"] = True      # the settle loop hit MAX_SETTLE_BLOCKS without two agreeing blocks: warm-up may have leaked in
    return {"value": med, "ms_per_step": 1e3 * float(np.median(secs)) / steps, "timed": timed}


def leg_summary(s):
    """The fields every side leg prints: rate, step time, and the block statistics behind them."""
    t = s["timed"]
    out = {"pairs_per_s": s["value"], "ms_per_step": s["ms_per_step"],
           "timed": {k: t[k] for k in ("blocks", "steps_per_block", "seconds_total", "pairs_per_s_min", "pairs_per_s_median",
                                       "pairs_per_s_max", "spread_rel", "settle_blocks_untimed", "settle_block_ms_per_step",
                                       "outlier_blocks", "spread_rel_without_outliers") if k in t}}
    if t.get("unstable"):
        out["unstable"] = True
    if t.get("unstable_without_outliers"):
        out["unstable_without_outliers"] = True
    if t.get("unsettled"):
        out["unsettled"] = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32, help="claims per GPU (weak scaling: fixed per-GPU work)")
    ap.add_argument("--global-batch", type=int, default=0,
                    help="fixed GLOBAL claim count, split evenly over the ranks (SURVEY 8(e): 256 -> 256/N per GPU; strong "
                         "scaling); ragged evidence counts are balanced by sort-then-stripe (dist.shard_claims)")
    ap.add_argument("--n-evd", type=int, default=30, help="evidences per claim (<=0: ragged U[1,30])")
    ap.add_argument("--evd-dist", choices=["fixed", "snopes"], default="fixed",
                    help="snopes: evidence counts from the empirical Snopes histogram (mean 6.9, the realistic series)")
    ap.add_argument("--len-right", type=int, default=100, help="evidence length R (configs[2]: 200)")
    ap.add_argument("--hidden", type=int, default=300, help="hidden size H (configs[4]: 768)")
    ap.add_argument("--word-heads", type=int, default=5)
    ap.add_argument("--window", type=int, default=3, help="gnn_window")
    ap.add_argument("--gsl-rate", type=float, default=0.6)
    ap.add_argument("--batches", type=int, default=4, help="distinct resident batches the step loop rotates through")
    ap.add_argument("--gemm-mode", choices=["fp32", "bf16", "fp32x3", "fp32x3p"], default="fp32",
                    help="bf16: opt-in bf16 MFMA path (configs[4]); fp32x3 / fp32x3p: opt-in fp32-accurate products from 3-way "
                         "bf16 splits on the bf16 MFMA (p: weight pieces pre-split once per update); the headline metric is fp32")
    ap.add_argument("--eval-mode", action="store_true", help="disable dropout (parity mode)")
    ap.add_argument("--forward-only", action="store_true",
                    help="auxiliary serving measurement: evaluation-mode forward only (not the headline metric)")
    ap.add_argument("--padded", action="store_true",
                    help="run every layer on all R padded node rows (the reference's layout) instead of the node-compact one")
    ap.add_argument("--reference-api", action="store_true",
                    help="ALSO time the path an unchanged fitter drives: dense float64 (B,n,R,R) adjacency handed over per step "
                         "through batch.kargs_from_reference_tensors, packed on the device (printed beside the headline)")
    ap.add_argument("--streamed", action="store_true",
                    help="ALSO time a fresh NativeBatch per step (H2D of the ids + m_real read-back, one batch ahead on a side stream)")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement beside the headline (off by default): the repeated-block statistics with the "
                         "live roofline, the per-kernel table, the phase split, the strong-scaling leg, the side regimes, the "
                         "realistic series, the other BASELINE configs, the parity slice, the CPU baseline and the box ceilings")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last timed step computed (logits, loss, updated parameters, "
                         "gradients) as DIR/<name>.npy")
    ap.add_argument("--no-side-modes", action="store_true", help="skip the --reference-api / --streamed legs the --full headline run adds by default")
    ap.add_argument("--collective", choices=["torch", "library"], default="torch",
                    help="who carries the gradient all-reduce: torch.distributed (default; backend nccl = RCCL) or the library's own "
                         "RCCL communicator (gh_comm_init / gh_flat_allreduce, include/get_hip.h); with --gpus 1 the library route "
                         "runs a world-size-1 communicator so that the collective is issued and timed on the device")
    ap.add_argument("--no-strong", dest="strong_too", action="store_false",
                    help="skip the strong-scaling leg (configs[3]: global batch 256 split over the ranks) a --full run prints beside the weak line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the CPU baseline of a --full run")
    ap.add_argument("--no-profile", action="store_true", help="skip the per-kernel HIP-event timing of a --full run")
    ap.add_argument("--no-series", action="store_true", help="skip the realistic evidence-count series of a --full run")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip the legs of BASELINE configs[2] / configs[4] fp32 / configs[4] bf16 the --full headline run prints beside its line")
    ap.add_argument("--cpu-threads", type=int, default=0, help="torch threads of the CPU baseline (default: the probe's fastest pool size)")
    ap.add_argument("--measure-build", action="store_true",
                    help="kernel A/B tooling only: load lib/libget_hip_measure.so (make -C get_amd/csrc measure), honour the GH_* "
                         "switches, and stamp the line as NOT a product measurement")
    ap.add_argument("--measure-lib", default="", help="kernel A/B tooling only: like --measure-build, but loads the variant build "
                                                      "get_amd/lib/libget_hip_NAME.so (make -C get_amd/csrc variant NAME=... EXTRA=...)")
    args = ap.parse_args()
    if args.measure_lib:
        args.measure_build = True

    # measurement switches of the library (GH_*) change what the kernels compute or how they are scheduled: a bench line
    # taken with one set is not a measurement of the product.  (The shipped .so ignores them -- they only exist in the
    # -DGH_MEASURE tool build -- but a GET_AMD_LIB override could point at such a build.)
    leaked = sorted(k for k in os.environ if k.startswith("GH_"))
    if args.measure_build:
        os.environ["GET_AMD_LIB"] = os.path.join(ROOT, "get_amd", "lib", f"libget_hip_{args.measure_lib or 'measure'}.so")
        from get_amd import _lib as _l
        _l.LIB_PATH = os.environ["GET_AMD_LIB"]
    elif leaked or os.environ.get("GET_AMD_LIB"):
        sys.stderr.write(f"bench.py: refusing to run with measurement switches in the environment: {leaked + (['GET_AMD_LIB'] if os.environ.get('GET_AMD_LIB') else [])}\n")
        sys.exit(4)

    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))

    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.stderr.write(f"bench.py: launched with WORLD_SIZE={world} but --gpus {args.gpus}; refusing to print a line whose "
                         "n_gpus is not the number of ranks that ran\n")
        sys.exit(5)
    backend = "none"
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # GET_AMD_BENCH_BACKEND=gloo: rehearsal of the N>1 code path on a box with fewer GPUs than ranks (ranks share
        # devices, the all-reduce goes through the host).  The real run is one rank per GPU over RCCL ("nccl").
        backend = os.environ.get("GET_AMD_BENCH_BACKEND", "nccl")
        if backend == "nccl" and torch.cuda.device_count() < world:
            sys.stderr.write(f"bench.py: {world} RCCL ranks need {world} GPUs, {torch.cuda.device_count()} visible\n")
            sys.exit(3)
        local_rank = local_rank % torch.cuda.device_count() if backend != "nccl" else local_rank
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(f"cuda:{local_rank}"))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    else:
        torch.cuda.set_device(0)
    device = f"cuda:{local_rank if world > 1 else 0}"

    from get_amd import _lib
    from get_amd.dist import FlatTrainer, shard_claims
    _lib.load()
    _lib.set_gemm_mode(args.gemm_mode)

    per_rank = args.batch
    shard = None
    if args.global_batch > 0:
        # strong scaling: ONE global batch (same seed on every rank), claims dealt by sort-then-stripe on their evidence counts
        per_rank = args.global_batch // world
        shard = (lambda counts: shard_claims(args.global_batch, rank, world, counts))
    cfg_in = SynthConfig(batch=args.global_batch if shard else per_rank, n_evd=args.n_evd, len_right=args.len_right,
                         hidden=args.hidden, emb_dim=args.hidden, word_heads=args.word_heads, window=args.window,
                         gsl_rate=args.gsl_rate)
    # replicas are identical by construction (model_seed is rank-independent); the data seed differs per rank (weak scaling)
    wl = build_workload(seed=SEED + (0 if shard else rank), device=device, cfg=cfg_in, compact=False if args.padded else None,
                        n_batches=args.batches, evd_dist=args.evd_dist, model_seed=SEED, claim_shard=shard)
    model, cfg = wl["model"], wl["cfg"]
    lib_comm = None
    if args.collective == "library":
        if world > 1 and torch.cuda.device_count() < world:
            sys.stderr.write(f"bench.py: --collective library builds an RCCL communicator with one device per rank; {world} ranks "
                             f"on {torch.cuda.device_count()} visible GPU(s) cannot (RCCL rejects duplicate devices)\n")
            sys.exit(3)
        from get_amd.dist import LibComm
        lib_comm = LibComm.from_process_group(device=device) if world > 1 else LibComm.single(device)
        backend = f"library-owned RCCL communicator ({lib_comm.library}); rendezvous over torch.distributed {backend}" if world > 1 \
            else f"library-owned RCCL communicator ({lib_comm.library}), world size 1"
    trainer = FlatTrainer(model, lr=1e-4, weight_decay=1e-3, comm=lib_comm, always_reduce=lib_comm is not None)
    from get_amd import ops
    ops.bump_weight_epoch()            # parameters were (re)written through .data: drop cached transposes
    if lib_comm is not None and world == 1:
        trainer.broadcast_parameters(0)
        trainer.attach_overlap()
    if world > 1:
        trainer.broadcast_parameters(0)      # two collectives (flat bucket + everything outside it), not one per tensor
        trainer.attach_overlap()             # 76 % of the gradient all-reduce runs underneath the first cell's backward
    model.train(not (args.eval_mode or args.forward_only))

    h = time_steps(args, wl, trainer, world, device, dist, args.steps, args.warmup)
    loss, step = h["loss"], h["step"]
    comm_bytes_step = trainer.comm_bytes / max(1, args.warmup + args.steps)
    comm_calls_step = trainer.comm_calls / max(1, args.warmup + args.steps)
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, step, trainer, loss, args.forward_only)
    # --full: the round-1..6 protocol of the headline as a leg of its own (untimed settle blocks, >= MIN_TIMED_BLOCKS timed
    # blocks of K steps, median) with the live roofline of the dominant kernel in its first timed steps
    m, prof_dom, prof = None, None, None
    if args.full:
        m = measure(args, wl, trainer, world, device, dist, args.steps, 0, profile=not args.no_profile)
        prof_dom = m["prof_dom"]
    PROFILE_EXTRA_STEPS = 5
    if args.full and not args.no_profile:
        _lib.profile_enable(True)                       # every instrumented kernel, outside the timed region
        _lib.profile_collect()
        for _ in range(PROFILE_EXTRA_STEPS):
            step()
        torch.cuda.synchronize()
        prof = _lib.profile_collect()
        _lib.profile_enable(False)
    split = None if (args.forward_only or not args.full) else phase_split(wl, trainer)      # collective inside: every rank runs it
    # whole-job pairs per block: sum over the ranks (the per-block seconds are already MAX over ranks)
    bp = torch.tensor([float(h["pairs"])] + (m["block_pairs"] if m else []) + [float(cfg.batch * args.steps)], device=device,
                      dtype=torch.float64)
    if world > 1:
        dist.all_reduce(bp, op=dist.ReduceOp.SUM)
    world_pairs = float(bp[0].item())
    world_pairs_blocks = [float(x) for x in bp[1:-1].tolist()]
    total_claims_block = float(bp[-1].item())

    # configs[3] in the same launch: ONE global batch of STRONG_GLOBAL_BATCH claims dealt over the ranks by sort-then-stripe
    # (256 / N claims per GPU), its own model replica and trainer, same step.  Every rank takes part (the
    # gradient all-reduce and the block barriers are collectives); the weak-scaling figure above stays `value`.
    strong = None
    # (configs[3] is defined on the Snopes shape: only the headline shape carries the leg -- at h = 768 a 256-claim batch on one
    #  GPU is 2.4 GB per activation, past what the fast kernels' buffer descriptors address)
    strong_shape = (args.len_right, args.hidden, args.word_heads, args.window, args.n_evd) == (100, 300, 5, 3, 30)
    if (args.full and args.strong_too and not args.no_side_modes and args.global_batch <= 0 and not args.forward_only and args.gemm_mode == "fp32" and
            STRONG_GLOBAL_BATCH % world == 0 and strong_shape):
        gshard = (lambda counts: shard_claims(STRONG_GLOBAL_BATCH, rank, world, counts))
        cfg_s = SynthConfig(**{**cfg_in.__dict__, "batch": STRONG_GLOBAL_BATCH})
        wls = build_workload(seed=SEED, device=device, cfg=cfg_s, compact=False if args.padded else None, n_batches=2,
                             evd_dist=args.evd_dist, model_seed=SEED, claim_shard=gshard)
        tr_s = FlatTrainer(wls["model"], lr=1e-4, weight_decay=1e-3, comm=lib_comm, always_reduce=lib_comm is not None)
        ops.bump_weight_epoch()
        if world > 1:
            tr_s.broadcast_parameters(0)
            tr_s.attach_overlap()
        wls["model"].train(not args.eval_mode)
        k_s = max(2, args.steps // (4 if world == 1 else 2))
        m_s = measure(args, wls, tr_s, world, device, dist, k_s, 2, profile=False, min_seconds=1.0)
        bps = torch.tensor(m_s["block_pairs"], device=device, dtype=torch.float64)
        if world > 1:
            dist.all_reduce(bps, op=dist.ReduceOp.SUM)
        s_s = summarize_blocks(m_s, k_s, [float(x) for x in bps.tolist()])
        strong = {**leg_summary(s_s), "scaling": "strong", "global_batch_claims": STRONG_GLOBAL_BATCH, "n_gpus": world,
                  "claims_per_gpu": wls["cfg"].batch, "pairs_this_rank": wls["b1"],
                  "sharding": "sort-then-stripe by evidence count (dist.shard_claims)",
                  "what": f"BASELINE configs[3]: the SAME global batch of {STRONG_GLOBAL_BATCH} claims at every N, "
                          f"{STRONG_GLOBAL_BATCH}/N claims per GPU, gradients averaged over the ranks (pairs_per_s is whole-job)"}
        del wls, tr_s, m_s
        ops.bump_weight_epoch()
        torch.cuda.empty_cache()

    headline_run = (args.len_right, args.hidden, args.word_heads, args.window, args.gsl_rate, args.n_evd, args.evd_dist) == \
                   (100, 300, 5, 3, 0.6, 30, "fixed") and per_rank == 32 and args.gemm_mode == "fp32" and not args.padded \
                   and not args.eval_mode and not args.forward_only
    if rank == 0:
        value, ms_per_step = world_pairs / h["seconds"], 1e3 * h["seconds"] / args.steps
        timed = {"blocks": 1, "steps": args.steps, "warmup_steps": args.warmup, "seconds_total": h["seconds"],
                 "note": f"{args.warmup} warm-up steps, then ONE block of exactly {args.steps} timed steps (barrier + synchronize "
                         "on both sides, MAX over ranks); value = whole-job pairs of the block / its seconds"}
        headline = headline_run
        real_nodes = wl["m_real"] / max(wl["b1"], 1)
        fl = flops_per_pair(cfg, wl["nnz_per_graph"], real_nodes if wl["compact"] else None)
        fl_run = fl.get("executed", fl["fwd_bwd"])
        evd_txt = "Snopes-histogram (mean 6.9)" if args.evd_dist == "snopes" else (str(args.n_evd) if args.n_evd > 0 else "U[1,30]")
        out = {
            "metric": (f"claim-evidence pairs/sec fwd+bwd (B={cfg.batch}, h={cfg.hidden})" if not args.forward_only
                       else "claim-evidence pairs/sec forward only, evaluation mode (auxiliary)"),
            "value": value, "unit": "pairs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
            "higher_is_better": True, "scaling": "strong" if args.global_batch > 0 else "weak", "vs_baseline": None,
            "dtype": {"fp32": "f32", "bf16": "bf16 operands / f32 accumulate in the big GEMMs, f32 elsewhere"}.get(
                args.gemm_mode, "f32 storage and results; big NT GEMM products from 3-way bf16 splits on the bf16 MFMA (opt-in)"),
            "data": "synthetic",
            "claims_per_s": total_claims_block * value / max(world_pairs, 1.0),
            "timed": timed,
            "rccl_ranks": (lib_comm.info()[1] if lib_comm is not None else (dist.get_world_size() if world > 1 else 1)),
            "collective": {"backend": backend, "allreduce_bytes_per_step_per_rank": comm_bytes_step,
                           "allreduce_ms_per_step": (split or {}).get("allreduce_ms"),
                           "calls_per_step": comm_calls_step,
                           "note": "one flat fp32 gradient bucket; the early-final range (head, attentions, second cell) is "
                                   "reduced asynchronously underneath the first cell's backward, the rest after backward"},
            "config": {"workload": ("BASELINE configs[1]: Snopes-shaped synthetic batch, " if headline
                                    else "non-headline shape (see flags): synthetic batch, ") +
                                   f"B={cfg.batch} claims x {evd_txt} evidences per GPU "
                                   f"(B1={wl['b1']:.0f} pairs), L_left={cfg.len_left}, L_right={cfg.len_right}, D=H={cfg.hidden}, "
                                   f"{cfg.word_heads} word heads / {cfg.evd_heads} evidence heads, gnn_window={cfg.window}, "
                                   f"gsl_rate={cfg.gsl_rate}",
                       "step": "device graph build + forward + CE loss + backward + flat grad all-reduce + fused Adam "
                               "(backward = get_amd.ops.backward(loss): loss.backward() with a cached constant 1 as the root gradient, so "
                               "autograd's ones_like fill and the multiply by it -- two scalar launches -- do not run; gradients bit-identical; "
                               "the reference_api legs call loss.backward() like the unchanged fitter)",
                       "batches": f"{len(wl['batches'])} distinct resident batches, rotated every step",
                       "mode": "eval (dropout off)" if args.eval_mode else "train (dropout on)",
                       "layout": (f"node-compact: {wl['m_real']:.0f} real-node rows of {wl['b1'] * cfg.len_right:.0f} padded rows "
                                  f"({real_nodes:.1f} unique tokens per {cfg.len_right}-token evidence); padding nodes only "
                                  "in the first cell's forward and the scorer") if wl["compact"]
                                 else "padded: every layer on all R node rows (reference layout)",
                       "parallelism": f"dp{world}", "pairs_per_gpu": wl["b1"],
                       "global_batch_claims": cfg.batch * world if args.global_batch <= 0 else args.global_batch,
                       "sharding": ("sort-then-stripe by evidence count (dist.shard_claims)" if shard else
                                    "one independent batch per rank (weak scaling)"),
                       "loss": float(loss.item())},
            "path_tflops": {"flops_per_pair_executed": fl_run, "flops_per_pair_padded_form": fl["fwd_bwd"],
                            "achieved_tflops_per_gpu": fl_run * value / world / 1e12,
                            "frac_of_f32_mfma_peak": fl_run * value / world / 1e12 / PEAK_F32_MFMA_TFLOPS},
        }
        if dumped is not None:
            out["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
        if m is not None:
            summ = summarize_blocks(m, args.steps, world_pairs_blocks)
            out["timed_blocks"] = {"pairs_per_s": summ["value"], "ms_per_step": summ["ms_per_step"], **summ["timed"],
                                   "what": "the same step and workload, measured again after the headline block with the "
                                           "repeated-block protocol (untimed settle blocks, then timed blocks, median)"}
        if prof is not None:
            kernels = {}
            for name, r in prof.items():
                if r["launches"] == 0:
                    continue
                per_step = r["ms"] / PROFILE_EXTRA_STEPS
                rate = r["work"] / (r["ms"] * 1e-3) if r["ms"] > 0 else 0.0
                entry = {"ms_per_step": per_step, "launches_per_step": r["launches"] / PROFILE_EXTRA_STEPS,
                         "avg_launch_ms": r["ms"] / r["launches"]}
                if name.startswith("gemm"):
                    pk = PEAK_BF16_MFMA_TFLOPS if (args.gemm_mode == "bf16" and name in ("gemm_big", "gemm_big_tn")) else PEAK_F32_MFMA_TFLOPS
                    entry.update(bound="mfma", achieved_tflops=rate / 1e12, frac=rate / 1e12 / pk)
                elif name == "few_row_streams":
                    # claim-side aggregation / gate kernels and the evidence-level attention kernels: a few MB per launch, bound
                    # by launch latency, kept apart so that they do not dilute the activation-sized launches' rates
                    entry.update(bound="latency", achieved_gbps=rate / 1e9, frac=rate / 1e9 / PEAK_HBM_GBPS)
                else:
                    entry.update(bound="hbm", achieved_gbps=rate / 1e9, frac=rate / 1e9 / PEAK_HBM_GBPS)
                kernels[name] = entry
            dom = max((k for k in kernels if k.startswith("gemm")), key=lambda k: kernels[k]["ms_per_step"])
            dom_note = None
            if dom != DOMINANT:      # unusual shapes: keep the live measurement of the instrumented kernel, say which one leads
                dom_note = f"{dom} takes more time per step than {DOMINANT} at this shape; the live roofline below is {DOMINANT}'s"
                dom = DOMINANT
            rate = prof_dom["work"] / (prof_dom["ms"] * 1e-3)
            dom_peak = PEAK_BF16_MFMA_TFLOPS if args.gemm_mode == "bf16" else PEAK_F32_MFMA_TFLOPS
            d = {"achieved_tflops": rate / 1e12, "frac": rate / 1e12 / dom_peak,
                 "avg_launch_ms": prof_dom["ms"] / prof_dom["launches"], "launches_per_step": prof_dom["launches"] / prof_dom["steps"]}
            # HBM bytes per launch from the committed rocprofv3 PMC passes -- only for the invocation they were measured
            # on (the headline shape); any other shape reports null rather than a number that belongs to another run
            traffic, traffic_src = None, None
            if headline and world == 1:
                try:
                    pmj = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
                    pm = pmj[dom]
                    traffic = (pm["fetch_kib"] * pm["fetch_correction"] + pm["write_kib"]) * 1024.0
                    traffic_src = pmj.get("_source")
                except Exception:
                    traffic = None
            out["roofline"] = {"kernel": dom, "bound": "mfma", "achieved": d["achieved_tflops"],
                               "peak": dom_peak, "unit": "TFLOP/s", "frac": d["frac"], "traffic": traffic,
                               "traffic_source": traffic_src,
                               "avg_launch_ms": d["avg_launch_ms"], "launches_per_step": d["launches_per_step"],
                               "alg_flops_per_launch": prof_dom["work"] / prof_dom["launches"],
                               "measured": f"HIP events around every {dom} launch of the first {prof_dom['steps']} timed steps "
                                           "of the timed_blocks leg"}
            if dom_note:
                out["roofline"]["note"] = dom_note
            out["kernels_note"] = (f"per-kernel table from {PROFILE_EXTRA_STEPS} extra untimed steps with every library "
                                   "kernel bracketed by HIP events (costs ~0.4 ms/step, so it stays out of the timed region)")
            out["kernels"] = kernels
        if split is not None:
            out["step_split_ms"] = split
        if strong is not None:
            out["strong_scaling"] = strong
        if args.full and not args.no_profile and world == 1:
            out["box_reference"] = box_reference(device)
    default_side = (args.full and world == 1 and headline_run and not args.no_side_modes and not args.no_series)
    do_ref = world == 1 and not args.forward_only and (args.reference_api or default_side)
    do_stream = world == 1 and not args.forward_only and (args.streamed or default_side)
    if (do_ref or do_stream) and rank == 0:
        # VERDICT r2 item 8 -- the two regimes no headline line covers, printed beside it (single GPU):
        #   reference_api: what an UNCHANGED fitter hands over (dense f64 adjacency, resident on the device when the timed
        #                  region starts; the PCIe-inclusive figure adds bytes / 63 GB/s per step, stated)
        #   streamed     : a new batch per step from host arrays (H2D of ids + the m_real read-back), one batch ahead
        extra = {}
        if do_ref:
            wl["ref_batches"] = [ReferenceApiBatch(b) for b in wl["batches"][:2]]
            mr = measure(args, wl, trainer, 1, device, dist, max(4, args.steps // 2), 3, profile=False, source="reference",
                         min_seconds=1.0)
            sr = summarize_blocks(mr, max(4, args.steps // 2), mr["block_pairs"])
            hb = wl["ref_batches"][0].bytes_handed_over
            mr2 = measure(args, wl, trainer, 1, device, dist, max(4, args.steps // 2), 3, profile=False, source="reference_sync",
                          min_seconds=0.5)
            sr2 = summarize_blocks(mr2, max(4, args.steps // 2), mr2["block_pairs"])
            extra["reference_api_sync"] = {**leg_summary(sr2),
                                           "what": "the same hand-over WITHOUT the one-batch-ahead schedule: kargs_from_reference_tensors at the "
                                                   "start of every step, whose counter read-back waits for the previous step to drain"}
            extra["reference_api"] = {**leg_summary(sr),
                                      "bytes_handed_over_per_step": hb,
                                      "what": "dense float64 (B,n,R,R) adjacency + padded ids resident in HBM -> get_amd.batch.ReferenceDepad "
                                              "(gh_ref_depad: one launch -- ids narrowed, adjacency packed, D^-1/2 A D^-1/2 recognised -> bit rows + "
                                              "dinv, node-compact plan from the ids), launched one batch ahead on a side stream "
                                              "(batch.prefetch_reference) so that its 40-byte read-back never waits for a step; same model, same "
                                              "optimiser step (mz_sampler.py:146-160, char_man_fitter_query_repr1.py:92-107,204-250)"}
            # the same hand-over starting in HOST memory: measured, not estimated
            for key, pf, what in (("reference_api_host", False,
                                   "the UNCHANGED fitter loop: every numpy array of the batch through torch.from_numpy(a).cuda() at the start of the "
                                   "step (pageable memory, torch_utils.py:24-27; 76.8 MB of float64 adjacency at this shape), then the de-padding "
                                   "shim and its read-back, then the step"),
                                  ("reference_api_host_prefetch", True,
                                   "the same arrays in PINNED memory, copied and de-padded (gh_ref_depad) one batch ahead on a side stream "
                                   "(what a pin_memory DataLoader + batch.prefetch_reference give a fitter that keeps its dense tensors)")):
                wl["host_ref"] = HostReferenceBatches(wl["ref_batches"], device, prefetch=pf)
                mh = measure(args, wl, trainer, 1, device, dist, max(4, args.steps // 2), 3, profile=False, source="reference_host",
                             min_seconds=1.0)
                sh = summarize_blocks(mh, max(4, args.steps // 2), mh["block_pairs"])
                extra[key] = {**leg_summary(sh), "host_bytes_per_step": wl["host_ref"].bytes_per_step, "what": what}
                del wl["host_ref"]
            del wl["ref_batches"]
            torch.cuda.empty_cache()
        if do_stream:
            raws8 = wl["raws"] + [make_raw_batch(cfg, SEED + 1000 * (len(wl["raws"]) + i)) for i in range(4)]
            wl["streamed"] = StreamedBatches(raws8, cfg, device, wl["compact"])
            ms_ = measure(args, wl, trainer, 1, device, dist, args.steps, 3, profile=False, source="streamed", min_seconds=1.0)
            ss = summarize_blocks(ms_, args.steps, ms_["block_pairs"])
            extra["streamed"] = {**leg_summary(ss),
                                 "what": "a NEW NativeBatch per step from host numpy arrays: one pinned staging buffer -> one H2D copy, "
                                         "device graph build for the node count, 4-byte m_real read-back; prepared one batch ahead "
                                         "on a side stream while the previous step runs (8 distinct host batches rotated)"}
            del wl["streamed"]
        if default_side and args.gemm_mode == "fp32":
            # opt-in arithmetic mode, same step otherwise: fp32 storage and results, the products of the activation-sized NT
            # GEMMs formed on the bf16 MFMA from 3-way bf16 splits with the weight pieces pre-split once per update
            # (error against fp64 equals the exact mode's, results are not bit-identical to it)
            _lib.set_gemm_mode("fp32x3p")
            ops.bump_weight_epoch()
            try:
                mx = measure(args, wl, trainer, 1, device, dist, args.steps, 4, profile=False, min_seconds=1.0)
                sx = summarize_blocks(mx, args.steps, mx["block_pairs"])
                extra["fp32x3p"] = {**leg_summary(sx),
                                    "what": "gh_set_gemm_mode(3): fp32-equivalent products from pre-split bf16 weight pieces on "
                                            "v_mfma_f32_16x16x32_bf16 in the big-tile NT launches; weight-gradient GEMMs and all "
                                            "small GEMMs stay on the fp32 MFMA; NOT the headline (not bit-identical to fp32 MFMA)"}
            finally:
                ops.bump_weight_epoch()
                _lib.set_gemm_mode("fp32")
        out["other_regimes"] = extra
    if rank == 0:
        if args.full and world == 1 and not args.no_series and not args.forward_only and args.evd_dist == "fixed" and headline:
            # SURVEY 8(d) "realistic series": evidence counts from the empirical Snopes histogram (mean 6.9 per claim);
            # at B = 32 that is ~220 pairs per step, at B = 139 about the headline's 960
            series = []
            for bsz in (32, 139):
                c2 = SynthConfig(**{**cfg.__dict__, "batch": bsz})
                w2 = build_workload(seed=SEED, device=device, cfg=c2, n_batches=args.batches, evd_dist="snopes")
                w2["model"].train(True)
                t2 = FlatTrainer(w2["model"], lr=1e-4, weight_decay=1e-3)
                ops.bump_weight_epoch()
                S_W, S_K = 8, 32        # (3 + 10 steps were too few for a fresh model: allocator / workspace warm-up leaked in)
                m2 = measure(args, w2, t2, 1, device, dist, S_K, S_W, profile=False, min_seconds=1.0)
                s2 = summarize_blocks(m2, S_K, m2["block_pairs"])
                series.append({"claims": bsz, "pairs_per_step": w2["b1"], **leg_summary(s2),
                               "claims_per_s": s2["value"] * bsz / w2["b1"]})
                del w2, t2
            ops.bump_weight_epoch()
            out["realistic_series"] = {"evidence_counts": "empirical Snopes histogram (get_amd.synth.SNOPES_EVD_HIST, mean 6.9, max 26)",
                                       "rows": series}
        if world == 1 and headline and default_side and not args.no_other_configs:
            # the other BASELINE configs as legs of the same run (two of five configs had no driver-observed timing)
            out["other_configs"] = [other_config_leg(args, nm, ov, md, st, device, dist, other_config_seed(i))
                                    for i, (nm, ov, md, st) in enumerate(OTHER_CONFIGS)]
        if args.full and world == 1 and not args.forward_only:
            out["parity"] = parity_check(wl)
        if args.full and world == 1 and not args.no_cpu_baseline and not args.forward_only:
            probe = cpu_baseline_probe(wl)
            cb = cpu_baseline(wl, threads=args.cpu_threads or probe["cores"])
            cb["speedup_gpu_over_cpu"] = value / cb["value"]
            out["cpu_baseline"] = cb
            out["cpu_baseline_probe"] = probe
        if args.measure_build and os.environ.get("GH_NT_PHASES"):
            # tool build: per-kind tick sums of the 256-tile epilogue over everything run so far (gemm_nt_pp_epi.hip.h)
            import ctypes
            from get_amd import _lib as _l
            L_ = _l.load()
            buf = (ctypes.c_ulonglong * 64)()
            L_.gh_debug_nt_phases.argtypes = [ctypes.c_void_p, ctypes.c_int]
            torch.cuda.synchronize()
            if L_.gh_debug_nt_phases(buf, 0) == 0:
                out["nt_epilogue_phase_ticks"] = {str(k): [int(buf[k * 4 + j]) for j in range(4)] for k in range(16) if buf[k * 4 + 2]}
        if args.measure_build:
            out["metric"] = "MEASUREMENT BUILD (not a product number): " + out["metric"]
            out["measurement_switches"] = {k: os.environ[k] for k in leaked}
        print(json.dumps(out))
    if lib_comm is not None:
        lib_comm.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

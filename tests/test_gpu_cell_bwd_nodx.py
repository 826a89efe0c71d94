"""GGNN cell backward without an input gradient (csrc/cell_ops.hip): the weight gradients re-associated over
Y = A_hat X instead of da / dxp.  Every case is compared with a float64 restatement of the written-out cell backward on the
CPU; the bound is the one test_ggnn_cell_vs_golden_and_oracle applies to a cell's parameter gradients
(1e-3 of the largest entry + 1e-5).  Shapes: 3 graphs of 20 padded nodes with 20, 7 and 1 real nodes -- rows 4 to 8 floats
wide and din < h are where row-shape bugs have appeared before; 300 x 300 is the production width (column blocks, 10 x 10
fix-up tiles with a ragged edge)."""
import functools

import numpy as np
import pytest
import torch

from tests.util import cell_backward_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, R, COUNTS, VOCAB = 3, 20, (20, 7, 1), 128
W_NAMES = ("p", "z0", "z1", "r0", "r1", "h0", "h1")
B_NAMES = ("z0", "z1", "r0", "r1", "h0", "h1")


def bound(ref):
    return 1e-3 * float(ref.abs().max()) + 1e-5


# ----------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def _graphs():
    """Packed pattern-only adjacency (dinv) of the three graphs, node ids, node counts and the node-compact plan."""
    from get_amd import ops
    toks = np.zeros((N, R), np.int32)
    toks[0] = 100 + np.arange(R)                  # 20 distinct words
    toks[1] = 40 + np.arange(R) % 7               # 7 distinct words
    toks[2] = 5                                   # a single node
    lens = np.full((N,), R, np.int32)
    padj, node_ids, n_nodes = ops.graph_build(torch.from_numpy(toks).to(DEV), torch.from_numpy(lens).to(DEV), 3)
    assert tuple(n_nodes.cpu().tolist()) == COUNTS
    plan = ops.RaggedPlan(n_nodes, node_ids, sum(COUNTS))
    return padj, node_ids, plan


@functools.lru_cache(maxsize=None)
def _numbers(din, h):
    """Table, weights, biases, output gradient and the .grad pre-fills of one width pair (CPU, fp32)."""
    gen = torch.Generator().manual_seed(7919 * din + h)
    rn = lambda *s: torch.randn(*s, generator=gen)
    w = {"p": rn(h, din) / din ** 0.5}
    w.update({k: rn(h, h) / h ** 0.5 for k in W_NAMES[1:]})
    b = {k: 0.1 * rn(h) for k in B_NAMES}
    pre_w = {k: 0.3 * rn(*v.shape) for k, v in w.items()}
    pre_b = {k: 0.3 * rn(h) for k in B_NAMES}
    return dict(table=rn(VOCAB, din), w=w, b=b, pre_w=pre_w, pre_b=pre_b, g=rn(N * R, h), wscale=1.0 + 0.1 * rn(N, R, R))


def _adjacency(variant):
    """variant -> (PackedAdj, dropout p): pattern-only / weighted values / pattern with a keep set."""
    from get_amd import ops
    padj, node_ids, plan = _graphs()
    if variant == "pattern":
        return padj, 0.0
    if variant == "weighted_drop":
        dense = padj.to_dense() * _numbers(8, 8)["wscale"].to(DEV)
        return ops.PackedAdj.from_dense(dense), 0.2
    assert variant == "keep_drop"
    keep = np.zeros((N, R), bool)
    keep[:, ::3] = True
    keep[0, :6] = True
    kw = np.zeros((N, 1), np.uint64)
    for j in range(R):
        kw[:, 0] |= keep[:, j].astype(np.uint64) << np.uint64(j)
    return padj.with_keep(torch.from_numpy(kw.view(np.int64)).to(DEV)), 0.2


def _params(num, grads=True):
    """The thirteen cell parameters on the device in ops.ggnn_cell's order, their .grad pre-filled with non-zero values the
    kernels accumulate into (the trainer's flat-bucket convention, ops.weights._direct)."""
    def leaf(v, pre):
        t = v.clone().to(DEV).requires_grad_(True)
        if grads:
            t.grad = pre.clone().to(DEV)
            t._gh_direct_grad = True
        return t
    w = {k: leaf(num["w"][k], num["pre_w"][k]) for k in W_NAMES}
    b = {k: leaf(num["b"][k], num["pre_b"][k]) for k in B_NAMES}
    order = (w["p"], w["z0"], b["z0"], w["z1"], b["z1"], w["r0"], b["r0"], w["r1"], b["r1"], w["h0"], b["h0"], w["h1"], b["h1"])
    return w, b, order


# ----------------------------------------------------------------------------- float64 reference (tests/util.py)
def _reference(num, adj, drop_p, seed, compact, din, h):
    """Gradients of the call on the padded (compact = False) or the node-compact layout; the stateless dropout mask is
    indexed by the call's own row."""
    from get_amd import ops
    padj, node_ids, plan = _graphs()
    dense = adj.to_dense().double().cpu()
    ids = (plan.cids[:plan.m_real] if compact else node_ids.reshape(-1)).long().cpu()
    rows = ids.numel()
    x = num["table"].double()[ids]
    if drop_p > 0:
        x = x * torch.from_numpy(ops.dropout_mask_reference(seed, rows, din, drop_p)).double() / (1 - drop_p)
    g = num["g"][:rows].double()
    if compact:      # real rows scattered to their padded places; padding rows carry no gradient and have no edges
        src = plan.src[:rows].long().cpu()
        xpad, gpad = torch.zeros(N * R, din, dtype=torch.float64), torch.zeros(N * R, h, dtype=torch.float64)
        xpad[src], gpad[src] = x, g
        x, g = xpad, gpad
    return cell_backward_f64(dense, x.view(N, R, din), g.view(N, R, h), num["w"], num["b"])


def _check(num, w, b, dw, db, what):
    for k in W_NAMES:
        ref = num["pre_w"][k].double() + dw[k]
        err = float((w[k].grad.double().cpu() - ref).abs().max())
        print(f"{what} dw_{k}: err {err:.3e} bound {bound(dw[k]):.3e}")
        assert err <= bound(dw[k]), (what, "dw_" + k, err)
    for k in B_NAMES:
        ref = num["pre_b"][k].double() + db[k]
        err = float((b[k].grad.double().cpu() - ref).abs().max())
        print(f"{what} db_{k}: err {err:.3e} bound {bound(db[k]):.3e}")
        assert err <= bound(db[k]), (what, "db_" + k, err)


def _run_ids(din, h, variant, compact, seed=90210):
    """One forward / backward of the cell through ops' autograd on table + ids (no input gradient); returns the GEMM
    launches of the backward."""
    from get_amd import _lib, ops
    padj, node_ids, plan = _graphs()
    num = _numbers(din, h)
    adj, drop_p = _adjacency(variant)
    w, b, order = _params(num)
    table = num["table"].to(DEV)
    if compact:
        out = ops.ggnn_cell(adj, table, plan.cids[:plan.m_real].contiguous(), order, drop_p, seed, plan=plan, rows=plan.m_real)
    else:
        out = ops.ggnn_cell(adj, table, node_ids.reshape(-1), order, drop_p, seed)
    g = num["g"][:out.numel() // h].to(DEV).view(out.shape)
    _lib.gemm_path_counters(reset=True)
    out.backward(g)
    torch.cuda.synchronize()
    c = _lib.gemm_path_counters()
    dw, db, _ = _reference(num, adj, drop_p, seed, compact, din, h)
    _check(num, w, b, dw, db, f"din={din} h={h} {variant} compact={compact}")
    return c["fast"] + c["generic"]


# ----------------------------------------------------------------------------- the public entry: two-launch schedule
@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("variant", ["pattern", "weighted_drop", "keep_drop"])
@pytest.mark.parametrize("din,h", [(8, 8), (12, 20), (300, 300)])
def test_cell_backward_without_input_gradient_vs_float64(din, h, variant, compact):
    """gh_ggnn_cell_bwd with ids (dx == NULL) and five scratch tensors: the d(r xp) product, the weight-gradient launch over X
    and E, A_hat X into the freed dxp, the weight-gradient launch over Y, the fix-up.  All seven weight gradients and six bias
    gradients accumulate into pre-filled .grad buffers."""
    launches = _run_ids(din, h, variant, compact)
    assert launches == 3, f"expected one NT and two TN launches, counted {launches}"


def test_cell_backward_with_input_gradient_keeps_its_launches():
    """x itself wants a gradient (dx != NULL): today's chain -- the two da / dxp launches, the dX launch, one weight-gradient
    launch -- and its numbers."""
    from get_amd import _lib, ops
    din, h = 12, 20
    padj, node_ids, plan = _graphs()
    num = _numbers(din, h)
    w, b, order = _params(num)
    ids = node_ids.reshape(-1).long().cpu()
    x = num["table"][ids].to(DEV).view(N, R, din).requires_grad_(True)
    out = ops.ggnn_cell(padj, x, None, order)
    _lib.gemm_path_counters(reset=True)
    out.backward(num["g"].to(DEV).view(N, R, h))
    torch.cuda.synchronize()
    c = _lib.gemm_path_counters()
    assert c["fast"] + c["generic"] == 4, c
    dw, db, dx = _reference(num, padj, 0.0, 0, False, din, h)
    _check(num, w, b, dw, db, "dx")
    assert float((x.grad.double().cpu() - dx).abs().max()) <= 1e-3 * float(dx.abs().max()) + 1e-6


def test_cell_backward_without_workspace_takes_the_old_chain():
    """No split-K workspace registered for the stream: nowhere to keep T / S, so the call runs the da / dxp chain."""
    from get_amd import _lib
    _lib.ensure_workspace(DEV)
    _lib.call("gh_set_stream_workspace", _lib.stream(), None, 0)
    try:
        launches = _run_ids(12, 20, "weighted_drop", True)
    finally:
        torch.cuda.synchronize()
        _lib._workspaces.clear()          # the next ensure_workspace registers a default-sized buffer again
        _lib.ensure_workspace(DEV)
    assert launches == 3, launches       # two NT launches and one TN launch


# ----------------------------------------------------------------------------- the composite: one TN launch with ybuf
@functools.lru_cache(maxsize=None)
def _model_case(D, H):
    from get_amd.synth import SynthConfig, make_embeddings, make_raw_batch, make_state_dict
    from oracle import get_oracle as O
    from oracle.assemble import assemble_inputs
    cfg = SynthConfig(batch=2, n_evd=3, len_left=8, len_right=20, emb_dim=D, hidden=H, vocab=60, n_article_src=10,
                      n_claim_src=5, src_dim=8, word_heads=2, evd_heads=1)
    seed = 11
    raw = make_raw_batch(cfg, seed)
    inp = assemble_inputs(raw, cfg, O.convert_text)
    emb, art, clm = make_embeddings(cfg, seed)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    f64 = lambda a: T(a).double()
    p = {k: f64(v).requires_grad_(True) for k, v in make_state_dict(cfg, seed).items()}
    p["embedding.weight"] = f64(emb)
    p["article_source_embs.weight"] = f64(art).requires_grad_(True)
    phi, _, _ = O.model_forward(p, cfg.__dict__, T(inp["query"]), T(inp["document"]), f64(inp["query_adj"]), T(inp["doc_ids"]),
                                f64(inp["doc_adj"]), T(inp["query_lens"]), inp["evd_counts"], T(inp["doc_sources"]),
                                T(inp["query_sources"]))
    O.cross_entropy(phi, T(inp["labels"])).backward()
    return cfg, seed, raw, inp, {k: v.grad for k, v in p.items() if v.grad is not None}


@pytest.mark.parametrize("D,H", [(8, 8), (12, 20)])
def test_composite_backward_single_launch_schedule_vs_float64_oracle(D, H, monkeypatch):
    """Tiny model (B = 2, 3 evidences, R = 20, L = 8): the composite backward hands the first evidence cell a second row
    buffer (one weight-gradient launch) and keeps the few-row claim cell on the da / dxp chain; the module-by-module path runs
    both cells through the public entry (two launches each).  Every live gradient of both against the float64 oracle, and
    against each other."""
    from get_amd import fused, ops
    from oracle.assemble import reference_kargs
    from tests.test_gpu_model import build_model, to_dev
    cfg, seed, raw, inp, ref = _model_case(D, H)
    got = {}
    for on in (False, True):
        monkeypatch.setattr(fused, "ENABLED", on)
        model = build_model(cfg, seed)
        kargs = to_dev(reference_kargs(inp, torch, output_ranking=True))
        qa, _, _ = ops.graph_build(torch.from_numpy(raw["claim_tokens"]).to(DEV), torch.from_numpy(raw["claim_len"]).to(DEV), cfg.window)
        da, d_ids, d_n = ops.graph_build(torch.from_numpy(raw["evd_tokens"]).to(DEV), torch.from_numpy(raw["evd_len"]).to(DEV), cfg.window)
        kargs["query_adj"], kargs["docs_adj"] = qa, da.with_plan(ops.RaggedPlan(d_n, d_ids, int(d_n.sum().item())))
        phi, _ = model(torch.from_numpy(inp["query"]).to(DEV), torch.from_numpy(inp["document"]).to(DEV), **kargs)
        assert (getattr(model, "_gh_binding", None) is not None) == on, "the wrong path ran"
        torch.nn.functional.cross_entropy(phi, torch.from_numpy(inp["labels"]).to(DEV)).backward()
        torch.cuda.synchronize()
        got[on] = {k: q.grad.double().cpu() for k, q in model.named_parameters() if q.grad is not None}
    n_checked = 0
    for k, go in ref.items():
        if k not in got[True]:
            continue
        for on in (False, True):
            err = float((got[on][k] - go).abs().max())
            print(f"D={D} H={H} composite={on} {k}: err {err:.3e} bound {bound(go):.3e}")
            assert err <= bound(go), (k, on, err)
        assert float((got[True][k] - got[False][k]).abs().max()) <= bound(go), k
        n_checked += 1
    assert n_checked >= 40

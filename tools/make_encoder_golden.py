"""Golden vectors of the wrapper module's other graph encoders (GraphAttentionLayer, GAT, GCN), captured from the
upstream reference in the build container -- never on the GPU machine, and no test reads the reference.

Loads the reference's ``Models/BiDAF/wrapper.py`` (it imports only torch) from the directory ``oracle/_refshim.py``
points at, runs every case in evaluation mode in fp32 on the CPU with seeded weights and inputs, and writes

    tests/golden/g10_gat.npz   GraphAttentionLayer (concat True/False) and GAT (heads 1, 3; num_layers 1, 2)
    tests/golden/g11_gcn.npz   GCN (num_layers 1, 2) on convert_text's normalised adjacency and on an asymmetric
                               weighted one with zero rows
    tests/golden/encoder_contract.json   state_dict key / shape lists of every constructor configuration

Per case ``<case>::``: the inputs (x, adj, and for convert_text graphs the tokens they were built from), every parameter
(``param::<name>``), the output, the upstream gradient ``gout`` of the loss sum(out * gout), and the gradients of every
parameter (``grad::<name>``) and of x (``grad::x``).

    python tools/make_encoder_golden.py
"""
import json
import os
import zlib

import numpy as np
import torch

from golden_common import OUT, load_reference, write_contract      # puts the repository root on sys.path
from oracle.get_oracle import convert_text

# shapes: B graphs of L nodes; tokens shorter than L leave padding nodes (no edges: uniform attention rows)
B, L, WINDOW = 3, 12, 3
GAT_CASES = {     # name -> constructor kwargs; adjacency kind
    "layer_concat": dict(cls="GraphAttentionLayer", kw=dict(in_features=8, out_features=6, dropout=0.3, alpha=0.2, concat=True)),
    "layer_plain": dict(cls="GraphAttentionLayer", kw=dict(in_features=8, out_features=6, dropout=0.3, alpha=0.2, concat=False)),
    "gat_h1_l1": dict(cls="GAT", kw=dict(input_size=8, hidden_size=6, output_size=5, head_num=1, num_layers=1)),
    "gat_h3_l1": dict(cls="GAT", kw=dict(input_size=8, hidden_size=6, output_size=5, head_num=3, num_layers=1)),
    "gat_h1_l2": dict(cls="GAT", kw=dict(input_size=8, hidden_size=6, output_size=5, head_num=1, num_layers=2)),
    "gat_h3_l2": dict(cls="GAT", kw=dict(input_size=8, hidden_size=6, output_size=5, head_num=3, num_layers=2, alpha=0.1)),
}
GCN_CASES = {
    "gcn_l1": dict(cls="GCN", kw=dict(input_dim=8, hidden_dim=6, output_dim=7, num_layers=1)),
    "gcn_l2": dict(cls="GCN", kw=dict(input_dim=8, hidden_dim=6, output_dim=6, num_layers=2)),
}
ADJ_KINDS = ("text", "weighted")


def text_graphs(rng):
    """convert_text graphs of B token sequences with fewer distinct tokens than L (padding nodes)."""
    lengths = np.array([L, 7, 4], dtype=np.int64)
    tokens = np.zeros((B, L), dtype=np.int64)
    adj = np.zeros((B, L, L), dtype=np.float64)
    for b in range(B):
        tokens[b, :lengths[b]] = rng.integers(1, 9, size=lengths[b])
        _, a, _ = convert_text(tokens[b], L, int(lengths[b]), WINDOW)
        adj[b] = a
    return tokens, lengths, adj.astype(np.float32)


def weighted_graphs(rng):
    """Asymmetric weighted adjacency: mixed-sign values (GAT keeps the > 0 entries only), zero rows (isolated nodes),
    zero columns."""
    a = rng.uniform(-0.3, 1.0, size=(B, L, L)).astype(np.float32)
    a *= rng.uniform(size=(B, L, L)) < 0.35
    a[:, 3, :] = 0.0
    a[1, 7, :] = 0.0
    a[:, :, 5] = 0.0
    a[2, 9, :] = -0.5                      # only negative entries: no edge under adj > 0, a non-zero row sum for GCN
    return a


def run_case(ref, store, contract, name, spec, kind, adj_np, tokens=None, lengths=None):
    torch.manual_seed(zlib.crc32(f"{name}/{kind}".encode()))
    cls = getattr(ref, spec["cls"])
    m = cls(**spec["kw"]).train(False)
    contract.setdefault(name, {"class": spec["cls"], "kwargs": spec["kw"],
                               "state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()]})
    din = spec["kw"].get("in_features", spec["kw"].get("input_size", spec["kw"].get("input_dim")))
    g = torch.Generator().manual_seed(7 + len(name) + len(kind))
    x = torch.randn((B, L, din), generator=g).requires_grad_(True)
    adj = torch.from_numpy(adj_np)
    out = m(x, adj)
    gout = torch.randn(out.shape, generator=g)
    (out * gout).sum().backward()
    key = f"{name}/{kind}::"
    store[key + "x"] = x.detach().numpy()
    store[key + "adj"] = adj_np
    if tokens is not None:
        store[key + "tokens"] = tokens
        store[key + "lengths"] = lengths
    for k, v in m.state_dict().items():
        store[key + "param::" + k] = v.numpy().copy()
    store[key + "out"] = out.detach().numpy()
    store[key + "gout"] = gout.numpy()
    store[key + "grad::x"] = x.grad.numpy()
    for k, p in m.named_parameters():
        store[key + "grad::" + k] = p.grad.numpy().copy()


def main():
    ref = load_reference("Models/BiDAF/wrapper.py", "ref_bidaf_wrapper")
    torch.set_num_threads(4)
    rng = np.random.default_rng(20241016)
    tokens, lengths, text_adj = text_graphs(rng)
    w_adj = weighted_graphs(rng)
    # GCN on the weighted graph: the reference's row sums must be >= 0 for a finite result (pow(-0.5) of a negative
    # sum is nan); |a| keeps the zero rows, the asymmetry and the zero columns
    w_adj_gcn = np.abs(w_adj)
    contract = {}
    gat, gcn = {}, {}
    for name, spec in GAT_CASES.items():
        run_case(ref, gat, contract, name, spec, "text", text_adj, tokens, lengths)
        run_case(ref, gat, contract, name, spec, "weighted", w_adj)
    for name, spec in GCN_CASES.items():
        run_case(ref, gcn, contract, name, spec, "text", text_adj, tokens, lengths)
        run_case(ref, gcn, contract, name, spec, "weighted", w_adj_gcn)
    meta = {"B": B, "L": L, "window": WINDOW, "gat_cases": list(GAT_CASES), "gcn_cases": list(GCN_CASES),
            "adj_kinds": list(ADJ_KINDS)}
    enc = lambda d: np.frombuffer(json.dumps(d).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(OUT, "g10_gat.npz"), meta=enc(meta), **gat)
    np.savez_compressed(os.path.join(OUT, "g11_gcn.npz"), meta=enc(meta), **gcn)
    write_contract(os.path.join(OUT, "encoder_contract.json"), contract)
    for f in ("g10_gat.npz", "g11_gcn.npz", "encoder_contract.json"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()

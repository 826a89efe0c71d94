"""Golden vectors of the BiDAF model (Models/BiDAF/bidaf_model.py), captured from the upstream reference in the build
container -- never on the GPU machine, and no test reads the reference.

``oracle/_refshim.install()`` makes the whole reference importable on the CPU; every case runs in fp32 in eval() mode and
the generator writes

    tests/golden/g15_bidaf.npz           every case below
    tests/golden/bidaf_contract.json     the params of every case and its state_dict key / shape list, in order

Cases (V words of dimension D, hidden size H, B pairs, query ids (B,L), document ids (B,R); ragged lengths, one full-length
sequence per side unless noted; the index pairs are the stable argsort by descending length and its inverse):
  v50_h12      (50, 20, 12, 5, 7, 11), embedding frozen
  v60_h16      (60, 24, 16, 19, 9, 37), embedding trainable: three 16-row context tiles, more than one 16-sequence LSTM tile
  v80_h20      (80, 32, 20, 6, 33, 70), embedding frozen: three 16-column tiles of queries, five context tiles
  short_query  (40, 16, 8, 4, 9, 13), embedding trainable: the longest query has 6 of the id tensor's 9 positions

Parameters keep the reference's init, rounded to what float16 holds exactly (they are stored as float16: half the bytes),
except that every bias is seeded, non-zero and distinct, so a dropped bias shows.  Per case ``<case>::``: ``query``,
``document``, ``q_lens``, ``c_lens``, the four index arrays, every parameter (``param::<name>``), ``logits``, the seeded
upstream gradient ``g_logits`` of the loss sum(logits * g_logits), and the gradient of every trainable parameter
(``grad::<name>``).

Every case also runs in float64, and the reference's own fp32 result must lie within one tenth of the tolerance the tests
apply (logits 1e-4 + 1e-4 |want|, gradients 1e-5 + 1e-4 |want|, elementwise), so the fixture never eats the test's margin.

    python tools/make_bidaf_golden.py
"""
import json
import os
import zlib

import numpy as np
import torch

from golden_common import OUT, _refshim, margin, to_numpy, write_contract, write_npz

CASES = {
    "v50_h12": dict(V=50, D=20, H=12, q_lens=[7, 3, 5, 1, 4], c_lens=[4, 11, 2, 9, 6], L=7, R=11, freeze=True),
    "v60_h16": dict(V=60, D=24, H=16, q_lens=[9, 2, 5, 7, 1, 3, 8, 4, 6, 9, 2, 5, 7, 1, 3, 8, 4, 6, 5],
                    c_lens=[12, 37, 5, 20, 1, 33, 16, 17, 8, 29, 3, 24, 36, 10, 15, 32, 2, 21, 19], L=9, R=37, freeze=False),
    "v80_h20": dict(V=80, D=32, H=20, q_lens=[33, 16, 17, 5, 28, 1], c_lens=[48, 70, 65, 3, 16, 33], L=33, R=70, freeze=True),
    "short_query": dict(V=40, D=16, H=8, q_lens=[6, 2, 4, 3], c_lens=[13, 5, 2, 9], L=9, R=13, freeze=False),
}
TOL_LOGITS = (1e-4, 1e-4)
TOL_GRADS = (1e-5, 1e-4)


def run(BiDAF, name, spec, dtype):
    seed = zlib.crc32(name.encode())
    g = torch.Generator().manual_seed(seed ^ 0x5EED)
    emb = (0.5 * torch.randn(spec["V"], spec["D"], generator=g)).half().float().numpy()
    params = dict(embedding=emb, embedding_freeze=spec["freeze"], word_dim=spec["D"], hidden_size=spec["H"], dropout=0.2)
    torch.manual_seed(seed)
    m = BiDAF(params)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "bias" in k:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
            p.copy_(p.half().float())
    m = m.to(dtype).eval()
    q_lens, c_lens = torch.tensor(spec["q_lens"], dtype=torch.int64), torch.tensor(spec["c_lens"], dtype=torch.int64)
    B = len(spec["q_lens"])
    query = torch.randint(0, spec["V"], (B, spec["L"]), generator=g)
    document = torch.randint(0, spec["V"], (B, spec["R"]), generator=g)
    idx = {}
    for side, lens in (("q", q_lens), ("d", c_lens)):
        idx[side + "_new"] = torch.sort(lens, descending=True, stable=True)[1]
        idx[side + "_restoring"] = torch.argsort(idx[side + "_new"])
    logits = m(query, document, query_lens_indices=(idx["q_new"], idx["q_restoring"], q_lens),
               doc_lens_indices=(idx["d_new"], idx["d_restoring"], c_lens))
    assert logits.shape == (B, 1)
    g_logits = torch.randint(-16, 17, logits.shape, generator=g).float() / 16
    (logits * g_logits.to(dtype)).sum().backward()
    res = {"query": query.numpy().astype(np.int32), "document": document.numpy().astype(np.int32),
           "q_lens": q_lens.numpy().astype(np.int32), "c_lens": c_lens.numpy().astype(np.int32),
           "logits": logits, "g_logits": g_logits}
    res.update({k + "_indices": v.numpy() for k, v in idx.items()})
    for k, p in m.named_parameters():
        if p.requires_grad:
            res["grad::" + k] = p.grad
    res = to_numpy(res)
    for k, v in m.state_dict().items():
        h = v.detach().float().numpy().astype(np.float16)
        assert np.array_equal(h.astype(np.float64), v.detach().double().numpy()), k
        res["param::" + k] = h
    contract = {"params": {k: v for k, v in params.items() if k != "embedding"},
                "embedding_shape": list(emb.shape),
                "state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()]}
    return contract, res


def bound(k, want):
    atol, rtol = TOL_LOGITS if k == "logits" else TOL_GRADS
    return atol + rtol * np.abs(want)


def main():
    _refshim.install()
    from Models.BiDAF.bidaf_model import BiDAF
    torch.set_num_threads(1)
    store, contracts = {}, {}
    for name, spec in CASES.items():
        assert max(spec["c_lens"]) == spec["R"] and len(spec["q_lens"]) == len(spec["c_lens"]) >= 2 and min(spec["c_lens"]) >= 1
        contract, r32 = run(BiDAF, name, spec, torch.float32)
        _, r64 = run(BiDAF, name, spec, torch.float64)
        checked = [k for k in r32 if k == "logits" or k.startswith("grad::")]
        worst = margin(r32, r64, checked, bound)
        print(f"{name}: fp32 reference at {worst:.4f} of a tenth of the bound")
        assert worst <= 1.0, (name, worst)
        assert all(np.isfinite(v.astype(np.float64)).all() for v in r32.values())
        assert ("grad::word_emb.weight" in r32) == (not spec["freeze"])
        contracts[name] = contract
        for k, v in r32.items():
            store[f"{name}::{k}"] = v
    assert max(CASES["short_query"]["q_lens"]) < CASES["short_query"]["L"]
    store["meta"] = np.frombuffer(json.dumps({"cases": list(CASES)}).encode(), dtype=np.uint8)
    write_npz(os.path.join(OUT, "g15_bidaf.npz"), store)
    write_contract(os.path.join(OUT, "bidaf_contract.json"), contracts)
    for f in ("g15_bidaf.npz", "bidaf_contract.json"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()

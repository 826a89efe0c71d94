"""Golden vectors of the multi-head query/key/value attention family (ScaledDotProductAttention,
MultiHeadAttentionOriginal, ConcatNotEqualSelfAttTransFormer, MultiHeadAttentionSimple), captured from the upstream
reference in the build container -- never on the GPU machine, and no test reads the reference.

Loads the reference's ``thirdparty/two_branches_attention.py`` (it imports only torch and numpy) from the directory
``oracle/_refshim.py`` points at, runs every case in fp32 on the CPU with seeded weights and inputs, and writes

    tests/golden/g13_mha.npz            every case below in each of its geometries
    tests/golden/mha_contract.json      class, kwargs and state_dict key / shape lists of every configuration

Cases (geometry names spell the sizes: n = sequences, q / k = query / key rows, b / l = batch / length):
  sdpa_3x5          n2q3k5, dk=6, dv=5 (no width is a multiple of 4); row (0, 1) is fully masked, row (1, 0) keeps one key
  sdpa_35x70        n2q35k70, dk=8, dv=12: three query tiles, keys cross 64, ragged key padding, one fully masked row
  sdpa_offset_pos / sdpa_offset_neg   n2q3k12, dk=8, dv=5 with query[..., 0] = +-96 and key[..., 0] = 1: every score sits
                    near +-96 with an O(1) spread -- a softmax without max-subtraction overflows resp. underflows there
  mha_orig_h3       MultiHeadAttentionOriginal(3, 8, 4, 5) at b2q3k5 and b2q17k70, q distinct from k = v, one fully masked row
  mha_orig_h1       MultiHeadAttentionOriginal(1, 8, 8, 8) at b2q5k5 and b2q70k70 with q = k = v
  transformer_concat   ConcatNotEqualSelfAttTransFormer(16, 8) at b3l12 and b2l70 (mask (B,1,L) bool, True = pad)
  mha_simple_h3 / mha_simple_h3_ln    MultiHeadAttentionSimple(3, 8, 8, 8, use_layer_norm=False / True), same geometries;
                    no all-padding sequence

Per case ``<case>/<geometry>::``: the distinct input tensors by name (``meta["args"][case]`` lists the forward's positional
arguments, a name repeated where one tensor is passed twice), ``mask``, every parameter (``param::<name>``), ``out`` and
``weights`` (where the class returns them), the seeded upstream gradients ``gout`` / ``gweights`` of the loss
sum(out * gout) + sum(weights * gweights), and the gradients of every input (``grad::<name>``) and parameter.

Every case also runs in float64, and the reference's own fp32 result must lie within one tenth of the tolerance the GPU
test applies (tests/test_gpu_mha.py), so the fixture never eats the test's margin.

    python tools/make_mha_golden.py
"""
import json
import os
import zlib

import numpy as np
import torch

from golden_common import OUT, load_reference, margin, to_numpy, write_contract, write_npz

SEQ_GEOMS = {"b3l12": (3, 12), "b2l70": (2, 70)}
CASES = {
    "sdpa_3x5": dict(cls="ScaledDotProductAttention", kw=dict(temperature=1.0), kind="sdpa", dk=6, dv=5,
                     geoms={"n2q3k5": (2, 3, 5)}),
    "sdpa_35x70": dict(cls="ScaledDotProductAttention", kw=dict(temperature=1.0), kind="sdpa", dk=8, dv=12,
                       geoms={"n2q35k70": (2, 35, 70)}),
    "sdpa_offset_pos": dict(cls="ScaledDotProductAttention", kw=dict(temperature=1.0), kind="sdpa", dk=8, dv=5, offset=96.0,
                            geoms={"n2q3k12": (2, 3, 12)}),
    "sdpa_offset_neg": dict(cls="ScaledDotProductAttention", kw=dict(temperature=1.0), kind="sdpa", dk=8, dv=5, offset=-96.0,
                            geoms={"n2q3k12": (2, 3, 12)}),
    "mha_orig_h3": dict(cls="MultiHeadAttentionOriginal", kw=dict(n_head=3, d_model=8, d_k=4, d_v=5), kind="orig",
                        geoms={"b2q3k5": (2, 3, 5), "b2q17k70": (2, 17, 70)}),
    "mha_orig_h1": dict(cls="MultiHeadAttentionOriginal", kw=dict(n_head=1, d_model=8, d_k=8, d_v=8), kind="orig_self",
                        geoms={"b2q5k5": (2, 5, 5), "b2q70k70": (2, 70, 70)}),
    "transformer_concat": dict(cls="ConcatNotEqualSelfAttTransFormer", kw=dict(inp_dim=16, out_dim=8), kind="concat",
                               geoms=SEQ_GEOMS),
    "mha_simple_h3": dict(cls="MultiHeadAttentionSimple", kw=dict(num_heads=3, d_model=8, d_key=8, d_value=8,
                                                                 use_layer_norm=False), kind="simple", geoms=SEQ_GEOMS),
    "mha_simple_h3_ln": dict(cls="MultiHeadAttentionSimple", kw=dict(num_heads=3, d_model=8, d_key=8, d_value=8,
                                                                    use_layer_norm=True), kind="simple", geoms=SEQ_GEOMS),
}
ARGS = {"sdpa": ["query", "key", "value"], "orig": ["q", "k", "k"], "orig_self": ["q", "q", "q"],
        "concat": ["query", "key", "value"], "simple": ["left", "right"]}
OFFSET_CASES = ("sdpa_offset_pos", "sdpa_offset_neg")
# the GPU test's tolerances (elementwise atol + rtol |want|; offset cases: largest error over largest entry)
TOL_OUT, TOL_GRAD, TOL_REL = (1e-4, 1e-4), (1e-5, 1e-4), 1e-4


def pair_mask(n, lq, lk):
    """(n, lq, lk) bool, True = masked: ragged key padding (sequence 0 loses its last 1 + lk // 4 keys, sequence 1 its last
    one), an interior hole, row (0, 1) fully masked and row (1, 0) with a single unmasked key."""
    m = np.zeros((n, lq, lk), dtype=bool)
    m[0, :, lk - 1 - lk // 4:] = True          # sequence 0: suffix padding of the keys
    if n > 1:
        m[1, :, lk - 1:] = True                # sequence 1: one padded key
        m[1, 0, :] = True
        m[1, 0, 2] = False                     # a single unmasked key: one-hot weights
    m[0, 0, 1] = True                          # an interior hole
    m[0, 1, :] = True                          # a fully masked query row
    if lq > 32:
        m[1, lq - 3, :] = True                 # and one in the last query tile
    return m


def seq_mask(b, l):
    """(b, l) float, 0 = pad: interior zeros, suffix padding, a single real token; never an all-padding sequence."""
    m = np.ones((b, l), dtype=np.float32)
    m[0, 3] = m[0, 5] = 0.0
    m[1, (2 * l) // 3:] = 0.0
    if b > 2:
        m[2, :] = 0.0
        m[2, 4] = 1.0
    return m


def make_inputs(spec, dims, g):
    """(distinct input tensors by name, mask) of one case."""
    r = lambda *s: torch.randn(s, generator=g)
    kind = spec["kind"]
    if kind == "sdpa":
        n, lq, lk = dims
        query, key, value = r(n, lq, spec["dk"]), r(n, lk, spec["dk"]), r(n, lk, spec["dv"])
        if "offset" in spec:
            query[..., 0] = spec["offset"]
            key[..., 0] = 1.0
        return {"query": query, "key": key, "value": value}, torch.from_numpy(pair_mask(n, lq, lk))
    if kind == "orig":
        b, lq, lk = dims
        return {"q": r(b, lq, 8), "k": r(b, lk, 8)}, torch.from_numpy(pair_mask(b, lq, lk))
    if kind == "orig_self":
        b, lq, lk = dims
        return {"q": r(b, lq, 8)}, torch.from_numpy(pair_mask(b, lq, lk))
    b, l = dims
    if kind == "concat":
        return ({"query": r(b, 1, 8), "key": r(b, l, 8), "value": r(b, l, 5)},
                torch.from_numpy(seq_mask(b, l) == 0).unsqueeze(1))
    return {"left": r(b, 8), "right": r(b, l, 8)}, torch.from_numpy(seq_mask(b, l))


def run(ref, spec, name, geom, dtype, scale=1.0):
    dims = spec["geoms"][geom]
    torch.manual_seed(zlib.crc32(f"{name}/{geom}".encode()))
    m = getattr(ref, spec["cls"])(**spec["kw"]).to(dtype)
    g = torch.Generator().manual_seed(13 + len(name) + 7 * len(geom))
    raw, mask = make_inputs(spec, dims, g)
    inputs = {k: (t * scale).to(dtype).requires_grad_(True) for k, t in raw.items()}
    args = [inputs[k] for k in ARGS[spec["kind"]]]
    out, weights = m(*args, mask)
    gout = torch.randn(out.shape, generator=g)
    loss = (out * gout.to(dtype)).sum()
    res = {"mask": mask.numpy(), "out": out, "gout": gout}
    if weights is not None:
        gweights = torch.randn(weights.shape, generator=g)
        loss = loss + (weights * gweights.to(dtype)).sum()
        res["weights"], res["gweights"] = weights, gweights
    loss.backward()
    for k, t in inputs.items():
        res[k] = t
        res["grad::" + k] = t.grad
    for k, p in m.named_parameters():
        res["param::" + k] = p
        res["grad::" + k] = p.grad
    return m, to_numpy(res)


def margin_of(name, r32, r64):
    """The reference's fp32 result against its float64 one, as a fraction of a tenth of the GPU test's tolerance."""
    def bound(k, want):
        if name in OFFSET_CASES:
            return TOL_REL * (np.abs(want).max() + 1e-12)
        atol, rtol = TOL_OUT if k in ("out", "weights") else TOL_GRAD
        return atol + rtol * np.abs(want)
    return margin(r32, r64, [k for k in r32 if k in ("out", "weights") or k.startswith("grad::")], bound)


def main():
    ref = load_reference("thirdparty/two_branches_attention.py", "ref_two_branches_attention")
    torch.set_num_threads(1)
    store, contract, scales = {}, {}, {}
    for name, spec in CASES.items():
        for geom in spec["geoms"]:
            # a case whose fp32 reference alone misses a tenth of the bound (LayerNorm of small inputs amplifies their rounding)
            # has its inputs rescaled until it passes; the test's tolerance is never loosened
            for scale in (1.0, 0.5, 0.25, 0.125):
                m, r32 = run(ref, spec, name, geom, torch.float32, scale)
                _, r64 = run(ref, spec, name, geom, torch.float64, scale)
                worst = margin_of(name, r32, r64)
                if worst <= 1.0:
                    break
            assert worst <= 1.0, (name, geom, worst)
            scales[f"{name}/{geom}"] = scale
            print(f"{name}/{geom}: input scale {scale}, fp32 reference at {worst:.3f} of a tenth of the bound")
            contract.setdefault(name, {"class": spec["cls"], "kwargs": spec["kw"],
                                       "state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()]})
            for k, v in r32.items():
                store[f"{name}/{geom}::{k}"] = v
    meta = {"cases": {n: list(s["geoms"]) for n, s in CASES.items()},
            "geometries": {g: list(d) for s in CASES.values() for g, d in s["geoms"].items()},
            "args": {n: ARGS[s["kind"]] for n, s in CASES.items()}, "offset_cases": list(OFFSET_CASES), "input_scale": scales}
    store["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    write_npz(os.path.join(OUT, "g13_mha.npz"), store)
    write_contract(os.path.join(OUT, "mha_contract.json"), contract)
    for f in ("g13_mha.npz", "mha_contract.json"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()

"""Golden vectors of the single-query attention ablations (Dot, BiLinear, BiLinearTanh, SelfAttentionICLR2017,
MultiHeadSelfAttentionICLR17OnWord), captured from the upstream reference in the build container -- never on the GPU
machine, and no test reads the reference.

Loads the reference's ``thirdparty/two_branches_attention.py`` and ``thirdparty/self_attention.py`` (they import only
torch and numpy) from the directory ``oracle/_refshim.py`` points at, runs every case in fp32 on the CPU with seeded
weights and inputs, and writes

    tests/golden/g12_attention.npz         every case below in both geometries
    tests/golden/attention_contract.json   class, kwargs and state_dict key / shape lists of every configuration

Geometries: ``b3l12`` (B=3, L=12) and ``b2l70`` (B=2, L=70: a sequence crosses one wave of 64 lanes).  Masks: row 0 has
interior zeros (positions 3 and 5), row 1 suffix padding from 2L/3, and row 2 of the first geometry a single real token
(one-hot weights).  ``dot_offset_pos`` / ``dot_offset_neg``: ``left[:, 0] = +-96`` and ``right[:, :, 0] = 1`` put every
score near +-96 with an O(1) spread -- a softmax without max-subtraction overflows resp. underflows there, while the
gradients stay of ordinary size.

Per case ``<case>/<geometry>::``: the inputs by argument name, ``mask``, every parameter (``param::<name>``), ``out``
(the attended tensor) and ``weights`` (where the class returns them), the seeded upstream gradients ``gout`` and
``gweights`` of the loss sum(out * gout) + sum(weights * gweights), and the gradients of every input
(``grad::<argument>``) and parameter (``grad::<name>``).

Every case also runs in float64, and the reference's own fp32 result must lie within one tenth of the tolerance the GPU
test applies (tests/test_gpu_attention.py), so the fixture never eats the test's margin.

    python tools/make_attention_golden.py
"""
import json
import os
import zlib

import numpy as np
import torch

from golden_common import OUT, load_reference, margin, to_numpy, write_contract, write_npz

GEOMETRIES = {"b3l12": (3, 12), "b2l70": (2, 70)}
D, X = 8, 5
# name -> module file, class, constructor kwargs, input builder key
CASES = {
    "dot_d6": dict(mod="two", cls="Dot", kw={}, inputs="query", d=6),
    "dot_d8": dict(mod="two", cls="Dot", kw={}, inputs="query", d=8),
    "bilinear": dict(mod="two", cls="BiLinear", kw=dict(dim=8), inputs="query", d=8),
    "bilineartanh": dict(mod="two", cls="BiLinearTanh", kw=dict(left_dim=8, right_dim=5, out_dim=7), inputs="seq_query"),
    "selfatt": dict(mod="self", cls="SelfAttentionICLR2017", kw=dict(inp_dim=8, out_dim=7), inputs="seq"),
    "onword_h1": dict(mod="self", cls="MultiHeadSelfAttentionICLR17OnWord", kw=dict(inp_dim=8, out_dim=7, num_heads=1),
                      inputs="onword"),
    "onword_h3": dict(mod="self", cls="MultiHeadSelfAttentionICLR17OnWord", kw=dict(inp_dim=8, out_dim=7, num_heads=3),
                      inputs="onword"),
    "dot_offset_pos": dict(mod="two", cls="Dot", kw={}, inputs="query", d=8, offset=96.0),
    "dot_offset_neg": dict(mod="two", cls="Dot", kw={}, inputs="query", d=8, offset=-96.0),
}
OFFSET_CASES = ("dot_offset_pos", "dot_offset_neg")
# the GPU test's tolerances (elementwise atol + rtol |want|; offset cases: largest error over largest entry)
TOL_OUT, TOL_GRAD, TOL_REL = (1e-4, 1e-4), (1e-5, 1e-4), 1e-4


def make_mask(b, l):
    m = np.ones((b, l), dtype=np.float32)
    m[0, 3] = m[0, 5] = 0.0
    m[1, (2 * l) // 3:] = 0.0
    if b > 2:
        m[2, :] = 0.0
        m[2, 4] = 1.0
    return m


def make_inputs(spec, b, l, g):
    """Ordered (argument name, tensor) pairs of the forward, the mask excluded."""
    r = lambda *s: torch.randn(s, generator=g)
    kind = spec["inputs"]
    if kind == "query":
        left, right = r(b, spec["d"]), r(b, l, spec["d"])
        if "offset" in spec:
            left[:, 0] = spec["offset"]
            right[:, :, 0] = 1.0
        return [("left", left), ("right", right)]
    if kind == "seq_query":
        return [("left_tsr", r(b, l, D)), ("right_tsr", r(b, X))]
    if kind == "seq":
        return [("tsr", r(b, l, D))]
    return [("original", r(b, l, X)), ("tsr", r(b, l, D))]


def forward(m, spec, inputs, mask):
    args = [t for _, t in inputs]
    if spec["inputs"] == "onword":
        return m(*args, mask, return_att_weights=True)
    out = m(*args, mask)
    return out if isinstance(out, tuple) else (out, None)


def run(ref, spec, name, geom, dtype):
    b, l = GEOMETRIES[geom]
    torch.manual_seed(zlib.crc32(f"{name}/{geom}".encode()))
    m = getattr(ref[spec["mod"]], spec["cls"])(**spec["kw"]).to(dtype)
    g = torch.Generator().manual_seed(11 + len(name) + 7 * len(geom))
    inputs = [(k, t.to(dtype).requires_grad_(True)) for k, t in make_inputs(spec, b, l, g)]
    mask = torch.from_numpy(make_mask(b, l))
    out, weights = forward(m, spec, inputs, mask)
    gout = torch.randn(out.shape, generator=g)
    loss = (out * gout.to(dtype)).sum()
    res = {"mask": mask.numpy(), "out": out, "gout": gout}
    if weights is not None:
        gweights = torch.randn(weights.shape, generator=g)
        loss = loss + (weights * gweights.to(dtype)).sum()
        res["weights"], res["gweights"] = weights, gweights
    loss.backward()
    for k, t in inputs:
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
    ref = {"two": load_reference("thirdparty/two_branches_attention.py", "ref_two_branches_attention"),
           "self": load_reference("thirdparty/self_attention.py", "ref_self_attention")}
    torch.set_num_threads(1)
    store, contract = {}, {}
    for name, spec in CASES.items():
        for geom in GEOMETRIES:
            m, r32 = run(ref, spec, name, geom, torch.float32)
            _, r64 = run(ref, spec, name, geom, torch.float64)
            worst = margin_of(name, r32, r64)
            assert worst <= 1.0, (name, geom, worst)
            contract.setdefault(name, {"class": spec["cls"], "kwargs": spec["kw"],
                                       "state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()]})
            for k, v in r32.items():
                store[f"{name}/{geom}::{k}"] = v
    meta = {"cases": list(CASES), "geometries": {k: list(v) for k, v in GEOMETRIES.items()}, "offset_cases": list(OFFSET_CASES)}
    store["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    write_npz(os.path.join(OUT, "g12_attention.npz"), store)
    write_contract(os.path.join(OUT, "attention_contract.json"), contract)
    for f in ("g12_attention.npz", "attention_contract.json"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()

"""Golden vectors of the matchzoo/modules family (Attention, BidirectionalAttention, MatchModule, Matching, GaussianKernel,
StackedBRNN; RNNDropout is the identity in eval mode and has no case), captured from the upstream reference in the build
container -- never on the GPU machine, and no test reads the reference.

The five files matchzoo/modules/{attention,matching,gaussian_kernel,stacked_brnn,dropout}.py are loaded by path
(golden_common.load_reference): they import only torch, so the ``matchzoo`` package and its data pipeline are never imported.
Every case runs in fp32 and in float64, in eval() mode, and the generator writes

    tests/golden/g17_match.npz           every case below
    tests/golden/match_contract.json     class, kwargs and the state_dict key / shape list of every case, in order

Shapes (B, L1, L2, D): s5x3 (3,5,3,6), s21x9 (2,21,9,10), s37x35 (2,37,35,70), s19x40 (2,19,40,20) for ``bidir`` (
BidirectionalAttention), ``match`` (MatchModule, hidden_size D), ``dot`` / ``dotn`` (Matching('dot'), normalize off / on;
``dotn`` runs on the inputs stored under ``dot``), ``att`` (Attention on (B,L1,D) with exact-zero rows at t >= len) and
``gauss`` (GaussianKernel(mu=0.5, sigma=0.1) on values in [-1, 1]); the first two shapes only for ``mul``, ``plus``,
``minus``, ``concat`` (the broadcast outputs are B L1 L2 D large).
``brnn`` (StackedBRNN) as (B, L, D, H, layers, concat, type): lstm2c (3,7,10,6,2,True,LSTM), lstm3 (19,12,8,20,3,False,LSTM: more
than one 16-sequence tile), gru2c (5,9,6,12,2,True,GRU).

Inputs are 0.7 randn rounded to what float16 holds exactly; parameters keep the reference's seeded init (torch.manual_seed(
crc32(key)) right before the constructor), rounded likewise; both are stored as float16.  Upstream gradients are
randint(-16, 17) / 16.  Masks are built from lengths (True at t >= len) with one full-length sequence per side.  Per case
``<family>::<shape>::``: the inputs, ``len1`` / ``len2``, ``param::<name>``, ``out<i>``, ``g<i>``, ``grad::<input or parameter>``.
The gradient of MatchModule's 140 x 280 ``proj.weight`` at s37x35 alone would be a seventh of the archive's 1 MB: every 7th
row of it is stored, as ``grad::proj.weight::rows7`` (the other three shapes store that gradient whole).

The reference's own fp32 result must lie within one tenth of the bound the tests apply: outputs 1e-4 + 1e-4 |want| and
gradients 1e-5 + 1e-4 |want| elementwise, except the gradients of ``bidir`` and ``match``, which are bounded by 1e-4 of the
largest float64 entry of their tensor (softmax cancellation leaves near-zero entries whose fp32 error is relative to the
terms that cancel, not to the entry).

    python tools/make_match_golden.py
"""
import json
import os
import zlib

import numpy as np
import torch
import torch.nn as nn

from golden_common import OUT, load_reference, margin, to_numpy, write_contract, write_npz

SHAPES = {"s5x3": (3, 5, 3, 6), "s21x9": (2, 21, 9, 10), "s37x35": (2, 37, 35, 70), "s19x40": (2, 19, 40, 20)}
LENS = {"s5x3": ([5, 2, 4], [1, 3, 2]), "s21x9": ([21, 10], [4, 9]), "s37x35": ([17, 37], [35, 20]), "s19x40": ([19, 3], [33, 40])}
BCAST_SHAPES = ["s5x3", "s21x9"]
BRNN = {"lstm2c": (3, 7, 10, 6, 2, True, "LSTM"), "lstm3": (19, 12, 8, 20, 3, False, "LSTM"), "gru2c": (5, 9, 6, 12, 2, True, "GRU")}
FAMILIES = ["bidir", "match", "dot", "dotn", "att", "gauss", "mul", "plus", "minus", "concat", "brnn"]
MAX_SCALED = ("bidir", "match")
# the one gradient too large for the archive's 1 MB: every `step`-th row is stored (and compared) instead of the whole tensor
SUBSETS = {"match::s37x35": {"grad::proj.weight": 7}}
TOL_OUT = (1e-4, 1e-4)
TOL_GRAD = (1e-5, 1e-4)
TOL_MAX = 1e-4


def half_exact(t):
    return t.half().float()


def randn(g, *shape):
    return half_exact(0.7 * torch.randn(*shape, generator=g))


def upstream(g, shape):
    return torch.randint(-16, 17, tuple(shape), generator=g).float() / 16


def pad_mask(lens, length):
    return torch.arange(length)[None, :] >= torch.tensor(lens)[:, None]


def build(ref, family, key, shape_name):
    """(module or None, kwargs, inputs in forward order as (name, tensor, differentiable), extra arrays to store)."""
    g = torch.Generator().manual_seed(zlib.crc32(key.replace("dotn::", "dot::").encode()) ^ 0x5EED)      # dotn: the inputs of dot
    torch.manual_seed(zlib.crc32(key.encode()))
    if family == "brnn":
        B, L, D, H, layers, concat, kind = BRNN[shape_name]
        kwargs = dict(input_size=D, hidden_size=H, num_layers=layers, dropout_rate=0.2, dropout_output=True, rnn_type=kind,
                      concat_layers=concat)
        m = ref["StackedBRNN"](**dict(kwargs, rnn_type=getattr(nn, kind)))
        return m, "StackedBRNN", kwargs, [("x", randn(g, B, L, D), True), ("x_mask", torch.zeros(B, L, dtype=torch.bool), False)], {}
    B, L1, L2, D = SHAPES[shape_name]
    len1, len2 = LENS[shape_name]
    assert len(len1) == len(len2) == B and max(len1) == L1 and max(len2) == L2 and min(len1 + len2) >= 1
    m1, m2 = pad_mask(len1, L1), pad_mask(len2, L2)
    extra = {"len1": np.array(len1, np.int32), "len2": np.array(len2, np.int32)}
    if family == "bidir":
        return (ref["BidirectionalAttention"](), "BidirectionalAttention", {},
                [("v1", randn(g, B, L1, D), True), ("v1_mask", m1, False), ("v2", randn(g, B, L2, D), True), ("v2_mask", m2, False)], extra)
    if family == "match":
        kwargs = dict(hidden_size=D, dropout_rate=0.2)
        return (ref["MatchModule"](**kwargs), "MatchModule", kwargs,
                [("v1", randn(g, B, L1, D), True), ("v2", randn(g, B, L2, D), True), ("v2_mask", m2, False)], extra)
    if family == "att":
        kwargs = dict(input_size=D, mask=0)
        x = randn(g, B, L1, D) * (~m1).unsqueeze(2)
        return ref["Attention"](**kwargs), "Attention", kwargs, [("x", x, True)], extra
    if family == "gauss":
        kwargs = dict(mu=0.5, sigma=0.1)
        x = half_exact(2 * torch.rand(B, L1, L2, generator=g) - 1)
        return ref["GaussianKernel"](**kwargs), "GaussianKernel", kwargs, [("x", x, True)], extra
    kwargs = dict(normalize=family == "dotn", matching_type="dot" if family in ("dot", "dotn") else family)
    return (ref["Matching"](**kwargs), "Matching", kwargs, [("x", randn(g, B, L1, D), True), ("y", randn(g, B, L2, D), True)], extra)


def run(ref, family, key, shape_name, dtype):
    m, cls, kwargs, inputs, extra = build(ref, family, key, shape_name)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(half_exact(p))
    m = m.to(dtype).eval()
    args = []
    for _, t, diff in inputs:
        t = t.to(dtype) if t.is_floating_point() else t
        args.append(t.clone().requires_grad_(True) if diff else t)
    outs = m(*args)
    outs = outs if isinstance(outs, tuple) else (outs,)
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()) ^ 0xC0FFEE)
    gs = [upstream(g, o.shape) for o in outs]
    sum((o * u.to(dtype)).sum() for o, u in zip(outs, gs)).backward()
    res = dict(extra)
    for i, (o, u) in enumerate(zip(outs, gs)):
        res[f"out{i}"] = o
        res[f"g{i}"] = u.numpy().astype(np.float16)
        assert np.array_equal(res[f"g{i}"].astype(np.float32), u.numpy())
    for (name, t, diff), a in zip(inputs, args):
        if t.dtype == torch.bool:
            continue
        res[name] = t.numpy().astype(np.float16)
        assert np.array_equal(res[name].astype(np.float32), t.numpy()), name
        if diff:
            res["grad::" + name] = a.grad
    for k, p in m.named_parameters():
        res["grad::" + k] = p.grad
    res = to_numpy(res)
    for k, step in SUBSETS.get(key, {}).items():
        res[f"{k}::rows{step}"] = res.pop(k)[::step]
    for k, v in m.state_dict().items():
        h = v.detach().float().numpy().astype(np.float16)
        assert np.array_equal(h.astype(np.float64), v.detach().double().numpy()), k
        res["param::" + k] = h
    contract = {"class": cls, "kwargs": kwargs, "state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()]}
    return contract, res


def bound_for(family):
    def bound(k, want):
        if k.startswith("out"):
            return TOL_OUT[0] + TOL_OUT[1] * np.abs(want)
        if family in MAX_SCALED:
            return TOL_MAX * np.abs(want).max()
        return TOL_GRAD[0] + TOL_GRAD[1] * np.abs(want)
    return bound


def main():
    ref = {}
    for path, names in (("attention.py", ("Attention", "BidirectionalAttention", "MatchModule")), ("matching.py", ("Matching",)),
                        ("gaussian_kernel.py", ("GaussianKernel",)), ("stacked_brnn.py", ("StackedBRNN",)), ("dropout.py", ("RNNDropout",))):
        mod = load_reference(os.path.join("matchzoo", "modules", path), "_ref_matchzoo_" + path[:-3])
        for n in names:
            ref[n] = getattr(mod, n)
    torch.set_num_threads(1)
    store, contracts, cases = {}, {}, []
    for family in FAMILIES:
        shapes = list(BRNN) if family == "brnn" else (BCAST_SHAPES if family in ("mul", "plus", "minus", "concat") else list(SHAPES))
        for shape_name in shapes:
            key = f"{family}::{shape_name}"
            contract, r32 = run(ref, family, key, shape_name, torch.float32)
            _, r64 = run(ref, family, key, shape_name, torch.float64)
            outs = [k for k in r32 if k.startswith("out")]
            grads = [k for k in r32 if k.startswith("grad::")]
            w_out, w_grad = margin(r32, r64, outs, bound_for(family)), margin(r32, r64, grads, bound_for(family))
            print(f"{key}: fp32 reference at {w_out:.4f} (outputs) and {w_grad:.4f} (gradients) of a tenth of the bound")
            assert w_out <= 1.0 and w_grad <= 1.0, (key, w_out, w_grad)
            assert all(np.isfinite(v.astype(np.float64)).all() for v in r32.values()), key
            contracts[key] = contract
            cases.append(key)
            for k, v in r32.items():
                if not (family == "dotn" and k in ("x", "y")):      # read from dot::<shape>
                    store[f"{key}::{k}"] = v
    store["meta"] = np.frombuffer(json.dumps({"cases": cases}).encode(), dtype=np.uint8)
    write_npz(os.path.join(OUT, "g17_match.npz"), store)
    write_contract(os.path.join(OUT, "match_contract.json"), contracts)
    for f in ("g17_match.npz", "match_contract.json"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")
    assert os.path.getsize(os.path.join(OUT, "g17_match.npz")) < 1024 * 1024


if __name__ == "__main__":
    main()

"""CPU-side checks of the multi-head query/key/value attention family (thirdparty/two_branches_attention.py
ScaledDotProductAttention, MultiHeadAttentionOriginal, ConcatNotEqualSelfAttTransFormer, MultiHeadAttentionSimple,
CoDaAttention): the install() shim exports them, their constructors build the reference's state_dict for every
configuration in tests/golden/mha_contract.json, the golden archive g13_mha.npz is complete, the modules refuse CPU
tensors, and the float64 restatements the GPU tests compare the kernels with (tests/mha_ref.py) reproduce the archive on
their own while keeping the exact-zero conventions."""
import os

import numpy as np
import pytest
import torch

from tests.mha_ref import module64, sdpa64
from tests.util import golden_ratio, load_golden, rel_close, run_in_fresh_interpreter

CASES = {"sdpa_3x5": {"n2q3k5": [2, 3, 5]}, "sdpa_35x70": {"n2q35k70": [2, 35, 70]},
         "sdpa_offset_pos": {"n2q3k12": [2, 3, 12]}, "sdpa_offset_neg": {"n2q3k12": [2, 3, 12]},
         "mha_orig_h3": {"b2q3k5": [2, 3, 5], "b2q17k70": [2, 17, 70]},
         "mha_orig_h1": {"b2q5k5": [2, 5, 5], "b2q70k70": [2, 70, 70]},
         "transformer_concat": {"b3l12": [3, 12], "b2l70": [2, 70]},
         "mha_simple_h3": {"b3l12": [3, 12], "b2l70": [2, 70]},
         "mha_simple_h3_ln": {"b3l12": [3, 12], "b2l70": [2, 70]}}
NO_WEIGHTS = ("mha_orig_h3", "mha_orig_h1")


def _archive(golden_dir):
    return load_golden(golden_dir, "g13_mha.npz", "mha_contract.json")


def test_install_shim_exports_the_multi_head_family(tmp_path):
    run_in_fresh_interpreter(tmp_path, r"""
from thirdparty.two_branches_attention import *
from get_amd import modules
assert ScaledDotProductAttention is modules.ScaledDotProductAttention
assert MultiHeadAttentionOriginal is modules.MultiHeadAttentionOriginal
assert ConcatNotEqualSelfAttTransFormer is modules.ConcatNotEqualSelfAttTransFormer
assert MultiHeadAttentionSimple is modules.MultiHeadAttentionSimple
assert CoDaAttention is modules.CoDaAttention
assert CoDaAttention(4)(1, 2) is None and not list(CoDaAttention(4).parameters())
""")


def test_mha_state_dicts_match_the_reference_contract(golden_dir):
    from get_amd import modules
    _, _, contract = _archive(golden_dir)
    assert set(contract) == set(CASES)
    assert {c["class"] for c in contract.values()} == {"ScaledDotProductAttention", "MultiHeadAttentionOriginal",
                                                       "ConcatNotEqualSelfAttTransFormer", "MultiHeadAttentionSimple"}
    for name, c in contract.items():
        m = getattr(modules, c["class"])(**c["kwargs"])
        got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert got == c["state_dict"], name
    keys = [k for k, _ in contract["mha_orig_h3"]["state_dict"]]
    assert keys == ["w_qs.weight", "w_qs.bias", "w_ks.weight", "w_ks.bias", "w_vs.weight", "w_vs.bias", "layer_norm.weight",
                    "layer_norm.bias", "fc.weight", "fc.bias"]
    keys = [k for k, _ in contract["mha_simple_h3_ln"]["state_dict"]]
    assert keys[6:8] == ["attention_func.linear1.weight", "attention_func.linear2.weight"] and keys[-2:] == \
        ["layer_norm.weight", "layer_norm.bias"]
    with pytest.raises(AssertionError):
        modules.MultiHeadAttentionSimple(2, 8, 8, 4)
    m = modules.MultiHeadAttentionSimple(2, 8, 8, 8, init_weights=True)
    assert not hasattr(m, "layer_norm") and m.fc.weight.shape == (8, 16)


def test_mha_golden_archive_is_complete(golden_dir):
    z, meta, contract = _archive(golden_dir)
    assert meta["cases"] == {k: list(v) for k, v in CASES.items()}
    assert meta["geometries"] == {g: d for v in CASES.values() for g, d in v.items()}
    assert set(meta["offset_cases"]) == {"sdpa_offset_pos", "sdpa_offset_neg"}
    for name, geoms in CASES.items():
        for geom, dims in geoms.items():
            key = f"{name}/{geom}::"
            have = {k[len(key):] for k in z if k.startswith(key)}
            assert {"mask", "out", "gout"} <= have, key
            if name in NO_WEIGHTS:
                assert "weights" not in have
            else:
                assert {"weights", "gweights"} <= have, key
            for k in have:
                if k.startswith("param::"):
                    assert "grad::" + k[len("param::"):] in have, key + k
            assert {k[len("param::"):] for k in have if k.startswith("param::")} == {k for k, _ in contract[name]["state_dict"]}
            args = meta["args"][name]
            assert all(a in have and "grad::" + a in have for a in args), (key, args)
            mask = z[key + "mask"]
            if name.startswith(("sdpa", "mha_orig")):
                assert mask.dtype == np.bool_ and list(mask.shape) == dims
                assert mask.all(-1).any(), key + ": no fully masked row"
            elif name == "transformer_concat":
                assert mask.dtype == np.bool_ and list(mask.shape) == [dims[0], 1, dims[1]] and not mask.all(-1).any()
            else:
                assert list(mask.shape) == dims and (mask != 0).any(-1).all()
    single = ~z["sdpa_3x5/n2q3k5::mask"]
    assert (single.sum(-1) == 1).any()
    for k in z:
        if k != "meta":
            assert np.isfinite(z[k]).all(), k
    assert os.path.getsize(os.path.join(golden_dir, "g13_mha.npz")) < 1 << 20


def test_mha_modules_refuse_cpu_tensors():
    from get_amd import modules, ops
    mask = torch.zeros(2, 3, 4, dtype=torch.bool)
    x = torch.zeros(2, 3, 8)
    kv = torch.zeros(2, 4, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        modules.ScaledDotProductAttention(1.0)(x, kv, kv, mask)
    with pytest.raises(RuntimeError, match="no CPU path"):
        modules.MultiHeadAttentionOriginal(2, 8, 4, 4)(x, kv, kv, mask)
    with pytest.raises(RuntimeError, match="no CPU path"):
        modules.ConcatNotEqualSelfAttTransFormer(16, 8)(torch.zeros(2, 1, 8), kv, kv, torch.zeros(2, 1, 4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU path"):
        modules.MultiHeadAttentionSimple(2, 8, 8, 8)(torch.zeros(2, 8), kv, torch.ones(2, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.mha_sdpa(x, kv, kv, mask, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.add_layernorm(x, None, torch.ones(8), torch.zeros(8), 1e-5)
    with pytest.raises(TypeError):
        modules.ScaledDotProductAttention(1.0)(x, kv, kv, None)
    with pytest.raises(TypeError):
        modules.MultiHeadAttentionOriginal(2, 8, 4, 4)(x, kv, kv)


def test_transformer_concat_refuses_a_multi_row_query():
    from get_amd import modules
    m = modules.ConcatNotEqualSelfAttTransFormer(16, 8)
    kv = torch.zeros(2, 4, 8)
    with pytest.raises(RuntimeError, match="single query row"):
        m(torch.zeros(2, 4, 8), kv, kv, torch.zeros(2, 1, 4, dtype=torch.bool))


def _run64(z, meta, contract, name, geom):
    key = f"{name}/{geom}::"
    c = contract[name]
    p64 = {k[len(key) + len("param::"):]: torch.from_numpy(z[k]).double().requires_grad_(True)
           for k in z if k.startswith(key + "param::")}
    in64 = {a: torch.from_numpy(z[key + a]).double().requires_grad_(True) for a in dict.fromkeys(meta["args"][name])}
    out, weights = module64(c["class"], c["kwargs"], p64, [in64[a] for a in meta["args"][name]], torch.from_numpy(z[key + "mask"]))
    loss = (out * torch.from_numpy(z[key + "gout"]).double()).sum()
    if weights is not None:
        loss = loss + (weights * torch.from_numpy(z[key + "gweights"]).double()).sum()
    loss.backward()
    return key, p64, in64, out, weights


def test_float64_restatements_reproduce_the_mha_goldens(golden_dir):
    """tests/mha_ref.py alone, in float64 on the archive's inputs and parameters, against every captured output, weight and
    gradient at the GPU golden test's bounds: 1e-4 + 1e-4 |want| for outputs and weights, 1e-5 + 1e-4 |want| for gradients,
    the two offset cases by largest error over largest entry <= 1e-4."""
    z, meta, contract = _archive(golden_dir)
    worst, checked = 0.0, set()
    for name, geoms in meta["cases"].items():
        for geom in geoms:
            key, p64, in64, out, weights = _run64(z, meta, contract, name, geom)
            checks = [("out", out, 1e-4)] + ([("weights", weights, 1e-4)] if weights is not None else [])
            checks += [("grad::" + k, t.grad, 1e-5) for k, t in in64.items()]
            checks += [("grad::" + k, t.grad, 1e-5) for k, t in p64.items()]
            for k, got, atol in checks:
                if name in meta["offset_cases"]:
                    rel_close(got, z[key + k], 1e-4, key + k)
                else:
                    worst = max(worst, golden_ratio(got, z[key + k], atol, 1e-4, key + k))
                checked.add(key + k)
    recorded = {k for k in z if k.split("::", 1)[-1].split("::")[0] in ("out", "weights", "grad")}
    assert checked == recorded, sorted(recorded ^ checked)
    print(f"g13_mha.npz: worst ratio of the bound {worst:.3f}")


def test_restatements_keep_the_exact_zero_conventions(golden_dir):
    """Masked weights are exactly 0.0, a fully masked row has all-zero weights, an all-zero output row and sends exactly zero
    gradient to its query row; nothing is NaN -- in the restatement as in the archive."""
    z, meta, contract = _archive(golden_dir)
    for name in ("sdpa_3x5", "sdpa_35x70"):
        (geom,) = meta["cases"][name]
        key, _, in64, out, weights = _run64(z, meta, contract, name, geom)
        mask = torch.from_numpy(z[key + "mask"])
        dead = mask.all(-1)
        assert dead.any()
        for w, o, dq in ((weights.detach(), out.detach(), in64["query"].grad),
                         (torch.from_numpy(z[key + "weights"]), torch.from_numpy(z[key + "out"]),
                          torch.from_numpy(z[key + "grad::query"]))):
            assert bool((w[mask] == 0).all()) and bool((o[dead] == 0).all()) and bool((dq[dead] == 0).all())
            live = w.sum(-1)[~dead]
            assert float((live - 1).abs().max()) <= 1e-5
        for t in list(in64.values()):
            assert bool(torch.isfinite(t.grad).all())
    # every head sees the same mask, head-major weights
    q, k, v = torch.randn(2, 3, 8).double(), torch.randn(2, 5, 8).double(), torch.randn(2, 5, 12).double()
    mask = torch.zeros(2, 3, 5, dtype=torch.bool)
    mask[1, 2] = True
    out, w = sdpa64(q, k, v, mask, 4)
    assert w.shape == (8, 3, 5) and bool((w.reshape(4, 2, 3, 5)[:, 1, 2] == 0).all()) and bool((out[1, 2] == 0).all())
    one, w1 = sdpa64(q[..., 2:4], k[..., 2:4], v[..., 3:6], mask, 1)
    assert torch.allclose(out[..., 3:6], one) and torch.allclose(w.reshape(4, 2, 3, 5)[1], w1)

"""CPU-side checks of the single-query attention ablations (thirdparty/two_branches_attention.py Dot, BiLinear,
BiLinearTanh; thirdparty/self_attention.py SelfAttentionICLR2017, MultiHeadSelfAttentionICLR17OnWord, SelfAttentionType):
the install() shim exports them under the reference's module paths, their constructors build the reference's state_dict
for every configuration captured in tests/golden/attention_contract.json, the golden archive is complete, and the float64
restatements the GPU tests compare the kernels with (tests/util.py) reproduce that archive on their own."""
import numpy as np
import pytest
import torch

from tests.util import _module64, golden_ratio, load_golden, run_in_fresh_interpreter


def test_install_shim_exports_the_attention_ablations(tmp_path):
    run_in_fresh_interpreter(tmp_path, r"""
from thirdparty.two_branches_attention import Dot, BiLinear, BiLinearTanh, ConcatNotEqualSelfAtt, ConcatSelfAtt
from thirdparty.self_attention import (SelfAttentionICLR2017, MultiHeadSelfAttentionICLR17OnWord, SelfAttentionType,
                                       MultiHeadSelfAttentionICLR2017Extend)
from get_amd import modules
assert Dot is modules.Dot and BiLinear is modules.BiLinear and BiLinearTanh is modules.BiLinearTanh
assert SelfAttentionICLR2017 is modules.SelfAttentionICLR2017
assert MultiHeadSelfAttentionICLR17OnWord is modules.MultiHeadSelfAttentionICLR17OnWord
assert ConcatNotEqualSelfAtt is modules.ConcatNotEqualSelfAtt and ConcatSelfAtt is modules.ConcatSelfAtt
assert MultiHeadSelfAttentionICLR2017Extend is modules.MultiHeadSelfAttentionICLR2017Extend
assert int(SelfAttentionType.MultiHeadAttentionTanh) == 1 and int(SelfAttentionType.MultiHeadAttentionTransformer) == 2
assert [t.name for t in SelfAttentionType] == ['MultiHeadAttentionTanh', 'MultiHeadAttentionTransformer']
""")


def test_attention_state_dicts_match_the_reference_contract(golden_dir):
    from get_amd import modules
    _, _, contract = load_golden(golden_dir, "g12_attention.npz", "attention_contract.json")
    assert {c["class"] for c in contract.values()} == {"Dot", "BiLinear", "BiLinearTanh", "SelfAttentionICLR2017",
                                                       "MultiHeadSelfAttentionICLR17OnWord"}
    for name, c in contract.items():
        m = getattr(modules, c["class"])(**c["kwargs"])
        got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert got == c["state_dict"], name


def test_self_attention_keeps_the_constructors_head_count():
    from get_amd import modules
    m = modules.SelfAttentionICLR2017(8, 7, num_heads=3)
    assert m.linear2.weight.shape == (3, 7) and m.linear1.weight.shape == (7, 8) and m.linear1.bias is None
    t = modules.BiLinearTanh(8, 5, 7)
    assert t.left_linear.bias is not None and t.right_linear.bias is None and t.combine.weight.shape == (1, 7)


def test_attention_modules_refuse_cpu_tensors():
    from get_amd import modules
    mask = torch.ones(2, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        modules.Dot()(torch.zeros(2, 8), torch.zeros(2, 4, 8), mask)
    with pytest.raises(RuntimeError, match="no CPU path"):
        modules.BiLinear(8)(torch.zeros(2, 8), torch.zeros(2, 4, 8), mask)
    with pytest.raises(RuntimeError, match="no CPU path"):
        modules.BiLinearTanh(8, 5, 7)(torch.zeros(2, 4, 8), torch.zeros(2, 5), mask)
    with pytest.raises(RuntimeError, match="no CPU path"):
        modules.SelfAttentionICLR2017(8, 7)(torch.zeros(2, 4, 8), mask)
    with pytest.raises(RuntimeError, match="no CPU path"):
        modules.MultiHeadSelfAttentionICLR17OnWord(8, 7, 2)(torch.zeros(2, 4, 5), torch.zeros(2, 4, 8), mask)


def test_attention_golden_archive_is_complete(golden_dir):
    z, meta, contract = load_golden(golden_dir, "g12_attention.npz", "attention_contract.json")
    assert set(meta["cases"]) == {"dot_d6", "dot_d8", "bilinear", "bilineartanh", "selfatt", "onword_h1", "onword_h3",
                                  "dot_offset_pos", "dot_offset_neg"}
    assert meta["geometries"] == {"b3l12": [3, 12], "b2l70": [2, 70]}
    assert set(contract) == set(meta["cases"])
    for name in meta["cases"]:
        for geom, (b, l) in meta["geometries"].items():
            key = f"{name}/{geom}::"
            have = {k[len(key):] for k in z if k.startswith(key)}
            assert {"mask", "out", "gout"} <= have, key
            assert z[key + "mask"].shape == (b, l)
            if name != "selfatt":          # the only class that returns no weights
                assert {"weights", "gweights"} <= have, key
            # a gradient for every input and parameter
            for k in have:
                if k.startswith("param::"):
                    assert "grad::" + k[len("param::"):] in have, key + k
            inputs = have - {"mask", "out", "gout", "weights", "gweights"} - {k for k in have if "::" in k}
            assert inputs and all("grad::" + k in have for k in inputs), (key, inputs)
    for k in z:
        if k != "meta":
            assert np.isfinite(z[k]).all(), k


ARGS = {"Dot": ("left", "right"), "BiLinear": ("left", "right"), "BiLinearTanh": ("left_tsr", "right_tsr"),
        "SelfAttentionICLR2017": ("tsr",), "MultiHeadSelfAttentionICLR17OnWord": ("original", "tsr")}


def test_float64_restatements_reproduce_the_attention_goldens(golden_dir):
    """_query64 / _tanh64 / _module64 alone, in float64 on the archive's inputs and parameters, against every captured
    output, weight and gradient at the GPU golden test's elementwise bounds (1e-4 + 1e-4 |want| for outputs and weights,
    1e-5 + 1e-4 |want| for gradients), the offset cases included."""
    z, meta, contract = load_golden(golden_dir, "g12_attention.npz", "attention_contract.json")
    worst, checked = 0.0, set()
    for name in meta["cases"]:
        cls = contract[name]["class"]
        for geom in meta["geometries"]:
            key = f"{name}/{geom}::"
            p64 = {k[len(key) + len("param::"):]: torch.from_numpy(z[k]).double().requires_grad_(True)
                   for k in z if k.startswith(key + "param::")}
            in64 = [torch.from_numpy(z[key + k]).double().requires_grad_(True) for k in ARGS[cls]]
            out, weights = _module64(cls, p64, in64, torch.from_numpy(z[key + "mask"]))
            loss = (out * torch.from_numpy(z[key + "gout"]).double()).sum()
            if weights is not None:
                loss = loss + (weights * torch.from_numpy(z[key + "gweights"]).double()).sum()
            loss.backward()
            checks = [("out", out, 1e-4)] + ([("weights", weights, 1e-4)] if weights is not None else [])
            checks += [("grad::" + k, t.grad, 1e-5) for k, t in zip(ARGS[cls], in64)]
            checks += [("grad::" + k, t.grad, 1e-5) for k, t in p64.items()]
            for k, got, atol in checks:
                worst = max(worst, golden_ratio(got, z[key + k], atol, 1e-4, key + k))
                checked.add(key + k)
    recorded = {k for k in z if k.split("::", 1)[-1].split("::")[0] in ("out", "weights", "grad")}
    assert checked == recorded, sorted(recorded ^ checked)
    print(f"g12_attention.npz: worst ratio of the bound {worst:.3f}")

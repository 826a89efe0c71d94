"""CPU-side checks of the matchzoo/modules drop-ins: the float64 restatements the GPU tests compare the kernels with
(tests/match_ref.py) reproduce the reference's goldens on their own, install() serves ``matchzoo.modules`` (without
BertModule), the constructors build the reference's state_dict (keys, order, shapes) and draw what the reference draws from a
seed, an unknown matching type or recurrent class raises at construction, and the new ops refuse CPU tensors."""
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.match_ref import check_golden, golden_args, golden_params, restate64
from tests.util import load_golden, run_in_fresh_interpreter

SHAPES = ["s5x3", "s21x9", "s37x35", "s19x40"]
CASES = ([f"{fam}::{s}" for fam in ("bidir", "match", "dot", "dotn", "att", "gauss") for s in SHAPES]
         + [f"{fam}::{s}" for fam in ("mul", "plus", "minus", "concat") for s in SHAPES[:2]]
         + [f"brnn::{s}" for s in ("lstm2c", "lstm3", "gru2c")])
RNN_KEYS = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse",
            "bias_ih_l0_reverse", "bias_hh_l0_reverse"]


def _archive(golden_dir):
    return load_golden(golden_dir, "g17_match.npz", "match_contract.json")


def build_dropin(contract_entry):
    """The get_amd.modules class of a contract entry from its kwargs (StackedBRNN's rnn_type is stored by name)."""
    from get_amd import modules
    kwargs = dict(contract_entry["kwargs"])
    if "rnn_type" in kwargs:
        kwargs["rnn_type"] = getattr(nn, kwargs["rnn_type"])
    return getattr(modules, contract_entry["class"])(**kwargs)


def test_match_golden_archive_is_complete(golden_dir):
    z, meta, contract = _archive(golden_dir)
    assert meta["cases"] == CASES and set(contract) == set(CASES)
    dims = {"s5x3": (3, 5, 3, 6), "s21x9": (2, 21, 9, 10), "s37x35": (2, 37, 35, 70), "s19x40": (2, 19, 40, 20)}
    for key in CASES:
        family, shape = key.split("::")
        args = golden_args(z, key)
        assert f"{key}::out0" in z and f"{key}::g0" in z and z[f"{key}::out0"].shape == z[f"{key}::g0"].shape, key
        for name, t, diff in args:
            assert (f"{key}::grad::{name}" in z) == diff, (key, name)
        params = golden_params(z, key)
        assert {k: s for k, s in contract[key]["state_dict"]} == {k: list(v.shape) for k, v in params.items()}, key
        for k in params:
            assert any(n.startswith(f"{key}::grad::{k}") for n in z), (key, k)
        if family == "brnn":
            continue
        B, L1, L2, D = dims[shape]
        l1, l2 = z[f"{key}::len1"], z[f"{key}::len2"]
        assert len(l1) == len(l2) == B and l1.max() == L1 and l2.max() == L2 and l1.min() >= 1 and l2.min() >= 1
        assert len(set(l1)) > 1 and len(set(l2)) > 1                       # ragged on both sides
        assert args[0][1].shape == ((B, L1, L2) if family == "gauss" else (B, L1, D))
        if family == "att":                                                # exact-zero rows at t >= len, and only there
            zero = (args[0][1] == 0).all(dim=2)
            assert torch.equal(zero, torch.arange(L1)[None, :] >= torch.from_numpy(l1.astype(np.int64))[:, None])
        if family == "gauss":
            assert float(args[0][1].abs().max()) <= 1.0 and contract[key]["kwargs"] == {"mu": 0.5, "sigma": 0.1}
    assert z["bidir::s37x35::out0"].shape == (2, 37, 70) and z["bidir::s37x35::out1"].shape == (2, 35, 70)
    assert z["match::s37x35::out0"].shape == (2, 37, 140) and z["concat::s21x9::out0"].shape == (2, 21, 9, 20)
    assert z["brnn::lstm2c::out0"].shape == (3, 7, 24) and z["brnn::lstm3::out0"].shape == (19, 12, 40)
    assert z["brnn::gru2c::out0"].shape == (5, 9, 48)
    assert z["match::s37x35::grad::proj.weight::rows7"].shape == (20, 280) and "match::s37x35::grad::proj.weight" not in z
    assert os.path.getsize(os.path.join(golden_dir, "g17_match.npz")) < 1024 * 1024


@pytest.mark.parametrize("key", CASES)
def test_float64_restatement_reproduces_the_match_goldens(golden_dir, key):
    """tests/match_ref.py alone, in float64 on the archive's inputs and parameters, at the golden bounds (check_golden)."""
    z, _, contract = _archive(golden_dir)
    family = key.split("::")[0]
    p64 = {k: v.double().requires_grad_(True) for k, v in golden_params(z, key).items()}
    named = golden_args(z, key)
    args = [t.double().requires_grad_(True) if diff else t for _, t, diff in named]
    outs = restate64(family, contract[key]["kwargs"], p64, args)
    sum((o * torch.from_numpy(z[f"{key}::g{i}"].astype(np.float64))).sum() for i, o in enumerate(outs)).backward()
    grads = {name: a.grad for (name, _, diff), a in zip(named, args) if diff}
    grads.update({k: v.grad for k, v in p64.items()})
    assert check_golden(z, key, outs, grads) == len(grads)


def test_match_state_dicts_match_the_reference_contract(golden_dir):
    z, _, contract = _archive(golden_dir)
    for key in CASES:
        m = build_dropin(contract[key])
        assert type(m).__module__ == "get_amd.modules" and type(m).__name__ == contract[key]["class"]
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == contract[key]["state_dict"], key
        m.load_state_dict(golden_params(z, key), strict=True)
    from get_amd import modules
    assert list(modules.MatchModule(6).state_dict()) == ["v2_proj.weight", "v2_proj.bias", "proj.weight", "proj.bias"]
    assert list(modules.Attention().state_dict()) == ["linear.weight"] and modules.Attention().linear.weight.shape == (1, 100)
    m = modules.StackedBRNN(5, 3, 2, rnn_type=nn.GRU)
    assert list(m.state_dict()) == [f"rnns.{i}.{k}" for i in range(2) for k in RNN_KEYS]
    assert m.rnns[1].weight_ih_l0.shape == (9, 6) and m.last_seeds == [None, None]
    # the reference's defaults
    m = modules.MatchModule(4)
    assert m.dropout.p == 0 and m.last_seed is None
    k = modules.GaussianKernel()
    assert (k.mu, k.sigma) == (1.0, 1.0)
    mt = modules.Matching()
    assert (mt._normalize, mt._matching_type) == (False, "dot")
    d = modules.RNNDropout(0.3)
    assert isinstance(d, nn.Dropout) and d.p == 0.3 and d.last_seed is None
    x = torch.randn(2, 3, 4)
    assert d.eval()(x) is x                                               # eval mode: the input values


@pytest.mark.parametrize("key", ["match::s21x9", "att::s5x3", "brnn::lstm2c", "brnn::gru2c"])
def test_seeded_construction_draws_what_the_reference_draws(golden_dir, key):
    """The generator seeds torch with crc32(case key) right before it builds the reference's module; the same seed here gives
    the same parameters (rounded to float16, as the archive stores them)."""
    z, _, contract = _archive(golden_dir)
    torch.manual_seed(zlib.crc32(key.encode()))
    m = build_dropin(contract[key])
    sd = m.state_dict()
    assert len(sd) > 0
    for k, v in sd.items():
        assert np.array_equal(v.numpy().astype(np.float16), z[f"{key}::param::{k}"]), k


def test_install_serves_matchzoo_modules_without_bert(tmp_path):
    names = ["Attention", "BidirectionalAttention", "MatchModule", "RNNDropout", "StackedBRNN", "GaussianKernel", "Matching"]
    body = "import matchzoo.modules as mm\n" + "".join(
        f"from matchzoo.modules import {n}\nassert {n} is M.{n} and {n}.__module__ == 'get_amd.modules'\n" for n in names)
    body += ("try:\n    from matchzoo.modules import BertModule\nexcept ImportError:\n    pass\nelse:\n"
             "    raise AssertionError('BertModule must not be served')\n"
             "import torch\nassert mm.torch is torch and mm.nn is torch.nn\n")
    run_in_fresh_interpreter(tmp_path, body, packages=("matchzoo",))


def test_wrong_constructor_arguments_raise():
    from get_amd import modules
    with pytest.raises(ValueError, match="x is not a valid matching type"):
        modules.Matching(matching_type="x")
    with pytest.raises(TypeError, match="RNN"):
        modules.StackedBRNN(4, 3, 1, rnn_type=nn.RNN)
    for t in ("dot", "mul", "plus", "minus", "concat"):
        modules.Matching(matching_type=t)


def test_match_ops_refuse_cpu_tensors():
    from get_amd import modules, ops
    x, y = torch.zeros(2, 5, 4), torch.zeros(2, 3, 4)
    fill = torch.zeros(2, 3, dtype=torch.bool)
    calls = [lambda: ops.soft_align(x, y, y, fill), lambda: ops.lin_att(x, torch.zeros(1, 4)), lambda: ops.match_dot(x, y),
             lambda: ops.match_dot(x, y, normalize=True), lambda: ops.match_bcast(x, y, "mul"), lambda: ops.gauss_kernel(x, 1.0, 1.0),
             lambda: modules.BidirectionalAttention()(x, torch.zeros(2, 5, dtype=torch.bool), y, fill),
             lambda: modules.MatchModule(4)(x, y, fill), lambda: modules.Attention(4)(x), lambda: modules.Matching()(x, y),
             lambda: modules.GaussianKernel()(x), lambda: modules.RNNDropout(0.5)(x), lambda: modules.StackedBRNN(4, 3, 1)(x, fill)]
    for i, f in enumerate(calls):
        with pytest.raises(RuntimeError, match="no CPU path"):
            f()
    with pytest.raises(ValueError, match="match_bcast"):
        ops.match_bcast(x, y, "times")
    with pytest.raises(RuntimeError, match="boolean masks"):            # before anything touches the device
        modules.BidirectionalAttention()(x, torch.zeros(2, 5), y, fill)

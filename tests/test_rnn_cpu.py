"""CPU-side checks of the two sequence encoders (Models/BiDAF/wrapper.py: LSTM :229-276, GRU :279-327), once per cell: the
float64 restatement the GPU tests compare the kernels with (tests/rnn_ref.py) reproduces the reference's goldens on its own,
the drop-in's constructor builds the reference's state_dict for every configuration in tests/golden/lstm_contract.json /
gru_contract.json and initialises a stand-alone module as the reference does (the GRU: as the reference's constructor does
once its one raising line runs), the C-ABI declares and binds the two recurrence entries, the shim exports the classes, and
the modules refuse CPU tensors."""
import os
import re

import numpy as np
import pytest
import torch

from tests.rnn_ref import CELLS
from tests.util import golden_ratio, load_golden, run_in_fresh_interpreter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["bi_b5", "bi_b5_max25", "uni_h5", "two_layers", "bi_b37", "bi_l70", "bi_b5_saturated"]


@pytest.fixture(params=list(CELLS))
def cell(request):
    return CELLS[request.param]


def _cls(cell):
    from get_amd import modules
    return getattr(modules, cell.module)


def _archive(golden_dir, cell):
    return load_golden(golden_dir, cell.archive, cell.contract)


def _params(z, name):
    key = f"{name}::param::"
    return {k[len(key):]: torch.from_numpy(z[k]) for k in z if k.startswith(key)}


def test_golden_archive_is_complete(golden_dir, cell):
    z, meta, contract = _archive(golden_dir, cell)
    assert meta["cases"] == CASES and set(contract) == set(CASES)
    for name in CASES:
        have = {k[len(name) + 2:] for k in z if k.startswith(name + "::")}
        assert {"x", "lens", "new_indices", "restoring_indices", "y", "h", "gy", "gh", "grad::x"} <= have, name
        names = [k for k, _ in contract[name]["state_dict"]]
        assert {k[len("param::"):] for k in have if k.startswith("param::")} == set(names)
        assert all("grad::" + k in have for k in names)
        new, rest = z[name + "::new_indices"], z[name + "::restoring_indices"]
        assert (new[rest] == np.arange(len(new))).all()                      # inverse permutations
        assert (np.diff(z[name + "::lens"][new]) <= 0).all()                 # sorted by descending length
        for k in names:                                                       # biases non-zero and distinct
            if "bias_ih" in k:
                bi, bh = z[f"{name}::param::{k}"], z[f"{name}::param::{k.replace('bias_ih', 'bias_hh')}"]
                assert (bi != 0).all() and (bh != 0).all() and (bi != bh).all()
    assert list(z["bi_b5::lens"]) == [21, 9, 9, 1, 14] and z["bi_b5_max25::y"].shape == (5, 25, 16)
    assert (z["bi_b5_max25::y"][:, 21:] == 0).all()
    assert np.array_equal(z["bi_b5_saturated::x"], np.float32(30.0) * z["bi_b5::x"])
    assert "bi_b37::h_raw" in z and z["bi_b37::h_raw"].shape == (2, 37, 12)
    assert os.path.getsize(os.path.join(golden_dir, cell.archive)) < 300 * 1024


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_reproduces_the_goldens(golden_dir, cell, name):
    """tests/rnn_ref.py alone, in float64 on the archive's inputs and parameters: y, h and every gradient within
    1e-5 + 1e-4 |want| of the reference's fp32 results."""
    z, _, contract = _archive(golden_dir, cell)
    c = contract[name]
    p64 = {k: v.double().requires_grad_(True) for k, v in _params(z, name).items()}
    x = torch.from_numpy(z[name + "::x"]).double().requires_grad_(True)
    lens = torch.from_numpy(z[name + "::lens"])
    T = c["max_len"] or int(lens.max())
    y, h = cell.ref64(p64, x, lens, T, c["kwargs"].get("num_layers", 1), c["kwargs"].get("bidirectional", False))
    ((y * torch.from_numpy(z[name + "::gy"]).double()).sum() + (h * torch.from_numpy(z[name + "::gh"]).double()).sum()).backward()
    worst = 0.0
    for k, got in [("y", y), ("h", h), ("grad::x", x.grad)] + [("grad::" + k, v.grad) for k, v in p64.items()]:
        worst = max(worst, golden_ratio(got, z[f"{name}::{k}"], 1e-5, 1e-4, f"{name}::{k}"))
    if name == "bi_b37":      # the raw second value of return_h=False: (layers * dirs, B, H) in the sorted order
        raw = h.detach().view(37, 2, 12).permute(1, 0, 2)[:, torch.from_numpy(z[name + "::new_indices"])]
        worst = max(worst, golden_ratio(raw, z[name + "::h_raw"], 1e-5, 1e-4, name + "::h_raw"))
    print(f"{name}: worst ratio of the bound {worst:.3f}")
    # padding: exact zeros in y and in the gradient of x at t >= len
    dead = torch.arange(y.shape[1])[None, :] >= lens[:, None]
    assert bool((y.detach()[dead] == 0).all()) and bool((x.grad[dead[:, :x.shape[1]]] == 0).all())


def test_state_dicts_match_the_reference_contract(golden_dir, cell):
    z, _, contract = _archive(golden_dir, cell)
    for name, c in contract.items():
        m = _cls(cell)(**c["kwargs"])
        assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == c["state_dict"], name
        m.load_state_dict({"rnn." + k if not k.startswith("rnn.") else k: v for k, v in _params(z, name).items()}, strict=True)
        assert torch.equal(m.rnn.weight_hh_l0, torch.from_numpy(z[name + "::param::rnn.weight_hh_l0"]))
    assert [k for k, _ in contract["bi_b5"]["state_dict"]] == [
        "rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0", "rnn.bias_hh_l0",
        "rnn.weight_ih_l0_reverse", "rnn.weight_hh_l0_reverse", "rnn.bias_ih_l0_reverse", "rnn.bias_hh_l0_reverse"]


def test_stand_alone_lstm_initialises_as_the_reference():
    """reset_params (wrapper.py:241-254): zero biases, weight_hh with orthonormal columns, per layer and direction."""
    from get_amd import modules
    torch.manual_seed(3)
    m = modules.LSTM(12, 8, num_layers=2, bidirectional=True)
    seen = 0
    for k, p in m.named_parameters():
        if "bias" in k:
            assert bool((p == 0).all()), k
        elif "weight_hh" in k:
            w = p.detach().double()
            assert float((w.t() @ w - torch.eye(8, dtype=torch.float64)).abs().max()) <= 1e-5, k
            seen += 1
    assert seen == 4 and isinstance(m.dropout, torch.nn.Dropout) and m.dropout.p == 0.2
    # the model keeps nn.LSTM's own init for its two encoders (its seeded construction is unchanged): biases are not zeroed
    torch.manual_seed(3)
    keep = modules.LSTM(12, 8, bidirectional=True, _reset_params=False)
    assert bool((keep.rnn.bias_ih_l0 != 0).any())


def test_stand_alone_gru_initialises_as_described():
    """reset_params (wrapper.py:291-304 under no_grad): zero bias_ih, weight_hh with orthonormal columns, bias_hh equal to 1
    exactly on chunk(4)[1] of the 3H-vector -- elements [ceil(3H/4), 2 ceil(3H/4)), straddling the r and z thirds -- and 0
    elsewhere, per layer and direction."""
    from get_amd import modules
    torch.manual_seed(3)
    for H in (8, 5):       # 3H = 24: pieces of 6; 3H = 15: pieces of 4, 4, 4, 3
        m = modules.GRU(12, H, num_layers=2, bidirectional=True)
        q = -(-3 * H // 4)
        seen = 0
        for k, p in m.named_parameters():
            assert p.requires_grad and p.is_leaf, k
            if "bias_ih" in k:
                assert bool((p == 0).all()), k
            elif "bias_hh" in k:
                want = torch.zeros(3 * H)
                want[q:2 * q] = 1
                assert torch.equal(p.detach(), want), k
                assert q < H < 2 * q      # the ones straddle the r and z thirds
                seen += 1
            elif "weight_hh" in k:
                w = p.detach().double()
                assert float((w.t() @ w - torch.eye(H, dtype=torch.float64)).abs().max()) <= 1e-5, k
                seen += 1
        assert seen == 8 and isinstance(m.dropout, torch.nn.Dropout) and m.dropout.p == 0.2 and m.last_seed is None
        assert isinstance(m.rnn, torch.nn.GRU)


def test_header_declares_and_binding_matches_the_entries(cell):
    from get_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "get_hip.h")).read(), flags=re.S)
    for name in ("gh_%s_seq_fwd" % cell.module.lower(), "gh_%s_seq_bwd" % cell.module.lower()):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, src, flags=re.S)
        assert m, f"{name} is not declared in include/get_hip.h"
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == nargs, name
    assert "#define GH_ABI_VERSION 10" in src and _lib.ABI_VERSION == 10


def test_install_serves_the_gru_import_path(tmp_path):
    run_in_fresh_interpreter(tmp_path, "from Models.BiDAF.wrapper import GRU, LSTM\n"
                             "assert GRU is M.GRU and GRU.__module__ == 'get_amd.modules' and LSTM is M.LSTM",
                             packages=("Models", "Models/BiDAF"))


def test_refuses_cpu_tensors_and_bad_lengths(cell):
    from get_amd import ops
    m = _cls(cell)(6, 4, bidirectional=True).eval()
    x, idx = torch.zeros(2, 5, 6), torch.arange(2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m((x, torch.tensor([5, 3]), idx, idx), max_len=5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        if cell.module == "LSTM":
            ops.lstm_seq([torch.zeros(2, 5, 16)], [torch.zeros(16, 4)], torch.ones(2, dtype=torch.int32), None, 5)
        else:
            ops.gru_seq([torch.zeros(2, 5, 12)], [torch.zeros(12, 4)], [torch.zeros(12)], torch.ones(2, dtype=torch.int32), None, 5)
    # host lengths outside [1, T] raise as the reference's pack / pad functions do
    with pytest.raises(ValueError):
        m((x, torch.tensor([5, 0]), idx, idx), max_len=5)
    with pytest.raises(ValueError):
        m((x, torch.tensor([5, 3]), idx, idx), max_len=4)

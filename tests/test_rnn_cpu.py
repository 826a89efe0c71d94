"""CPU-side checks of the two sequence encoders (Models/BiDAF/wrapper.py: LSTM :229-276, GRU :279-327), once per cell: the
float64 restatement the GPU tests compare the kernels with (tests/rnn_ref.py) reproduces the reference's goldens on its own,
the drop-in's constructor builds the reference's state_dict for every configuration in tests/golden/lstm_contract.json /
gru_contract.json and initialises a stand-alone module as the reference does (the GRU: as the reference's constructor does
once its one raising line runs), the C-ABI declares and binds the two recurrence entries, the shim exports the classes, and
the modules refuse CPU tensors.  The per-step restatement at the kernels' interface (lstm_steps64 / gru_steps64, what
tests/test_gpu_rnn_paths.py compares the four recurrence entries with) agrees with lstm64 / gru64 and their autograd, and its
own fp32 evaluation stays within half of that file's elementwise bound at every one of its cases."""
import os
import re

import numpy as np
import pytest
import torch

from tests.rnn_ref import ARG_CASES, BWD_STREAMS, CELLS, CHAIN_CASES, FWD_STREAMS, STEPS, WIDTH_CASES, case_name, case_reference
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


# ----------------------------------------------------------------------------- the per-step restatement (tests/rnn_ref.py)
@pytest.fixture(params=list(CELLS))
def kind(request):
    return request.param


def _names(kind, bidirectional):
    return [f"{k}_l0{sfx}" for sfx in (("", "_reverse") if bidirectional else ("",)) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


@pytest.mark.parametrize("shape", [(5, 7, 6, 4, 7), (19, 6, 3, 9, 8)], ids=["b5-l7-h4", "b19-l6-h9-t8"])
@pytest.mark.parametrize("bidirectional", [False, True], ids=["uni", "bi"])
def test_steps_agree_with_the_encoder_restatement(kind, shape, bidirectional):
    """Fed with gx = x W_ih^T + b, the per-step function gives lstm64's / gru64's y and h; with W_ih a selection of x's columns
    (x = [gx0 | gx1], so that the gradient of x IS the gradient of gx) autograd through lstm64 / gru64 gives its dgates / dgx.
    All to 1e-12 in float64."""
    B, L, D, H, T = shape
    G, dirs = CELLS[kind].gates, 2 if bidirectional else 1
    gen = torch.Generator().manual_seed(B + H)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    lens = torch.randint(1, L + 1, (B,), generator=gen)
    lens[0], lens[1] = L, 1
    g_y, g_hn = rn(B, T, dirs * H), rn(dirs, B, H)

    def both(params, x, gx):
        w_hh = [params[f"weight_hh_l0{s}"] for s in ("", "_reverse")[:dirs]]
        extra = [[params[f"bias_hh_l0{s}"] for s in ("", "_reverse")[:dirs]]] if kind == "gru" else []
        st = STEPS[kind](gx, w_hh, *extra, lens, L, T, g_y, g_hn, backward=True)
        x = x.clone().requires_grad_(True)
        y, hcat = CELLS[kind].ref64(params, x, lens, T, 1, bidirectional)
        ((y * g_y).sum() + (hcat.view(B, dirs, H).permute(1, 0, 2) * g_hn).sum()).backward()
        assert float((st["y"] - y.detach()).abs().max()) <= 1e-12
        assert float((st["h_n"] - hcat.detach().view(B, dirs, H).permute(1, 0, 2)).abs().max()) <= 1e-12
        return st, x.grad

    # a general input projection: y and h
    params = {}
    for k in _names(kind, bidirectional):
        params[k] = rn(G * H, D) / D ** 0.5 if "weight_ih" in k else rn(G * H, H) / H ** 0.5 if "weight_hh" in k else 0.3 * rn(G * H)
    x = rn(B, L, D)
    fold = lambda s: params["bias_ih_l0" + s] + (params["bias_hh_l0" + s] if kind == "lstm" else 0.0)
    both(params, x, [x @ params["weight_ih_l0" + s].t() + fold(s) for s in ("", "_reverse")[:dirs]])
    # W_ih selects direction d's columns of x = [gx0 | gx1]: the gradient of x is the gradient of gx
    gx = [rn(B, L, G * H) for _ in range(dirs)]
    eye = torch.eye(dirs * G * H, dtype=torch.float64)
    for d, s in enumerate(("", "_reverse")[:dirs]):
        params["weight_ih_l0" + s] = eye[d * G * H:(d + 1) * G * H]
        params["bias_ih_l0" + s] = torch.zeros(G * H, dtype=torch.float64)
    bias = lambda s: params["bias_hh_l0" + s] if kind == "lstm" else 0.0
    st, gxgrad = both(params, torch.cat(gx, dim=2), [g + bias(s) for g, s in zip(gx, ("", "_reverse"))])
    got = st["dgates" if kind == "lstm" else "dgx"]
    assert float((torch.cat(list(got), dim=2) - gxgrad).abs().max()) <= 1e-12
    dead = torch.arange(L)[None, :] >= lens.clamp(max=min(L, T))[:, None]
    assert bool((got[:, dead] == 0).all()) and bool((st["h_prev"][:, dead] == 0).all()) and bool(torch.isnan(st["gates"][:, dead]).all())


@pytest.mark.parametrize("c", WIDTH_CASES + ARG_CASES + CHAIN_CASES, ids=case_name)
def test_fp32_evaluation_stays_within_half_the_elementwise_bound(kind, c):
    """What makes 1e-5 + 1e-4 |want| a bound on the KERNELS in tests/test_gpu_rnn_paths.py: at every case of that file the
    restatement evaluated in fp32 on the CPU -- the same operations in another order -- is within half of it, on every forward
    and backward stream."""
    want, got = case_reference(kind, c), case_reference(kind, c, torch.float32)
    worst = 0.0
    for k in FWD_STREAMS[kind] + BWD_STREAMS[kind]:
        live = ~torch.isnan(want[k])
        assert torch.equal(live, ~torch.isnan(got[k])), k
        worst = max(worst, golden_ratio(got[k][live], want[k][live], 0.5e-5, 0.5e-4, f"{kind} {case_name(c)} {k} fp32 vs float64"))
    print(f"{kind} {case_name(c)}: fp32 restatement at {worst:.3f} of half the bound")

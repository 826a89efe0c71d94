"""CPU-side checks of the graph encoders GraphAttentionLayer / GAT / GCN (Models/BiDAF/wrapper.py:7-151): the install()
shim exports them under the reference's module path, and their constructors build the reference's state_dict (names,
shapes) and init distributions, for every configuration captured in tests/golden/encoder_contract.json; the float64
restatements the GPU tests compare the kernels with (tests/util.py) reproduce the golden archives on their own."""
import math

import torch

from tests.util import _gat64, _gat_head64, _gcn64, golden_ratio, load_golden, run_in_fresh_interpreter


def _contract(golden_dir):
    return load_golden(golden_dir, "g11_gcn.npz", "encoder_contract.json")[2]


def test_install_shim_exports_the_encoders(tmp_path):
    run_in_fresh_interpreter(tmp_path, r"""
from Models.BiDAF.wrapper import GAT, GCN, GraphAttentionLayer, Linear
from get_amd import modules
assert GAT is modules.GAT and GCN is modules.GCN and GraphAttentionLayer is modules.GraphAttentionLayer
assert Linear is modules.Linear
""", packages=("Models", "Models/BiDAF"))


def test_encoder_state_dicts_match_the_reference_contract(golden_dir):
    from get_amd import modules
    contract = _contract(golden_dir)
    assert {c["class"] for c in contract.values()} == {"GraphAttentionLayer", "GAT", "GCN"}
    for name, c in contract.items():
        m = getattr(modules, c["class"])(**c["kwargs"])
        got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
        assert got == c["state_dict"], name


def test_encoder_init_distributions():
    from get_amd import modules
    torch.manual_seed(0)
    lay = modules.GraphAttentionLayer(40, 30, dropout=0.6, alpha=0.2)
    # xavier_uniform_(gain=1.414): U(-b, b), b = gain * sqrt(6 / (fan_in + fan_out))
    for p, (fi, fo) in ((lay.W, (30, 40)), (lay.a, (1, 60))):
        b = 1.414 * math.sqrt(6.0 / (fi + fo))
        assert p.abs().max().item() <= b and p.abs().max().item() > 0.8 * b
    assert lay.dropout == 0.6 and lay.alpha == 0.2 and lay.concat is True
    gat = modules.GAT(16, 8, 4)
    assert len(gat.out_att) == 3 and gat.attentions == [] and gat.dropout == 0.6
    assert all(not h.concat for h in gat.out_att)
    gat2 = modules.GAT(16, 8, 4, head_num=2, num_layers=3)
    assert [len(l) for l in gat2.attentions] == [2, 2] and gat2.attentions[1][0].W.shape == (16, 8)
    assert gat2.out_att[0].W.shape == (16, 4)
    gcn = modules.GCN(20, 12, 12, num_layers=2, dropout=0.5)
    # kaiming-normal weights, nn.Linear's default bias (the reference's bias zeroing never fires)
    w = gcn.Linear[0].linear.weight
    assert abs(w.std().item() - math.sqrt(2.0 / 20)) < 0.1 * math.sqrt(2.0 / 20)
    assert gcn.Linear[0].linear.bias.abs().max().item() > 0
    assert gcn.dropout == 0.5 and gcn.num_layers == 2


def test_gcn_keeps_the_reference_layer_width_quirk():
    from get_amd import modules
    g1 = modules.GCN(10, 6, 7, num_layers=1)
    assert g1.Linear[0].linear.weight.shape == (6, 10)          # the last layer maps to hidden_dim
    g3 = modules.GCN(10, 6, 7, num_layers=3)
    assert [tuple(l.linear.weight.shape) for l in g3.Linear] == [(7, 10), (7, 6), (6, 6)]


def test_gat_dropout_mask_replica_is_the_cells_mask():
    from get_amd import ops
    m = ops.gat_dropout_mask(1234, 1, 3, 4, 5, 0.4)
    assert m.shape == (3, 4, 5, 5)
    full = ops.dropout_mask_reference(1234, 2 * 3 * 4 * 5, 5, 0.4)
    assert (m.reshape(-1, 5) == full[3 * 4 * 5:]).all()
    assert 0.45 < m.mean() < 0.75


def _restatement_against(golden_dir, npz, kinds_key):
    """Every out / grad entry of one encoder archive against the float64 restatement of its case; (worst ratio, cases)."""
    z, meta, contract = load_golden(golden_dir, npz, "encoder_contract.json")
    worst, checked, n_cases = 0.0, set(), 0
    for name in meta[kinds_key]:
        c = contract[name]
        kw = c["kwargs"]
        for kind in meta["adj_kinds"]:
            key = f"{name}/{kind}::"
            p64 = {k[len(key) + len("param::"):]: torch.from_numpy(z[k]).double().requires_grad_(True)
                   for k in z if k.startswith(key + "param::")}
            x = torch.from_numpy(z[key + "x"]).double().requires_grad_(True)
            adj = torch.from_numpy(z[key + "adj"]).double()
            if c["class"] == "GraphAttentionLayer":
                out = _gat_head64(x, adj, p64["W"], p64["a"], kw["alpha"], None, 0.0, "elu" if kw["concat"] else "plain")
            elif c["class"] == "GAT":
                out = _gat64(p64, x, adj, kw["head_num"], kw["num_layers"], kw.get("alpha", 0.2))
            else:
                out = _gcn64(p64, x, adj, kw["num_layers"])
            (out * torch.from_numpy(z[key + "gout"]).double()).sum().backward()
            checks = [("out", out, 1e-4), ("grad::x", x.grad, 1e-5)] + [("grad::" + k, t.grad, 1e-5) for k, t in p64.items()]
            for k, got, atol in checks:
                worst = max(worst, golden_ratio(got, z[key + k], atol, 1e-4, key + k))
                checked.add(key + k)
            n_cases += 1
    prefixes = tuple(f"{name}/" for name in meta[kinds_key])
    recorded = {k for k in z if k.startswith(prefixes) and k.split("::")[1] in ("out", "grad")}
    assert checked == recorded, sorted(recorded ^ checked)
    print(f"{npz}: worst ratio of the bound {worst:.3f}")
    return n_cases


def test_float64_restatements_reproduce_the_gat_goldens(golden_dir):
    """_gat_head64 / _gat64 alone against every output and gradient of g10_gat.npz at the GPU golden test's elementwise
    bounds (1e-4 + 1e-4 |want| outputs, 1e-5 + 1e-4 |want| gradients)."""
    assert _restatement_against(golden_dir, "g10_gat.npz", "gat_cases") == 12


def test_float64_restatement_reproduces_the_gcn_goldens(golden_dir):
    """_gcn64 alone against every output and gradient of g11_gcn.npz, same bounds."""
    assert _restatement_against(golden_dir, "g11_gcn.npz", "gcn_cases") == 4

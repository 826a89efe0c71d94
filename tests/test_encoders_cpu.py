"""CPU-side checks of the graph encoders GraphAttentionLayer / GAT / GCN (Models/BiDAF/wrapper.py:7-151): the install()
shim exports them under the reference's module path, and their constructors build the reference's state_dict (names,
shapes) and init distributions, for every configuration captured in tests/golden/encoder_contract.json."""
import json
import math
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _contract(golden_dir):
    with open(os.path.join(golden_dir, "encoder_contract.json")) as fh:
        return json.load(fh)


def test_install_shim_exports_the_encoders(tmp_path):
    for pkg in ("Models", "Models/BiDAF"):
        os.makedirs(os.path.join(tmp_path, pkg), exist_ok=True)
        open(os.path.join(tmp_path, pkg, "__init__.py"), "w").close()
    code = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import get_amd
M = get_amd.install()
from Models.BiDAF.wrapper import GAT, GCN, GraphAttentionLayer, Linear
from get_amd import modules
assert GAT is modules.GAT and GCN is modules.GCN and GraphAttentionLayer is modules.GraphAttentionLayer
assert Linear is modules.Linear
print('ok')
""" % (ROOT, str(tmp_path))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


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

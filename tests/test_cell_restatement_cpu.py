"""The float64 restatement of the GGNN cell in tests/util.py (cell_forward_f64 / cell_backward_f64: the reference of
tests/test_gpu_cell_paths.py and tests/test_gpu_cell_bwd_nodx.py), checked without any kernel: its outputs and its hand-written
gradients against autograd through oracle.get_oracle.ggnn_cell in float64 (1e-12 of the largest entry), and its forward against
the golden captured from the reference (tests/golden/g2_ggnn.npz) at the bound the oracle's own golden test applies (2e-5
absolute, tests/test_oracle_golden.py)."""
import numpy as np
import pytest
import torch

from oracle import cases
from oracle import get_oracle as O
from tests.util import CELL_B, CELL_SAVED, CELL_W, cell_backward_f64, cell_forward_f64, load

ORACLE_W = {"p": "proj.linear.weight", "z0": "linearz0.linear.weight", "z1": "linearz1.linear.weight",
            "r0": "linearr0.linear.weight", "r1": "linearr1.linear.weight", "h0": "linearh0.linear.weight",
            "h1": "linearh1.linear.weight"}
ORACLE_B = {k: f"linear{k}.linear.bias" for k in CELL_B}


def _close(got, want, what):
    scale = float(want.abs().max()) + 1e-300
    err = float((got - want).abs().max())
    print(f"{what}: err {err:.3e} over scale {scale:.3e} = {err / scale:.3e}")
    assert got.shape == want.shape and err <= 1e-12 * scale, (what, err, scale)


@pytest.mark.parametrize("n,r,din,h,weighted", [(3, 20, 12, 20, False), (2, 9, 5, 7, True), (2, 33, 16, 1, False)])
def test_restatement_equals_autograd_through_the_oracle_cell(n, r, din, h, weighted):
    """Forward streams, output, dx, the seven dw and the six db; a graph with all, some and one real node (rows and columns of
    the padding nodes are zero); normalised and arbitrary (asymmetric) edge values."""
    gen = torch.Generator().manual_seed(100 * n + r + din + h)
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)
    counts = [r, max(r // 3, 1), 1][:n]
    adj = torch.zeros(n, r, r, dtype=torch.float64)
    for g, c in enumerate(counts):
        on = (torch.rand(c, c, generator=gen) < 0.4) | torch.eye(c, dtype=torch.bool)
        on = on | on.t()
        if weighted:
            adj[g, :c, :c] = on * rn(c, c)
        else:
            d = on.sum(-1).double().pow(-0.5)
            adj[g, :c, :c] = on * d[:, None] * d[None, :]
    w = {"p": rn(h, din) / din ** 0.5}
    w.update({k: rn(h, h) / h ** 0.5 for k in CELL_W[1:]})
    b = {k: 0.1 * rn(h) for k in CELL_B}
    x, g = rn(n, r, din), rn(n, r, h)
    p = {ORACLE_W[k]: v.clone().requires_grad_(True) for k, v in w.items()}
    p.update({ORACLE_B[k]: v.clone().requires_grad_(True) for k, v in b.items()})
    xo = x.clone().requires_grad_(True)
    out = O.ggnn_cell(adj, xo, p)
    out.backward(g)
    fwd = cell_forward_f64(adj, x, w, b)
    _close(fwd["out"], out.detach(), "out")
    scratch = {}
    dw, db, dx = cell_backward_f64(adj, x, g, w, b, scratch=scratch)
    _close(dx, xo.grad, "dx")
    for k in CELL_W:
        _close(dw[k], p[ORACLE_W[k]].grad, "dw_" + k)
    for k in CELL_B:
        _close(db[k], p[ORACLE_B[k]].grad, "db_" + k)
    # starting from given saved streams is the same computation
    dw2, db2, dx2 = cell_backward_f64(adj, x, g, w, b, saved={k: fwd[k] for k in CELL_SAVED})
    assert torch.equal(dx2, dx) and all(torch.equal(dw2[k], dw[k]) for k in CELL_W) and all(torch.equal(db2[k], db[k]) for k in CELL_B)
    # the scratch streams are the gradients of the pre-activations: dxp is d loss / d xp, da is d loss / d a
    xp = fwd["xp"].clone().requires_grad_(True)
    a = fwd["a"].clone().requires_grad_(True)
    W = {k: v for k, v in w.items()}
    z = torch.sigmoid(a @ W["z0"].t() + b["z0"] + xp @ W["z1"].t() + b["z1"])
    rr = torch.sigmoid(a @ W["r0"].t() + b["r0"] + xp @ W["r1"].t() + b["r1"])
    hh = torch.tanh(a @ W["h0"].t() + b["h0"] + (rr * xp) @ W["h1"].t() + b["h1"])
    (hh * z + xp * (1 - z)).backward(g)
    _close(scratch["da"], a.grad, "da")
    _close(scratch["dxp"], xp.grad + adj.transpose(1, 2) @ a.grad, "dxp")


@pytest.mark.parametrize("ci", range(len(cases.G2_CASES)))
def test_restatement_forward_against_the_reference_golden(ci):
    z, _ = load("g2_ggnn.npz")
    c = cases.g2_inputs(ci, O.convert_text)
    assert np.array_equal(c["toks"], z[f"c{ci}_tokens"])
    T = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    w = {k: T(c["p"][ORACLE_W[k]]) for k in CELL_W}
    b = {k: T(c["p"][ORACLE_B[k]]) for k in CELL_B}
    out = cell_forward_f64(T(c["adj"]).float(), T(c["x"]), w, b)["out"]
    err = float(np.abs(out.numpy() - z[f"c{ci}_out"]).max())
    print(f"G2 case {ci}: max err {err:.3e}, {err / 2e-5:.3f} of the 2e-5 bound")
    assert err <= 2e-5

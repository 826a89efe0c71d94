"""The numpy / float64 restatements of the graph kernels in tests/util.py (the references of
tests/test_gpu_graph_paths.py), checked without any kernel against goldens captured from the reference: G1 (word graphs),
G3 (keep-sets, where the reference's tie order is defined) and the scores and refined pattern of G4.  Bounds are those of
the existing golden tests (tests/test_gpu_ops.py, tests/test_oracle_golden.py); the worst ratio of each is printed."""
import numpy as np
import torch

from oracle import cases
from oracle import get_oracle as O
from tests.util import (dense_from_coo, g_pack_bits, g_plan, g_refined64, g_scorer64, g_text_graphs, g_topk, g_unpack_bits,
                        load)


def test_word_graphs_against_g1():
    z, meta = load("g1_convert_text.npz")
    worst = 0.0
    for i, m in enumerate(meta):
        fl = m["fixed_length"]
        ids, nn, pattern, dinv, _ = g_text_graphs([z[f"c{i}_tokens"]], [m["length"]], fl, m["window"], O.convert_text)
        exp = dense_from_coo(z, i, fl)
        assert int(nn[0]) == m["n_nodes"] and np.array_equal(ids[0], z[f"c{i}_words"]), i
        assert np.array_equal(pattern[0], exp != 0), i
        # the pattern survives packing to bit words and back, with no bit beyond the row
        back, spare = g_unpack_bits(g_pack_bits(pattern), fl)
        assert np.array_equal(back, pattern) and not spare, i
        err = np.abs(g_refined64(pattern, dinv=dinv)[0] - exp).max()
        worst = max(worst, err / 2e-7)
        assert err <= 2e-7, i                                   # product of two fp32 dinv (tests/test_gpu_ops.py)
    print(f"G1 values: worst {worst:.3f} of the 2e-7 bound over {len(meta)} cases")


def test_topk_against_g3_where_the_reference_has_no_ties():
    z, meta = load("g3_gsl.npz")
    checked = 0
    for ci, m in enumerate(meta):
        if m["ties"]:
            continue
        r = m["r"]
        exp_mask = np.unpackbits(z[f"c{ci}_mask"], axis=-1)[..., :r].astype(bool)
        keep = g_topk(z[f"c{ci}_score"][..., 0], m["k"])
        assert keep.sum(-1).tolist() == [m["k"]] * m["b"], ci
        got = g_refined64(np.ones((m["b"], r, r), bool), keep=keep, vals=np.ones((m["b"], r, r), np.float32)) != 0
        assert np.array_equal(got, exp_mask), ci
        checked += 1
    assert checked >= 1
    assert g_topk(np.array([[.9, .1, .8, .2]]), 2).tolist() == [[True, False, True, False]]
    assert g_topk(np.array([[1., 1., 1.]]), 2).tolist() == [[True, True, False]]          # ties: the lower index
    assert g_topk(np.array([[0.0, -0.0, 0.0]]), 1).tolist() == [[True, False, False]]     # -0.0 == 0.0
    assert g_topk(np.array([[1., 2.]]), 0).tolist() == [[False, False]] and g_topk(np.array([[1., 2.]]), 7).all()


def test_scorer_against_g4_scores_and_refined_pattern():
    z, meta = load("g4_ggnn_gsl.npz")
    worst = 0.0
    for ci, m in enumerate(meta):
        n, r, d, h, window, rate = cases.G4_CASES[ci]
        c = cases.g4_inputs(ci, O.convert_text)
        p = {k: torch.from_numpy(v).double() for k, v in c["p"].items()}
        adj = torch.from_numpy(c["adj"]).float().double()
        f1 = O.ggnn_cell(adj, torch.from_numpy(c["x"]).double(), p, "feat_prop1.").numpy()
        _, _, pattern, dinv, _ = g_text_graphs(c["toks"], c["lens"], r, window, O.convert_text)
        assert np.array_equal(pattern, c["adj"] != 0)
        g = lambda k: float(c["p"][f"word_scorer1.linear{k}.linear.weight"][0, 0])
        b = lambda k: float(c["p"][f"word_scorer1.linear{k}.linear.bias"][0])
        gate = [v for k in ("z0", "z1", "r0", "r1", "h0", "h1") for v in (g(k), b(k))]
        xproj = f1 @ c["p"]["word_scorer1.proj.linear.weight"][0].astype(np.float64)
        score = g_scorer64(g_refined64(pattern, dinv=dinv), xproj, gate)
        err = np.abs(score - z[f"c{ci}_score"]).max()
        worst = max(worst, err / 1e-5)
        assert err <= 1e-5, (ci, err)                           # the bound of test_g4_ggnn_with_gsl
        keep = g_topk(score, int(rate * r))
        exp_nz = np.unpackbits(z[f"c{ci}_adjr_nz"], axis=-1)[..., :r].astype(bool)
        assert np.array_equal(g_refined64(pattern, keep=keep, dinv=dinv) != 0, exp_nz), ci
    print(f"G4 scores: worst {worst:.3f} of the 1e-5 bound")


def test_plan_is_a_permutation_with_real_rows_first():
    nn = np.array([3, 0, 9, 4, -2], np.int32)                   # 9 and -2 are clamped into [0, 4]
    ids = np.arange(1, 21, dtype=np.int32).reshape(5, 4)
    pl = g_plan(nn, 4, ids)
    assert pl["goff"].tolist() == [0, 3, 3, 7, 11, 11]
    assert sorted(pl["src"].tolist()) == list(range(20))
    assert pl["src"][:11].tolist() == [0, 1, 2, 8, 9, 10, 11, 12, 13, 14, 15]
    assert pl["src"][11:].tolist() == [3, 4, 5, 6, 7, 16, 17, 18, 19]
    assert np.array_equal(pl["rowg"], pl["src"] // 4) and np.array_equal(pl["cids"], ids.reshape(-1)[pl["src"]])

"""The pairwise helpers without a GPU: the float64 restatements of tests/pair_ref.py against the reference's goldens
(tests/golden/g20_pair.npz, tools/make_pair_golden.py), the argument errors of get_amd.pairwise and ops.pair, patch() on
stand-in modules, and the header's declarations."""
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import pair_ref as R
from tests.util import ROOT, load_golden, rel_close

GOLDEN_TOL = 1e-4            # of the largest entry of the stored result: the generator's bound
HIST_MODES = ("CH", "NH", "LCH")


def archive(golden_dir):
    z, meta, _ = load_golden(golden_dir, "g20_pair.npz")
    return z, meta


def cases_of(family):
    z, meta = archive(os.path.join(ROOT, "tests", "golden"))
    return [k for k in meta["cases"] if k.split("::")[0] in family]


def arr(z, key, name):
    """A stored array of a case as a tensor; float16 inputs widen to fp32; l1 reads the operands stored under l2."""
    if key.startswith("l1::") and name in ("a", "b"):
        key = "l2::" + key.split("::")[1]
    v = z[f"{key}::{name}"]
    return torch.from_numpy(v.astype(np.float32) if v.dtype == np.float16 else v)


def check_golden(z, key, got, what):
    """{name: tensor} against the stored fp32 results of the reference, each within GOLDEN_TOL of its largest entry."""
    for name, t in got.items():
        want = arr(z, key, name)
        assert tuple(t.shape) == tuple(want.shape), (key, name, tuple(t.shape), tuple(want.shape))
        if want.numel():
            rel_close(t, want, GOLDEN_TOL, f"{what} {key} {name}")


def window_args(meta, key):
    """(window, left, right) of a ma / mod / ctx case."""
    w = meta["params"][key]["window"]
    return (w, w // 2, w - w // 2 - 1) if key.startswith("ctx::") else (w, 0, 0)


@pytest.mark.parametrize("key", cases_of(("l2", "l1")))
def test_distance_restatements_match_the_goldens(golden_dir, key):
    z, _ = archive(golden_dir)
    a, b, g = arr(z, key, "a"), arr(z, key, "b"), arr(z, key, "g")
    out, da, db = (R.pair_l2_grads64 if key.startswith("l2::") else R.pair_l1_grads64)(a, b, g)
    check_golden(z, key, {"out": out, "grad::a": da, "grad::b": db}, "restatement")
    # the closed-form gradients are what autograd gives for the forward restatement
    a64, b64 = a.double().requires_grad_(True), b.double().requires_grad_(True)
    o = R.pair_l2_64(a64, b64) if key.startswith("l2::") else R.pair_l1_64(a64, b64)
    (o * g.double()).sum().backward()
    rel_close(da, a64.grad, 1e-12, f"{key} da closed form")
    rel_close(db, b64.grad, 1e-12, f"{key} db closed form")


@pytest.mark.parametrize("key", cases_of(("ma", "mod", "ctx")))
def test_window_restatements_match_the_goldens(golden_dir, key):
    z, meta = archive(golden_dir)
    w, left, right = window_args(meta, key)
    x, g = arr(z, key, "x"), arr(z, key, "g")
    mask = arr(z, key, "mask") if key.startswith("ctx::") else None
    out = R.window_mean64(x, w, left, right, mask)
    dx = R.window_mean_bwd64(g, x.shape[1], w, left, right, mask)
    check_golden(z, key, {"out": out, "grad::x": dx}, "restatement")
    if key == "ma::over":
        assert tuple(out.shape) == (x.shape[0], 0, x.shape[2]) and float(dx.abs().max()) == 0.0
    if mask is not None:
        assert bool((arr(z, key, "out")[mask == 0] == 0).all())


@pytest.mark.parametrize("key", cases_of(("hist",)))
def test_histogram_restatement_matches_the_goldens(golden_dir, key):
    z, meta = archive(golden_dir)
    p = meta["params"][key]
    table = arr(z, key, "table").double().numpy()
    if p["normalize"]:
        table = R.normalize_table64(table)
    il, ir, ln = z[f"{key}::ids_left"], z[f"{key}::ids_right"], z[f"{key}::len_right"]
    scaled = z[f"{key}::scaled"]
    for i, n in enumerate(ln):
        assert np.isfinite(scaled[i, :, :n]).all() and np.isnan(scaled[i, :, n:]).all()
        mine = R.hist_scaled64(table, il[i], ir[i, :n], p["bins"])
        assert np.abs(mine - scaled[i, :, :n]).max(initial=0.0) <= 1e-12 * p["bins"]
        # the reference's own counts follow from its own scaled values
        counts = R.hist_counts(R.hist_bins(scaled[i, :, :n], p["bins"]), p["bins"])
        assert np.array_equal(counts, z[f"{key}::out::CH"][i].astype(np.int64)), key
        assert np.array_equal(counts.sum(1), np.full(len(il[i]), n + p["bins"]))
        for mode in HIST_MODES:
            rel_close(R.hist_mode(counts, mode), z[f"{key}::out::{mode}"][i], GOLDEN_TOL, f"{key} sample {i} {mode}")
    if key == "hist::dyadic":
        assert np.array_equal(scaled[np.isfinite(scaled)] * 128, np.round(scaled[np.isfinite(scaled)] * 128))
        for mode in HIST_MODES:
            rel_close(R.match_hist64(table, il, ir, ln, p["bins"], mode), z[f"{key}::out::{mode}"], GOLDEN_TOL, f"{key} batch {mode}")


def test_the_reference_docstring_example_is_what_the_restatement_gives():
    table = R.normalize_table64(np.array([[1.0, -1.0], [1.0, 2.0], [1.0, 3.0]]))
    got = R.match_hist64(table, [[0, 1]], [[1, 2]], [2], 3, "CH")[0]
    assert got.tolist() == [[3.0, 1.0, 1.0], [1.0, 2.0, 2.0]]


# ----------------------------------------------------------------------------- argument errors (no device is touched)
def test_moving_average_refuses_what_the_reference_gets_wrong():
    from get_amd import pairwise
    x = torch.zeros(2, 5, 3)
    for bad in (0, 2, -1):
        with pytest.raises(ValueError, match="dim 1"):
            pairwise.moving_average(x, 2, bad)
        with pytest.raises(ValueError, match="dim 1"):
            pairwise.MovingAverage(2, bad)(x)
    with pytest.raises(ValueError, match="dim 1"):
        pairwise.moving_average(torch.zeros(5, 3), 2, 1)


def test_argument_errors_of_the_host_layer():
    from get_amd import ops, pairwise
    x = torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match="window >= 1"):
        ops.pair.window_mean(x, 0)
    with pytest.raises(ValueError, match="left, right >= 0"):
        ops.pair.window_mean(x, 2, left=-1)
    with pytest.raises(ValueError, match="limited to 1024"):
        ops.pair.window_mean(torch.zeros(1, 2000, 3), 1025)
    with pytest.raises(ValueError, match=r"mask \(2, 5\)"):
        ops.pair.window_mean(x, 3, 1, 1, mask=torch.ones(2, 4))
    with pytest.raises(ValueError, match=r"\(B,L,D\)"):
        ops.pair.window_mean(torch.zeros(5, 3), 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pair.window_mean(x, 2)
    for fn in (ops.pair.pair_l2, ops.pair.pair_l1):
        with pytest.raises(ValueError, match=r"a \(B,L,D\) and b \(B,R,D\)"):
            fn(torch.zeros(2, 5, 3), torch.zeros(2, 4, 2))
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(x, x)
    with pytest.raises(AssertionError):
        pairwise.cosine_distance(torch.zeros(5, 3), torch.zeros(5, 3))
    ids = torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="not one of"):
        ops.pair.match_hist(torch.zeros(4, 3), None, ids, ids, torch.ones(2, dtype=torch.int64), 30, "XH")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pair.match_hist(torch.zeros(4, 3), None, ids, ids, torch.ones(2, dtype=torch.int64), 30, "CH")
    assert ops.pair.window_out_len(3, 5) == 0 and ops.pair.window_out_len(100, 4, 2, 1) == 100


def test_matching_histogram_constructor_errors():
    from get_amd import pairwise
    table = np.array([[1.0, -1.0], [0.0, 0.0], [1.0, 3.0]])
    with pytest.raises(ValueError, match=r"rows \[1\] have norm 0"):
        pairwise.MatchingHistogram(3, table, True, "CH")
    with pytest.raises(ValueError, match="mode"):
        pairwise.MatchingHistogram(3, table, False, "NG")
    with pytest.raises(ValueError, match="required"):
        pairwise.MatchingHistogram(3)
    with pytest.raises(ValueError, match="bin_size"):
        pairwise.MatchingHistogram(257, table, False, "CH")
    with pytest.raises(ValueError, match=r"\(V,D\)"):
        pairwise.MatchingHistogram(3, np.zeros(4), False, "CH")


# ----------------------------------------------------------------------------- patch()
def test_patch_sets_the_drop_ins_on_stand_in_modules():
    from get_amd import pairwise
    keep = object()
    tu = types.ModuleType("torch_utils")
    tu.cosine_distance = tu.l1_distance = tu.moving_average = tu._get_doc_context_copacrr = tu.idf = keep
    layers = types.ModuleType("layers")
    layers.MovingAverage = layers.Highway = keep
    units = types.ModuleType("matchzoo.preprocessors.units")
    units.MatchingHistogram = units.Vocabulary = keep
    units.matching_histogram = types.ModuleType("matchzoo.preprocessors.units.matching_histogram")
    units.matching_histogram.MatchingHistogram = keep
    assert pairwise.patch() == []
    done = pairwise.patch(torch_utils=tu)
    assert done == ["torch_utils.cosine_distance", "torch_utils.l1_distance", "torch_utils.moving_average",
                    "torch_utils._get_doc_context_copacrr"]
    assert tu.cosine_distance is pairwise.cosine_distance and tu.l1_distance is pairwise.l1_distance
    assert tu.moving_average is pairwise.moving_average and tu._get_doc_context_copacrr is pairwise._get_doc_context_copacrr
    assert tu.idf is keep and layers.MovingAverage is keep and units.MatchingHistogram is keep
    done = pairwise.patch(layers=layers, units=units)
    assert done == ["layers.MovingAverage", "matchzoo.preprocessors.units.MatchingHistogram",
                    "matchzoo.preprocessors.units.matching_histogram.MatchingHistogram"]
    assert layers.MovingAverage is pairwise.MovingAverage and layers.Highway is keep
    assert units.MatchingHistogram is pairwise.MatchingHistogram and units.Vocabulary is keep
    assert units.matching_histogram.MatchingHistogram is pairwise.MatchingHistogram
    bare = types.ModuleType("units")           # a package whose submodule was never loaded
    assert pairwise.patch(units=bare) == ["units.MatchingHistogram"]


def test_install_leaves_the_big_reference_modules_alone(tmp_path):
    from tests.util import run_in_fresh_interpreter
    run_in_fresh_interpreter(tmp_path, "assert not any(n in sys.modules for n in ('torch_utils', 'layers', 'matchzoo.preprocessors', "
                                       "'matchzoo.preprocessors.units'))\nimport get_amd.pairwise")


# ----------------------------------------------------------------------------- the header
def test_header_declares_the_seven_entry_points_under_abi_10():
    from get_amd import _lib
    src = open(os.path.join(ROOT, "include", "get_hip.h")).read()
    assert re.search(r"#define\s+GH_ABI_VERSION\s+10\b", src) and _lib.ABI_VERSION == 10
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gh_pair_l2_fwd", "gh_pair_l2_bwd", "gh_pair_l1_fwd", "gh_pair_l1_bwd", "gh_window_mean_fwd", "gh_window_mean_bwd",
                 "gh_match_hist"):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, code, flags=re.S)
        assert m, f"{name} is not declared"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == len(_lib.SIGNATURES[name]), name
    for cite in ("torch_utils.py:311-329", "torch_utils.py:332-348", "torch_utils.py:292-308", "layers.py:42-66",
                 "matching_histogram.py:44-60"):
        assert cite in src, cite

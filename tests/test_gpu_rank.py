"""The ranking family on the GPU (csrc/rank_ops.hip: ops.rank_metrics / rank_hinge / rank_cross_entropy, get_amd.ranking,
modules.RankHingeLoss / RankCrossEntropyLoss) against the reference's goldens (tests/golden/g19_rank.npz) and the float64
restatements of tests/rank_ref.py.

Ranks and every integer output are exact.  The fp64 metric outputs are bounded by 1e-12 max(1, |want|): each is a sum of at most
1024 non-negative terms (or a ratio of two such sums), every term correct to a few ulp, so the result is within 1024 * 4 * 2^-53 =
4.5e-13 relative of the reference's left-to-right sum; a value that is 0 in the reference must be exactly 0.  The losses are held
to the match family's bounds against the float64 goldens: outputs 1e-4 + 1e-4 |want|, gradients 1e-5 + 1e-4 |want|."""
import ctypes

import numpy as np
import pytest
import torch

from tests import rank_ref as R
from tests.util import DEV, bits_equal, golden_ratio, load_golden

pytestmark = pytest.mark.gpu

BATCHES = ["edges", "doctest", "get", "graded"]
LOSS_CASES = ["1x1x1", "5x3x1", "67x4x1", "300x9x1", "33x2x3"]
TOL_OUT = (1e-4, 1e-4)
TOL_GRAD = (1e-5, 1e-4)
SENTINEL = -77
# the dispatch paths csrc/rank_ops.hip names in its header, by group length
PATHS = {"wave": lambda n: n <= 64, "workgroup": lambda n: 65 <= n <= 1024}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_golden(golden_dir, "g19_rank.npz", "rank_contract.json")


def _device_batch(z, name, score_dtype=torch.float64):
    scores, labels, offsets = R.metric_batch(z, name)
    return torch.from_numpy(scores).to(DEV).to(score_dtype), torch.from_numpy(labels).to(DEV), offsets


def _run(z, name, thr, ks, score_dtype=torch.float64):
    from get_amd import ops
    scores, labels, offsets = _device_batch(z, name, score_dtype)
    out = ops.rank_metrics(scores, labels, offsets, ks, threshold=float(thr))
    torch.cuda.synchronize()
    return out


def _all_metrics(ks, thr):
    from get_amd import ranking as K
    return ([("ap", 0, K.AveragePrecision(thr)), ("map", 0, K.MeanAveragePrecision(thr)), ("mrr", 0, K.MeanReciprocalRank(thr))]
            + [("precision", i, K.Precision(k, thr)) for i, k in enumerate(ks)]
            + [("dcg", i, K.DiscountedCumulativeGain(k, thr)) for i, k in enumerate(ks)]
            + [("ndcg", i, K.NormalizedDiscountedCumulativeGain(k, thr)) for i, k in enumerate(ks)])


def test_every_dispatch_path_is_hit_by_the_golden_batches(golden):
    z, meta, _ = golden
    lengths = np.concatenate([np.diff(R.metric_batch(z, b)[2]) for b in BATCHES])
    assert all(any(on(int(n)) for n in lengths) for on in PATHS.values())
    assert all(sum(on(int(n)) for on in PATHS.values()) == 1 for n in lengths)            # every group takes exactly one
    edges = np.diff(R.metric_batch(z, "edges")[2])
    # both sides of the path boundary, a workgroup-path group with one, with two and with four items per thread (the tile full and
    # one short of full), an empty group, and a workgroup whose four groups take different paths (groups 4 .. 7 of `edges`)
    assert {0, 64, 65, 256, 257, 1023, 1024} <= set(edges.tolist())
    assert {(int(n) + 255) // 256 for n in edges if n > 64} >= {1, 2, 4}
    assert [PATHS["wave"](int(n)) for n in edges[4:8]] == [True, False, False, False]


@pytest.mark.parametrize("thr", [0, 1])
@pytest.mark.parametrize("batch", BATCHES)
def test_rank_metrics_against_the_goldens(golden, batch, thr):
    z, meta, _ = golden
    ks = meta["ks"]
    rank, gi, gd, nan_count = _run(z, batch, thr, ks)
    want_rank, want_int, _ = R.restated(z, batch, thr, ks)
    # exact: ties, signed zeros, infinities, empty groups, k beyond the group
    assert nan_count.tolist() == [0, 0]
    assert np.array_equal(rank.cpu().numpy(), z[f"m::{batch}::rank"].astype(np.int32)), "rank against the reference's ordering"
    assert np.array_equal(rank.cpu().numpy(), want_rank), "rank against the restatement"
    assert np.array_equal(gi.cpu().numpy(), want_int), "count, n_rel, first relevant position, hits"
    R.assert_metrics_close(gd.cpu().numpy(), R.golden_f64(z, batch, thr), f"{batch} thr {thr}: per group")


@pytest.mark.parametrize("thr", [0, 1])
@pytest.mark.parametrize("batch", BATCHES)
def test_ranking_metrics_means_against_the_goldens(golden, batch, thr):
    from get_amd import ranking
    z, meta, _ = golden
    scores, labels, offsets = _device_batch(z, batch)
    metrics = _all_metrics(meta["ks"], thr)
    res = ranking.ranking_metrics([m for _, _, m in metrics], scores, labels, offsets)
    assert len(res) == len(metrics) and all(type(v) is float for v in res.values())
    got = [res[m] for _, _, m in metrics]
    want = [float(np.reshape(z[f"m::{batch}::thr{thr}::mean::{name}"], -1)[i]) for name, i, _ in metrics]
    R.assert_metrics_close(got, want, f"{batch} thr {thr}: means")
    # device offsets (int32 and int64) give what host offsets give
    for dtype in (torch.int32, torch.int64):
        again = ranking.ranking_metrics([m for _, _, m in metrics], scores, labels, torch.from_numpy(offsets).to(DEV).to(dtype))
        assert [again[m] for _, _, m in metrics] == got


def test_mixed_thresholds_and_one_metric(golden):
    from get_amd import ranking as K
    z, _, _ = golden
    scores, labels, offsets = _device_batch(z, "graded")
    metrics = [K.MeanAveragePrecision(0.), K.MeanAveragePrecision(1.), K.AveragePrecision(1.), K.Precision(3, 1.)]
    res = K.ranking_metrics(metrics, scores, labels, offsets)
    want = [z["m::graded::thr0::mean::map"], z["m::graded::thr1::mean::map"], z["m::graded::thr1::mean::ap"],
            z["m::graded::thr1::mean::precision"][1]]
    R.assert_metrics_close([res[m] for m in metrics], [float(np.reshape(v, -1)[0]) for v in want], "two thresholds in one call")
    only = K.ranking_metrics([K.AveragePrecision()], scores, labels, offsets)
    R.assert_metrics_close(list(only.values()), [float(z["m::graded::thr0::mean::ap"].reshape(-1)[0])], "AveragePrecision alone")


def test_single_group_calls_reproduce_the_doctests(golden):
    from get_amd import ranking
    _, _, contract = golden
    for ex in contract["doctests"]:
        m = getattr(ranking, ex["class"])(**ex["kwargs"])
        got = m(ex["y_true"], ex["y_pred"])
        assert type(got) is float
        R.assert_metrics_close([got], [ex["value"]], f"{ex['class']} {ex['kwargs']} on lists")
        dev = m(torch.tensor(ex["y_true"], device=DEV), torch.tensor(ex["y_pred"], dtype=torch.float64, device=DEV))
        assert dev == got
        assert m(np.array(ex["y_true"]), np.array(ex["y_pred"], np.float64)) == got


def test_labels_do_not_pass_through_fp32():
    """A graded label of 0.1 is not above the threshold 0.1 -- float32(0.1), which is larger than the double, would be."""
    from get_amd import ranking
    assert float(np.float32(0.1)) > 0.1
    assert ranking.MeanReciprocalRank(threshold=0.1)([0.1, 0.0], [1.0, 2.0]) == 0.0
    assert ranking.MeanReciprocalRank(threshold=0.0999)([0.1, 0.0], [1.0, 2.0]) == 0.5
    labels = torch.tensor([0.1, 0.0], dtype=torch.float64, device=DEV)
    assert ranking.MeanReciprocalRank(threshold=0.1)(labels, torch.tensor([1.0, 2.0], device=DEV).half()) == 0.0
    assert ranking.MeanReciprocalRank(threshold=0.1)(labels.float(), torch.tensor([1.0, 2.0], device=DEV)) == 0.5       # an fp32 label is what it is


@pytest.mark.parametrize("batch", ["edges", "get", "graded"])
def test_two_calls_and_both_score_widths_are_bit_identical(golden, batch):
    z, meta, _ = golden
    first = _run(z, batch, 1, meta["ks"])
    for what, other in (("two calls", _run(z, batch, 1, meta["ks"])), ("fp32 scores", _run(z, batch, 1, meta["ks"], torch.float32))):
        for a, b, name in zip(first, other, ("rank", "group_int", "group_f64", "nan_count")):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), f"{what}: {name} differs"


def _raw_rank_metrics(scores, labels, offsets_host, n, ks, outs):
    """gh_rank_metrics itself, on outputs the caller has filled."""
    from get_amd import _lib
    off_host = np.ascontiguousarray(offsets_host, dtype=np.int32)
    off_dev = torch.from_numpy(off_host).to(DEV)
    ks_host = (ctypes.c_int32 * len(ks))(*ks)
    rank, gi, gd, nan_count = outs
    _lib.call("gh_rank_metrics", _lib.ptr(scores), 0, _lib.ptr(labels), _lib.ptr(off_dev), off_host.ctypes.data, n, len(off_host) - 1, 0.0,
              ctypes.cast(ks_host, ctypes.c_void_p), len(ks), _lib.ptr(rank), _lib.ptr(gi), _lib.ptr(gd), _lib.ptr(nan_count), _lib.stream())


@pytest.mark.parametrize("what,offsets,ks", [
    ("a group of 1025 items", [0, 5, 1030, 1100], [1, 3]),
    ("nine cut-offs", [0, 500, 1100], list(range(1, 10))),
    ("a cut-off of 0", [0, 500, 1100], [3, 0]),
    ("decreasing offsets", [0, 600, 500, 1100], [1]),
    ("offsets that do not end at n", [0, 500, 1000], [1]),
    ("offsets that do not start at 0", [1, 500, 1100], [1]),
])
def test_a_broken_limit_is_an_error_and_nothing_is_written(what, offsets, ks):
    n, g = 1100, len(offsets) - 1
    scores = torch.randn(n, device=DEV)
    labels = torch.ones(n, device=DEV, dtype=torch.float64)
    outs = (torch.full((n,), SENTINEL, device=DEV, dtype=torch.int32), torch.full((g, 3 + 9), SENTINEL, device=DEV, dtype=torch.int32),
            torch.full((g, 3 + 27), float(SENTINEL), device=DEV, dtype=torch.float64), torch.full((2,), SENTINEL, device=DEV, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="rank_metrics"):
        _raw_rank_metrics(scores, labels, offsets, n, ks, outs)
    torch.cuda.synchronize()
    for t in outs:
        assert bool((t == SENTINEL).all()), f"{what}: an output was written"
    # the same call within the limits succeeds and fills what it owns
    gi, gd = torch.full((2, 5), SENTINEL, device=DEV, dtype=torch.int32), torch.full((2, 9), float(SENTINEL), device=DEV, dtype=torch.float64)
    _raw_rank_metrics(scores, labels, [0, 500, 1100], n, [1, 3], (outs[0], gi, gd, outs[3]))
    torch.cuda.synchronize()
    assert bool((outs[0] != SENTINEL).all()) and outs[3].tolist() == [0, 0] and bool((gd != SENTINEL).all())
    assert gi.tolist() == [[500, 500, 1, 1, 3], [600, 600, 1, 1, 3]]


def test_python_front_refuses_what_the_library_refuses():
    from get_amd import ops
    scores, labels = torch.randn(1100, device=DEV), torch.ones(1100, device=DEV)
    with pytest.raises(RuntimeError, match="more than 1024"):
        ops.rank_metrics(scores, labels, [0, 1025, 1100], [1])
    with pytest.raises(RuntimeError, match="nk = 9"):
        ops.rank_metrics(scores, labels, [0, 500, 1100], list(range(1, 10)))
    with pytest.raises(RuntimeError, match="decrease"):
        ops.rank_metrics(scores, labels, torch.tensor([0, 600, 500, 1100], device=DEV), [1])


def test_a_nan_is_counted_and_refused():
    from get_amd import ops, ranking
    scores = torch.tensor([1.0, float("nan"), 0.5, 2.0, 3.0], device=DEV)
    labels = torch.tensor([1.0, 0.0, float("nan"), float("nan"), 1.0], dtype=torch.float64, device=DEV)
    rank, gi, gd, nan_count = ops.rank_metrics(scores, labels, [0, 3, 5], [1])
    assert nan_count.tolist() == [1, 2]
    assert bool(((rank >= 0) & (rank < 3)).all())
    with pytest.raises(ValueError, match="NaN"):
        ranking.ranking_metrics([ranking.MeanReciprocalRank()], scores, labels, [0, 3, 5])
    with pytest.raises(ValueError, match="NaN"):
        ranking.Precision()([1.0, 0.0], [float("nan"), 1.0])


# ----------------------------------------------------------------------------- losses
def _loss_inputs(z, case):
    key = f"l::{case}::"
    f = lambda k: torch.from_numpy(z[key + k].astype(np.float32)).to(DEV)
    return key, f("y_pred"), f("y_true"), f("hinge_none::g")


def _hinge(y0, num_neg, margin, red, upstream):
    from get_amd import modules
    y = y0.clone().requires_grad_(True)
    out = modules.RankHingeLoss(num_neg=num_neg, margin=margin, reduction=red)(y, None)
    ((out * upstream).sum() if red == "none" else out * upstream).backward()
    return out.detach(), y.grad


def _ce(y0, yt, num_neg, upstream):
    from get_amd import modules
    y = y0.clone().requires_grad_(True)
    out = modules.RankCrossEntropyLoss(num_neg=num_neg)(y, yt)
    (out * upstream).backward()
    return out.detach(), y.grad


@pytest.mark.parametrize("case", LOSS_CASES)
def test_losses_against_the_goldens(golden, case):
    z, meta, _ = golden
    num_neg = int(case.split("x")[1])
    key, y0, yt, g_none = _loss_inputs(z, case)
    for red in ("none", "mean", "sum"):
        up = g_none if red == "none" else meta["scalar_upstream"]
        out, grad = _hinge(y0, num_neg, meta["margin"], red, up)
        golden_ratio(out, z[f"{key}hinge_{red}::out"].reshape(tuple(out.shape)), *TOL_OUT, f"{case} hinge {red}: loss")
        golden_ratio(grad, z[f"{key}hinge_{red}::grad"], *TOL_GRAD, f"{case} hinge {red}: gradient")
        again = _hinge(y0, num_neg, meta["margin"], red, up)
        bits_equal(out, again[0], f"{case} hinge {red}: loss of two runs")
        bits_equal(grad, again[1], f"{case} hinge {red}: gradient of two runs")
    out, grad = _ce(y0, yt, num_neg, meta["scalar_upstream"])
    golden_ratio(out, z[key + "ce::out"].reshape(()), *TOL_OUT, f"{case} cross-entropy: loss")
    golden_ratio(grad, z[key + "ce::grad"], *TOL_GRAD, f"{case} cross-entropy: gradient")
    again = _ce(y0, yt, num_neg, meta["scalar_upstream"])
    bits_equal(out, again[0], f"{case} cross-entropy: loss of two runs")
    bits_equal(grad, again[1], f"{case} cross-entropy: gradient of two runs")


@pytest.mark.parametrize("b,num_neg,c", [(5, 3, 1), (33, 2, 3), (3, 1, 70)])
def test_losses_on_a_column_slice_against_the_restatement(b, num_neg, c):
    """y_pred and y_true as column slices of wider tensors (read in place, rows a stride apart); c = 70 takes the lane loop twice."""
    from get_amd import ops
    g = torch.Generator().manual_seed(1000 * b + 10 * num_neg + c)
    rows = b * (num_neg + 1)
    wide = (0.7 * torch.randn(rows, c + 5, generator=g)).half().float().to(DEV)
    wide_t = (torch.randint(0, 3, (rows, c + 2), generator=g).float() / 2).to(DEV)
    up = (torch.randint(-16, 17, (b, c), generator=g).float() / 16).to(DEV)
    y0, yt = wide[:, 2:2 + c], wide_t[:, 1:1 + c]
    assert not y0.is_contiguous() and not yt.is_contiguous()
    for red in ("none", "mean", "sum"):
        y = y0.detach().requires_grad_(True)
        out = ops.rank_hinge(y, num_neg, 0.5, red)
        ((out * up).sum() if red == "none" else out * 1.5).backward()
        y64 = y0.double().cpu().requires_grad_(True)
        want = R.rank_hinge64(y64, num_neg, 0.5, red)
        ((want * up.double().cpu()).sum() if red == "none" else want * 1.5).backward()
        golden_ratio(out, want.detach(), *TOL_OUT, f"strided hinge {red}: loss")
        golden_ratio(y.grad, y64.grad, *TOL_GRAD, f"strided hinge {red}: gradient")
    y = y0.detach().requires_grad_(True)
    out = ops.rank_cross_entropy(y, yt, num_neg)
    (out * 1.5).backward()
    y64 = y0.double().cpu().requires_grad_(True)
    want = R.rank_cross_entropy64(y64, yt.double().cpu(), num_neg)
    (want * 1.5).backward()
    golden_ratio(out, want.detach(), *TOL_OUT, "strided cross-entropy: loss")
    golden_ratio(y.grad, y64.grad, *TOL_GRAD, "strided cross-entropy: gradient")


def test_rows_that_are_no_multiple_of_the_instance_are_refused():
    from get_amd import _lib, modules
    y = torch.zeros(7, 2, device=DEV)
    with pytest.raises(ValueError, match="multiple"):
        modules.RankHingeLoss(num_neg=2)(y, None)
    with pytest.raises(ValueError, match="multiple"):
        modules.RankCrossEntropyLoss(num_neg=1)(y, y)
    out = torch.full((8,), float(SENTINEL), device=DEV)
    with pytest.raises(RuntimeError, match="no multiple"):
        _lib.call("gh_rank_hinge_fwd", _lib.ptr(y), 2, 7, 2, 2, 0.5, 1, _lib.ptr(out), None, _lib.ptr(out), _lib.ptr(out), _lib.stream())
    with pytest.raises(RuntimeError, match="no multiple"):
        _lib.call("gh_rank_ce_fwd", _lib.ptr(y), 2, _lib.ptr(y), 2, 7, 2, 1, _lib.ptr(out), _lib.ptr(out), _lib.ptr(out), _lib.stream())
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_cross_entropy_is_finite_where_the_reference_underflows(golden):
    """Q3: logits [0, -200] with labels [1, 0] give nan in the reference (recorded in the contract); the stable form gives
    log(1 + exp(-200)) = 0 and a zero gradient."""
    from get_amd import modules
    _, _, contract = golden
    assert contract["ce_q3_reference_is_nan"] is True
    y = torch.tensor([[0.0], [-200.0]], device=DEV, requires_grad=True)
    loss = modules.RankCrossEntropyLoss(num_neg=1)(y, torch.tensor([[1.0], [0.0]], device=DEV))
    loss.backward()
    assert loss.item() == 0.0 and y.grad.abs().max().item() == 0.0

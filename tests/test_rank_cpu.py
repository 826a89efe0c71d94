"""The ranking family without a GPU: the float64 restatements of tests/rank_ref.py against the reference's goldens
(tests/golden/g19_rank.npz, written by tools/make_rank_golden.py), the install() shim for matchzoo.metrics and matchzoo.losses,
the contract of the six metric classes and the two losses, and the refusal of CPU tensors."""
import numpy as np
import pytest
import torch

from tests import rank_ref as R
from tests.util import load_golden, run_in_fresh_interpreter

METRIC_CLASSES = ["Precision", "AveragePrecision", "MeanAveragePrecision", "MeanReciprocalRank", "DiscountedCumulativeGain",
                  "NormalizedDiscountedCumulativeGain"]
METRIC_FILES = {"precision": "Precision", "average_precision": "AveragePrecision", "mean_average_precision": "MeanAveragePrecision",
                "mean_reciprocal_rank": "MeanReciprocalRank", "discounted_cumulative_gain": "DiscountedCumulativeGain",
                "normalized_discounted_cumulative_gain": "NormalizedDiscountedCumulativeGain"}


@pytest.fixture(scope="module")
def golden(golden_dir):
    return load_golden(golden_dir, "g19_rank.npz", "rank_contract.json")


def test_golden_cases_are_the_ones_the_kernel_can_go_wrong_at(golden):
    z, meta, _ = golden
    assert meta["ks"] == [1, 3, 10, 2000] and meta["thresholds"] == [0, 1]
    _, _, offsets = R.metric_batch(z, "edges")
    lengths = np.diff(offsets).tolist()
    assert lengths[:11] == [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024]
    scores, _, offsets = R.metric_batch(z, "edges")
    equal, special = scores[offsets[11]:offsets[12]], z["m::edges::scores"][offsets[12]:offsets[13]]
    assert len(equal) == 70 and (equal == equal[0]).all()
    assert np.isposinf(special).any() and np.isneginf(special).any()
    zeros = special[special == 0]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()
    _, labels, offsets = R.metric_batch(z, "get")
    assert len(offsets) - 1 == 2000 and np.diff(offsets).max() == 30 and np.diff(offsets).min() == 0
    assert set(np.unique(labels)) == {0.0, 1.0, 2.0, 3.0}
    assert (R.metric_batch(z, "graded")[1] % 1 == 0.5).any()
    assert meta["ks"][-1] > max(np.diff(R.metric_batch(z, b)[2]).max() for b in meta["batches"])


@pytest.mark.parametrize("thr", [0, 1])
@pytest.mark.parametrize("batch", ["edges", "doctest", "get", "graded"])
def test_restatement_reproduces_the_reference_metrics(golden, batch, thr):
    z, meta, _ = golden
    ks = meta["ks"]
    rank, ints, f64 = R.restated(z, batch, thr, ks)
    assert np.array_equal(rank, z[f"m::{batch}::rank"].astype(np.int32)), "ranks"
    want = R.golden_f64(z, batch, thr)
    R.assert_metrics_close(f64, want, f"{batch} thr {thr}: per group")
    cols = R.f64_columns(len(ks))
    for name, sl in cols.items():
        R.assert_metrics_close(f64[:, sl].mean(axis=0).reshape(-1), np.reshape(z[f"m::{batch}::thr{thr}::mean::{name}"], -1),
                               f"{batch} thr {thr}: mean {name}")
    # the integers against the floats they determine
    offsets = R.metric_batch(z, batch)[2]
    assert np.array_equal(ints[:, 0], np.diff(offsets))
    assert np.array_equal(ints[:, 3:] / np.array(ks, np.float64), want[:, cols["precision"]])
    first = ints[:, 2].astype(np.float64)
    assert np.array_equal(np.where(first > 0, 1.0 / np.maximum(first, 1), 0.0), want[:, 2])
    assert ((ints[:, 1] == 0) == (ints[:, 2] == 0)).all() and (ints[:, 3:] <= ints[:, 1:2]).all()
    # the ranks of a group are a permutation of its positions
    for q in range(len(offsets) - 1):
        assert np.array_equal(np.sort(rank[offsets[q]:offsets[q + 1]]), np.arange(offsets[q + 1] - offsets[q]))


def test_average_precision_ignores_its_threshold(golden):
    z, _, _ = golden
    assert np.array_equal(z["m::graded::thr0::ap"], z["m::graded::thr1::ap"])
    assert not np.array_equal(z["m::graded::thr0::map"], z["m::graded::thr1::map"])


def test_restatement_reproduces_the_doctest_examples(golden):
    _, _, contract = golden
    for ex in contract["doctests"]:
        k = ex["kwargs"].get("k", 1)
        r = R.group_metrics(ex["y_true"], ex["y_pred"], [max(k, 1)], 0.)
        got = {"Precision": r["precision"][0], "AveragePrecision": r["ap"], "MeanAveragePrecision": r["map"], "MeanReciprocalRank": r["mrr"],
               "DiscountedCumulativeGain": r["dcg"][0] if k > 0 else 0., "NormalizedDiscountedCumulativeGain": r["ndcg"][0] if k > 0 else 0.}
        R.assert_metrics_close([got[ex["class"]]], [ex["value"]], f"{ex['class']} {ex['kwargs']}")


@pytest.mark.parametrize("case", ["1x1x1", "5x3x1", "67x4x1", "300x9x1", "33x2x3"])
def test_restatement_reproduces_the_reference_losses(golden, case):
    z, meta, _ = golden
    assert case in meta["loss_cases"]
    num_neg = int(case.split("x")[1])
    key = f"l::{case}::"
    y0, yt = torch.from_numpy(z[key + "y_pred"].astype(np.float64)), torch.from_numpy(z[key + "y_true"].astype(np.float64))
    g_none = torch.from_numpy(z[key + "hinge_none::g"].astype(np.float64))
    for red in ("none", "mean", "sum"):
        y = y0.clone().requires_grad_(True)
        out = R.rank_hinge64(y, num_neg, meta["margin"], red)
        ((out * g_none).sum() if red == "none" else out * meta["scalar_upstream"]).backward()
        assert np.allclose(out.detach().numpy(), z[f"{key}hinge_{red}::out"], rtol=1e-12, atol=1e-14), red
        assert np.allclose(y.grad.numpy(), z[f"{key}hinge_{red}::grad"], rtol=1e-12, atol=1e-14), red
    y = y0.clone().requires_grad_(True)
    out = R.rank_cross_entropy64(y, yt, num_neg)
    (out * meta["scalar_upstream"]).backward()
    assert np.allclose(out.item(), z[key + "ce::out"], rtol=1e-12, atol=1e-14)
    assert np.allclose(y.grad.numpy(), z[key + "ce::grad"], rtol=1e-11, atol=1e-14)
    assert (np.abs(z[key + "y_pred"].astype(np.float64)).max() <= 10)       # every logit within 20 of its row maximum (Q3)


def test_install_shim_serves_matchzoo_metrics_and_losses(tmp_path):
    """What Fitting/densebaseline_fit.py:19-20 imports, and the two loss files, resolve to the get_amd classes."""
    body = "\n".join(
        ["import matchzoo.metrics as MM, get_amd.ranking as R",
         "from matchzoo.metrics import average_precision, discounted_cumulative_gain, mean_average_precision, mean_reciprocal_rank, "
         "normalized_discounted_cumulative_gain, precision"]
        + [f"import matchzoo.metrics.{f} as sub; assert sub.{c} is R.{c} and MM.{c} is R.{c} and MM.{f} is sub"
           for f, c in METRIC_FILES.items()]
        + ["from matchzoo.metrics import " + ", ".join(METRIC_CLASSES),
           "assert precision.Precision is R.Precision and normalized_discounted_cumulative_gain.NormalizedDiscountedCumulativeGain "
           "is R.NormalizedDiscountedCumulativeGain",
           "from matchzoo.losses import RankHingeLoss, RankCrossEntropyLoss, rank_hinge_loss, rank_cross_entropy_loss",
           "from matchzoo.losses.rank_hinge_loss import RankHingeLoss as H",
           "from matchzoo.losses.rank_cross_entropy_loss import RankCrossEntropyLoss as C",
           "assert H is M.RankHingeLoss is RankHingeLoss is rank_hinge_loss.RankHingeLoss",
           "assert C is M.RankCrossEntropyLoss is RankCrossEntropyLoss is rank_cross_entropy_loss.RankCrossEntropyLoss",
           "assert Precision.__module__ == 'get_amd.ranking' and H.__module__ == 'get_amd.modules'"])
    run_in_fresh_interpreter(str(tmp_path), body, packages=("matchzoo",))


def test_metric_classes_keep_the_reference_contract(golden):
    from get_amd import ranking
    _, _, contract = golden
    for name in METRIC_CLASSES:
        cls, want = getattr(ranking, name), contract[name]
        assert cls.ALIAS == want["ALIAS"], name
        a = cls()
        assert {k.lstrip("_"): v for k, v in vars(a).items()} == want["defaults"], name
        other = cls(**{k: v + 1 for k, v in want["defaults"].items()})
        assert repr(a) == want["repr"] and repr(other) == want["repr_other_args"], name            # Q2: the unformatted format string
        assert (a == cls()) is want["equal_same_args"] and (a == other) is want["equal_other_args"], name
        assert (hash(a) == hash(other)) is want["hash_equal_other_args"] and hash(a) == hash(repr(a)), name
        assert a != object() and isinstance(a, ranking.BaseMetric)
    assert ranking.Precision(1, 0.) != ranking.DiscountedCumulativeGain(1, 0.)
    assert len({ranking.Precision(1), ranking.Precision(2), ranking.Precision(1)}) == 2            # equal hashes, __eq__ decides


def test_loss_modules_keep_the_reference_contract(golden):
    from get_amd import modules
    _, _, contract = golden
    h, c = modules.RankHingeLoss(), modules.RankCrossEntropyLoss()
    want = contract["RankHingeLoss"]
    assert list(h.__constants__) == want["__constants__"] and list(c.__constants__) == contract["RankCrossEntropyLoss"]["__constants__"]
    assert (h.num_neg, h.margin, h.reduction) == (want["num_neg"], want["margin"], want["reduction"])
    assert c.num_neg == contract["RankCrossEntropyLoss"]["num_neg"]
    h.num_neg, h.margin, c.num_neg = 4, 0.25, 2
    assert (h._num_neg, h._margin, c._num_neg) == (4, 0.25, 2)
    assert isinstance(type(h).num_neg, property) and isinstance(type(h).margin, property) and isinstance(type(c).num_neg, property)
    assert not list(h.parameters()) and not list(c.parameters())
    assert contract["ce_q3_reference_is_nan"] is True and contract["hinge_gradient_at_the_kink"] == [-1.0, 1.0]
    assert contract["loss_fp32_margin_of_a_tenth_of_the_bound"] <= 1.0


def test_cutoffs_below_one(golden):
    """Q4: Precision(k <= 0) raises when called, the two DCG classes return 0.; the batched interface wants k >= 1."""
    from get_amd import ranking
    _, _, contract = golden
    assert contract["precision_k0"] == "ValueError" and contract["dcg_k0"] == 0.0 and contract["ndcg_k0"] == 0.0
    for k in (0, -1):
        with pytest.raises(ValueError, match="greater than 0"):
            ranking.Precision(k=k)([1], [1.0])
        assert ranking.DiscountedCumulativeGain(k=k)([1], [1.0]) == 0.
        assert ranking.NormalizedDiscountedCumulativeGain(k=k)([1], [1.0]) == 0.
        for cls in (ranking.Precision, ranking.DiscountedCumulativeGain, ranking.NormalizedDiscountedCumulativeGain):
            with pytest.raises(ValueError, match="k >= 1"):
                ranking.ranking_metrics([cls(k=k)], torch.zeros(1), torch.zeros(1), [0, 1])
    with pytest.raises(TypeError):
        ranking.ranking_metrics([object()], torch.zeros(1), torch.zeros(1), [0, 1])


def test_cpu_tensors_are_refused():
    from get_amd import modules, ops, ranking
    y = torch.zeros(4, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rank_metrics(torch.zeros(3), torch.zeros(3), [0, 3], [1])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ranking.ranking_metrics([ranking.MeanReciprocalRank()], torch.zeros(3), torch.zeros(3), [0, 3])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rank_hinge(y, 1, 1., "mean")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.rank_cross_entropy(y, y, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        modules.RankHingeLoss()(y, None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        modules.RankCrossEntropyLoss()(y, y)
    with pytest.raises(ValueError, match="not one of"):
        ops.rank_hinge(y, 1, 1., "average")

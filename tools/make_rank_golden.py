"""Golden vectors of the ranking family -- the six metrics of matchzoo/metrics and the two losses of matchzoo/losses --, captured
from the upstream reference in the build container: never on the GPU machine, and no test reads the reference.

The eight files matchzoo/metrics/{precision, average_precision, mean_average_precision, mean_reciprocal_rank,
discounted_cumulative_gain, normalized_discounted_cumulative_gain}.py and matchzoo/losses/{rank_hinge_loss,
rank_cross_entropy_loss}.py are loaded by path (golden_common.load_reference).  The metric files import
``matchzoo.engine.base_metric`` and each other: empty stand-in packages ``matchzoo``, ``matchzoo.engine`` and ``matchzoo.metrics``
are registered in sys.modules and base_metric.py is loaded by path as well, so the real ``matchzoo`` package and its data pipeline
are never imported.  ``np.asscalar`` (average_precision.py:45), which numpy no longer has, is supplied as ``lambda a: a.item()``.
The generator writes

    tests/golden/g19_rank.npz            every case below
    tests/golden/rank_contract.json      ALIAS, repr string, constructor defaults and the __eq__ / __hash__ facts of the six metric
                                         classes, __constants__ and defaults of the two losses, the reference's doctest examples
                                         and the recorded fp32 margin of the loss cases

Metric batches (``m::<batch>::``: scores float16 and labels float16 -- both exact; float64 in ``doctest`` --, offsets int32,
``rank`` int16 = every item's position in base_metric.py:36-39's ordering of its group, and per threshold t in (0, 1)
``thr<t>::<metric>`` float64 per group, the cut-off metrics as (g, 4) for ks = [1, 3, 10, 2000]; ``thr<t>::mean::<metric>`` =
np.mean over the groups):
  edges   group lengths 0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024 (every length the smallest at which a wave or tile boundary
          is crossed), one all-equal group of 70 and one group holding +-inf and both zeros; integer labels 0..3
  doctest the groups of the reference's docstring examples (their scores, 0.2 and the like, are no fp32 numbers)
  get     2000 groups of 0..30 items, integer labels 0..3 (the GET-style evaluation shape)
  graded  48 groups of 0..120 items, labels in halves 0, 0.5 .. 3
Scores are 2 randn rounded to a quarter, so a group of any length holds many ties.

Loss cases (``l::<B>x<num_neg>x<c>::``): y_pred and y_true float16 (0.7 randn rounded to what float16 holds exactly; labels in
{0, 0.5, 1}, the positive row's at least 0.5), RankHingeLoss(margin=0.5) for 'none', 'mean' and 'sum' and RankCrossEntropyLoss, each
with a non-unit upstream gradient (``hinge_none::g`` (B, c) = randint(-16, 17) / 16; the scalars are multiplied by 1.5), in fp32
and in float64; the float64 results and gradients are stored.  The reference's own fp32 result must lie within one tenth of the
bounds the tests apply (outputs 1e-4 + 1e-4 |want|, gradients 1e-5 + 1e-4 |want|): golden_common.margin, recorded in the contract.

    python tools/make_rank_golden.py
"""
import inspect
import json
import os
import sys
import types
import zlib

import numpy as np
import torch

from golden_common import OUT, load_reference, margin, write_contract, write_npz

KS = [1, 3, 10, 2000]
THRESHOLDS = [0, 1]
EDGE_LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024]
LOSS_CASES = [(1, 1, 1), (5, 3, 1), (67, 4, 1), (300, 9, 1), (33, 2, 3)]
MARGIN = 0.5
SCALAR_UPSTREAM = 1.5
TOL_OUT = (1e-4, 1e-4)
TOL_GRAD = (1e-5, 1e-4)
METRIC_FILES = [("precision", "Precision"), ("average_precision", "AveragePrecision"),
                ("discounted_cumulative_gain", "DiscountedCumulativeGain"), ("mean_reciprocal_rank", "MeanReciprocalRank"),
                ("mean_average_precision", "MeanAveragePrecision"),
                ("normalized_discounted_cumulative_gain", "NormalizedDiscountedCumulativeGain")]
# the examples of the reference's docstrings: (class, kwargs, y_true, y_pred, the value printed there, digits it is rounded to)
DOCTESTS = [("Precision", {"k": 1}, [0, 0, 0, 1], [0.2, 0.4, 0.3, 0.1], 0.0, None),
            ("Precision", {"k": 2}, [0, 0, 0, 1], [0.2, 0.4, 0.3, 0.1], 0.0, None),
            ("Precision", {"k": 4}, [0, 0, 0, 1], [0.2, 0.4, 0.3, 0.1], 0.25, None),
            ("Precision", {"k": 5}, [0, 0, 0, 1], [0.2, 0.4, 0.3, 0.1], 0.2, None),
            ("AveragePrecision", {}, [0, 1], [0.1, 0.6], 0.75, 2),
            ("AveragePrecision", {}, [], [], 0.0, 2),
            ("MeanAveragePrecision", {}, [0, 1, 0, 0], [0.1, 0.6, 0.2, 0.3], 1.0, None),
            ("MeanReciprocalRank", {}, [1, 0, 0, 0], [0.2, 0.3, 0.7, 1.0], 0.25, None),
            ("DiscountedCumulativeGain", {"k": 1}, [0, 1, 2, 0], [0.4, 0.2, 0.5, 0.7], 0.0, None),
            ("DiscountedCumulativeGain", {"k": -1}, [0, 1, 2, 0], [0.4, 0.2, 0.5, 0.7], 0.0, 2),
            ("DiscountedCumulativeGain", {"k": 2}, [0, 1, 2, 0], [0.4, 0.2, 0.5, 0.7], 2.73, 2),
            ("DiscountedCumulativeGain", {"k": 3}, [0, 1, 2, 0], [0.4, 0.2, 0.5, 0.7], 2.73, 2),
            ("NormalizedDiscountedCumulativeGain", {"k": 1}, [0, 1, 2, 0], [0.4, 0.2, 0.5, 0.7], 0.0, None),
            ("NormalizedDiscountedCumulativeGain", {"k": 2}, [0, 1, 2, 0], [0.4, 0.2, 0.5, 0.7], 0.52, 2),
            ("NormalizedDiscountedCumulativeGain", {"k": 3}, [0, 1, 2, 0], [0.4, 0.2, 0.5, 0.7], 0.52, 2)]


def rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def load_metrics():
    """The six metric classes and sort_and_couple, with stand-in packages instead of the real matchzoo."""
    assert "matchzoo" not in sys.modules
    for pkg in ("matchzoo", "matchzoo.engine", "matchzoo.metrics"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    base = load_reference(os.path.join("matchzoo", "engine", "base_metric.py"), "matchzoo.engine.base_metric")
    sys.modules["matchzoo.engine.base_metric"] = base
    sys.modules["matchzoo.engine"].base_metric = base
    if not hasattr(np, "asscalar"):
        np.asscalar = lambda a: a.item()
    ref = {"sort_and_couple": base.sort_and_couple}
    for fname, cls in METRIC_FILES:
        mod = load_reference(os.path.join("matchzoo", "metrics", fname + ".py"), "matchzoo.metrics." + fname)
        sys.modules["matchzoo.metrics." + fname] = mod
        setattr(sys.modules["matchzoo.metrics"], fname, mod)
        setattr(sys.modules["matchzoo.metrics"], cls, getattr(mod, cls))
        ref[cls] = getattr(mod, cls)
    assert not hasattr(sys.modules["matchzoo"], "__file__")
    return ref


def quarter_scores(g, n):
    return np.round(2 * g.standard_normal(n) * 4) / 4 + 0.0           # + 0.0: no -0.0 from the rounding


def metric_batches():
    """name -> (scores float64, labels float64, offsets int32)."""
    out = {}
    g = rng("edges")
    groups = [(quarter_scores(g, n), g.integers(0, 4, n).astype(np.float64)) for n in EDGE_LENGTHS]
    groups.append((np.full(70, 0.25), g.integers(0, 4, 70).astype(np.float64)))
    special = np.array([0.0, -0.0, np.inf, 1.0, -np.inf, -0.0, 0.0, np.inf, -1.0, -np.inf, 0.0, 2.5])
    groups.append((special, np.array([1, 2, 0, 3, 1, 0, 2, 1, 0, 3, 1, 2], np.float64)))
    out["edges"] = groups
    seen = []
    for _, _, y_true, y_pred, _, _ in DOCTESTS:
        if (y_true, y_pred) not in seen:
            seen.append((y_true, y_pred))
    out["doctest"] = [(np.array(y_pred, np.float64), np.array(y_true, np.float64)) for y_true, y_pred in seen]
    g = rng("get")
    out["get"] = [(quarter_scores(g, n), g.integers(0, 4, n).astype(np.float64)) for n in g.integers(0, 31, 2000)]
    g = rng("graded")
    out["graded"] = [(quarter_scores(g, n), g.integers(0, 7, n) / 2.0) for n in g.integers(0, 121, 48)]
    res = {}
    for name, groups in out.items():
        offsets = np.zeros(len(groups) + 1, np.int32)
        offsets[1:] = np.cumsum([len(s) for s, _ in groups])
        res[name] = (np.concatenate([s for s, _ in groups]), np.concatenate([l for _, l in groups]), offsets)
    return res


def record_metrics(ref, store):
    for name, (scores, labels, offsets) in metric_batches().items():
        key = f"m::{name}::"
        for arr, k in ((scores, "scores"), (labels, "labels")):
            store[key + k] = arr.astype(np.float64 if name == "doctest" else np.float16)
            assert np.array_equal(store[key + k].astype(np.float64), arr) and \
                np.array_equal(np.signbit(store[key + k]), np.signbit(arr)), (name, k)
        store[key + "offsets"] = offsets
        n_groups = len(offsets) - 1
        rank = np.zeros(len(scores), np.int16)
        for q in range(n_groups):
            lo, hi = offsets[q], offsets[q + 1]
            s, l = [float(v) for v in scores[lo:hi]], [float(v) for v in labels[lo:hi]]
            # base_metric.py:38-39 on (index, score) instead of (label, score): the same key, the same stable sort
            order = [i for i, _ in sorted(list(zip(range(hi - lo), s)), key=lambda x: x[1], reverse=True)]
            coupled = ref["sort_and_couple"](l, s)
            assert [l[i] for i in order] == [float(v) for v in coupled[:, 0]] if hi > lo else len(coupled) == 0
            rank[lo + np.array(order, np.int64)] = np.arange(hi - lo)
        store[key + "rank"] = rank
        for thr in THRESHOLDS:
            res = {"ap": np.zeros(n_groups), "map": np.zeros(n_groups), "mrr": np.zeros(n_groups),
                   "precision": np.zeros((n_groups, len(KS))), "dcg": np.zeros((n_groups, len(KS))), "ndcg": np.zeros((n_groups, len(KS)))}
            for q in range(n_groups):
                lo, hi = offsets[q], offsets[q + 1]
                s, l = [float(v) for v in scores[lo:hi]], [float(v) for v in labels[lo:hi]]
                res["ap"][q] = ref["AveragePrecision"](threshold=thr)(l, s)
                res["map"][q] = ref["MeanAveragePrecision"](threshold=thr)(l, s)
                res["mrr"][q] = ref["MeanReciprocalRank"](threshold=thr)(l, s)
                for i, k in enumerate(KS):
                    res["precision"][q, i] = ref["Precision"](k=k, threshold=thr)(l, s)
                    res["dcg"][q, i] = ref["DiscountedCumulativeGain"](k=k, threshold=thr)(l, s)
                    res["ndcg"][q, i] = ref["NormalizedDiscountedCumulativeGain"](k=k, threshold=thr)(l, s)
            for k, v in res.items():
                assert np.isfinite(v).all(), (name, thr, k)
                store[f"{key}thr{thr}::{k}"] = v
                store[f"{key}thr{thr}::mean::{k}"] = np.mean(v, axis=0)
        print(name, n_groups, "groups,", len(scores), "items")


def metric_contract(ref):
    contract = {}
    for _, cls in METRIC_FILES:
        c = ref[cls]
        sig = inspect.signature(c.__init__)
        defaults = {k: p.default for k, p in sig.parameters.items() if k != "self"}
        a, b = c(), c(**{k: (v + 1) for k, v in defaults.items()})
        contract[cls] = {"ALIAS": c.ALIAS, "defaults": defaults, "repr": repr(a), "repr_other_args": repr(b),
                         "equal_same_args": a == c(), "equal_other_args": a == b, "hash_equal_other_args": hash(a) == hash(b)}
    examples = []
    for cls, kwargs, y_true, y_pred, printed, digits in DOCTESTS:
        value = ref[cls](**kwargs)(y_true, y_pred)
        assert (round(value, digits) if digits is not None else value) == printed, (cls, kwargs, value)
        examples.append({"class": cls, "kwargs": kwargs, "y_true": y_true, "y_pred": y_pred, "value": float(value)})
    contract["doctests"] = examples
    try:
        ref["Precision"](k=0)([1], [1.0])
        raise AssertionError("Precision(k=0) did not raise")
    except ValueError:
        contract["precision_k0"] = "ValueError"
    contract["dcg_k0"] = float(ref["DiscountedCumulativeGain"](k=0)([1], [1.0]))
    contract["ndcg_k0"] = float(ref["NormalizedDiscountedCumulativeGain"](k=0)([1], [1.0]))
    return contract


def half_exact(t):
    return t.half().float()


def run_losses(ref, case, dtype):
    b, num_neg, c = case
    name = "%dx%dx%d" % case
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()) ^ 0x5EED)
    rows = b * (num_neg + 1)
    y0 = half_exact(0.7 * torch.randn(rows, c, generator=g))
    yt = torch.randint(0, 3, (rows, c), generator=g).float() / 2
    yt[::num_neg + 1] = yt[::num_neg + 1].clamp_min(0.5)
    g_none = torch.randint(-16, 17, (b, c), generator=g).float() / 16
    res = {"y_pred": y0.numpy().astype(np.float16), "y_true": yt.numpy().astype(np.float16), "hinge_none::g": g_none.numpy().astype(np.float16)}
    for red in ("none", "mean", "sum"):
        y = y0.to(dtype).clone().requires_grad_(True)
        out = ref["RankHingeLoss"](num_neg=num_neg, margin=MARGIN, reduction=red)(y, None)
        ((out * g_none.to(dtype)).sum() if red == "none" else out * SCALAR_UPSTREAM).backward()
        res[f"hinge_{red}::out"], res[f"hinge_{red}::grad"] = out.detach().numpy().copy(), y.grad.numpy().copy()
    y = y0.to(dtype).clone().requires_grad_(True)
    out = ref["RankCrossEntropyLoss"](num_neg=num_neg)(y, yt.to(dtype))
    (out * SCALAR_UPSTREAM).backward()
    res["ce::out"], res["ce::grad"] = out.detach().numpy().copy(), y.grad.numpy().copy()
    return res


def loss_bound(k, want):
    atol, rtol = TOL_OUT if k.endswith("::out") else TOL_GRAD
    return atol + rtol * np.abs(want)


def record_losses(store, contract):
    ref = {"RankHingeLoss": load_reference(os.path.join("matchzoo", "losses", "rank_hinge_loss.py"), "_ref_rank_hinge_loss").RankHingeLoss,
           "RankCrossEntropyLoss": load_reference(os.path.join("matchzoo", "losses", "rank_cross_entropy_loss.py"),
                                                  "_ref_rank_cross_entropy_loss").RankCrossEntropyLoss}
    torch.set_num_threads(1)
    worst = 0.0
    for case in LOSS_CASES:
        r32, r64 = run_losses(ref, case, torch.float32), run_losses(ref, case, torch.float64)
        keys = [k for k in r64 if k.endswith("::out") or k.endswith("::grad")]
        w = margin(r32, r64, keys, loss_bound)
        print("%dx%dx%d: fp32 reference at %.4f of a tenth of the bound" % (*case, w))
        assert w <= 1.0, (case, w)
        worst = max(worst, w)
        for k, v in r64.items():
            assert np.isfinite(v.astype(np.float64)).all(), (case, k)
            store["l::%dx%dx%d::%s" % (*case, k)] = v
    hinge, ce = ref["RankHingeLoss"](), ref["RankCrossEntropyLoss"]()
    contract["RankHingeLoss"] = {"__constants__": list(hinge.__constants__), "num_neg": hinge.num_neg, "margin": hinge.margin,
                                 "reduction": hinge.reduction}
    contract["RankCrossEntropyLoss"] = {"__constants__": list(ce.__constants__), "num_neg": ce.num_neg}
    contract["loss_fp32_margin_of_a_tenth_of_the_bound"] = worst
    q3 = ce(torch.tensor([[0.0], [-200.0]]), torch.tensor([[1.0], [0.0]]))
    contract["ce_q3_reference_is_nan"] = bool(torch.isnan(q3))
    tie = torch.tensor([[1.0], [0.5]], dtype=torch.float64, requires_grad=True)
    ref["RankHingeLoss"](margin=MARGIN, reduction="sum")(tie, None).backward()
    contract["hinge_gradient_at_the_kink"] = [float(v) for v in tie.grad.reshape(-1)]


def main():
    ref = load_metrics()
    store = {}
    record_metrics(ref, store)
    contract = metric_contract(ref)
    record_losses(store, contract)
    meta = {"ks": KS, "thresholds": THRESHOLDS, "batches": ["edges", "doctest", "get", "graded"], "edge_lengths": EDGE_LENGTHS,
            "loss_cases": ["%dx%dx%d" % c for c in LOSS_CASES], "margin": MARGIN, "scalar_upstream": SCALAR_UPSTREAM}
    store["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    write_npz(os.path.join(OUT, "g19_rank.npz"), store)
    write_contract(os.path.join(OUT, "rank_contract.json"), contract)
    for f in ("g19_rank.npz", "rank_contract.json"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")
    assert os.path.getsize(os.path.join(OUT, "g19_rank.npz")) < 1024 * 1024


if __name__ == "__main__":
    main()

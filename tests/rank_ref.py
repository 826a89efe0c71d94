"""Plain numpy / torch float64 restatements of the ranking family (tests only): the six metrics of matchzoo/metrics on ONE group
and the two losses of matchzoo/losses.  tests/test_rank_cpu.py checks them against the reference's goldens without any kernel;
tests/test_gpu_rank.py uses them as the reference of csrc/rank_ops.hip."""
import math

import numpy as np
import torch


def order_of(keys):
    """Item indices in the order of Python's stable sorted(key=keys, reverse=True): descending, ties to the lower index."""
    keys = np.asarray(keys, dtype=np.float64)
    return sorted(range(len(keys)), key=lambda i: keys[i], reverse=True)


def rank_of(keys):
    """int32 (n,): the position of every item in order_of(keys)."""
    rank = np.zeros(len(keys), np.int32)
    rank[order_of(keys)] = np.arange(len(keys), dtype=np.int32)
    return rank


def _gain(label):
    return math.pow(2., label) - 1.


def group_metrics(labels, scores, ks, threshold=0.):
    """One group: dict with rank int32 (n,), ints [count, n_rel, first, hits per k], and the floats ap, map, mrr (numbers) and
    precision, dcg, ndcg (one per k), every sum taken left to right in ranking order."""
    labels = np.asarray(labels, dtype=np.float64)
    n = len(labels)
    order = order_of(scores)
    by_score = labels[order] if n else labels
    by_label = labels[order_of(labels)] if n else labels
    rel = by_score > threshold
    rel0 = by_score > 0.
    rels = np.flatnonzero(rel)
    first = int(rels[0]) + 1 if len(rels) else 0
    hits = [int(rel[:k].sum()) for k in ks]

    def dcg(seq, k):
        return sum((_gain(l) / math.log(2. + i) for i, l in enumerate(seq[:k]) if l > threshold), 0.)

    hits0 = np.cumsum(rel0)           # AveragePrecision: Precision(k + 1) at the default threshold 0, whatever `threshold` is
    ap = sum((int(hits0[k]) / (k + 1.) for k in range(n)), 0.) / n if n else 0.
    seen, acc = 0, 0.
    for idx in range(n):
        if rel[idx]:
            seen += 1
            acc += seen / (idx + 1.)
    dcgs = [dcg(by_score, k) for k in ks]
    idcgs = [dcg(by_label, k) for k in ks]
    rank = np.zeros(n, np.int32)
    rank[order] = np.arange(n, dtype=np.int32)
    return dict(rank=rank, ints=np.array([n, int(rel.sum()), first] + hits, np.int32), ap=ap, map=acc / seen if seen else 0.,
                mrr=1. / first if first else 0., precision=np.array([h / k for h, k in zip(hits, ks)], np.float64),
                dcg=np.array(dcgs, np.float64), ndcg=np.array([d / i if i != 0 else 0. for d, i in zip(dcgs, idcgs)], np.float64))


def batch_metrics(labels, scores, offsets, ks, threshold=0.):
    """All groups of a ragged batch: rank int32 (n,), ints int32 (g, 3 + nk), f64 (g, 3 + 3 nk) laid out as gh_rank_metrics
    lays them out: [ap, map, mrr, precision per k, dcg per k, ndcg per k]."""
    labels, scores = np.asarray(labels, dtype=np.float64), np.asarray(scores, dtype=np.float64)
    g, nk = len(offsets) - 1, len(ks)
    rank = np.zeros(len(labels), np.int32)
    ints = np.zeros((g, 3 + nk), np.int32)
    f64 = np.zeros((g, 3 + 3 * nk), np.float64)
    for q in range(g):
        lo, hi = int(offsets[q]), int(offsets[q + 1])
        r = group_metrics(labels[lo:hi], scores[lo:hi], ks, threshold)
        rank[lo:hi] = r["rank"]
        ints[q] = r["ints"]
        f64[q] = np.concatenate([[r["ap"], r["map"], r["mrr"]], r["precision"], r["dcg"], r["ndcg"]])
    return rank, ints, f64


def f64_columns(nk):
    """name -> columns of the f64 layout above."""
    return {"ap": slice(0, 1), "map": slice(1, 2), "mrr": slice(2, 3), "precision": slice(3, 3 + nk), "dcg": slice(3 + nk, 3 + 2 * nk),
            "ndcg": slice(3 + 2 * nk, 3 + 3 * nk)}


# ----------------------------------------------------------------------------- the goldens (tests/golden/g19_rank.npz)
METRIC_TOL = 1e-12            # of max(1, |want|): at most 1024 non-negative terms, each good to a few ulp (include/get_hip.h)
_RESTATED = {}


def metric_batch(z, name):
    """(scores float64, labels float64, offsets int32) of a golden batch."""
    key = f"m::{name}::"
    return z[key + "scores"].astype(np.float64), z[key + "labels"].astype(np.float64), z[key + "offsets"]


def golden_f64(z, name, thr):
    """The reference's per-group values of a golden batch in the f64 layout of batch_metrics."""
    key = f"m::{name}::thr{thr}::"
    return np.concatenate([z[key + "ap"][:, None], z[key + "map"][:, None], z[key + "mrr"][:, None], z[key + "precision"],
                           z[key + "dcg"], z[key + "ndcg"]], axis=1)


def restated(z, name, thr, ks):
    """batch_metrics of a golden batch, computed once per process and shared: nobody writes into what this returns."""
    if (name, thr) not in _RESTATED:
        scores, labels, offsets = metric_batch(z, name)
        _RESTATED[(name, thr)] = batch_metrics(labels, scores, offsets, ks, float(thr))
    return _RESTATED[(name, thr)]


def assert_metrics_close(got, want, what):
    """|got - want| <= 1e-12 max(1, |want|) elementwise, and exactly 0 where want is 0; prints the worst fraction of the bound."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    frac = np.abs(got - want) / (METRIC_TOL * np.maximum(1.0, np.abs(want)))
    print(f"{what}: {frac.max() if frac.size else 0.0:.4f} of the bound")
    assert (frac <= 1.0).all(), f"{what}: {frac.max():.3f} x the bound at {np.unravel_index(frac.argmax(), frac.shape)}"
    assert (got[want == 0] == 0).all(), f"{what}: a value that is 0 in the reference is not exactly 0"


def rank_hinge64(y_pred, num_neg, margin, reduction):
    """y_pred (B (num_neg + 1), c) torch float64 -> the hinge loss of rank_hinge_loss.py:54-66."""
    rows, c = y_pred.shape
    if rows % (num_neg + 1):
        raise ValueError("rows is no multiple of num_neg + 1")
    inst = y_pred.reshape(rows // (num_neg + 1), num_neg + 1, c)
    pos = inst[:, 0]
    neg_mean = inst[:, 1:].reshape(inst.shape[0], -1).mean(dim=1, keepdim=True)
    elem = torch.clamp_min(margin - (pos - neg_mean), 0.)
    return elem if reduction == "none" else (elem.mean() if reduction == "mean" else elem.sum())


def rank_cross_entropy64(y_pred, y_true, num_neg):
    """y_pred, y_true (B (num_neg + 1), c) torch float64 -> rank_cross_entropy_loss.py:29-38 with a stable log-softmax."""
    rows, c = y_pred.shape
    if rows % (num_neg + 1):
        raise ValueError("rows is no multiple of num_neg + 1")
    logits = y_pred.reshape(rows // (num_neg + 1), (num_neg + 1) * c)
    labels = y_true.reshape(rows // (num_neg + 1), (num_neg + 1) * c)
    return -(labels * torch.log_softmax(logits, dim=-1)).sum(dim=-1).mean()

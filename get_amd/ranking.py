"""Ranking evaluation on the device: the six metrics of the reference's ``matchzoo/metrics`` as drop-in classes, and one batched
pass over all queries.

The reference scores one query at a time on the host: ``sorted(zip(labels, scores), key=score, reverse=True)``
(matchzoo/engine/base_metric.py:36-39) and a Python loop per metric.  ``gh_rank_metrics`` ranks every group of a ragged batch by
counting and produces all six metrics of all groups in ONE launch:

    res = ranking_metrics([MeanAveragePrecision(), NormalizedDiscountedCumulativeGain(k=3)], scores, labels, offsets)

The classes keep the reference's names, ``ALIAS``, constructor arguments, ``__eq__`` and ``__hash__``; calling one scores a single
group (``metric(y_true, y_pred) -> float``), host arrays are uploaded.  Quirks of the reference that are kept:

  * ``AveragePrecision`` ignores its own threshold: it averages ``Precision(k + 1)`` built with the DEFAULT threshold 0
    (average_precision.py:41), i.e. (1/n) sum_k hits0(k) / k -- not the usual average precision.  It returns a Python float
    (the reference's ``np.asscalar`` is gone from numpy).
  * ``__repr__`` returns its format string unformatted (the reference calls ``str.format`` on a %-style string), and
    ``__hash__`` hashes that string: all instances of one class hash alike; ``__eq__`` still tells them apart.
  * ``Precision(k <= 0)`` raises ValueError when called, ``DiscountedCumulativeGain(k <= 0)`` returns 0. (and so does the
    normalised one).  The batched interface requires k >= 1.
  * A label above 1000 overflows ``math.pow`` in the reference; here it is not supported either (the gain is inf).
"""
from __future__ import annotations

import abc

import numpy as np
import torch

from . import ops

_K_MAX = 2 ** 31 - 1


class BaseMetric(abc.ABC):
    """matchzoo/engine/base_metric.py:8-33."""

    ALIAS = 'base_metric'
    _REPR = ''

    @abc.abstractmethod
    def __call__(self, y_true, y_pred) -> float:
        """The metric of ONE group: y_true its labels, y_pred its scores (device tensors, or host arrays, which are uploaded)."""

    def __repr__(self):
        return self._REPR            # the reference's format string, which it never fills in

    def __eq__(self, other):
        return (type(self) is type(other)) and (vars(self) == vars(other))

    def __hash__(self):
        return str(self).__hash__()

    # ---- what the batched pass needs to know: the cut-off to request (None: none) and the threshold
    def _cutoff(self):
        return getattr(self, "_k", None)

    def _pick(self, gd, ks):
        """This metric's column of group_f64 (g, 3 + 3 nk) for the cut-offs `ks` of the launch."""
        raise NotImplementedError

    def _one_group(self, y_true, y_pred) -> float:
        scores, labels = _on_device(y_pred), _on_device(y_true)
        k = self._cutoff()
        ks = [1 if k is None else min(int(k), _K_MAX)]
        _, _, gd, nan_count = ops.rank_metrics(scores, labels, [0, scores.shape[0]], ks, threshold=self._threshold)
        out = torch.cat([self._pick(gd, ks).reshape(-1), nan_count.double()]).tolist()
        _refuse_nan(out[1], out[2])
        return float(out[0])


def _on_device(a):
    if torch.is_tensor(a) and a.is_cuda:
        return a.reshape(-1)
    t = torch.as_tensor(np.asarray(a.cpu() if torch.is_tensor(a) else a))
    if t.dtype == torch.float16 or t.dtype == torch.bfloat16:
        t = t.float()
    elif not t.is_floating_point():
        t = t.double()
    return t.reshape(-1).to(torch.device("cuda", torch.cuda.current_device()))


def _refuse_nan(nan_scores, nan_labels):
    if nan_scores or nan_labels:
        raise ValueError(f"ranking metrics: {int(nan_scores)} NaN scores and {int(nan_labels)} NaN labels (the order of a group that "
                         "holds a NaN is undefined)")


class Precision(BaseMetric):
    """matchzoo/metrics/precision.py: relevant items among the first k of the ranking, over k (not over the group's length)."""

    ALIAS = 'precision'
    _REPR = '%s@%s(%s)'

    def __init__(self, k: int = 1, threshold: float = 0.):
        self._k = k
        self._threshold = threshold

    def _pick(self, gd, ks):
        return gd[:, 3 + ks.index(min(int(self._k), _K_MAX))]

    def __call__(self, y_true, y_pred) -> float:
        if self._k <= 0:
            raise ValueError("k must be greater than 0. %s received." % (self._k,))
        return self._one_group(y_true, y_pred)


class AveragePrecision(BaseMetric):
    """matchzoo/metrics/average_precision.py: the mean over k = 1 .. n of Precision(k) AT THRESHOLD 0 (see the module text)."""

    ALIAS = ['average_precision', 'ap']
    _REPR = '%s(%s)'

    def __init__(self, threshold: float = 0.):
        self._threshold = threshold

    def _pick(self, gd, ks):
        return gd[:, 0]

    def __call__(self, y_true, y_pred) -> float:
        return self._one_group(y_true, y_pred)


class MeanAveragePrecision(BaseMetric):
    """matchzoo/metrics/mean_average_precision.py."""

    ALIAS = ['mean_average_precision', 'map']
    _REPR = '%s(%s)'

    def __init__(self, threshold: float = 0.):
        self._threshold = threshold

    def _pick(self, gd, ks):
        return gd[:, 1]

    def __call__(self, y_true, y_pred) -> float:
        return self._one_group(y_true, y_pred)


class MeanReciprocalRank(BaseMetric):
    """matchzoo/metrics/mean_reciprocal_rank.py."""

    ALIAS = ['mean_reciprocal_rank', 'mrr']
    _REPR = '%s(%s)'

    def __init__(self, threshold: float = 0.):
        self._threshold = threshold

    def _pick(self, gd, ks):
        return gd[:, 2]

    def __call__(self, y_true, y_pred) -> float:
        return self._one_group(y_true, y_pred)


class DiscountedCumulativeGain(BaseMetric):
    """matchzoo/metrics/discounted_cumulative_gain.py: gain 2^label - 1, discount ln(2 + position), natural logarithm."""

    ALIAS = ['discounted_cumulative_gain', 'dcg']
    _REPR = '%s@%s(%s)'

    def __init__(self, k: int = 1, threshold: float = 0.):
        self._k = k
        self._threshold = threshold

    def _pick(self, gd, ks):
        nk = len(ks)
        return gd[:, 3 + nk + ks.index(min(int(self._k), _K_MAX))]

    def __call__(self, y_true, y_pred) -> float:
        if self._k <= 0:
            return 0.
        return self._one_group(y_true, y_pred)


class NormalizedDiscountedCumulativeGain(BaseMetric):
    """matchzoo/metrics/normalized_discounted_cumulative_gain.py: DCG over the DCG of the group ordered by label; 0 when that is 0."""

    ALIAS = ['normalized_discounted_cumulative_gain', 'ndcg']
    _REPR = '%s@%s(%s)'

    def __init__(self, k: int = 1, threshold: float = 0.):
        self._k = k
        self._threshold = threshold

    def _pick(self, gd, ks):
        nk = len(ks)
        return gd[:, 3 + 2 * nk + ks.index(min(int(self._k), _K_MAX))]

    def __call__(self, y_true, y_pred) -> float:
        if self._k <= 0:
            return 0.
        return self._one_group(y_true, y_pred)


METRICS = (Precision, AveragePrecision, MeanAveragePrecision, MeanReciprocalRank, DiscountedCumulativeGain,
           NormalizedDiscountedCumulativeGain)


def ranking_metrics(metrics, scores, labels, offsets) -> dict:
    """{metric: the mean of the metric over all g groups} for a list of metric instances, from scores (n,) and labels (n,) on the
    device and the g + 1 group offsets (ops.rank_metrics says what they may be; a host sequence keeps the call free of any
    synchronisation but the final read-back).  An empty group counts as 0, which is what the reference's classes return for
    ``[]``.  Metrics that share a threshold share a launch -- one launch when they all do, as an evaluation's usually do
    (AveragePrecision goes with any: it does not read its threshold) --, the values are read back once and the mean is taken in
    float64 on the host.  Every metric with a cut-off needs k >= 1; at most eight different cut-offs per threshold.

    Raises ValueError when a score or a label is NaN."""
    metrics = list(metrics)
    for m in metrics:
        if not isinstance(m, METRICS):
            raise TypeError(f"ranking_metrics: {m!r} is none of the six ranking metrics")
        if m._cutoff() is not None and m._cutoff() < 1:
            raise ValueError(f"ranking_metrics: {type(m).__name__} with k = {m._cutoff()}: the batched interface requires k >= 1")
    if not metrics:
        return {}
    by_thr = {}
    for m in metrics:
        if not isinstance(m, AveragePrecision):
            by_thr.setdefault(float(m._threshold), []).append(m)
    if not by_thr:
        by_thr[0.0] = []
    first = next(iter(by_thr))
    by_thr[first] += [m for m in metrics if isinstance(m, AveragePrecision)]
    columns, nans = [], []
    for thr, group in by_thr.items():
        ks = sorted({min(int(m._cutoff()), _K_MAX) for m in group if m._cutoff() is not None}) or [1]
        _, _, gd, nan_count = ops.rank_metrics(scores, labels, offsets, ks, threshold=thr)
        columns += [(m, m._pick(gd, ks)) for m in group]
        nans.append(nan_count.double())
    host = torch.cat([torch.stack([col for _, col in columns]).reshape(-1)] + nans).cpu().numpy()      # the one read-back
    g = columns[0][1].shape[0]
    values, counts = host[:len(columns) * g].reshape(len(columns), g), host[len(columns) * g:].reshape(-1, 2)
    _refuse_nan(counts[:, 0].max(), counts[:, 1].max())
    return {m: float(np.mean(values[i])) for i, (m, _) in enumerate(columns)}

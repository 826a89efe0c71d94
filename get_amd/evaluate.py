"""Epoch-end evaluation on the device.

The reference's ``CharManFitterQueryRepr1.evaluate`` (Fitting/FittingFC/char_man_fitter_query_repr1.py:260-364) runs one B=1
forward per claim, reads the prediction and the class-1 score back per claim (:359-360) and hands the lists to sklearn
(``_computing_metrics``, :366-420).  Every one of its 13 numbers is an exact function of a few integers -- the confusion matrix
and a pair count for the AUC -- which ``gh_cls_metrics`` produces from the logits of ONE batched pass:

    results = evaluate(model, batch)                       # batched_predict + one metrics launch + one 8 (c*c + 8)-byte read-back
    improved = selection.update(results, epoch)            # declare_fitter.py:149-162

:func:`classification_metrics` takes any logits, so a data-parallel caller gathers its ranks' logits and labels first.
sklearn is not needed.
"""
from __future__ import annotations

import math

from . import ops
from .batch import batched_predict
from .keywords import KeyWordSettings as K


def metrics_from_counts(counts, c: int, output_size: int = None) -> dict:
    """The 13 values of ``_computing_metrics`` (:381-418), float64 host arithmetic on the integers of gh_cls_metrics
    (`counts`: c*c + 8 of them, include/get_hip.h).  sklearn's conventions: a ratio with a zero denominator is 0.0 (its
    ``zero_division`` default), the macro average runs over the classes that occur among the labels or the predictions, not
    over all c; the AUC is nan when either side is empty."""
    counts = [int(v) for v in counts]
    if len(counts) != c * c + ops.CLS_EXTRA:
        raise ValueError(f"metrics_from_counts: {c * c + ops.CLS_EXTRA} integers expected for c = {c}, got {len(counts)}")
    output_size = c if output_size is None else int(output_size)
    conf = [counts[t * c:(t + 1) * c] for t in range(c)]
    u2, n_pos, n_neg, bad_label, nan_rows = counts[c * c:c * c + 5]
    if bad_label or nan_rows:
        raise ValueError(f"classification_metrics: {bad_label} rows with a label outside [0, {c}) and {nan_rows} rows with a NaN "
                         "logit (sklearn raises on such input as well)")
    rows = [sum(conf[k]) for k in range(c)]
    cols = [sum(conf[t][k] for t in range(c)) for k in range(c)]
    n = sum(rows)

    def ratio(a, b):
        return a / b if b else 0.0

    def prf(k):
        if k >= c:                      # a class the model has no logit for: absent from labels and predictions alike
            return 0.0, 0.0, 0.0
        p, r = ratio(conf[k][k], cols[k]), ratio(conf[k][k], rows[k])
        return p, r, ratio(2.0 * p * r, p + r)

    present = [k for k in range(c) if rows[k] + cols[k] > 0]
    res = {
        K.AUC_metric: u2 / (2.0 * n_pos * n_neg) if n_pos and n_neg else math.nan,
        K.F1_macro: ratio(sum(prf(k)[2] for k in present), len(present)),
        K.F1_micro: ratio(sum(conf[k][k] for k in range(c)), n),
        K.F1: prf(1)[2],
    }
    res[K.PrecisionTrueCls], res[K.RecallTrueCls], res[K.F1TrueCls] = prf(1)
    res[K.PrecisionFalseCls], res[K.RecallFalseCls], res[K.F1FalseCls] = prf(0)
    res[K.PrecisionMixedCls], res[K.RecallMixedCls], res[K.F1MixedCls] = prf(2) if output_size == 3 else (0.0, 0.0, 0.0)
    return res


def classification_metrics(phi, labels, output_size: int = None) -> dict:
    """The results dict of the reference's ``_computing_metrics`` (keys: ``KeyWordSettings.CLS_METRICS``) from logits
    phi (n, c) and labels (n,) on the device: one kernel call, one read-back of c*c + 8 integers, float64 on the host.

    Predictions are ``phi.argmax(1)`` and the AUC ranks by the raw class-1 logit ``phi[:, 1]`` (:353-360; the reference applies no
    softmax either), against ``label == 1`` as the positive class (``roc_curve(pos_label=1)``: a class-2 row is a negative).
    `output_size` (default c) is the fitter's ``self.output_size``: the mixed-class triple is 0.0 unless it is 3 (:396-401).

    One deviation: with three classes the reference's ``f1_score(true, pred)`` (:385, ``average='binary'``) raises on the
    multiclass targets, so its evaluate never returns; here ``"f1"`` carries the class-1 F1 for every c (what it is for c = 2).

    Raises ValueError when a label lies outside [0, c) or a row holds a NaN logit."""
    out, _ = ops.cls_metrics(phi, labels, pos_class=1)
    return metrics_from_counts(out.tolist(), phi.shape[1], output_size)


def evaluate(model, batch, output_ranking: bool = False, claims_per_call: int = 0):
    """``CharManFitterQueryRepr1.evaluate`` (:260-364) on a device-resident :class:`~get_amd.batch.NativeBatch` holding the
    validation or test claims: one batched forward (``batched_predict``; `claims_per_call` bounds its peak memory) and
    :func:`classification_metrics` on its logits and ``batch.labels``.  The model's training flag is left as it was.

    Returns the results dict; with ``output_ranking=True`` returns ``(dict, (phi, word_att, evd_att))``, the observables
    ``_prepare_error_analysis`` (:422-472) consumes, as ``batched_predict`` returns them."""
    phi, word_att, evd_att = batched_predict(model, batch, claims_per_call=claims_per_call)
    results = classification_metrics(phi, batch.labels, output_size=phi.shape[1])
    if output_ranking:
        return results, (phi, word_att, evd_att)
    return results


class ModelSelection:
    """The model-selection and early-stopping rule of the reference's epoch loop (Fitting/FittingFC/declare_fitter.py:149-162),
    pure host logic: an epoch is the new best when its ``f1_macro`` is higher, or equal with a higher ``auc`` (a nan AUC never
    wins a tie); every other epoch counts against the patience, and ``should_stop`` turns true once MORE than `patience`
    epochs in a row have failed to improve (``>``, :159)."""

    def __init__(self, patience: int = None):
        self.patience = patience
        self.best = None                    # results dict of the best epoch so far
        self.best_epoch = None
        self.count_patience_epochs = 0

    def update(self, results: dict, epoch: int) -> bool:
        f1, auc = results[K.F1_macro], results[K.AUC_metric]
        # the reference starts from a best of (0, 0) (:86): an epoch that scores nothing is never the winner
        best_f1, best_auc = (self.best[K.F1_macro], self.best[K.AUC_metric]) if self.best is not None else (0.0, 0.0)
        improved = f1 > best_f1 or (f1 == best_f1 and auc > best_auc)        # nan > x and x > nan are both False
        if improved:
            self.best, self.best_epoch = dict(results), epoch
            self.count_patience_epochs = 0
        else:
            self.count_patience_epochs += 1
        return improved

    @property
    def should_stop(self) -> bool:
        # a patience of None or 0 never stops, as `self._early_stopping_patience and ...` (:160)
        return bool(self.patience) and self.count_patience_epochs > self.patience

"""Plain numpy float64 restatement of what the evaluation path computes: the integers of gh_cls_metrics (argmax, confusion
matrix, the O(n^2) AUC pair count, the rejected-row counts) and the 13 formulas of the reference's `_computing_metrics`
(Fitting/FittingFC/char_man_fitter_query_repr1.py:381-418) under sklearn's conventions.  No sklearn, no torch."""
import math

import numpy as np

KEYS = ["auc", "f1_macro", "f1_micro", "f1",
        "precision_true_cls", "recall_true_cls", "f1_true_cls",
        "precision_false_cls", "recall_false_cls", "f1_false_cls",
        "precision_mixed_cls", "recall_mixed_cls", "f1_mixed_cls"]
EXTRA = 8


def argmax_first(phi):
    """Row argmax, first index among equal maxima; a NaN counts as the maximum (numpy and torch agree)."""
    return np.argmax(np.asarray(phi), axis=1).astype(np.int32)


def counts(phi, labels, pos_class=1, block=1024):
    """(out [c*c + 8] int64, pred [n] int32) as include/get_hip.h states them for gh_cls_metrics."""
    phi = np.asarray(phi, dtype=np.float32)
    labels = np.asarray(labels).astype(np.int64)
    n, c = phi.shape
    pred = argmax_first(phi)
    bad = (labels < 0) | (labels >= c)
    nan = np.isnan(phi).any(axis=1) & ~bad
    ok = ~bad & ~nan
    out = np.zeros(c * c + EXTRA, dtype=np.int64)
    np.add.at(out, labels[ok] * c + pred[ok], 1)
    s = phi[:, pos_class].astype(np.float64)             # exact: every float32 is a float64, comparisons carry over
    sp, sn = s[ok & (labels == pos_class)], s[ok & (labels != pos_class)]
    u2 = 0
    for lo in range(0, len(sp), block):                  # every (positive, negative) pair, a block of positives at a time
        a = sp[lo:lo + block, None]
        u2 += 2 * int((a > sn[None, :]).sum()) + int((a == sn[None, :]).sum())
    out[c * c:c * c + 5] = [u2, len(sp), len(sn), int(bad.sum()), int(nan.sum())]
    return out, pred


def metrics_from_counts(out, c, output_size=None):
    out = [int(v) for v in out]
    output_size = c if output_size is None else output_size
    conf = np.array(out[:c * c], dtype=np.float64).reshape(c, c)
    u2, n_pos, n_neg = out[c * c:c * c + 3]
    rows, cols, diag = conf.sum(1), conf.sum(0), np.diag(conf)

    def div(a, b):
        return float(a) / float(b) if b else 0.0

    def prf(k):
        if k >= c:
            return 0.0, 0.0, 0.0
        p, r = div(diag[k], cols[k]), div(diag[k], rows[k])
        return p, r, div(2.0 * p * r, p + r)

    present = [k for k in range(c) if rows[k] + cols[k] > 0]
    res = {"auc": u2 / (2.0 * n_pos * n_neg) if n_pos and n_neg else math.nan,
           "f1_macro": div(sum(prf(k)[2] for k in present), len(present)),
           "f1_micro": div(diag.sum(), conf.sum()),
           "f1": prf(1)[2]}
    for name, k in (("true", 1), ("false", 0), ("mixed", 2)):
        p, r, f = prf(k) if (name != "mixed" or output_size == 3) else (0.0, 0.0, 0.0)
        res[f"precision_{name}_cls"], res[f"recall_{name}_cls"], res[f"f1_{name}_cls"] = p, r, f
    return res


def metrics(phi, labels, output_size=None):
    phi = np.asarray(phi, dtype=np.float32)
    out, _ = counts(phi, labels, pos_class=1)
    return metrics_from_counts(out, phi.shape[1], output_size)


def close(a, b, tol=1e-12):
    """|a - b| <= tol, nan equal to nan."""
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= tol

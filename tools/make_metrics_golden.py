"""Golden values of the evaluation metrics (tests/golden/g18_metrics.json), recorded in the build container -- never on the GPU
machine, and no test reads the reference.

Per case: logits (n, c) as float32-exact numbers, labels, the fitter's ``output_size`` and the 13 values of the results dict of
``CharManFitterQueryRepr1._computing_metrics`` (Fitting/FittingFC/char_man_fitter_query_repr1.py:366-420), fed as ``evaluate``
feeds it (:353-362): ``true_labels`` the labels, ``predicted_labels`` the row argmax as floats, ``predicted_probs`` the class-1
logit.  The method itself is called when the fitter imports through oracle/_refshim.py; otherwise, and for the three-class
cases -- where its ``f1_score(true, pred)`` (:385, average='binary') raises on multiclass targets --, the recorder makes the
same sklearn calls as :381-401 with ``"f1"`` taken as the class-1 F1.  ``meta.source`` and each case's ``source`` say which of the
two produced the values; the key strings come from the reference's ``KeyWordSettings.CLS_METRICS`` when it imports.
The file holds data only.  nan is stored as the string "nan".

    python tools/make_metrics_golden.py
"""
import json
import math
import os
import types
import warnings
import zlib

import numpy as np

from golden_common import OUT, _refshim

KEYS = ["auc", "f1_macro", "f1_micro", "f1",
        "precision_true_cls", "recall_true_cls", "f1_true_cls",
        "precision_false_cls", "recall_false_cls", "f1_false_cls",
        "precision_mixed_cls", "recall_mixed_cls", "f1_mixed_cls"]


def rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def gauss(name, n, c, labels_of=None):
    g = rng(name)
    phi = g.standard_normal((n, c)).astype(np.float32)
    labels = g.integers(0, c if labels_of is None else labels_of, n)
    phi[np.arange(n), labels] += np.float32(0.75)           # better than chance, far from perfect
    return phi, labels


def ties(name, n, c):
    g = rng(name)
    return g.integers(-3, 4, (n, c)).astype(np.float32), g.integers(0, c, n)


def cases():
    out = {}
    out["bin_gauss40"] = (*gauss("bin_gauss40", 40, 2), 2)
    out["bin_ties60"] = (*ties("bin_ties60", 60, 2), 2)
    out["bin_ties900"] = (*ties("bin_ties900", 900, 2), 2)
    # f1_score([0,0,0,1], [0,0,0,0], average='macro'): the macro mean runs over the classes that occur
    out["bin_all_pred0"] = (np.array([[1, 0], [2, -1], [.5, .25], [3, 1]], np.float32), np.array([0, 0, 0, 1]), 2)
    out["bin_only_pos"] = (gauss("bin_only_pos", 12, 2)[0], np.ones(12, np.int64), 2)          # AUC nan
    out["bin_only_neg"] = (gauss("bin_only_neg", 12, 2)[0], np.zeros(12, np.int64), 2)         # AUC nan
    lab = rng("bin_perfect").integers(0, 2, 30)
    out["bin_perfect"] = (np.stack([1.0 - lab, lab.astype(np.float64)], 1).astype(np.float32) * 2, lab, 2)
    z = np.array([[0.0, -0.0], [-0.0, 0.0], [0.0, 0.0], [-0.0, -0.0], [1.0, -0.0], [-1.0, 0.0]], np.float32)
    out["bin_signed_zero"] = (z, np.array([1, 0, 1, 0, 0, 1]), 2)
    out["tri_gauss50"] = (*gauss("tri_gauss50", 50, 3), 3)
    out["tri_ties80"] = (*ties("tri_ties80", 80, 3), 3)
    phi, labels = gauss("tri_no_class2", 30, 3, labels_of=2)
    phi[:, 2] = -9.0                                         # class 2 neither labelled nor predicted: absent from the macro mean
    out["tri_no_class2"] = (phi, labels, 3)
    phi, labels = gauss("tri_gauss300", 300, 3)
    out["tri_gauss300"] = (phi, labels, 3)
    return out


def sklearn_calls(true, pred, prob, output_size, binary_f1):
    """The calls of :381-401, in order; `binary_f1` False replaces :385 (which raises for three classes) by the class-1 F1."""
    import sklearn.metrics
    from sklearn.metrics import f1_score, precision_score, recall_score
    fpr, tpr, _ = sklearn.metrics.roc_curve(true, prob, pos_label=1)
    res = {"auc": sklearn.metrics.auc(fpr, tpr),
           "f1_macro": f1_score(true, pred, average="macro"),
           "f1_micro": f1_score(true, pred, average="micro"),
           "f1": f1_score(true, pred) if binary_f1 else f1_score(true, pred, labels=[1], average=None)[0]}
    for name, k in (("true", 1), ("false", 0), ("mixed", 2)):
        on = name != "mixed" or output_size == 3
        res[f"precision_{name}_cls"] = precision_score(true, pred, labels=[k], average=None)[0] if on else 0.0
        res[f"recall_{name}_cls"] = recall_score(true, pred, labels=[k], average=None)[0] if on else 0.0
        res[f"f1_{name}_cls"] = f1_score(true, pred, labels=[k], average=None)[0] if on else 0.0
    return res


def load_fitter():
    """(the fitter class, the reference's CLS_METRICS) or (None, None) when the fitter does not import."""
    try:
        _refshim.install()
        from Fitting.FittingFC import char_man_fitter_query_repr1 as mod
        from setting_keywords import KeyWordSettings
        return mod.CharManFitterQueryRepr1, list(KeyWordSettings.CLS_METRICS)
    except Exception as e:          # noqa: BLE001 -- any import problem of the upstream tree selects the sklearn path
        print(f"reference fitter not importable ({type(e).__name__}: {e}); recording from the sklearn calls")
        return None, None


def main():
    fitter, ref_keys = load_fitter()
    keys = ref_keys or KEYS
    assert keys == KEYS, keys
    recorded, sources = {}, set()
    for name, (phi, labels, output_size) in cases().items():
        phi = np.ascontiguousarray(phi, dtype=np.float32)
        true = [int(v) for v in labels]
        pred = [float(v) for v in phi.argmax(1)]
        prob = [float(v) for v in phi[:, 1]]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")          # sklearn warns about empty classes and one-sided ROC curves; the values stand
            res, source = None, "sklearn_calls"
            if fitter is not None and phi.shape[1] == 2:
                res = fitter._computing_metrics(types.SimpleNamespace(output_size=output_size), true_labels=true,
                                                predicted_labels=pred, predicted_probs=prob)
                source = "reference__computing_metrics"
            if res is None:
                res = sklearn_calls(true, pred, prob, output_size, binary_f1=phi.shape[1] == 2)
        sources.add(source)
        expected = {k: ("nan" if math.isnan(float(res[k])) else float(res[k])) for k in keys}
        recorded[name] = {"logits": [[float(v) for v in row] for row in phi], "labels": true, "output_size": output_size,
                          "expected": expected, "source": source}
        print(name, source, {k: expected[k] for k in keys[:4]})
    import sklearn
    doc = {"meta": {"keys": keys, "source": sorted(sources), "sklearn": sklearn.__version__,
                    "keys_from": "reference KeyWordSettings.CLS_METRICS" if ref_keys else "recorder"},
           "cases": recorded}
    path = os.path.join(OUT, "g18_metrics.json")
    with open(path, "w") as fh:
        json.dump(doc, fh, sort_keys=True, separators=(",", ":"))
        fh.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

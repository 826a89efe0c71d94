"""CPU checks of the evaluation path: the numpy restatement tests/eval_ref.py against the recorded values of the reference's
`_computing_metrics` (tests/golden/g18_metrics.json) and against sklearn where that is installed, the host arithmetic of
get_amd.evaluate on the same integers, the model-selection rule of declare_fitter.py:149-162, and the new key strings.

Bound 1e-12: the recorded AUC is a trapezoid sum of at most n <= 10^3 terms with a rounding of 1e-16 each, U2 / (2 n_pos n_neg)
is one division of exact integers; every other value is a handful of divisions."""
import json
import math
import os

import numpy as np
import pytest

from tests import eval_ref

TOL = 1e-12


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "g18_metrics.json")))


def expected_of(case):
    return {k: (math.nan if v == "nan" else float(v)) for k, v in case["expected"].items()}


def test_fixture_holds_about_a_dozen_cases_from_the_reference(golden):
    assert 10 <= len(golden["cases"]) <= 16
    assert "reference__computing_metrics" in golden["meta"]["source"]
    sizes = {len(c["labels"]) for c in golden["cases"].values()}
    assert max(sizes) <= 1000 and {2, 3} == {len(c["logits"][0]) for c in golden["cases"].values()}
    assert any(math.isnan(expected_of(c)["auc"]) for c in golden["cases"].values())


def test_eval_ref_reproduces_the_recorded_reference_values(golden):
    for name, case in golden["cases"].items():
        got = eval_ref.metrics(np.array(case["logits"], np.float32), case["labels"], case["output_size"])
        want = expected_of(case)
        assert list(got) == golden["meta"]["keys"]
        for k in want:
            assert eval_ref.close(got[k], want[k], TOL), (name, k, got[k], want[k])


def test_host_arithmetic_of_the_package_on_eval_ref_integers(golden):
    """get_amd.evaluate.metrics_from_counts is what runs behind the kernel: fed with eval_ref's integers it must give the
    recorded values, and refuse counts that report rejected rows."""
    from get_amd.evaluate import metrics_from_counts
    for name, case in golden["cases"].items():
        phi = np.array(case["logits"], np.float32)
        out, _ = eval_ref.counts(phi, case["labels"])
        got = metrics_from_counts(out.tolist(), phi.shape[1], case["output_size"])
        for k, w in expected_of(case).items():
            assert eval_ref.close(got[k], w, TOL), (name, k, got[k], w)
    out, _ = eval_ref.counts(np.array([[0, 1], [1, 0], [np.nan, 0]], np.float32), [0, 5, 1])
    assert out[4:9].tolist() == [0, 0, 1, 1, 1]
    with pytest.raises(ValueError, match="1 rows with a label outside.*1 rows with a NaN"):
        metrics_from_counts(out.tolist(), 2)


def test_eval_ref_counts_on_a_case_worked_by_hand():
    # scores s = phi[:, 1]: positives {2, 0, 0}, negatives {0, -0, 1, -inf}
    phi = np.array([[0, 2], [1, 0], [0, 0], [5, 0], [0, -0.0], [1, 1], [0, -np.inf]], np.float32)
    labels = [1, 1, 1, 0, 0, 0, 0]
    out, pred = eval_ref.counts(phi, labels)
    assert pred.tolist() == [1, 0, 0, 0, 0, 0, 0]            # ties go to the first index
    # s_i = 2 beats all four: 8; each 0 ties with 0 and -0 (2), loses to 1, beats -inf (2): 4 each
    assert out[4:9].tolist() == [16, 3, 4, 0, 0]
    assert out[:4].tolist() == [4, 0, 2, 1]
    m = eval_ref.metrics_from_counts(out, 2)
    assert m["auc"] == 16 / 24 and m["f1_micro"] == 5 / 7 and m["recall_true_cls"] == 1 / 3 and m["precision_true_cls"] == 1.0
    assert m["precision_mixed_cls"] == m["recall_mixed_cls"] == m["f1_mixed_cls"] == 0.0
    # the macro mean runs over the classes that occur: f1_score([0,0,0,1], [0,0,0,0], average='macro') = (6/7 + 0) / 2
    m = eval_ref.metrics(np.array([[1, 0]] * 4, np.float32), [0, 0, 0, 1])
    assert abs(m["f1_macro"] - 3 / 7) <= TOL
    m = eval_ref.metrics(np.array([[1, 0, 0]] * 4, np.float32), [0, 0, 0, 0], output_size=3)
    assert m["f1_macro"] == 1.0 and math.isnan(m["auc"])


def test_eval_ref_agrees_with_sklearn():
    sk = pytest.importorskip("sklearn.metrics")
    import warnings
    rng = np.random.default_rng(18)
    for trial in range(40):
        c = 2 + trial % 2
        n = int(rng.integers(2, 400))
        phi = (rng.integers(-3, 4, (n, c)) if trial % 4 < 2 else rng.standard_normal((n, c))).astype(np.float32)
        labels = rng.integers(0, c, n)
        if trial % 10 == 9:
            labels[:] = trial % 3 % c
        pred = phi.argmax(1)
        got = eval_ref.metrics(phi, labels, output_size=c)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fpr, tpr, _ = sk.roc_curve(labels, phi[:, 1], pos_label=1)
            want = {"auc": sk.auc(fpr, tpr), "f1_macro": sk.f1_score(labels, pred, average="macro"),
                    "f1_micro": sk.f1_score(labels, pred, average="micro"),
                    "f1": sk.f1_score(labels, pred, labels=[1], average=None)[0]}
            for name, k in (("true", 1), ("false", 0), ("mixed", 2)):
                on = name != "mixed" or c == 3
                want[f"precision_{name}_cls"] = sk.precision_score(labels, pred, labels=[k], average=None)[0] if on else 0.0
                want[f"recall_{name}_cls"] = sk.recall_score(labels, pred, labels=[k], average=None)[0] if on else 0.0
                want[f"f1_{name}_cls"] = sk.f1_score(labels, pred, labels=[k], average=None)[0] if on else 0.0
        for k in eval_ref.KEYS:
            assert eval_ref.close(got[k], float(want[k]), TOL), (trial, k, got[k], want[k])


def res(f1_macro, auc):
    return {"f1_macro": f1_macro, "auc": auc}


def test_model_selection_rule():
    from get_amd.evaluate import ModelSelection
    s = ModelSelection(patience=2)
    assert s.best is None and s.best_epoch is None and not s.should_stop
    assert s.update(res(0.5, 0.6), 0) and s.best_epoch == 0
    assert s.update(res(0.6, 0.1), 1) and s.best_epoch == 1                # improvement by f1_macro, whatever the AUC
    assert not s.update(res(0.6, 0.1), 2) and s.best_epoch == 1            # an exact tie does not win
    assert s.update(res(0.6, 0.2), 3) and s.best_epoch == 3                # tie broken by AUC
    assert s.best == res(0.6, 0.2) and s.count_patience_epochs == 0
    assert not s.update(res(0.6, math.nan), 4)                             # a nan AUC never wins a tie
    assert not s.update(res(0.59, 0.99), 5)
    assert s.count_patience_epochs == 2 and not s.should_stop              # patience boundary: >, not >=
    assert not s.update(res(0.1, 0.1), 6)
    assert s.count_patience_epochs == 3 and s.should_stop and s.best_epoch == 3
    assert s.update(res(0.7, math.nan), 7) and not s.should_stop           # f1_macro alone decides when it rises
    assert not s.update(res(0.7, 0.9), 8) and s.best_epoch == 7            # ... and nothing beats a nan AUC on a tie (:150)
    # the reference starts from (0, 0) (:86): an epoch that scores nothing is not the winner; no patience, no stop
    s = ModelSelection()
    assert not s.update(res(0.0, 0.0), 0) and s.best is None
    for e in range(1, 50):
        assert not s.update(res(0.0, math.nan), e)
    assert not s.should_stop and s.update(res(0.0, 0.5), 50) and s.best_epoch == 50
    stored = res(0.3, 0.3)
    s.update(stored, 51)
    stored["auc"] = 0.0
    assert s.best["auc"] == 0.3                                            # the winner is a copy


def test_key_strings_equal_the_reference(golden):
    from get_amd.keywords import KeyWordSettings as K
    keys = golden["meta"]["keys"]
    assert golden["meta"]["keys_from"].startswith("reference")
    assert K.CLS_METRICS == keys and len(keys) == 13
    names = ["AUC_metric", "F1_macro", "F1_micro", "F1", "PrecisionTrueCls", "RecallTrueCls", "F1TrueCls", "PrecisionFalseCls",
             "RecallFalseCls", "F1FalseCls", "PrecisionMixedCls", "RecallMixedCls", "F1MixedCls"]
    assert [getattr(K, n) for n in names] == keys
    assert eval_ref.KEYS == keys

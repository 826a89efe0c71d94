"""GPU checks of the evaluation path: the integers of gh_cls_metrics against the numpy restatement tests/eval_ref.py (exact),
get_amd.evaluate.classification_metrics against the values recorded from the reference's `_computing_metrics`
(tests/golden/g18_metrics.json, 1e-12: one division of exact integers against a trapezoid sum of n <= 10^3 terms), and
evaluate() on the small synthetic model.

Sizes: the issue's list plus the kernel's own widths -- 256 rows per workgroup, LDS tiles of 1024 scores, spans of 4096 rows
per workgroup (csrc/eval_ops.hip) -- straddled on both sides; 8193 gives a third span with a single row."""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle.cases_model import MODEL_CASES
from tests import eval_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-12
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 5000, 8193]


def run_kernel(phi, labels, pos_class, ld_extra=0, label_dtype=torch.int64):
    """ops.cls_metrics on phi laid out with rows ld_extra floats wider than c (the padding filled with NaN: never to be read)."""
    from get_amd import ops
    n, c = phi.shape
    wide = torch.full((n, c + ld_extra), float("nan"), dtype=torch.float32)
    wide[:, :c] = torch.from_numpy(phi)
    view = wide.to(DEV)[:, :c]
    out, pred = ops.cls_metrics(view, torch.from_numpy(np.asarray(labels)).to(label_dtype).to(DEV), pos_class=pos_class)
    assert out.dtype == torch.int64 and pred.dtype == torch.int32 and out.is_cuda and pred.is_cuda
    return out.cpu().numpy(), pred.cpu().numpy()


def check(phi, labels, pos_class=1, ld_extra=0, label_dtype=torch.int64, what=""):
    phi = np.ascontiguousarray(phi, dtype=np.float32)
    want_out, want_pred = eval_ref.counts(phi, labels, pos_class)
    out, pred = run_kernel(phi, labels, pos_class, ld_extra, label_dtype)
    assert out.shape == want_out.shape
    assert np.array_equal(out, want_out), (what, out.tolist(), want_out.tolist())
    assert np.array_equal(pred, want_pred), what
    return out


def scores(kind, rng, n, c):
    if kind == "ties":                   # integer-valued: heavy ties between rows and inside the argmax
        return rng.integers(-3, 4, (n, c)).astype(np.float32)
    if kind == "gauss":
        return rng.standard_normal((n, c)).astype(np.float32)
    if kind == "zeros":                  # +0.0 / -0.0 pairs: equal under IEEE comparison
        return np.where(rng.integers(0, 2, (n, c)) == 1, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    assert kind == "inf"                 # +-inf are ordinary values
    return rng.choice(np.array([-np.inf, -1.0, 0.0, 1.0, np.inf], np.float32), (n, c))


@pytest.mark.parametrize("c", [2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_integers_equal_the_restatement(n, c):
    rng = np.random.default_rng(1000 * c + n)
    for k, kind in enumerate(("ties", "gauss", "zeros", "inf")):
        phi = scores(kind, rng, n, c)
        labels = rng.integers(0, c, n)
        # alternate the row pitch, the label type and the positive class over the kinds and sizes; every combination of
        # (pitch, label type) and of (kind, positive class) occurs at some size for both c
        v = k + n + c
        check(phi, labels, pos_class=v % 2, ld_extra=5 * ((v // 2) % 2), label_dtype=(torch.int64, torch.int32)[(v // 4) % 2],
              what=f"{kind} n={n} c={c}")


@pytest.mark.parametrize("c", [2, 3])
@pytest.mark.parametrize("ld_extra", [0, 5])
@pytest.mark.parametrize("label_dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("pos_class", [0, 1])
def test_kernel_every_layout_at_one_size(c, ld_extra, label_dtype, pos_class):
    rng = np.random.default_rng(7)
    n = 1300                              # six workgroups of rows, two tiles
    for kind in ("ties", "gauss"):
        check(scores(kind, rng, n, c), rng.integers(0, c, n), pos_class, ld_extra, label_dtype, what=kind)


@pytest.mark.parametrize("c", [2, 3])
@pytest.mark.parametrize("n", [1, 257, 4097])
def test_kernel_single_class_labels(n, c):
    """All labels of one class: zero positives or zero negatives, U2 = 0."""
    rng = np.random.default_rng(n + c)
    phi = scores("ties", rng, n, c)
    for cls in range(c):
        for pos_class in (0, 1):
            out = check(phi, np.full(n, cls), pos_class, what=f"all {cls}")
            assert out[c * c] == 0 and out[c * c + 1] == (n if cls == pos_class else 0) and out[c * c + 1] + out[c * c + 2] == n


def test_kernel_largest_class_count_and_reserved_slots():
    rng = np.random.default_rng(8)
    out = check(scores("ties", rng, 700, 8), rng.integers(0, 8, 700), pos_class=7)
    assert out[64 + 5:].tolist() == [0, 0, 0] and out[:64].sum() == 700


@pytest.mark.parametrize("label_dtype", [torch.int64, torch.int32])
def test_rejected_rows_are_counted_and_left_out(label_dtype):
    from get_amd.evaluate import classification_metrics
    rng = np.random.default_rng(9)
    n, c = 1500, 3
    phi = scores("ties", rng, n, c)
    labels = rng.integers(0, c, n)
    bad = rng.choice(n, 40, replace=False)
    labels[bad[:10]] = -1
    labels[bad[10:20]] = c
    labels[bad[15:20]] = 2 ** 31 - 1
    phi[bad[18:30], rng.integers(0, c, 12)] = np.nan            # rows 18..19 carry both: counted as bad labels only
    phi[bad[30:40], :] = np.nan
    out = check(phi, labels, 1, label_dtype=label_dtype)
    assert out[c * c + 3] == 20 and out[c * c + 4] == 20
    keep = np.ones(n, bool)
    keep[bad] = False
    clean, _ = eval_ref.counts(phi[keep], labels[keep], 1)
    assert np.array_equal(out[:c * c + 3], clean[:c * c + 3])          # every other count is that of the clean rows alone
    T = lambda a, dt=None: torch.from_numpy(a).to(DEV) if dt is None else torch.from_numpy(a).to(dt).to(DEV)
    with pytest.raises(ValueError, match="20 rows with a label outside.*20 rows with a NaN"):
        classification_metrics(T(phi), T(labels, label_dtype))
    with pytest.raises(ValueError, match="0 rows with a label outside.*1 rows with a NaN"):
        classification_metrics(T(np.array([[0, 1], [np.nan, 0]], np.float32)), T(np.array([0, 1])))
    got = classification_metrics(T(phi[keep]), T(labels[keep], label_dtype))
    want = eval_ref.metrics(phi[keep], labels[keep])
    assert all(eval_ref.close(got[k], want[k], TOL) for k in want)


def test_classification_metrics_reproduces_the_recorded_reference_values(golden_dir):
    from get_amd.evaluate import classification_metrics
    from get_amd.keywords import KeyWordSettings as K
    golden = json.load(open(os.path.join(golden_dir, "g18_metrics.json")))
    for name, case in golden["cases"].items():
        phi = torch.tensor(case["logits"], dtype=torch.float32, device=DEV)
        labels = torch.tensor(case["labels"], device=DEV)
        got = classification_metrics(phi, labels, output_size=case["output_size"])
        assert list(got) == K.CLS_METRICS == golden["meta"]["keys"]
        for k, w in case["expected"].items():
            w = math.nan if w == "nan" else float(w)
            assert isinstance(got[k], float) and eval_ref.close(got[k], w, TOL), (name, k, got[k], w)


def test_bad_arguments_and_cpu_tensors_are_refused():
    from get_amd import ops
    from get_amd.evaluate import classification_metrics
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.cls_metrics(torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        classification_metrics(torch.zeros(4, 2, device=DEV), torch.zeros(4, dtype=torch.int64))
    z = lambda n, c: (torch.zeros(n, c, device=DEV), torch.zeros(n, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match=r"n = 0 outside"):
        ops.cls_metrics(*z(0, 2))
    with pytest.raises(RuntimeError, match=r"c = 9 outside"):
        ops.cls_metrics(*z(3, 9))
    with pytest.raises(RuntimeError, match=r"c = 1 outside"):
        ops.cls_metrics(*z(3, 1))
    with pytest.raises(RuntimeError, match=r"pos_class = 2 outside"):
        ops.cls_metrics(*z(3, 2), pos_class=2)
    with pytest.raises(ValueError, match="labels"):
        ops.cls_metrics(torch.zeros(3, 2, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV))


@pytest.fixture(scope="module")
def small_model_and_batch():
    from get_amd.batch import NativeBatch, batched_predict
    from get_amd.synth import make_raw_batch
    from tests.test_gpu_model import build_model
    cfg, seed = MODEL_CASES["small"]
    model = build_model(cfg, seed)
    raw = make_raw_batch(cfg, seed)
    mk = lambda labels: NativeBatch(raw["claim_tokens"], raw["claim_len"], raw["evd_tokens"], raw["evd_len"], raw["evd_counts"],
                                    raw["doc_sources"], raw["query_sources"], labels, window=cfg.window, device=DEV)
    # the case's own labels are all of class 0 (AUC nan); the second batch has both classes on the same claims
    batches = [(mk(raw["labels"]), raw["labels"]), (mk(np.array([1, 0, 1, 0])), np.array([1, 0, 1, 0]))]
    phi, words, evd = batched_predict(model, batches[0][0])
    return model, batches, (phi.clone(), [w.clone() for w in words], evd.clone())


@pytest.mark.parametrize("which", [0, 1])
def test_evaluate_on_the_small_model(small_model_and_batch, which):
    from get_amd.evaluate import evaluate
    from get_amd.keywords import KeyWordSettings as K
    model, batches, (phi, words, evd) = small_model_and_batch
    nb, labels = batches[which]
    want = eval_ref.metrics(phi.cpu().numpy(), labels, output_size=phi.shape[1])
    assert math.isnan(want["auc"]) == (which == 0)
    for chunk in (0, 1, 3):
        got = evaluate(model, nb, claims_per_call=chunk)
        assert list(got) == K.CLS_METRICS
        for k in want:
            # exact integers behind both: the logits of a chunked pass differ by rounding at most, never enough to move a
            # prediction or swap two scores of this case (the nearest pair of class-1 logits is > 1e-3 apart)
            assert eval_ref.close(got[k], want[k], TOL), (chunk, k, got[k], want[k])
    got, (phi2, words2, evd2) = evaluate(model, nb, output_ranking=True)
    assert all(eval_ref.close(got[k], want[k], TOL) for k in want)
    assert torch.equal(phi2, phi) and torch.equal(evd2, evd)
    assert len(words2) == len(words) and all(torch.equal(a, b) for a, b in zip(words2, words))


def test_evaluate_restores_the_training_flag(small_model_and_batch):
    from get_amd.evaluate import evaluate
    model, batches, _ = small_model_and_batch
    nb = batches[0][0]
    try:
        model.train(True)
        evaluate(model, nb)
        assert model.training
        model.train(False)
        evaluate(model, nb, claims_per_call=3)
        assert not model.training
    finally:
        model.train(False)

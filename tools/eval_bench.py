"""Time one validation pass three ways, on the same model, the same claims and the same device, in one process.

A tool, not a test.  The claims: --claims (780, one Snopes fold) synthetic claims whose evidence counts follow the empirical
Snopes histogram (get_amd.synth.SNOPES_EVD_HIST, mean 6.9), at the model size of bench.py's default configuration.

    a  per_claim   the reference protocol as ``CharManFitterQueryRepr1.evaluate`` issues it (char_man_fitter_query_repr1.py:278-362):
                   one B=1 forward per claim with output_ranking, then the prediction and the class-1 score read back per claim
                   (:359-360), then the host metrics.  The 780 one-claim batches are built BEFORE the clock starts (the reference
                   builds its tensors inside the loop), so this arm is timed in its favour.
    b  batched     get_amd.batch.batched_predict, one read-back of the logits, the host metrics
    c  evaluate    get_amd.evaluate.evaluate: batched_predict, gh_cls_metrics, one read-back of c*c + 8 integers

The host metrics are the sklearn calls of ``_computing_metrics`` (:381-401) when sklearn is installed, the same numbers from
numpy otherwise; the JSON says which.  Every arm ends in a device synchronise (its read-back); after a warm-up pass of every
arm the arms are alternated for --rounds rounds and the median wall time per pass is reported with the spread (min .. max).
The metrics kernel's own time is taken with device events around --kernel-reps back-to-back calls of gh_cls_metrics into
preallocated buffers (the zero fill of its 12 integers included), on the pass's own logits (n = --claims) and on n = 65 536
random ones; --kernel-only runs just that part, on random logits, for a kernel trace.

    python tools/eval_bench.py [--claims 780] [--rounds 5] [--claims-per-call 0] [--out FILE] [--kernel-only]

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def host_metrics_fn():
    """(name, fn(labels, pred, score, c) -> dict): what a user computes from the read-back predictions and class-1 scores."""
    from get_amd.evaluate import metrics_from_counts
    try:
        import sklearn.metrics as sk
    except ImportError:
        sk = None

    def with_numpy(labels, pred, score, c):
        out = np.zeros(c * c + 8, dtype=np.int64)
        np.add.at(out, labels * c + pred.astype(np.int64), 1)
        s = score.astype(np.float64)
        sp, sn = s[labels == 1], s[labels != 1]
        out[c * c:c * c + 3] = [2 * int((sp[:, None] > sn[None, :]).sum()) + int((sp[:, None] == sn[None, :]).sum()), len(sp), len(sn)]
        return metrics_from_counts(out.tolist(), c)

    def with_sklearn(labels, pred, score, c):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            fpr, tpr, _ = sk.roc_curve(labels, score, pos_label=1)
            res = {"auc": sk.auc(fpr, tpr), "f1_macro": sk.f1_score(labels, pred, average="macro"),
                   "f1_micro": sk.f1_score(labels, pred, average="micro"), "f1": sk.f1_score(labels, pred, labels=[1], average=None)[0]}
            for name, k in (("true", 1), ("false", 0)):
                res[f"precision_{name}_cls"] = sk.precision_score(labels, pred, labels=[k], average=None)[0]
                res[f"recall_{name}_cls"] = sk.recall_score(labels, pred, labels=[k], average=None)[0]
                res[f"f1_{name}_cls"] = sk.f1_score(labels, pred, labels=[k], average=None)[0]
        return res

    return ("sklearn", with_sklearn) if sk is not None else ("numpy", with_numpy)


def kernel_times(args, dev, phi, labels):
    """Microseconds per gh_cls_metrics call (zero fill + kernel): device events around --kernel-reps back-to-back calls of the
    C entry into preallocated buffers, so that the host issues faster than the device runs and the span is the device's."""
    from get_amd._lib import call, ptr, stream
    g = torch.Generator(device="cpu").manual_seed(args.seed)
    cases = {"n_claims": (phi, labels),
             "n_65536": (torch.randn(65536, 2, generator=g).to(dev), (torch.rand(65536, generator=g) < 0.27).long().to(dev))}
    res = {}
    for name, (p, y) in cases.items():
        n, c = p.shape
        p, y = p.float().contiguous(), y.long().contiguous()
        out = torch.empty(c * c + 8, device=dev, dtype=torch.int64)
        pred = torch.empty(n, device=dev, dtype=torch.int32)
        a = (ptr(p), c, ptr(y), 1, n, c, 1, ptr(pred), ptr(out))
        for _ in range(10):
            call("gh_cls_metrics", *a, stream())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.kernel_reps):
            call("gh_cls_metrics", *a, stream())
        e1.record()
        torch.cuda.synchronize()
        res[name] = 1e3 * e0.elapsed_time(e1) / args.kernel_reps
    return res


def emit(args, out):
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--claims", type=int, default=780)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--claims-per-call", type=int, default=0)
    ap.add_argument("--kernel-reps", type=int, default=200)
    ap.add_argument("--seed", type=int, default=20240229)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-only", action="store_true",
                    help="only the metrics kernel's calls, on random logits (the run to wrap in a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench: needs a GPU (there is no CPU path and no CPU timing)")

    from get_amd import modules
    from get_amd.batch import NativeBatch, batched_predict
    from get_amd.evaluate import evaluate
    from get_amd.keywords import KeyWordSettings as K
    from get_amd.synth import SynthConfig, make_embeddings, make_raw_batch, snopes_evidence_counts

    dev = torch.device("cuda:0")
    if args.kernel_only:
        g = torch.Generator(device="cpu").manual_seed(args.seed + 1)
        phi = torch.randn(args.claims, 2, generator=g).to(dev)
        labels = (torch.rand(args.claims, generator=g) < 0.27).long().to(dev)
        emit(args, {"tool": "eval_bench", "claims": args.claims, "metrics_kernel_us": kernel_times(args, dev, phi, labels),
                    "device": torch.cuda.get_device_name(0)})
        return
    counts = snopes_evidence_counts(np.random.default_rng(args.seed + 17), args.claims)
    cfg = SynthConfig(batch=args.claims, evd_counts=[int(x) for x in counts])
    emb, art, clm = make_embeddings(cfg, args.seed)
    torch.manual_seed(args.seed)
    model = modules.Graph_basedSemantiStructure(cfg.model_params(emb, art, clm)).to(dev).train(False)
    raw = make_raw_batch(cfg, args.seed)
    nb = NativeBatch(raw["claim_tokens"], raw["claim_len"], raw["evd_tokens"], raw["evd_len"], raw["evd_counts"], raw["doc_sources"],
                     raw["query_sources"], raw["labels"], window=cfg.window, n_max=cfg.fixed_num_evidences, device=dev)
    singles = [nb.subset(b, b + 1) for b in range(nb.b)]
    labels_host = raw["labels"].astype(np.int64)
    host_name, host_metrics = host_metrics_fn()

    def per_claim():
        preds, probs = [], []
        with torch.no_grad():
            for one in singles:
                q, d, k = one.inputs()
                p, _att = model.predict(q, d, **dict(k, **{K.OutputRankingKey: True}))
                preds.append(float(p.argmax(dim=1).cpu().numpy().flatten()[0]))
                probs.append(float(p[:, 1].cpu().numpy().flatten()[0]))
        res = host_metrics(labels_host, np.asarray(preds), np.asarray(probs), cfg.num_classes)      # the two lists are all _computing_metrics sees
        return res, np.asarray(preds)

    def batched():
        phi, _, _ = batched_predict(model, nb, claims_per_call=args.claims_per_call)
        host = phi.cpu().numpy()
        return host_metrics(labels_host, host.argmax(1), host[:, 1], host.shape[1]), phi

    def fused():
        return evaluate(model, nb, claims_per_call=args.claims_per_call), None

    arms = {"per_claim": per_claim, "batched": batched, "evaluate": fused}
    first = {}
    for name, fn in arms.items():          # warm-up: code objects, arenas, the allocator's pools
        first[name] = fn()
        torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(args.rounds):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)

    # the arms must agree: (b) and (c) on every value; (a) on the predictions (its AUC ranks the same scores)
    res_c, res_b = first["evaluate"][0], first["batched"][0]
    agree_bc = max((abs(res_c[k] - res_b[k]) for k in res_b if not (np.isnan(res_c[k]) and np.isnan(res_b[k]))), default=0.0)
    pred_b = first["batched"][1].argmax(1).cpu().numpy()
    agree_a = float((first["per_claim"][1] == pred_b).mean())

    def summary(ts):
        return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts),
                "claims_per_s": args.claims / statistics.median(ts)}

    phi_pass = first["batched"][1].contiguous()
    out = {"tool": "eval_bench", "claims": args.claims, "pairs": int(nb.b1), "rounds": args.rounds,
           "claims_per_call": args.claims_per_call, "host_metrics": host_name,
           "arms": {name: summary(ts) for name, ts in times.items()},
           "metrics_kernel_us": kernel_times(args, dev, phi_pass, nb.labels),
           "max_abs_diff_evaluate_vs_batched": agree_bc, "per_claim_predictions_equal_batched": agree_a,
           "results": {k: (None if np.isnan(v) else v) for k, v in res_c.items()},
           "device": torch.cuda.get_device_name(0)}
    emit(args, out)


if __name__ == "__main__":
    main()

"""Golden vectors of the BERT fine-tuning optimiser, captured from the upstream reference in the build container -- never on the
GPU machine, and no test reads the reference.

Loads the reference's ``pytorch_transformers/optimization.py`` by path at run time only (it imports logging, math and torch),
runs every case with its ``AdamW``, its schedules and torch's ``clip_grad_norm_`` in fp32 and in float64 on the CPU, and writes

    tests/golden/g22_optim.npz          every case below, and lr_lambda of the five schedules
    tests/golden/optim_contract.json    AdamW's constructor defaults, its param_groups keys and its state keys

Every case runs STEPS = 8 steps on nine parameters of the shapes SHAPES (1 to 576 elements: below, at and above the 64-element
block of the flat bucket, and more than one block), drawn normal(0, 1); a step's gradients are normal(0, 1) times the case's
gradient scale.  One group of lr 1e-3, weight decay 0.01, the reference's betas and eps, bias correction on and a constant
schedule, unless the case says otherwise:
  two_groups_linear   even-indexed parameters lr 1e-3, weight decay 0.01; odd-indexed lr 5e-4, weight decay 0;
                      WarmupLinearSchedule(2, 10); clip_grad_norm_(1.0) (the norm is about 37: the clip is active)
  no_bias_correction  correct_bias=False
  skipped             parameters 2 and 5 have grad = None on steps 1 and 2, so their step counts lag; clip_grad_norm_(1.0), so that
                      a gradient left over from an earlier step would show in the norm
  tiny_grads          gradients of scale 1e-6: eps is as large as sqrt(v)
  clip_inactive       clip_grad_norm_(1e3): the coefficient is clamped to 1

Per case ``<case>::``: ``p0::<i>`` the initial parameters; ``grad::<step>::<i>`` the gradients fed at step 1..8 (absent where the
parameter is skipped); ``lr::<step>`` every group's lr at that step and ``norm::<step>`` what clip_grad_norm_ returned;
``steps::<step>`` every parameter's step count; and after steps 1, 2 and 8 ``p::<step>::<i>``, ``exp_avg::<step>::<i>``,
``exp_avg_sq::<step>::<i>`` (zeros for a parameter that has no state yet).  These are the reference's fp32 results; its float64
results ride along as fp32 residuals (``<case>::resid::<key>`` = float64 result - fp32 result).  ``sched::<class>::<warmup>::
<t_total>::<cycles>`` holds lr_lambda(0..12) of the five schedule classes in float64 for warmup in {0, 3}, t_total in {3, 10},
cycles in {0.5, 1, 2} (a class ignores what its constructor does not take).

Tolerances of the GPU test (tests/test_gpu_optim.py), elementwise atol + rtol |want| against the float64 result:
    p          1e-5 + 1e-5 |want|
    exp_avg    1e-6 + 1e-5 |want|
    exp_avg_sq 1e-30 + 1e-5 |want|     (purely relative: v is a sum of non-negative terms)
The reference's own fp32 run must lie within a tenth of them (asserted below; measured per case, as fractions of that tenth: p 0.18 .. 0.38,
exp_avg 0.00 .. 0.62, exp_avg_sq 0.29 .. 0.42; the figures are printed and stored in ``meta``).  A case that misses takes smaller inputs; the tolerance is
never loosened.

    python tools/make_optim_golden.py
"""
import inspect
import json
import os
import warnings
import zlib

import numpy as np
import torch

from golden_common import OUT, load_reference, margin, write_contract, write_npz

SHAPES = [(1,), (3,), (63,), (64,), (65,), (5, 7), (24, 24), (300,), (260,)]
STEPS = 8
SNAPSHOTS = (1, 2, 8)
BASE = dict(lr=1e-3, weight_decay=0.01, correct_bias=True)
CASES = {
    "two_groups_linear": dict(groups=[dict(lr=1e-3, weight_decay=0.01), dict(lr=5e-4, weight_decay=0.0)], alternate=True,
                              sched=("WarmupLinearSchedule", dict(warmup_steps=2, t_total=10)), max_norm=1.0),
    "no_bias_correction": dict(groups=[dict(correct_bias=False)]),
    "skipped": dict(skip={1: (2, 5), 2: (2, 5)}, max_norm=1.0),
    "tiny_grads": dict(grad_scale=1e-6),
    "clip_inactive": dict(max_norm=1e3),
}
TOL = {"p": (1e-5, 1e-5), "exp_avg": (1e-6, 1e-5), "exp_avg_sq": (1e-30, 1e-5)}
SCHEDULES = ("ConstantLRSchedule", "WarmupConstantSchedule", "WarmupLinearSchedule", "WarmupCosineSchedule",
             "WarmupCosineWithHardRestartsSchedule")


def group_of(spec):
    return [i % 2 if spec.get("alternate") else 0 for i in range(len(SHAPES))]


def group_hypers(spec):
    return [dict(BASE, **g) for g in spec.get("groups", [{}])]


def run(ref, name, spec, dtype):
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    params = [torch.nn.Parameter(torch.randn(s, generator=g).to(dtype)) for s in SHAPES]
    res = {f"p0::{i}": p.detach().clone() for i, p in enumerate(params)}
    owner = group_of(spec)
    groups = [dict(params=[p for p, o in zip(params, owner) if o == k], **h) for k, h in enumerate(group_hypers(spec))]
    opt = ref.AdamW(groups)
    sched_name, sched_kw = spec.get("sched", ("ConstantLRSchedule", {}))
    sched = getattr(ref, sched_name)(opt, **sched_kw)
    for step in range(1, STEPS + 1):
        for i, p in enumerate(params):
            grad = torch.randn(p.shape, generator=g) * spec.get("grad_scale", 1.0)      # (drawn even where skipped: one stream per case)
            if i in spec.get("skip", {}).get(step, ()):
                p.grad = None
            else:
                p.grad = grad.to(dtype, copy=True)      # (clip_grad_norm_ rescales it in place: the stored one is what was fed)
                res[f"grad::{step}::{i}"] = grad
        res[f"lr::{step}"] = np.array([gr["lr"] for gr in opt.param_groups], dtype=np.float64)
        if spec.get("max_norm") is not None:
            res[f"norm::{step}"] = torch.nn.utils.clip_grad_norm_(params, spec["max_norm"]).detach().clone().reshape(())
        opt.step()
        sched.step()
        res[f"steps::{step}"] = np.array([opt.state[p].get("step", 0) for p in params], dtype=np.int64)
        if step in SNAPSHOTS:
            for i, p in enumerate(params):
                st = opt.state[p]
                res[f"p::{step}::{i}"] = p.detach().clone()
                for k in ("exp_avg", "exp_avg_sq"):
                    res[f"{k}::{step}::{i}"] = st[k].detach().clone() if k in st else torch.zeros_like(p)
    out = {k: (v.numpy().copy() if torch.is_tensor(v) else v) for k, v in res.items()}
    return opt, out


def is_result(k):
    return k.split("::")[0] in TOL


def schedule_table(ref):
    dummy = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    out = {}
    for cls in SCHEDULES:
        takes = inspect.signature(getattr(ref, cls).__init__).parameters
        for w in (0, 3):
            for t in (3, 10):
                for c in (0.5, 1.0, 2.0):
                    kw = {k: v for k, v in (("warmup_steps", w), ("t_total", t), ("cycles", c)) if k in takes}
                    s = getattr(ref, cls)(dummy, **kw)
                    fn = s.lr_lambdas[0]
                    out[f"sched::{cls}::{w}::{t}::{c}"] = np.array([fn(k) for k in range(13)], dtype=np.float64)
    return out


def main():
    warnings.simplefilter("ignore")          # the reference uses the deprecated add_(Number, Tensor) overloads
    ref = load_reference("pytorch_transformers/optimization.py", "ref_optimization")
    torch.set_num_threads(1)
    store, margins = {}, {}
    for name, spec in CASES.items():
        opt, r32 = run(ref, name, spec, torch.float32)
        _, r64 = run(ref, name, spec, torch.float64)
        keys = [k for k in r32 if is_result(k)]
        worst = {q: margin(r32, r64, [k for k in keys if k.split("::")[0] == q],
                           lambda k, want: TOL[k.split("::")[0]][0] + TOL[k.split("::")[0]][1] * np.abs(want)) for q in TOL}
        margins[name] = worst
        print(f"{name}: fp32 reference at " + ", ".join(f"{q} {w:.3f}" for q, w in worst.items()) + " of a tenth of the bound")
        assert max(worst.values()) <= 1.0, (name, worst)
        for k, v in r32.items():
            if is_result(k) or k.startswith("norm::"):
                v = v.astype(np.float32)
                store[f"{name}::resid::{k}"] = (r64[k].astype(np.float64) - v.astype(np.float64)).astype(np.float32)
            store[f"{name}::{k}"] = v
    store.update(schedule_table(ref))
    defaults = {k: (list(v.default) if isinstance(v.default, tuple) else v.default)
                for k, v in inspect.signature(ref.AdamW.__init__).parameters.items() if v.default is not inspect.Parameter.empty}
    contract = {"class": "AdamW", "defaults": defaults, "param_groups_keys": sorted(opt.param_groups[0].keys()),
                "state_keys": sorted(next(iter(opt.state.values())).keys()), "schedules": list(SCHEDULES)}
    meta = {"shapes": [list(s) for s in SHAPES], "steps": STEPS, "snapshots": list(SNAPSHOTS),
            "cases": {n: {"groups": group_hypers(s), "group_of": group_of(s), "sched": list(s.get("sched", ("ConstantLRSchedule", {}))),
                          "max_norm": s.get("max_norm"), "skip": {str(k): list(v) for k, v in s.get("skip", {}).items()},
                          "betas": [0.9, 0.999], "eps": 1e-6} for n, s in CASES.items()},
            "tol": {k: list(v) for k, v in TOL.items()}, "margins": margins}
    store["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    write_npz(os.path.join(OUT, "g22_optim.npz"), store)
    write_contract(os.path.join(OUT, "optim_contract.json"), contract)
    for f in ("g22_optim.npz", "optim_contract.json"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()

"""The BERT fine-tuning optimiser on the GPU: get_amd.optim.AdamW with its schedules against the reference's golden vectors
(tests/golden/g22_optim.npz, tools/make_optim_golden.py), three training steps of the h24 BertModel against the float64
restatement of tests/optim_ref.py fed the same GPU-produced gradients, and FlatTrainer's decoupled rule against AdamW.

Bounds of the golden cases, elementwise atol + rtol |want| against the reference's float64 result (the archive's meta): p 1e-5 +
1e-5 |want|, exp_avg 1e-6 + 1e-5 |want|, exp_avg_sq 1e-30 + 1e-5 |want|; the generator holds the reference's own fp32 run to a
tenth of them (measured there: at most 0.62 of that tenth).

Bound of the BertModel steps, 1e-6 + 1e-6 |want| on every parameter after each of three steps: a step rounds p once (half an ulp,
<= 6e-8 for |p| < 2) and adds an update of about lr = 1e-3 whose relative error is below 1e-4 (tests/test_gpu_optim_paths.py),
1e-7 a step, 3e-7 after three; the bound is three times that."""
import functools

import numpy as np
import pytest
import torch

from tests import optim_ref
from tests.test_optim_cpu import QUANTITIES, f64, grads_of, recipe_of
from tests.util import DEV, bits_equal, golden_ratio, load_golden

pytestmark = pytest.mark.gpu

CASES = ["two_groups_linear", "no_bias_correction", "skipped", "tiny_grads", "clip_inactive"]
TOL_NORM = 1.2e-6                                # tests/test_gpu_optim_paths.py
TOL_BERT = (1e-6, 1e-6)


def _archive(golden_dir):
    return load_golden(golden_dir, "g22_optim.npz", "optim_contract.json")


@pytest.mark.parametrize("case", CASES)
def test_golden_case_through_adamw_and_its_schedule(golden_dir, case):
    from get_amd import optim
    z, meta, _ = _archive(golden_dir)
    c = meta["cases"][case]
    n = len(meta["shapes"])
    params = [torch.nn.Parameter(torch.from_numpy(z[f"{case}::p0::{i}"]).to(DEV)) for i in range(n)]
    groups = [dict(params=[p for p, o in zip(params, c["group_of"]) if o == k], lr=g["lr"], weight_decay=g["weight_decay"],
                   correct_bias=g["correct_bias"]) for k, g in enumerate(c["groups"])]
    opt = optim.AdamW(groups, max_grad_norm=c["max_norm"])
    sched = getattr(optim, c["sched"][0])(opt, **c["sched"][1])
    index = {id(p): j for j, p in enumerate(opt._params)}          # bucket order: group by group
    worst = 0.0
    for step in range(1, meta["steps"] + 1):
        grads = grads_of(z, meta, case, step)
        for i, (p, g) in enumerate(zip(params, grads)):
            if g is None:
                p.grad = None
            elif step % 2 and p.grad is not None:
                p.grad.copy_(torch.from_numpy(g))                  # into the bucket's view, in place
            else:
                p.grad = torch.from_numpy(g).to(DEV)               # a foreign tensor: copied in and re-attached by step()
        np.testing.assert_allclose([g["lr"] for g in opt.param_groups], z[f"{case}::lr::{step}"], rtol=1e-14, atol=0)
        skipped = [i for i, g in enumerate(grads) if g is None]
        frozen = {i: [t.clone() for t in (params[i].data, *opt._moments[index[id(params[i])]])] for i in skipped}
        norm = opt.step()
        sched.step()
        if c["max_norm"] is None:
            assert norm is None
        else:
            want = float(f64(z, case, f"norm::{step}")[0])
            assert norm.dim() == 0 and norm.is_cuda and abs(float(norm) - want) <= TOL_NORM * want
        for i, p in enumerate(params):
            j = index[id(p)]
            if i in skipped:                                        # untouched bits, and still no gradient
                assert p.grad is None
                for a, b, q in zip((p.data, *opt._moments[j]), frozen[i], QUANTITIES):
                    bits_equal(a, b, f"{case} step {step}: {q} of the skipped parameter {i}")
            else:
                assert p.grad.data_ptr() == opt._views[j].data_ptr()
                st = opt.state[p]
                assert st["exp_avg"].data_ptr() == opt._moments[j][0].data_ptr()
        assert [opt.state.get(p, {}).get("step", 0) for p in params] == z[f"{case}::steps::{step}"].tolist()
        if step in meta["snapshots"]:
            for i, p in enumerate(params):
                got = (p.data, *opt._moments[index[id(p)]])
                for q, t in zip(QUANTITIES, got):
                    atol, rtol = meta["tol"][q]
                    worst = max(worst, golden_ratio(t, f64(z, case, f"{q}::{step}::{i}"), atol, rtol, f"{case} step {step} {q}[{i}]"))
    print(f"{case}: worst ratio of the bound {worst:.3f}")
    if case == "skipped":
        steps = [opt.state[p]["step"] for p in params]
        assert steps[2] == steps[5] == meta["steps"] - 2 and steps[0] == meta["steps"]


def test_three_training_steps_of_the_h24_bert_model(golden_dir):
    from get_amd import optim
    from get_amd.bert import BertConfig, BertModel
    from tests.test_gpu_bert import _archive as bert_archive, _build, _forward
    name = "mask_half"                                             # h24, B=2, L=12
    z, _, contract = bert_archive(golden_dir)
    m = _build(z, contract, name)
    named = list(m.named_parameters())
    no_decay = ("bias", "LayerNorm.weight")
    owner = [1 if any(s in k for s in no_decay) else 0 for k, _ in named]
    assert 0 < sum(owner) < len(owner)
    hyper = dict(betas=(0.9, 0.999), eps=1e-6, correct_bias=False)
    groups = [dict(lr=1e-3, weight_decay=0.01, **hyper), dict(lr=1e-3, weight_decay=0.0, **hyper)]
    start = [p.detach().cpu().numpy() for _, p in named]
    opt = optim.AdamW([dict(params=[p for (_, p), o in zip(named, owner) if o == k], weight_decay=g["weight_decay"]) for k, g in
                       enumerate(groups)], lr=1e-3, correct_bias=False, max_grad_norm=1.0, model=m)
    sched = optim.WarmupLinearSchedule(opt, 1, 4)
    emb = {id(p) for k, p in named if "embeddings" in k}
    assert opt._matrices and not any(id(p) in emb for p in opt._matrices)
    ref = optim_ref.Recipe(start, owner, groups, sched=("WarmupLinearSchedule", dict(warmup_steps=1, t_total=4)), max_norm=1.0,
                           one_at_or_below=True)
    g_seq, g_pooled = (torch.from_numpy(z[f"{name}::{k}"]).to(DEV) for k in ("g_seq", "g_pooled"))
    worst = 0.0
    for step in range(3):
        opt.zero_grad()
        seq, pooled = _forward(m, z, name)
        ((seq * g_seq).sum() + (pooled * g_pooled).sum()).backward()
        grads = [p.grad.detach().cpu().numpy().copy() for _, p in named]
        assert all(np.abs(g).max() > 0 for g in grads)
        norm = opt.step()
        sched.step()
        ref.step(grads)
        assert abs(float(norm) - ref.last_norm) <= TOL_NORM * ref.last_norm
        if step == 0:
            assert ref.last_norm > 1.0, "the clip must be active in this test"
        for (k, p), want in zip(named, ref.p):
            worst = max(worst, golden_ratio(p.data, want, *TOL_BERT, f"step {step + 1} {k}"))
    print(f"three BERT steps: worst ratio of the bound {worst:.3f}")
    # a stale transpose or twin would show here: the trained model against a fresh one loaded from its state_dict
    with torch.no_grad():
        seq, pooled = _forward(m, z, name)
        fresh = BertModel(BertConfig.from_dict(contract["h24"]["config"]))
        fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, strict=True)
        fresh = fresh.to(DEV).eval()
        seq2, pooled2 = _forward(fresh, z, name)
    bits_equal(seq, seq2, "sequence_output after three steps against a fresh model")
    bits_equal(pooled, pooled2, "pooled_output after three steps against a fresh model")
    assert not torch.equal(seq.cpu(), torch.from_numpy(z[name + "::sequence_output"]))


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(24, 65)
        self.LayerNorm = torch.nn.LayerNorm(65)
        self.out = torch.nn.Linear(65, 3)


def _nets():
    torch.manual_seed(11)
    a = _Net()
    b = _Net()
    b.load_state_dict(a.state_dict())
    return a.to(DEV), b.to(DEV)


def test_flat_trainer_decoupled_rule_leaves_adamws_bits():
    from get_amd import optim
    from get_amd.dist import FlatTrainer
    a, b = _nets()
    no_decay = ("bias", "LayerNorm")
    tr = FlatTrainer(a, lr=2e-3, weight_decay=0.05, eps=1e-6, late_prefixes=(), decoupled_weight_decay=True, correct_bias=False,
                     no_decay=no_decay, max_grad_norm=1.0,
                     lr_lambda=functools.partial(optim.warmup_linear_schedule, warmup_steps=1, t_total=5))
    named = list(b.named_parameters())
    assert [k for k, _ in named] == tr.live_names                 # one group per parameter: the same bucket order, the same norm bits
    opt = optim.AdamW([dict(params=[p], weight_decay=0.0 if any(s in k for s in no_decay) else 0.05) for k, p in named], lr=2e-3,
                      eps=1e-6, correct_bias=False, max_grad_norm=1.0, model=b)
    sched = optim.WarmupLinearSchedule(opt, 1, 5)
    g = torch.Generator().manual_seed(3)
    for step in range(3):
        flat = torch.randn(tr.numel, generator=g).to(DEV)
        for gv, ov in zip(tr._views, opt._views):                  # only the slots: the padding of a bucket holds zeros
            n = gv.numel()
            off = gv.data_ptr() - tr.flat_g.data_ptr()
            gv.copy_(flat[off // 4: off // 4 + n].view_as(gv))
            ov.copy_(gv)
        tr.step()
        norm = opt.step()
        sched.step()
        bits_equal(tr.last_grad_norm, norm, f"step {step + 1}: norm")
        for q, x, y in zip(QUANTITIES, (tr.flat_p, tr.flat_m, tr.flat_v), (opt.flat_p, opt.flat_m, opt.flat_v)):
            bits_equal(x, y, f"step {step + 1}: flat {q}")
    assert float(norm) > 1.0 and tr.t == 3


def test_flat_trainer_with_default_arguments_is_the_adam_step_it_always_was():
    from get_amd import ops
    from get_amd.dist import FlatTrainer
    a, _ = _nets()
    tr = FlatTrainer(a, late_prefixes=())
    g = torch.Generator().manual_seed(4)
    p, m, v = tr.flat_p.clone(), tr.flat_m.clone(), tr.flat_v.clone()
    for step in (1, 2):
        for gv in tr._views:
            gv.copy_(torch.randn(gv.shape, generator=g))
        ops.adam_step_flat(p, tr.flat_g, m, v, step, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3, grad_scale=1.0)
        tr.step()
        for q, x, y in zip(QUANTITIES, (tr.flat_p, tr.flat_m, tr.flat_v), (p, m, v)):
            bits_equal(x, y, f"step {step}: flat {q}")
    assert tr.last_grad_norm is None and tr._flat_step is None

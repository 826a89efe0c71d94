"""The BERT fine-tuning optimiser without a GPU: the float64 restatement tests/optim_ref.py against the reference's golden
vectors (tests/golden/g22_optim.npz, tools/make_optim_golden.py), the schedules, the pure-host builders of the block map and the
segment table, and the host behaviour of get_amd.optim.AdamW and of FlatTrainer's new keywords."""
import math

import numpy as np
import pytest
import torch

from tests import optim_ref
from tests.util import load_golden

SCHEDULE_FNS = {"ConstantLRSchedule": "constant_schedule", "WarmupConstantSchedule": "warmup_constant_schedule",
                "WarmupLinearSchedule": "warmup_linear_schedule", "WarmupCosineSchedule": "warmup_cosine_schedule",
                "WarmupCosineWithHardRestartsSchedule": "warmup_cosine_hard_restarts_schedule"}
QUANTITIES = ("p", "exp_avg", "exp_avg_sq")


def _archive(golden_dir):
    return load_golden(golden_dir, "g22_optim.npz", "optim_contract.json")


def f64(z, case, key):
    """The reference's float64 result: its fp32 result plus the stored residual."""
    return z[f"{case}::{key}"].astype(np.float64) + z[f"{case}::resid::{key}"].astype(np.float64)


def recipe_of(z, meta, case, **kw):
    c = meta["cases"][case]
    groups = [dict(lr=g["lr"], betas=tuple(c["betas"]), eps=c["eps"], weight_decay=g["weight_decay"], correct_bias=g["correct_bias"])
              for g in c["groups"]]
    params = [z[f"{case}::p0::{i}"] for i in range(len(meta["shapes"]))]
    return optim_ref.Recipe(params, c["group_of"], groups, sched=(c["sched"][0], c["sched"][1]), max_norm=c["max_norm"], **kw)


def grads_of(z, meta, case, step):
    return [z.get(f"{case}::grad::{step}::{i}") for i in range(len(meta["shapes"]))]


@pytest.mark.parametrize("case", ["two_groups_linear", "no_bias_correction", "skipped", "tiny_grads", "clip_inactive"])
def test_restatement_reproduces_the_reference_in_float64(golden_dir, case):
    """Bound per element: 2^-23 |residual| (the residual is stored in fp32) + 1e-12 (|want| + the largest |want| of that
    quantity at that step) for the float64 roundings of two differently ordered evaluations; a wrong formula is off by 1e-3."""
    z, meta, _ = _archive(golden_dir)
    r = recipe_of(z, meta, case)
    n = len(meta["shapes"])
    for step in range(1, meta["steps"] + 1):
        r.step(grads_of(z, meta, case, step))
        np.testing.assert_allclose(r.last_lr, z[f"{case}::lr::{step}"], rtol=1e-14, atol=0)
        assert r.steps == z[f"{case}::steps::{step}"].tolist()
        if meta["cases"][case]["max_norm"] is not None:
            want = float(f64(z, case, f"norm::{step}")[0])
            assert abs(r.last_norm - want) <= 1e-12 * want
        if step in meta["snapshots"]:
            for q, got_all in zip(QUANTITIES, (r.p, r.m, r.v)):
                wants = [f64(z, case, f"{q}::{step}::{i}") for i in range(n)]
                scale = max(np.abs(w).max() for w in wants)
                for i in range(n):
                    resid = np.abs(z[f"{case}::resid::{q}::{step}::{i}"].astype(np.float64))
                    tol = 2.0 ** -23 * resid + 1e-12 * (np.abs(wants[i]) + scale)
                    err = np.abs(got_all[i] - wants[i])
                    assert (err <= tol).all(), f"{case} {q} step {step} parameter {i}: {(err / tol).max():.2f} x bound"
    if case == "skipped":
        assert r.steps[2] == r.steps[5] == meta["steps"] - 2 and r.steps[0] == meta["steps"]


def test_schedule_functions_and_classes_match_the_recorded_lr_lambda(golden_dir):
    """Within 1e-12: a few double roundings on values in [0, 1]; a wrong formula is off by at least 1e-3 at these steps."""
    from get_amd import optim
    z, _, contract = _archive(golden_dir)
    assert list(SCHEDULE_FNS) == contract["schedules"]
    dummy = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    seen = 0
    for key in (k for k in z if k.startswith("sched::")):
        _, cls, w, t, c = key.split("::")
        w, t, c = int(w), int(t), float(c)
        want = z[key]
        fn = getattr(optim, SCHEDULE_FNS[cls])
        ctor = {"ConstantLRSchedule": lambda: optim.ConstantLRSchedule(dummy),
                "WarmupConstantSchedule": lambda: optim.WarmupConstantSchedule(dummy, w),
                "WarmupLinearSchedule": lambda: optim.WarmupLinearSchedule(dummy, w, t),
                "WarmupCosineSchedule": lambda: optim.WarmupCosineSchedule(dummy, w, t, c),
                "WarmupCosineWithHardRestartsSchedule": lambda: optim.WarmupCosineWithHardRestartsSchedule(dummy, w, t, c)}[cls]
        sched = ctor()
        for step in range(13):
            assert abs(fn(step, w, t, c) - want[step]) <= 1e-12, (key, step)
            assert abs(sched.lr_lambda(step) - want[step]) <= 1e-12, (key, step)
            assert abs(optim_ref.schedule(cls, step, w, t, c) - want[step]) <= 1e-12, (key, step)
        seen += 1
    assert seen == 5 * 2 * 2 * 3


def test_schedule_defaults_are_the_references():
    from get_amd import optim
    dummy = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    assert optim.WarmupCosineSchedule(dummy, 1, 5).cycles == 0.5
    assert optim.WarmupCosineWithHardRestartsSchedule(dummy, 1, 5).cycles == 1.0
    assert optim.warmup_cosine_schedule(3, 1, 5) == optim.warmup_cosine_schedule(3, 1, 5, 0.5)
    assert optim.warmup_cosine_hard_restarts_schedule(3, 1, 5) == optim.warmup_cosine_hard_restarts_schedule(3, 1, 5, 1.0)


def test_every_schedule_is_a_lambdalr_that_moves_the_groups_lr():
    from get_amd import optim
    for make in (lambda o: optim.ConstantLRSchedule(o), lambda o: optim.WarmupConstantSchedule(o, 2),
                 lambda o: optim.WarmupLinearSchedule(o, 2, 6), lambda o: optim.WarmupCosineSchedule(o, 2, 6),
                 lambda o: optim.WarmupCosineWithHardRestartsSchedule(o, 2, 6, 2.0)):
        ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
        opt = optim.AdamW([dict(params=[ps[0]], lr=1e-3), dict(params=[ps[1]], lr=5e-4)])
        sched = make(opt)
        assert isinstance(sched, torch.optim.lr_scheduler.LambdaLR)
        for step in range(8):
            f = sched.lr_lambda(step)
            assert opt.param_groups[0]["lr"] == pytest.approx(1e-3 * f, abs=1e-18) and opt.param_groups[1]["lr"] == pytest.approx(5e-4 * f, abs=1e-18)
            opt._opt_called = True          # (no step on a CPU bucket: keep LambdaLR's order-of-calls warning quiet)
            sched.step()


def test_block_map_and_segment_table():
    from get_amd import ops
    from get_amd.dist import slot_offsets
    sizes = [1, 63, 64, 65, 260]
    offsets, total = slot_offsets(sizes)
    assert offsets == [0, 64, 128, 192, 320] and total == 640
    bm = ops.adamw_block_map(offsets, sizes, total)
    assert bm.dtype == np.uint16 and bm.tolist() == [1, 2, 3, 4, 4, 5, 5, 5, 5, 5]      # bucket order; every data block its parameter
    # a bucket with spare blocks between and behind the slots: they map to the skip segment
    spread = [0, 128, 256, 384, 576]
    bm = ops.adamw_block_map(spread, sizes, 960)
    assert bm.tolist() == [1, 0, 2, 0, 3, 0, 4, 4, 0, 5, 5, 5, 5, 5, 0]
    skip = ops.optim.SKIP_SEGMENT
    assert skip == 0 and all(bm[b] == skip for b in (1, 3, 5, 8, 14))
    for bad in (([0, 32], [1, 1], 128), ([0, 64], [65, 1], 128), ([0, 64], [1, 65], 128), ([0], [1], 100)):
        with pytest.raises(ValueError):
            ops.adamw_block_map(*bad)
    # the table: entry 0 skips, a parameter without a gradient skips, the others carry double-precision values rounded once
    h = (1e-3, (0.9, 0.999), 1e-6, 0.01, True, 3)
    tab = ops.adamw_segment_table([h, None, (5e-4, (0.8, 0.99), 1e-8, 0.0, False, 7)])
    assert tab.dtype.itemsize == 32 and tab.shape == (4,)
    assert tab["skip"].tolist() == [1, 0, 1, 0]
    want = np.float32(1e-3 * math.sqrt(1 - 0.999 ** 3) / (1 - 0.9 ** 3))
    assert tab["step_size"][1] == want and tab["lr_wd"][1] == np.float32(1e-3 * 0.01)
    assert tab["one_minus_beta1"][1] == np.float32(1.0 - 0.9) and tab["one_minus_beta2"][1] == np.float32(1.0 - 0.999)
    assert tab["step_size"][3] == np.float32(5e-4) and tab["lr_wd"][3] == 0 and tab["beta1"][3] == np.float32(0.8) and tab["eps"][3] == np.float32(1e-8)
    with pytest.raises(ValueError):
        ops.adamw_segment_table([None] * 65535)


def test_adamw_raises_the_references_value_errors():
    from get_amd import optim
    p = lambda: [torch.nn.Parameter(torch.zeros(3))]
    for kw, msg in ((dict(lr=-1.0), "Invalid learning rate"), (dict(betas=(1.0, 0.9)), "Invalid beta parameter"),
                    (dict(betas=(0.9, -0.1)), "Invalid beta parameter"), (dict(eps=-1e-6), "Invalid epsilon value"),
                    (dict(max_grad_norm=0.0), "Invalid max_grad_norm")):
        with pytest.raises(ValueError, match=msg):
            optim.AdamW(p(), **kw)


def test_adamw_contract_defaults_groups_and_state_keys(golden_dir):
    import inspect
    from get_amd import optim
    _, _, contract = _archive(golden_dir)
    sig = inspect.signature(optim.AdamW.__init__).parameters
    for k, v in contract["defaults"].items():
        assert (list(sig[k].default) if isinstance(sig[k].default, tuple) else sig[k].default) == v, k
    assert list(sig)[:8] == ["self", "params", "lr", "betas", "eps", "weight_decay", "correct_bias", "max_grad_norm"]
    assert sig["max_grad_norm"].default is None
    ps = [torch.nn.Parameter(torch.randn(3)), torch.nn.Parameter(torch.randn(5, 7))]
    opt = optim.AdamW(ps)
    optim.ConstantLRSchedule(opt)
    assert sorted(opt.param_groups[0].keys()) == contract["param_groups_keys"]
    assert len(opt.state) == 0                                   # lazily, at a parameter's first update, like the reference
    assert sorted(opt._state_of(1).keys()) == contract["state_keys"]


def test_adamw_bucket_views_and_state_dict_round_trip_on_a_cpu_bucket():
    from get_amd import optim
    from get_amd.dist import slot_offsets
    shapes = [(3,), (5, 7), (65,)]
    g = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    before = [p.detach().clone() for p in ps]
    opt = optim.AdamW([dict(params=ps[:1], weight_decay=0.0), dict(params=ps[1:])], weight_decay=0.01)
    offsets, total = slot_offsets([p.numel() for p in ps])
    assert opt._offsets == offsets == [0, 64, 128] and opt.flat_p.numel() == total == 256
    es = opt.flat_p.element_size()
    for p, b, off in zip(ps, before, offsets):
        assert torch.equal(p.detach(), b)
        assert p.data_ptr() == opt.flat_p.data_ptr() + off * es and p.grad.data_ptr() == opt.flat_g.data_ptr() + off * es
        assert p._gh_direct_grad
    # a state in the reference's layout, loaded: the moments land in the bucket and the state's tensors are its views
    m1, v1 = torch.randn(5, 7, generator=g), torch.rand(5, 7, generator=g)
    sd = opt.state_dict()
    assert sd["state"] == {} and [grp["params"] for grp in sd["param_groups"]] == [[0], [1, 2]]
    sd["state"] = {1: {"step": 4, "exp_avg": m1.clone(), "exp_avg_sq": v1.clone()}}
    sd["param_groups"][1]["lr"] = 3e-4
    for m, _ in opt._moments:
        m.fill_(7.0)
    opt.load_state_dict(sd)
    assert opt.param_groups[1]["lr"] == 3e-4
    assert torch.equal(opt.flat_m[64:99].view(5, 7), m1) and torch.equal(opt.flat_v[64:99].view(5, 7), v1)
    assert bool((opt.flat_m[:64] == 0).all()) and bool((opt.flat_m[128:] == 0).all())          # no state: zero moments
    st = opt.state[ps[1]]
    assert st["step"] == 4 and st["exp_avg"].data_ptr() == opt.flat_m.data_ptr() + 64 * es
    assert st["exp_avg_sq"].data_ptr() == opt.flat_v.data_ptr() + 64 * es
    for p, off in zip(ps, offsets):                                                              # nothing was detached
        assert p.data_ptr() == opt.flat_p.data_ptr() + off * es and p.grad.data_ptr() == opt.flat_g.data_ptr() + off * es
    out = opt.state_dict()
    assert set(out["state"]) == {1} and out["state"][1]["step"] == 4 and torch.equal(out["state"][1]["exp_avg"], m1)
    assert out["state"][1]["exp_avg"].data_ptr() != st["exp_avg"].data_ptr()                    # a copy, not the view
    # zero_grad: one memset, views re-attached; set_to_none detaches
    ps[0].grad = torch.ones(3)
    opt.flat_g.fill_(2.0)
    opt.zero_grad()
    assert bool((opt.flat_g == 0).all()) and ps[0].grad.data_ptr() == opt.flat_g.data_ptr()
    opt.zero_grad(set_to_none=True)
    assert all(p.grad is None for p in ps)
    with pytest.raises(RuntimeError, match="no CPU path"):
        opt.step()


def test_adamw_leaves_frozen_parameters_out_and_refuses_a_late_group():
    from get_amd import optim
    ps = [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(5), requires_grad=False), torch.nn.Parameter(torch.ones(2, 2))]
    opt = optim.AdamW(ps, max_grad_norm=1.0)
    assert [id(p) for p in opt._params] == [id(ps[0]), id(ps[2])] and opt.flat_p.numel() == 128
    assert ps[1].grad is None and not getattr(ps[1], "_gh_direct_grad", False)          # untouched: no view, no bucket slot
    assert ps[1].data_ptr() != opt.flat_p.data_ptr() + 4 * 64
    assert opt.last_grad_norm is None
    with pytest.raises(RuntimeError, match="add_param_group"):
        opt.add_param_group(dict(params=[torch.nn.Parameter(torch.ones(2))]))
    with pytest.raises(ValueError, match="requires a gradient"):
        optim.AdamW([torch.nn.Parameter(torch.ones(2), requires_grad=False)])


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.emb = torch.nn.Embedding(7, 6)
        self.fc = torch.nn.Linear(6, 5)
        self.LayerNorm = torch.nn.LayerNorm(5)
        self.out = torch.nn.Linear(5, 2)


def test_flat_trainer_layout_is_the_same_with_the_new_keywords():
    from get_amd import optim
    from get_amd.dist import FlatTrainer
    import functools
    torch.manual_seed(3)
    a, b = _Net(), _Net()
    b.load_state_dict(a.state_dict())
    ta = FlatTrainer(a, late_prefixes=("out.",))
    tb = FlatTrainer(b, late_prefixes=("out.",), decoupled_weight_decay=True, correct_bias=False, no_decay=("bias", "LayerNorm"),
                     max_grad_norm=1.0, lr_lambda=functools.partial(optim.warmup_linear_schedule, warmup_steps=2, t_total=10))
    assert ta.live_names == tb.live_names and ta.numel == tb.numel and ta.n_early == tb.n_early and ta._offsets == tb._offsets
    assert ta._offsets == [0, 64, 128, 192, 256, 320, 384] and ta.numel == 448 and ta.n_early == 320
    assert torch.equal(ta.flat_p, tb.flat_p)
    assert [id(p) for p in ta._matrices] == [id(a.fc.weight), id(a.out.weight)]
    for t, net in ((ta, a), (tb, b)):
        for (n, p), off in zip(((n, dict(net.named_parameters())[n]) for n in t.live_names), t._offsets):
            assert p.data_ptr() == t.flat_p.data_ptr() + 4 * off and p.grad.data_ptr() == t.flat_g.data_ptr() + 4 * off
    # the default rule's state_dict is what it always was; the decoupled rule adds its settings to "hyper"
    sa, sb = ta.state_dict(), tb.state_dict()
    assert set(sa) == set(sb) == {"t", "m", "v", "names", "numel", "hyper"}
    assert sa["hyper"] == {"lr": 1e-4, "weight_decay": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8}
    assert sb["hyper"]["decoupled_weight_decay"] is True and sb["hyper"]["max_grad_norm"] == 1.0
    # settings of the decoupled rule without it are refused, not ignored
    for kw in (dict(no_decay=("bias",)), dict(max_grad_norm=1.0), dict(correct_bias=False)):
        with pytest.raises(ValueError, match="decoupled"):
            FlatTrainer(_Net(), **kw)

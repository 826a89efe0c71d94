"""The validity rule of the weight-derived caches (get_amd/ops/weights.py) on CPU tensors: the two doors to the library are
replaced by torch, everything else is the code the model runs.  The rule decides whether a step runs on stale weights: an
entry holds while its source is the same object at the same address and in-place version and the weight epoch stands still
(a frozen entry ignores the trainer's epoch).  Every table starts empty in every test."""
import gc

import pytest
import torch

from get_amd import _lib, ops

W = ops.weights
TABLES = ("_WT_CACHE", "_BF16_CACHE", "_DERIVED_CACHE", "_WT_PERSIST", "_BF16_PERSIST", "_X3P_SIG")


@pytest.fixture
def log(monkeypatch):
    """The list of launches and notifications, with the library's part done by torch."""
    events = []

    def transpose(ws, wts, twins=None):
        events.append("transpose")
        for i, (w, wt) in enumerate(zip(ws, wts)):
            wt.copy_(w.detach().t())
            if twins is not None and twins[i] is not None:
                twins[i][0].copy_(w.detach())
                twins[i][1].copy_(w.detach().t())

    monkeypatch.setattr(W, "_transpose", transpose)
    monkeypatch.setattr(W, "_notify", events.append)
    for name in TABLES:
        monkeypatch.setattr(W, name, {})
    return events


def param(rows=5, cols=7):
    return torch.nn.Parameter(torch.randn(rows, cols))


def test_derived_hits_and_misses(log):
    w = param()
    made = []

    def get(frozen=False):
        return ops.derived("colsum", (w,), lambda: made.append(1) or w.detach().sum(0), frozen=frozen)

    first = get()
    assert get() is first and len(made) == 1                       # hit on repeat
    with torch.no_grad():
        w.add_(1)
    assert torch.equal(get(), w.detach().sum(0)) and len(made) == 2       # in-place update: _version moved
    w.data = torch.randn(5, 7)
    assert torch.equal(get(), w.detach().sum(0)) and len(made) == 3       # storage replaced: data_ptr moved
    W._bump_trainer_epoch()
    get()
    assert len(made) == 4                                          # the trainer's epoch
    before = get()
    w.data += 1                                                    # a raw write moves neither _version nor data_ptr ...
    assert get() is before and len(made) == 4                      # ... and is NOT noticed: what bump_weight_epoch is for
    ops.bump_weight_epoch()
    assert torch.equal(get(), w.detach().sum(0)) and len(made) == 5


def test_frozen_derived_entry_survives_the_trainer_epoch_only(log):
    w = param()
    made = []
    get = lambda: ops.derived("frozen", (w,), lambda: made.append(1) or w.detach().clone(), frozen=True)
    first = get()
    W._bump_trainer_epoch()
    assert get() is first and len(made) == 1
    assert ops.derived("frozen", (w,), lambda: made.append(1) or w.detach().clone()) is not first      # asked unfrozen: a miss
    get()
    ops.bump_weight_epoch()
    assert get() is not first and len(made) == 4
    with torch.no_grad():
        w.add_(1)
    assert torch.equal(get(), w.detach())                          # frozen ignores the epoch, not the tensor


def transposed_of(w):
    return ops.transposed(w)


def twin_of(w):
    return ops.bf16_twins(w)[1].float()


@pytest.mark.parametrize("get", [transposed_of, twin_of])
def test_transposed_and_twins_hit_and_miss(log, get):
    w = param()
    ref = lambda: w.detach().t().to(torch.bfloat16).float() if get is twin_of else w.detach().t()
    assert torch.equal(get(w), ref())
    n = len(log)
    if get is transposed_of:
        assert ops.transposed(w) is ops.transposed(w)
    else:
        assert ops.bf16_twins(w)[0] is ops.bf16_twins(w)[0] and ops.bf16_twins(w)[1] is ops.bf16_twins(w)[1]
    assert len(log) == n                                           # hits launch nothing
    with torch.no_grad():
        w.add_(1)
    assert torch.equal(get(w), ref()) and len(log) == n + 1
    w.data = torch.randn(5, 7)
    assert torch.equal(get(w), ref()) and len(log) == n + 2
    W._bump_trainer_epoch()
    assert torch.equal(get(w), ref()) and len(log) == n + 3
    ops.bump_weight_epoch()
    assert torch.equal(get(w), ref()) and len(log) == n + 4
    w.data += 1                                                    # not noticed, as for `derived`
    get(w)
    assert len(log) == n + 4


def test_refresh_primes_the_caches_and_keeps_the_addresses(log):
    w, v = param(5, 7), param(8, 12)
    w16, wt16 = ops.bf16_twins(w)                                  # w has twins, v has none
    ops.refresh_transposes([w, v, torch.nn.Parameter(torch.randn(4))])      # (vectors are skipped)
    wt, vt = ops.transposed(w), ops.transposed(v)
    n = len(log)
    addresses = [t.data_ptr() for t in (wt, vt, w16, wt16)]
    with torch.no_grad():
        w.add_(1)
        v.mul_(2)
    W._bump_trainer_epoch()
    ops.refresh_transposes([w, v])
    assert len(log) == n + 1                                       # one launch for everything
    assert ops.transposed(w) is wt and ops.transposed(v) is vt and ops.bf16_twins(w)[0] is w16 and ops.bf16_twins(w)[1] is wt16
    assert len(log) == n + 1                                       # and all of them primed
    assert [t.data_ptr() for t in (wt, vt, w16, wt16)] == addresses
    assert torch.equal(wt, w.detach().t()) and torch.equal(vt, v.detach().t())
    assert torch.equal(w16, w.detach().to(torch.bfloat16)) and torch.equal(wt16, w.detach().t().to(torch.bfloat16))
    assert id(v) not in W._BF16_CACHE


def test_presplit_mode_keeps_the_transpose_address_and_tells_the_library(log, monkeypatch):
    monkeypatch.setattr(_lib, "_GEMM_MODE", "fp32x3p")
    w = param()
    wt = ops.transposed(w)
    assert log == ["gh_weights_changed", "transpose"]
    with torch.no_grad():
        w.add_(1)
    again = ops.transposed(w)
    assert again.data_ptr() == wt.data_ptr() and torch.equal(again, w.detach().t())
    ops.refresh_transposes([w])
    assert ops.transposed(w).data_ptr() == wt.data_ptr() and log[-2:] == ["transpose", "gh_fp32x3_refresh"]
    W._bump_trainer_epoch()
    assert log[-1] == "gh_weights_changed"
    ops.bump_weight_epoch()
    assert log[-1] == "gh_fp32x3_clear"


@pytest.mark.parametrize("shape", [(8, 12), (5, 7)])
def test_recycled_id_gets_fresh_buffers(log, shape):
    """An entry left by a dead parameter, met again under the id of a new one (planted: the allocator is not relied on)."""
    w = param(5, 7)
    ops.bf16_twins(w)
    stale = {name: next(iter(getattr(W, name).values())) for name in TABLES[:2] + TABLES[3:5]}
    old = [stale["_WT_PERSIST"].value[-1], stale["_BF16_PERSIST"].value[-1]]
    del w
    gc.collect()
    v = param(*shape)
    for name, entry in stale.items():
        getattr(W, name)[id(v)] = entry
    wt, (v16, vt16) = ops.transposed(v), ops.bf16_twins(v)
    assert torch.equal(wt, v.detach().t()) and torch.equal(v16, v.detach().to(torch.bfloat16))
    assert torch.equal(vt16, v.detach().t().to(torch.bfloat16))
    assert wt is not old[0] and vt16 is not old[1] and wt.data_ptr() != old[0].data_ptr() and vt16.data_ptr() != old[1].data_ptr()


def test_dead_entries_are_swept_from_every_table(log):
    alive = []
    for _ in range(600):            # 600 distinct ids: all alive until every table holds them
        w, m = param(2, 3), torch.nn.Linear(2, 1)
        ops.transposed(w)
        ops.bf16_twins(w)
        ops.derived("sweep", (w,), lambda: 0)
        ops.fp32x3p_guard(m)
        alive.append((w, m))
    assert all(len(getattr(W, name)) == 600 for name in TABLES)
    del alive, w, m
    gc.collect()
    w, m = param(2, 3), torch.nn.Linear(2, 1)
    ops.transposed(w)
    ops.bf16_twins(w)
    ops.derived("sweep", (w,), lambda: 0)
    ops.fp32x3p_guard(m)
    for name in TABLES:
        assert len(getattr(W, name)) < 600, name


def test_fp32x3p_guard_fires_once_per_change(log):
    m = torch.nn.Linear(3, 2)
    ops.fp32x3p_guard(m)
    ops.fp32x3p_guard(m)
    assert log == ["gh_weights_changed"]
    with torch.no_grad():
        m.weight.add_(1)
    ops.fp32x3p_guard(m)
    ops.fp32x3p_guard(m)
    assert log == ["gh_weights_changed"] * 2


def test_fp32x3p_guard_misses_on_a_recycled_module_id(log):
    m = torch.nn.Linear(3, 2)
    ops.fp32x3p_guard(m)
    other = torch.nn.Linear(3, 2)
    other.weight, other.bias = m.weight, m.bias                    # the same parameters: the same signature
    stale = W._X3P_SIG.pop(id(m))
    del m
    gc.collect()
    W._X3P_SIG[id(other)] = stale                                  # what a recycled id(module) would find
    ops.fp32x3p_guard(other)
    assert log == ["gh_weights_changed"] * 2

"""The BERT task models (get_amd/bert.py) on the GPU against the reference's golden vectors (tests/golden/g23_bert_heads.npz,
captured by tools/make_heads_golden.py) and, in training mode and over three optimiser steps, against the float64 restatement
of tests/heads_ref.py.

Bounds, elementwise against the reference's fp32 result, those of tests/test_gpu_bert.py: outputs and loss 1e-4 + 1e-4 |want|,
parameter gradients 1e-5 + 1e-4 |want| (the generator holds the reference's own fp32-vs-float64 error to a tenth of them)."""
import pytest
import torch

from tests import heads_ref
from tests.test_bert_heads_cpu import CASES, TIED, archive, as_stored, case_inputs, objective, pset_params, state_of
from tests.util import DEV, bits_equal, golden_ratio

pytestmark = pytest.mark.gpu

OUT_TOL, GRAD_TOL = (1e-4, 1e-4), (1e-5, 1e-4)


def _build(z, contract, name, **config_changes):
    from get_amd import bert
    c = contract[CASES[name]]
    m = getattr(bert, c["class"])(bert.BertConfig.from_dict(dict(c["config"], **config_changes)))
    m.load_state_dict(state_of(pset_params(z, CASES[name]), c), strict=True)
    return m.to(DEV).eval()


def _inputs(z, name, int32=False):
    out = {k: v.to(DEV) for k, v in case_inputs(z, name).items()}
    if int32:
        out = {k: (v.int() if v.dtype == torch.int64 else v) for k, v in out.items()}
    return out


def _grads(m, z, meta, name, out):
    m.zero_grad(set_to_none=True)
    objective(z, meta, name, out, torch.float32).backward()
    torch.cuda.synchronize()
    return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def _check_case(m, z, meta, name, out, grads, what):
    worst = 0.0
    n_out = len([k for k in z if k.startswith(name + "::out::")])
    assert len(out) == n_out, (what, len(out), n_out)
    for i, t in enumerate(out):
        worst = max(worst, golden_ratio(as_stored(t), z[f"{name}::out::{i}"], *OUT_TOL, f"{what} out::{i}"))
    want = {k[len(name) + len("::grad::"):] for k in z if k.startswith(name + "::grad::")}
    assert set(grads) == want, (what, set(grads) ^ want)
    for k, g in grads.items():
        worst = max(worst, golden_ratio(g, z[f"{name}::grad::{k}"], *GRAD_TOL, f"{what} grad::{k}"))
    print(f"{what}: worst ratio of the bound {worst:.3f}")


@pytest.mark.parametrize("name", list(CASES))
def test_golden_case_through_the_drop_in(golden_dir, name):
    """Outputs, loss and every parameter gradient of every golden case; two forward + backward passes give the same bits."""
    z, meta, contract = archive(golden_dir)
    m = _build(z, contract, name)
    inputs = _inputs(z, name)
    before = {k: v.clone() for k, v in inputs.items()}
    out = m(**inputs)
    grads = _grads(m, z, meta, name, out)
    _check_case(m, z, meta, name, out, grads, name)
    for k, v in inputs.items():      # (the reference clamps the question-answering positions in place; the drop-in does not)
        assert torch.equal(v, before[k]), f"{name}: the caller's {k} was changed"
    out2 = m(**inputs)
    for i, (a, b) in enumerate(zip(out, out2)):
        bits_equal(as_stored(a), as_stored(b), f"{name}: out::{i} of two forward passes")
    again = _grads(m, z, meta, name, out2)
    for k, g in grads.items():
        bits_equal(g, again[k], f"{name} grad::{k}: two backward passes")


@pytest.mark.parametrize("name", ["pretraining", "tokcls_mask", "qa"])
def test_int32_ids_and_labels_give_the_same_bits(golden_dir, name):
    z, meta, contract = archive(golden_dir)
    m = _build(z, contract, name)
    out = m(**_inputs(z, name))
    grads = _grads(m, z, meta, name, out)
    out32 = m(**_inputs(z, name, int32=True))
    for i, (a, b) in enumerate(zip(out, out32)):
        bits_equal(as_stored(a), as_stored(b), f"{name}: out::{i} with int32 ids and labels")
    for k, g in _grads(m, z, meta, name, out32).items():
        bits_equal(grads[k], g, f"{name}: grad::{k} with int32 ids and labels")


def test_the_tied_gradient_is_the_sum_and_survives_an_optimiser_step(golden_dir):
    """grad of the word table = the table's deterministic row sums + the decoder's weight gradient (the golden holds their sum
    under one name); after an AdamW step both state_dict names still share one storage that has moved."""
    from get_amd.optim import AdamW
    z, meta, contract = archive(golden_dir)
    name = "mlm_labels"
    m = _build(z, contract, name).train(False)
    word = m.bert.embeddings.word_embeddings.weight
    assert m.cls.predictions.decoder.weight is word and TIED[1] not in dict(m.named_parameters())
    opt = AdamW(m.parameters(), lr=1e-2)
    out = m(**_inputs(z, name))
    grads = _grads(m, z, meta, name, out)
    golden_ratio(grads[TIED[0]], z[f"{name}::grad::{TIED[0]}"], *GRAD_TOL, "tied gradient against the golden sum")
    # either part alone is not the sum: the rows of ids that are no label carry only the table's part, and vice versa
    before = word.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    sd = m.state_dict()
    assert m.cls.predictions.decoder.weight is m.bert.embeddings.word_embeddings.weight
    assert sd[TIED[0]].data_ptr() == sd[TIED[1]].data_ptr()
    assert float((sd[TIED[1]] - before).abs().max()) > 1e-3


def _head_keep(seed, rows, cols, p):
    from get_amd import ops
    return torch.from_numpy(ops.dropout_mask_reference(seed, rows, cols, p))


@pytest.mark.parametrize("name", ["seqcls_n5", "tokcls_mask", "choice"])
def test_training_mode_head_dropout_follows_the_predicted_mask(golden_dir, name):
    """The heads' own dropout (the pooled output of the classification and multiple-choice heads, the sequence output of the
    token classifier), with the encoder's dropout off: one seed, drawn after the encoder's, and the result is the float64
    restatement's under the mask that seed predicts."""
    from get_amd import ops
    z, meta, contract = archive(golden_dir)
    p = 0.3
    m = _build(z, contract, name, hidden_dropout_prob=p, attention_probs_dropout_prob=0.0).train()
    for mod in m.bert.modules():      # the encoder's sites off: this test is about the head's
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    torch.manual_seed(77)
    out = m(**_inputs(z, name))
    seeds = list(m.last_dropout_seeds)
    torch.manual_seed(77)
    assert seeds == [ops.new_dropout_seed()]
    grads = _grads(m, z, meta, name, out)
    c = contract[CASES[name]]
    site = out[1].shape[:-1] if name == "tokcls_mask" else (out[1].numel() // (1 if name == "choice" else out[1].shape[-1]),)
    h = c["config"]["hidden_size"]
    rows = 1
    for n in site:
        rows *= n
    keep = _head_keep(seeds[0], rows, h, p).reshape(*site, h)
    assert 0.1 < 1.0 - float(keep.double().mean()) < 0.5
    p64 = {k: v.requires_grad_(True) for k, v in pset_params(z, CASES[name], torch.float64).items()}
    conf = dict(c["config"], hidden_dropout_prob=p, attention_probs_dropout_prob=0.0)
    want = heads_ref.task_model(c["class"], state_of(p64, c), conf, case_inputs(z, name), masks=None, head_keep=keep)
    objective(z, meta, name, want, torch.float64).backward()
    for i, (a, b) in enumerate(zip(out, want)):
        golden_ratio(a, b, *OUT_TOL, f"{name} training mode out::{i}")
    assert float((out[0].detach().double().cpu() - torch.from_numpy(z[f"{name}::out::0"]).double()).abs().max()) > 1e-3      # dropout acted
    for k, g in grads.items():
        golden_ratio(g, p64[k].grad, *GRAD_TOL, f"{name} training mode grad::{k}")


def test_head_dropout_seed_follows_the_encoders(golden_dir):
    """With every site on, the head's seed is the last of 1 + 3 * layers + 1 draws in forward order."""
    from get_amd import ops
    z, meta, contract = archive(golden_dir)
    m = _build(z, contract, "seqcls_n2", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1).train()
    torch.manual_seed(9)
    m(**_inputs(z, "seqcls_n2"))
    seeds = list(m.last_dropout_seeds)
    torch.manual_seed(9)
    assert seeds == [ops.new_dropout_seed() for _ in range(1 + 3 * m.config.num_hidden_layers + 1)]


def test_three_training_steps_follow_the_float64_restatement(golden_dir):
    """BertForSequenceClassification (h24, num_labels 2), eval-mode forward, AdamW with clipping at 1.0 and the linear warmup
    schedule: the three losses are the float64 restatement's (optimization.py:159-187 written out on autograd's float64
    gradients).  warmup_steps = 0, t_total = 4: the schedule's factors are 1, 0.75 and 0.5 -- with a warmup its factor at step 0 is 0
    and the first update would move nothing -- so the second and the third loss each follow a real update."""
    from get_amd.optim import AdamW, WarmupLinearSchedule
    z, meta, contract = archive(golden_dir)
    name = "seqcls_n2"
    c = contract[CASES[name]]
    m = _build(z, contract, name)
    lr, wd, max_norm, warmup, total = 5e-3, 0.01, 1.0, 0, 4
    opt = AdamW(m.parameters(), lr=lr, weight_decay=wd, correct_bias=False, max_grad_norm=max_norm)
    sched = WarmupLinearSchedule(opt, warmup_steps=warmup, t_total=total)
    inputs = _inputs(z, name)
    got = []
    for _ in range(3):
        loss = m(**inputs)[0]
        got.append(loss.detach().clone())
        opt.zero_grad()
        loss.backward()
        opt.step()
        sched.step()
    torch.cuda.synchronize()
    # float64
    p64 = {k: v.clone().requires_grad_(True) for k, v in pset_params(z, CASES[name], torch.float64).items()}
    state = {k: (torch.zeros_like(v), torch.zeros_like(v)) for k, v in p64.items()}
    want = []
    for step in range(3):
        loss = heads_ref.task_model(c["class"], p64, c["config"], case_inputs(z, name))[0]
        want.append(loss.detach())
        grads = torch.autograd.grad(loss, list(p64.values()))
        norm = torch.sqrt(sum((g * g).sum() for g in grads))
        clip = min(1.0, max_norm / (float(norm) + 1e-6)) if float(norm) > max_norm else 1.0
        factor = (step / max(1, warmup)) if step < warmup else max(0.0, (total - step) / max(1.0, total - warmup))
        with torch.no_grad():
            for (k, p), g in zip(p64.items(), grads):
                mom, var = state[k]
                g = g * clip
                mom.mul_(0.9).add_(g, alpha=0.1)
                var.mul_(0.999).addcmul_(g, g, value=0.001)
                p.addcdiv_(mom, var.sqrt() + 1e-6, value=-lr * factor)
                p.add_(p, alpha=-lr * factor * wd)
    for i, (a, b) in enumerate(zip(got, want)):
        golden_ratio(a, b, *OUT_TOL, f"loss of step {i}")
    assert float((want[0] - want[1]).abs()) > 1e-3 and float((want[1] - want[2]).abs()) > 1e-3, "every step moved the loss"


def test_the_op_on_a_view_equals_the_op_on_its_copy(golden_dir):
    """ops.softmax_cross_entropy on the question-answering head's strided columns against their contiguous copies, bit for bit."""
    from get_amd import ops
    z, meta, contract = archive(golden_dir)
    m = _build(z, contract, "qa")
    inputs = _inputs(z, "qa")
    _, start, end = m(**inputs)
    assert not start.is_contiguous() and start.data_ptr() + 4 == end.data_ptr()
    L = start.shape[1]
    for lg, pos in ((start, inputs["start_positions"]), (end, inputs["end_positions"])):
        pos = pos.squeeze(-1).clamp(0, L)
        a = ops.softmax_cross_entropy(lg.detach(), pos, ignore_index=L)
        b = ops.softmax_cross_entropy(lg.detach().contiguous(), pos, ignore_index=L)
        bits_equal(a.reshape(1), b.reshape(1), "view against copy")

"""The references of tests/test_gpu_concat_att_paths.py and tests/test_gpu_ragged_paths.py, checked without any kernel:
tests/util.py's float64 `_concat64` against the oracle and against the goldens captured from the reference, at the golden
tests' own bounds (values and all four gradients), the numpy ragged restatements against the oracle's pad_left /
pad_right, and the conditions the GPU cases rely on (no all-masked pair outside the two named cases, non-zero floors)."""
import numpy as np
import pytest
import torch

from oracle import cases
from oracle import get_oracle as O
from tests.util import (_concat64, check_grad, load, r_evd_assemble, r_evd_assemble_bwd, r_masked_mean, r_masked_mean_bwd,
                        r_seg_offsets, r_seg_pad, r_seg_sum, r_seg_unpad)


def _t64(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).double().requires_grad_(grad)


def _maxerr(a, b):
    return float((a.detach().double() - torch.as_tensor(np.asarray(b)).double()).abs().max())


@pytest.mark.parametrize("ci", range(len(cases.G5_CASES)))
def test_concat64_matches_the_oracle_and_the_g5_golden(ci):
    z, _ = load("g5_concat_att.npz")
    c = cases.g5_inputs(ci)
    left, right, w1, w2 = (_t64(c[k], True) for k in ("left", "right", "w1", "w2"))
    mask = _t64(c["mask"].astype(np.float32))
    u, t, e, w, att = _concat64(left, right, mask, w1, w2)
    att_o, w_o = O.concat_att(left, right, mask, w1, w2)
    assert _maxerr(att, att_o.detach()) <= 1e-12 and _maxerr(w, w_o.detach()) <= 1e-12
    assert _maxerr(att, z[f"c{ci}_att"]) <= 1e-5            # bounds of test_concat_att_vs_golden
    assert _maxerr(w, z[f"c{ci}_w"]) <= 1e-6
    assert float((w.detach().sum(1) - 1.0).abs().max()) <= 1e-5
    ((att * _t64(c["g_att"])).sum() + (w * _t64(c["g_w"])).sum()).backward()
    check_grad(z, f"c{ci}_dleft", left.grad.numpy())
    check_grad(z, f"c{ci}_dright", right.grad.numpy())
    check_grad(z, f"c{ci}_g::linear1.weight", w1.grad.numpy())
    check_grad(z, f"c{ci}_g::linear2.weight", w2.grad.numpy())
    # the saved tensors are what the definition says they are
    xl = left.shape[1]
    assert _maxerr(u, (left @ w1[:, :xl].t()).detach()) == 0.0
    assert _maxerr(e, (t @ w2.t()).detach()) == 0.0


@pytest.mark.parametrize("ci", range(len(cases.G6_CASES)))
def test_concat64_without_left_matches_the_oracle_and_the_g6_golden(ci):
    z, _ = load("g6_self_att.npz")
    c = cases.g6_inputs(ci)
    tsr, w1, w2 = (_t64(c[k], True) for k in ("tsr", "w1", "w2"))
    mask = _t64(c["mask"])
    u, t, e, w, att = _concat64(None, tsr, mask, w1, w2)
    assert float(u.abs().max()) == 0.0
    att = att.transpose(1, 2)                                # (B, C, D) of self_attention.py:98
    att_o, w_o = O.self_att_extend(tsr, mask, w1, w2)
    assert _maxerr(att, att_o.detach()) <= 1e-12 and _maxerr(w, w_o.detach()) <= 1e-12
    assert _maxerr(att, z[f"c{ci}_att"]) <= 1e-5            # bounds of test_self_att_extend_vs_golden
    assert _maxerr(w, z[f"c{ci}_w"]) <= 1e-6
    ((att * _t64(c["g_att"])).sum() + (w * _t64(c["g_w"])).sum()).backward()
    check_grad(z, f"c{ci}_dtsr", tsr.grad.numpy())
    check_grad(z, f"c{ci}_g::linear1.weight", w1.grad.numpy())
    check_grad(z, f"c{ci}_g::linear2.weight", w2.grad.numpy())


def test_concat64_all_masked_pair_is_nan_and_only_that_pair():
    g = torch.Generator().manual_seed(4)
    right, left = torch.randn(3, 5, 8, generator=g).double(), torch.randn(3, 4, generator=g).double()
    w1, w2 = torch.randn(6, 12, generator=g).double(), torch.randn(2, 6, generator=g).double()
    mask = torch.ones(3, 5)
    mask[1] = 0
    _, _, _, w, att = _concat64(left, right, mask, w1, w2)
    assert bool(torch.isnan(w[1]).all()) and bool(torch.isnan(att[1]).all())
    assert bool(torch.isfinite(w[[0, 2]]).all()) and bool(torch.isfinite(att[[0, 2]]).all())


# ----------------------------------------------------------------------------- ragged restatements
@pytest.mark.parametrize("counts,n_max", [([2, 5, 1], 5), ([0, 3, 0, 4, 1, 0], 4), ([7], 7)])
def test_ragged_restatements_match_pad_left_and_pad_right(counts, n_max):
    rng = np.random.default_rng(sum(counts))
    b, b1, x = len(counts), sum(counts), 6
    offsets, p2c, has = r_seg_offsets(counts, b1)
    assert offsets.tolist() == [0] + np.cumsum(counts).tolist()
    assert has.tolist() == [1.0 if c > 0 else 0.0 for c in counts]
    per_claim = rng.standard_normal((b, x)).astype(np.float32)
    assert np.array_equal(per_claim[p2c], O.pad_left(torch.from_numpy(per_claim), counts).numpy())
    per_pair = rng.standard_normal((b1, x)).astype(np.float32)
    padded = r_seg_pad(per_pair, offsets, n_max)
    assert np.array_equal(padded, O.pad_right(torch.from_numpy(per_pair), counts, n_max).numpy())
    # unpad is the inverse on the rows pad copied; the sum is the adjoint of pad_left
    assert np.array_equal(r_seg_unpad(padded, offsets, np.full((b1, x), np.nan, np.float32)), per_pair)
    t = torch.from_numpy(per_claim).double().requires_grad_(True)
    (O.pad_left(t, counts) * torch.from_numpy(per_pair).double()).sum().backward()
    assert np.abs(r_seg_sum(per_pair, offsets) - t.grad.numpy()).max() <= 1e-12


def test_seg_offsets_restatement_tail_and_overflow():
    _, p2c, _ = r_seg_offsets([1, 2], 6)                  # sum(counts) < b1: the tail maps to claim 0
    assert p2c.tolist() == [0, 1, 1, 0, 0, 0]
    _, p2c, _ = r_seg_offsets([1, 4, 2], 4)               # sum(counts) > b1: only b1 pairs exist
    assert p2c.tolist() == [0, 1, 1, 1]


def test_evd_assemble_restatement_matches_the_oracle_statements():
    """right = [pad_right(avg) | table[max(src, 0)]], mask = (sum of ids >= 1); the backward is autograd's of the same."""
    rng = np.random.default_rng(9)
    counts, n_max, xa, ds, rows, r = [2, 0, 3], 3, 4, 5, 6, 7
    b, b1 = len(counts), sum(counts)
    offsets, _, _ = r_seg_offsets(counts, b1)
    avg = rng.standard_normal((b1, xa)).astype(np.float32)
    table = rng.standard_normal((rows, ds)).astype(np.float32)
    sources = rng.integers(-1, rows, size=(b, n_max))
    sources[0, 0], sources[2, 1] = 2, 2
    document = rng.integers(0, 3, size=(b, n_max, r)) * (rng.random((b, n_max, 1)) < 0.7)
    right, mask, clamped = r_evd_assemble(avg, offsets, table, sources, document, n_max)
    assert clamped == 0
    ta, tt = torch.from_numpy(avg).double().requires_grad_(True), torch.from_numpy(table).double().requires_grad_(True)
    want = torch.cat([O.pad_right(ta, counts, n_max), tt[torch.from_numpy(np.maximum(sources, 0))]], dim=-1)
    assert np.array_equal(right, want.detach().float().numpy())
    assert np.array_equal(mask, (document.sum(-1) >= 1).astype(np.float32))
    # the kernel's backward contract: gradient rows of padding slots are exact zeros (they are masked out of the softmax)
    g = rng.standard_normal(right.shape).astype(np.float32)
    g *= (np.arange(n_max)[None, :] < np.asarray(counts)[:, None])[:, :, None]
    (want * torch.from_numpy(g).double()).sum().backward()
    d_avg, d_table = r_evd_assemble_bwd(g, offsets, sources, rows, xa, np.zeros((rows, ds)))
    assert np.abs(d_avg - ta.grad.numpy()).max() <= 1e-7
    assert np.abs(d_table - tt.grad.numpy()).max() <= 1e-12
    assert r_evd_assemble(avg, offsets, table, np.where(sources == 2, rows + 3, sources), document, n_max)[2] == 2


def test_masked_mean_restatement_is_its_own_adjoint():
    rng = np.random.default_rng(3)
    hid = rng.standard_normal((3, 5, 4))
    ids = rng.integers(0, 3, size=(3, 5))
    ids[:, 0] = 1
    lens = (ids > 0).sum(1).astype(np.float64)
    g = rng.standard_normal((3, 4))
    lhs = (r_masked_mean(hid, ids, lens) * g).sum()
    rhs = (hid * r_masked_mean_bwd(g, ids, lens)).sum()
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    assert not r_masked_mean_bwd(g, ids, lens)[ids == 0].any()


# ----------------------------------------------------------------------------- what the GPU cases rely on
def test_gpu_cases_have_no_all_masked_pair_and_non_zero_floors():
    """Collected from the GPU file's own case builders (they are plain CPU code): outside the all-masked forward case and
    the 0-row pair of the compact layout every pair keeps a live row, and every floor a case passes is non-zero."""
    from tests import test_gpu_concat_att_paths as P
    n_floor = 0
    for spec in P.all_specs():
        c = P.make_case(spec)
        live = c.mask_padded.sum(1) > 0
        dead = set(np.nonzero(~live.numpy())[0].tolist())
        assert dead == set(c.dead_pairs), (spec, dead, c.dead_pairs)
        if not spec.get("all_masked") and spec.get("rows") is None:
            assert not dead, spec
        if c.de_floor is not None:
            n_floor += 1
            assert c.de_floor > 0.0, spec
    assert n_floor >= 3

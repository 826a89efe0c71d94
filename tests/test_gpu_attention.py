"""GPU checks of the single-query attention ablations Dot / BiLinear / BiLinearTanh / SelfAttentionICLR2017 /
MultiHeadSelfAttentionICLR17OnWord (get_amd.modules, ops.query_att / ops.tanh_att, csrc/attention_ops.hip) against the
reference's captured outputs and gradients (tests/golden/g12_attention.npz), the padding and all-masked conventions, the
weights-gradient-free backward, the project's word- and evidence-level shapes against float64 restatements, and the
documented length limits."""
import pytest
import torch

from tests.util import _module64, _query64, _tanh64, build_from_contract, golden_ratio, load_golden, rel_close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0") if torch.cuda.is_available() else None

CASES = ["dot_d6", "dot_d8", "bilinear", "bilineartanh", "selfatt", "onword_h1", "onword_h3", "dot_offset_pos",
         "dot_offset_neg"]
# forward arguments in order, the mask excluded
ARGS = {"Dot": ("left", "right"), "BiLinear": ("left", "right"), "BiLinearTanh": ("left_tsr", "right_tsr"),
        "SelfAttentionICLR2017": ("tsr",), "MultiHeadSelfAttentionICLR17OnWord": ("original", "tsr")}


def _golden(golden_dir):
    return load_golden(golden_dir, "g12_attention.npz", "attention_contract.json")


def _build(z, key, c):
    return build_from_contract(z, key, c).to(DEV)


def _forward(m, cls, inputs, mask):
    """(out, weights or None) of a module of class `cls` on the ordered input tensors."""
    if cls == "MultiHeadSelfAttentionICLR17OnWord":
        return m(*inputs, mask, return_att_weights=True)
    out = m(*inputs, mask)
    return out if isinstance(out, tuple) else (out, None)


def _golden_run(z, contract, name, geom, mask_dtype=None, mask_edit=None):
    """Forward + backward of one golden case; returns (module, inputs by name, out, weights)."""
    key = f"{name}/{geom}::"
    c = contract[name]
    m = _build(z, key, c)
    inputs = {k: torch.from_numpy(z[key + k]).to(DEV).requires_grad_(True) for k in ARGS[c["class"]]}
    mask = torch.from_numpy(z[key + "mask"]).clone()
    if mask_edit is not None:
        mask_edit(mask)
    mask = mask.to(DEV) if mask_dtype is None else mask.to(DEV).to(mask_dtype)
    out, weights = _forward(m, c["class"], [inputs[k] for k in ARGS[c["class"]]], mask)
    loss = (out * torch.from_numpy(z[key + "gout"]).to(DEV)).sum()
    if weights is not None:
        loss = loss + (weights * torch.from_numpy(z[key + "gweights"]).to(DEV)).sum()
    loss.backward()
    return m, inputs, out, weights


@pytest.mark.parametrize("name", CASES)
def test_attention_matches_reference_goldens(golden_dir, name):
    """Outputs 1e-4 + 1e-4 |want|, gradients 1e-5 + 1e-4 |want| elementwise (the bounds of test_gpu_encoders.py against
    reference fp32 goldens); the two offset cases, whose scores sit near +-96 where the reference's own fp32 rounding
    exceeds the elementwise bound, by largest error over largest entry <= 1e-4."""
    z, meta, contract = _golden(golden_dir)
    assert set(meta["cases"]) == set(CASES)
    offset = name in meta["offset_cases"]
    for geom in meta["geometries"]:
        key = f"{name}/{geom}::"
        m, inputs, out, weights = _golden_run(z, contract, name, geom)
        checks = [(out, "out", 1e-4)]
        if weights is not None:
            checks.append((weights, "weights", 1e-4))
        checks += [(t.grad, "grad::" + k, 1e-5) for k, t in inputs.items()]
        checks += [(p.grad, "grad::" + k, 1e-5) for k, p in m.named_parameters()]
        for got, k, atol in checks:
            assert got is not None, key + k
            if offset:
                rel_close(got, z[key + k], 1e-4, key + k)
            else:
                golden_ratio(got, z[key + k], atol, 1e-4, key + k)


@pytest.mark.parametrize("name", CASES)
def test_masked_positions_are_exact_zeros(golden_dir, name):
    """Weights at mask == 0 are exactly 0.0, the unmasked ones sum to 1 within 1e-5, the sequence operand's gradient rows
    at padded positions are exactly zero, and a bool mask gives the float mask's results bit for bit."""
    z, meta, contract = _golden(golden_dir)
    cls = contract[name]["class"]
    for geom in meta["geometries"]:
        key = f"{name}/{geom}::"
        pad = torch.from_numpy(z[key + "mask"]) == 0
        m, inputs, out, weights = _golden_run(z, contract, name, geom)
        mb, inputs_b, out_b, weights_b = _golden_run(z, contract, name, geom, mask_dtype=torch.bool)
        assert torch.equal(out, out_b)
        for k in inputs:
            assert torch.equal(inputs[k].grad, inputs_b[k].grad), key + k
        for p, q in zip(m.parameters(), mb.parameters()):
            assert torch.equal(p.grad, q.grad)
        if weights is not None:
            assert torch.equal(weights, weights_b)
            w = weights.detach().cpu()
            w = w if w.dim() == 3 else w.unsqueeze(-1)
            assert bool((w[pad] == 0.0).all()), key
            assert (w.sum(1) - 1.0).abs().max().item() <= 1e-5, key
        # the sequence operands: every gradient row of a padded position is exactly zero
        seq = {"Dot": ["right"], "BiLinear": ["right"], "BiLinearTanh": ["left_tsr"], "SelfAttentionICLR2017": ["tsr"],
               "MultiHeadSelfAttentionICLR17OnWord": ["original", "tsr"]}[cls]
        for k in seq:
            g = inputs[k].grad.cpu()
            assert bool((g[pad] == 0.0).all()), key + k
            assert bool((g[~pad] != 0.0).any()), key + k


def test_masked_rows_of_the_kernels_own_gradients(golden_dir):
    """ops.query_att / ops.tanh_att themselves: dright, dpre and dvalues rows of padded positions are exact zeros."""
    from get_amd import ops
    g = torch.Generator().manual_seed(21)
    for b, l, d, ha, heads, dv in ((3, 12, 6, 7, 3, 5), (2, 70, 8, 8, 2, 12)):
        mask = torch.ones(b, l)
        mask[0, 3] = mask[0, 5] = 0
        mask[1, 2 * l // 3:] = 0
        pad = mask == 0
        r = lambda *s: torch.randn(s, generator=g).to(DEV).requires_grad_(True)
        q, right = r(b, d), r(b, l, d)
        avg, w = ops.query_att(q, right, mask.to(DEV))
        ((avg * torch.randn(avg.shape, generator=g).to(DEV)).sum() + (w * torch.randn(w.shape, generator=g).to(DEV)).sum()).backward()
        assert bool((w.detach().cpu()[pad] == 0).all()) and bool((right.grad.cpu()[pad] == 0).all())
        assert bool(torch.isfinite(right.grad).all()) and bool(torch.isfinite(q.grad).all())
        pre, u, w2, values = r(b, l, ha), r(b, ha), r(heads, ha), r(b, l, dv)
        att, w = ops.tanh_att(pre, u, w2, mask.to(DEV), values)
        ((att * torch.randn(att.shape, generator=g).to(DEV)).sum() + (w * torch.randn(w.shape, generator=g).to(DEV)).sum()).backward()
        assert bool((w.detach().cpu()[pad] == 0).all())
        assert bool((pre.grad.cpu()[pad] == 0).all()) and bool((values.grad.cpu()[pad] == 0).all())
        for t in (pre, u, w2, values):
            assert bool(torch.isfinite(t.grad).all())


@pytest.mark.parametrize("name", ["dot_d6", "bilinear", "bilineartanh", "selfatt", "onword_h3"])
def test_all_masked_row_is_nan_and_leaves_the_others_alone(golden_dir, name):
    """A row whose mask is all zero yields NaN weights and a NaN output row (the reference's softmax of all -inf); every
    other row equals the run in which that row keeps its tokens, bit for bit."""
    z, meta, contract = _golden(golden_dir)
    cls = contract[name]["class"]
    for geom in meta["geometries"]:
        key = f"{name}/{geom}::"
        m = _build(z, key, contract[name])
        inputs = [torch.from_numpy(z[key + k]).to(DEV) for k in ARGS[cls]]
        mask = torch.from_numpy(z[key + "mask"]).to(DEV)
        dead = mask.clone()
        dead[1, :] = 0
        with torch.no_grad():
            out, weights = _forward(m, cls, inputs, mask)
            out_d, weights_d = _forward(m, cls, inputs, dead)
        keep = [i for i in range(mask.shape[0]) if i != 1]
        assert bool(torch.isnan(out_d[1]).all()), key
        assert torch.equal(out[keep], out_d[keep]) and bool(torch.isfinite(out_d[keep]).all()), key
        if weights is not None:
            assert bool(torch.isnan(weights_d[1]).all()), key
            assert torch.equal(weights[keep], weights_d[keep]), key


def test_self_attention_rejects_more_than_one_head():
    from get_amd import modules
    m = modules.SelfAttentionICLR2017(8, 7, num_heads=3).to(DEV)
    with pytest.raises(RuntimeError, match="num_heads"):
        m(torch.randn(2, 5, 8, device=DEV), torch.ones(2, 5, device=DEV))


def test_backward_without_a_weights_gradient(golden_dir):
    """A loss on the attended output alone (g_w = NULL in the kernels): finite gradients equal to the float64
    restatement's, at the golden suite's gradient bound 1e-5 + 1e-4 |want|."""
    z, meta, contract = _golden(golden_dir)
    for name in ("dot_d6", "bilinear", "bilineartanh", "onword_h3"):
        cls = contract[name]["class"]
        for geom in meta["geometries"]:
            key = f"{name}/{geom}::"
            m = _build(z, key, contract[name])
            inputs = [torch.from_numpy(z[key + k]).to(DEV).requires_grad_(True) for k in ARGS[cls]]
            mask = torch.from_numpy(z[key + "mask"]).to(DEV)
            gout = torch.from_numpy(z[key + "gout"]).to(DEV)
            out, _ = _forward(m, cls, inputs, mask)
            (out * gout).sum().backward()
            p64 = {k: v.detach().double().requires_grad_(True) for k, v in m.named_parameters()}
            in64 = [t.detach().double().requires_grad_(True) for t in inputs]
            out64, _ = _module64(cls, p64, in64, mask)
            (out64 * gout.double()).sum().backward()
            for k, got, want in ([(a, t.grad, t64.grad) for a, t, t64 in zip(ARGS[cls], inputs, in64)]
                                 + [(k, p.grad, p64[k].grad) for k, p in m.named_parameters()]):
                assert got is not None and bool(torch.isfinite(got).all()), key + k
                golden_ratio(got, want, 1e-5, 1e-4, key + "grad::" + k)


# ----------------------------------------------------------------------------- the project's shapes
def _project_module(cls, d):
    from get_amd import modules
    if cls == "Dot":
        return modules.Dot()
    if cls == "BiLinear":
        return modules.BiLinear(d)
    if cls == "BiLinearTanh":
        return modules.BiLinearTanh(d, d, d)
    return modules.MultiHeadSelfAttentionICLR17OnWord(d, d, 4)


@pytest.mark.parametrize("shape", [(960, 100, 300), (32, 30, 1200)], ids=["word", "evidence"])
@pytest.mark.parametrize("cls", ["Dot", "BiLinear", "BiLinearTanh", "MultiHeadSelfAttentionICLR17OnWord"])
def test_project_shapes_against_float64(cls, shape):
    """Word level (960 pairs x 100 nodes x 300) and evidence level (32 claims x 30 slots x 1200), lengths drawn in [1, L]:
    outputs, weights and every gradient within 1e-4 of the largest entry of a float64 restatement (the bench-scale bound of
    test_bench_scale_gat_and_gcn); two runs bit-identical on everything the attention kernels write."""
    b, l, d = shape
    torch.manual_seed(17)
    g = torch.Generator().manual_seed(b + l + d)
    m = _project_module(cls, d).to(DEV)
    lengths = torch.randint(1, l + 1, (b,), generator=g)
    mask = (torch.arange(l)[None, :] < lengths[:, None]).to(DEV)
    r = lambda *s: (0.2 * torch.randn(s, generator=g)).to(DEV)
    seq, query = r(b, l, d), r(b, d)
    raw = {"Dot": [query, seq], "BiLinear": [query, seq], "BiLinearTanh": [seq, query],
           "MultiHeadSelfAttentionICLR17OnWord": [r(b, l, d), seq]}[cls]
    runs = []
    for _ in range(2):
        for p in m.parameters():
            p.grad = None
        inputs = [t.clone().requires_grad_(True) for t in raw]
        out, weights = _forward(m, cls, inputs, mask)
        if not runs:
            gout = torch.randn(out.shape, generator=g).to(DEV)
            gweights = torch.randn(weights.shape, generator=g).to(DEV)
        ((out * gout).sum() + (weights * gweights).sum()).backward()
        runs.append((out.detach(), weights.detach(), [t.grad for t in inputs],
                     {k: p.grad.clone() for k, p in m.named_parameters()}))
    (o1, w1, gi1, gp1), (o2, w2, gi2, gp2) = runs
    assert torch.equal(o1, o2) and torch.equal(w1, w2)
    assert all(torch.equal(a, c) for a, c in zip(gi1, gi2))
    for k in ("combine.weight", "linear2.weight"):
        if k in gp1:
            assert torch.equal(gp1[k], gp2[k]), k
    p64 = {k: v.detach().double().requires_grad_(True) for k, v in m.named_parameters()}
    in64 = [t.double().requires_grad_(True) for t in raw]
    out64, weights64 = _module64(cls, p64, in64, mask)
    ((out64 * gout.double()).sum() + (weights64 * gweights.double()).sum()).backward()
    rel_close(o1, out64, 1e-4, "out")
    rel_close(w1, weights64, 1e-4, "weights")
    for k, got, t64 in zip(ARGS[cls], gi1, in64):
        rel_close(got, t64.grad, 1e-4, "grad::" + k)
    for k in gp1:
        rel_close(gp1[k], p64[k].grad, 1e-4, "grad::" + k)


def test_sequences_beyond_the_documented_limits_are_rejected():
    """include/get_hip.h: gh_tanh_att_* take l * heads <= 8192 (l = 1024 at eight heads is accepted), gh_query_att_*
    l <= 4096; a longer sequence raises with the library's message and leaves the device usable."""
    from get_amd import modules
    torch.manual_seed(3)
    m = modules.MultiHeadSelfAttentionICLR17OnWord(8, 8, 8).to(DEV)
    x = torch.randn(1, 1025, 8, device=DEV)
    with pytest.raises(RuntimeError, match=r"l=1025 with heads=8 exceeds"):
        m(x, x, torch.ones(1, 1025, device=DEV))
    xr = x[:, :1024].clone().requires_grad_(True)
    out = m(xr, xr, torch.ones(1, 1024, device=DEV))
    out.sum().backward()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(xr.grad).all())
    dot = modules.Dot()
    with pytest.raises(RuntimeError, match=r"l=4097 exceeds"):
        dot(torch.randn(1, 8, device=DEV), torch.randn(1, 4097, 8, device=DEV), torch.ones(1, 4097, device=DEV))
    right = torch.randn(2, 4096, 8, device=DEV)
    left = torch.randn(2, 8, device=DEV)
    avg, w = dot(left, right, torch.ones(2, 4096, device=DEV))
    avg64, w64 = _query64(left.double(), right.double(), torch.ones(2, 4096, device=DEV))
    rel_close(avg, avg64, 1e-4, "avg after a rejected call")
    rel_close(w, w64, 1e-4, "weights after a rejected call")

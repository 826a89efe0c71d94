"""GPU checks of the multi-head query/key/value attention family (get_amd.modules ScaledDotProductAttention,
MultiHeadAttentionOriginal, ConcatNotEqualSelfAttTransFormer, MultiHeadAttentionSimple; ops.mha_sdpa / ops.add_layernorm,
csrc/mha_ops.hip) against the reference's captured outputs and gradients (tests/golden/g13_mha.npz), the masking
conventions, operands read in place from a wider tensor, run-to-run determinism, the project's word- and evidence-level
shapes against the float64 restatements of tests/mha_ref.py, the LayerNorm alone, and the documented limits."""
import pytest
import torch

from tests.mha_ref import layernorm64, module64
from tests.util import build_from_contract, golden_ratio, load_golden, rel_close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0") if torch.cuda.is_available() else None

CASES = ["sdpa_3x5", "sdpa_35x70", "sdpa_offset_pos", "sdpa_offset_neg", "mha_orig_h3", "mha_orig_h1", "transformer_concat",
         "mha_simple_h3", "mha_simple_h3_ln"]


def _golden(golden_dir):
    return load_golden(golden_dir, "g13_mha.npz", "mha_contract.json")


def _golden_run(z, meta, contract, name, geom, with_gweights=True):
    """Forward + backward of one golden case; returns (module, inputs by name, out, weights)."""
    key = f"{name}/{geom}::"
    m = build_from_contract(z, key, contract[name]).to(DEV)
    inputs = {a: torch.from_numpy(z[key + a]).to(DEV).requires_grad_(True) for a in dict.fromkeys(meta["args"][name])}
    out, weights = m(*[inputs[a] for a in meta["args"][name]], torch.from_numpy(z[key + "mask"]).to(DEV))
    loss = (out * torch.from_numpy(z[key + "gout"]).to(DEV)).sum()
    if weights is not None and with_gweights:
        loss = loss + (weights * torch.from_numpy(z[key + "gweights"]).to(DEV)).sum()
    loss.backward()
    return m, inputs, out, weights


@pytest.mark.parametrize("name", CASES)
def test_mha_matches_reference_goldens(golden_dir, name):
    """Outputs and weights 1e-4 + 1e-4 |want|, gradients 1e-5 + 1e-4 |want| elementwise (the bounds of
    test_gpu_attention.py against reference fp32 goldens); the two offset cases by largest error over largest entry <= 1e-4."""
    z, meta, contract = _golden(golden_dir)
    assert set(meta["cases"]) == set(CASES)
    offset = name in meta["offset_cases"]
    for geom in meta["cases"][name]:
        key = f"{name}/{geom}::"
        m, inputs, out, weights = _golden_run(z, meta, contract, name, geom)
        assert (weights is None) == (key + "weights" not in z)
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


@pytest.mark.parametrize("name", ["sdpa_3x5", "sdpa_35x70", "mha_orig_h3"])
def test_masking_conventions(golden_dir, name):
    """Masked weights are exactly 0.0, the unmasked ones sum to 1 within 1e-5, a fully masked row gives an exactly zero
    output row and exactly zero dq for that row, no gradient holds a NaN, and a backward without g_weights equals one with
    a zero g_weights."""
    from get_amd import ops
    z, meta, contract = _golden(golden_dir)
    geom = meta["cases"][name][-1]
    key = f"{name}/{geom}::"
    mask = torch.from_numpy(z[key + "mask"]).to(DEV)
    dead = mask.all(-1)
    assert bool(dead.any())
    if name == "mha_orig_h3":      # the kernel's weights behind the module: three heads sharing one mask
        g = torch.Generator().manual_seed(5)
        b, lq, lk = mask.shape
        heads = 3
        q = torch.randn(b, lq, 12, generator=g).to(DEV).requires_grad_(True)
        k = torch.randn(b, lk, 12, generator=g).to(DEV).requires_grad_(True)
        v = torch.randn(b, lk, 15, generator=g).to(DEV).requires_grad_(True)
    else:
        heads = 1
        q, k, v = (torch.from_numpy(z[key + a]).to(DEV).requires_grad_(True) for a in ("query", "key", "value"))
    out, w = ops.mha_sdpa(q, k, v, mask, heads)
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
    wh = w.view(heads, *mask.shape)
    assert bool((wh[:, mask] == 0).all()), "a masked weight is not exactly 0"
    assert float((wh.detach().sum(-1)[:, ~dead] - 1).abs().max()) <= 1e-5
    assert bool((wh[:, dead] == 0).all()) and bool((out[dead] == 0).all())
    grads = torch.autograd.grad((out * gout).sum(), (q, k, v), retain_graph=True)
    assert all(bool(torch.isfinite(t).all()) for t in grads)
    assert bool((grads[0][dead] == 0).all()), "a fully masked row sends a gradient to q"
    grads0 = torch.autograd.grad((out * gout).sum() + (w * torch.zeros_like(w)).sum(), (q, k, v))
    for a, c in zip(grads, grads0):
        assert torch.equal(a, c)


def test_operands_are_read_in_place_from_a_wider_tensor():
    """q / k / v as column slices of a wider tensor (ld > heads * width, the middle slice not 16-byte aligned for v): results
    and gradients equal those on contiguous copies bit for bit."""
    from get_amd import ops
    g = torch.Generator().manual_seed(17)
    b, lq, lk, heads, dk, dv = 3, 21, 37, 2, 8, 5
    wide_q = torch.randn(b, lq, 3 * heads * dk, generator=g).to(DEV)
    wide_kv = torch.randn(b, lk, heads * dk + heads * dv + 3, generator=g).to(DEV)
    mask = (torch.rand(b, lq, lk, generator=g) < 0.3).to(DEV)
    mask[1, 4] = True
    gout = torch.randn(b, lq, heads * dv, generator=g).to(DEV)
    gw = torch.randn(heads * b, lq, lk, generator=g).to(DEV)

    def run(copy):
        q = wide_q[..., heads * dk:2 * heads * dk]
        k = wide_kv[..., 3:3 + heads * dk]
        v = wide_kv[..., 3 + heads * dk:]
        assert not q.is_contiguous() and not k.is_contiguous() and not v.is_contiguous()
        if copy:
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
        out, w = ops.mha_sdpa(q, k, v, mask, heads)
        return (out, w) + torch.autograd.grad((out * gout).sum() + (w * gw).sum(), (q, k, v))

    for a, c in zip(run(False), run(True)):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))


def test_two_runs_are_bit_identical(golden_dir):
    z, meta, contract = _golden(golden_dir)
    runs = []
    for _ in range(2):
        m, inputs, out, _ = _golden_run(z, meta, contract, "mha_orig_h3", "b2q17k70")
        runs.append([out] + [t.grad for t in inputs.values()] + [p.grad for p in m.parameters()])
    for a, c in zip(*runs):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))


SHAPES = {"word_like": dict(b=8, l=100, d_model=300, n_head=5, d=60), "evidence_like": dict(b=4, l=30, d_model=428, n_head=4, d=107)}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_original_at_project_shapes_against_float64(shape):
    """MultiHeadAttentionOriginal forward + backward at a word-level and an evidence-level shape (suffix padding, q distinct
    from k = v) against tests/mha_ref.py in float64: largest error over largest entry <= 1e-5 for the output and <= 1e-4 for
    every gradient.  Both bounds are looser than exact fp32 arithmetic needs; the achieved ratios are printed so that they
    can be tightened from the record.  The gradient of w_ks.bias is identically zero (a bias on the keys shifts every score
    of a query row by the same amount, which the softmax ignores): the column sums of the projected keys' gradient cancel, in
    float64 to 1e-15 of their terms, so its error is taken relative to the largest column sum of |d kp| instead.
    Measured on an MI355X: output 1.6e-7 / 1.9e-7 (word / evidence), gradients at most 8.2e-7 / 6.9e-7."""
    from get_amd import modules
    s = SHAPES[shape]
    b, l, dm = s["b"], s["l"], s["d_model"]
    torch.manual_seed(23)
    m = modules.MultiHeadAttentionOriginal(s["n_head"], dm, s["d"], s["d"])
    g = torch.Generator().manual_seed(29)
    q0, kv0 = torch.randn(b, l, dm, generator=g), torch.randn(b, l, dm, generator=g)
    lens = torch.tensor([l - (7 * i) % (l - 1) for i in range(b)])
    mask = (torch.arange(l)[None, None, :] >= lens[:, None, None]).expand(b, l, l).contiguous()
    gout = torch.randn(b, l, dm, generator=g)
    p64 = {k: v.detach().double().requires_grad_(True) for k, v in m.state_dict().items()}
    q64, kv64 = q0.double().requires_grad_(True), kv0.double().requires_grad_(True)
    keep = {}
    want, _ = module64("MultiHeadAttentionOriginal", dict(n_head=s["n_head"]), p64, [q64, kv64, kv64], mask, keep)
    (want * gout.double()).sum().backward()
    cancelling = keep["kp"].grad.abs().sum((0, 1)).max().item()
    m = m.to(DEV)
    q, kv = q0.to(DEV).requires_grad_(True), kv0.to(DEV).requires_grad_(True)
    out, none = m(q, kv, kv, mask.to(DEV))
    assert none is None
    (out * gout.to(DEV)).sum().backward()
    rel_close(out, want, 1e-5, f"{shape} out")
    rel_close(q.grad, q64.grad, 1e-4, f"{shape} grad q")
    rel_close(kv.grad, kv64.grad, 1e-4, f"{shape} grad k=v")
    for k, p in m.named_parameters():
        rel_close(p.grad, p64[k].grad, 1e-4, f"{shape} grad {k}", floor=cancelling if k == "w_ks.bias" else None,
                  floor_replaces_zero=True)      # asserts that this float64 gradient is numerically zero before using floor


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("d", [5, 8, 300, 1628])
def test_add_layernorm_against_float64(d, with_res):
    """ops.add_layernorm at rows = 7 against float64, largest error over largest entry: <= 1e-5 for y (some 170 fp32
    roundings of an O(1) normalised value: the mean and the variance are sums of d <= 1628 terms, each carrying at most a few
    roundings that largely average out) and <= 1e-4 for the gradients, as for the attention at project shapes.  dgamma and
    dbeta are ACCUMULATED by the kernel: a second call on the same buffers doubles them exactly."""
    from get_amd import _lib, ops
    rows = 7
    g = torch.Generator().manual_seed(31 + d)
    x0, r0 = torch.randn(rows, d, generator=g), torch.randn(rows, d, generator=g) if with_res else None
    w0, b0, gy = 1 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g), torch.randn(rows, d, generator=g)
    leaves64 = [t.double().requires_grad_(True) for t in (x0, w0, b0)]
    r64 = r0.double().requires_grad_(True) if with_res else None
    want = layernorm64(leaves64[0] + r64 if with_res else leaves64[0], leaves64[1], leaves64[2])
    (want * gy.double()).sum().backward()
    x, w, bb = (t.to(DEV).requires_grad_(True) for t in (x0, w0, b0))
    r = r0.to(DEV).requires_grad_(True) if with_res else None
    y = ops.add_layernorm(x, r, w, bb, 1e-5)
    (y * gy.to(DEV)).sum().backward()
    what = f"layernorm d={d} res={with_res}"
    rel_close(y, want, 1e-5, what + " y")
    rel_close(x.grad, leaves64[0].grad, 1e-4, what + " dx")
    rel_close(w.grad, leaves64[1].grad, 1e-4, what + " dgamma")
    rel_close(bb.grad, leaves64[2].grad, 1e-4, what + " dbeta")
    if with_res:
        assert torch.equal(r.grad, x.grad)
    # the kernel itself accumulates
    xs, gs = x.detach(), gy.to(DEV)
    mean, rstd = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    yy, dx = torch.empty_like(xs), torch.empty_like(xs)
    P = lambda t: None if t is None else t.data_ptr()
    rr = r.detach() if with_res else None
    _lib.call("gh_add_layernorm_fwd", P(xs), P(rr), P(w.detach()), P(bb.detach()), 1e-5, rows, d, P(yy), P(mean), P(rstd), _lib.stream())
    assert torch.equal(yy, y.detach())
    _lib.ensure_workspace(DEV)
    dg, db = torch.zeros(d, device=DEV), torch.zeros(d, device=DEV)
    for _ in range(2):
        _lib.call("gh_add_layernorm_bwd", P(xs), P(rr), P(w.detach()), P(mean), P(rstd), P(gs), rows, d, P(dx), P(dg), P(db),
                  _lib.stream())
    assert torch.equal(dx, x.grad) and torch.equal(dg, 2 * w.grad) and torch.equal(db, 2 * bb.grad)


LIMITS = {"heads": dict(heads=17), "lq": dict(lq=1025), "lk": dict(lk=1025), "dk": dict(dk=513), "dv": dict(dv=513)}


@pytest.mark.parametrize("which", list(LIMITS))
def test_sizes_beyond_the_limits_are_rejected(which):
    """One call just outside each documented limit (heads <= 16, lq <= 1024, lk <= 1024, dk <= 512, dv <= 512): RuntimeError
    that names the limit, before anything is launched -- the output buffers keep their contents."""
    from get_amd import _lib, ops
    s = dict(b=1, heads=1, lq=4, lk=4, dk=4, dv=4)
    s.update(LIMITS[which])
    b, heads, lq, lk, dk, dv = (s[k] for k in ("b", "heads", "lq", "lk", "dk", "dv"))
    q = torch.zeros(b, lq, heads * dk, device=DEV)
    k = torch.zeros(b, lk, heads * dk, device=DEV)
    v = torch.zeros(b, lk, heads * dv, device=DEV)
    mask = torch.zeros(b, lq, lk, dtype=torch.bool, device=DEV)
    with pytest.raises(RuntimeError, match=which):
        ops.mha_sdpa(q, k, v, mask, heads)
    weights = torch.full((heads * b, lq, lk), 7.0, device=DEV)
    out = torch.full((b, lq, heads * dv), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match=which):
        _lib.call("gh_mha_sdpa_fwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), heads * dk, heads * dk, heads * dv,
                  mask.view(torch.uint8).data_ptr(), b, heads, lq, lk, dk, dv, weights.data_ptr(), out.data_ptr(), heads * dv,
                  _lib.stream())
    dq, dkk, dvv, ds = torch.full_like(q, 7.0), torch.full_like(k, 7.0), torch.full_like(v, 7.0), torch.full_like(weights, 7.0)
    with pytest.raises(RuntimeError, match=which):
        _lib.call("gh_mha_sdpa_bwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), heads * dk, heads * dk, heads * dv,
                  weights.data_ptr(), out.data_ptr(), heads * dv, None, b, heads, lq, lk, dk, dv, ds.data_ptr(), dq.data_ptr(),
                  heads * dk, dkk.data_ptr(), heads * dk, dvv.data_ptr(), heads * dv, _lib.stream())
    torch.cuda.synchronize()
    for t in (weights, out, dq, dkk, dvv, ds):
        assert bool((t == 7.0).all())


def test_layernorm_beyond_its_width_limit_is_rejected():
    from get_amd import ops
    x = torch.full((2, 2049), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match="2048"):
        ops.add_layernorm(x, None, torch.ones(2049, device=DEV), torch.zeros(2049, device=DEV), 1e-5)
    y = ops.add_layernorm(x[:, :2048].contiguous() + torch.arange(2048, device=DEV), None, torch.ones(2048, device=DEV),
                          torch.zeros(2048, device=DEV), 1e-5)
    assert bool(torch.isfinite(y).all()) and float(y.mean().abs()) < 1e-4


def test_sizes_at_the_limits_run():
    """The largest documented attention problem in every dimension at once (heads aside): lq = lk = 1024, dk = dv = 512 --
    the LDS plans of all three kernels at their maxima -- against float64 on one head."""
    from get_amd import ops
    from tests.mha_ref import sdpa64
    g = torch.Generator().manual_seed(41)
    q0 = 0.05 * torch.randn(1, 1024, 512, generator=g)
    k0 = torch.randn(1, 1024, 512, generator=g)
    v0 = torch.randn(1, 1024, 512, generator=g)
    mask = torch.zeros(1, 1024, 1024, dtype=torch.bool)
    mask[0, :, 1000:] = True
    mask[0, 1023] = True
    gout = torch.randn(1, 1024, 512, generator=g)
    l64 = [t.double().requires_grad_(True) for t in (q0, k0, v0)]
    want, w64 = sdpa64(*l64, mask, 1)
    (want * gout.double()).sum().backward()
    q, k, v = (t.to(DEV).requires_grad_(True) for t in (q0, k0, v0))
    out, w = ops.mha_sdpa(q, k, v, mask.to(DEV), 1)
    (out * gout.to(DEV)).sum().backward()
    rel_close(out, want, 1e-5, "limits out")
    rel_close(w, w64, 1e-5, "limits weights")
    for a, c, n in zip((q, k, v), l64, "qkv"):
        rel_close(a.grad, c.grad, 1e-4, "limits grad " + n)

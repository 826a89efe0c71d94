"""GPU checks of the graph encoders GraphAttentionLayer / GAT / GCN (get_amd.modules, csrc/encoder_ops.hip) against the
reference's captured outputs and gradients (tests/golden/g10_gat.npz, g11_gcn.npz), dense vs packed adjacency,
replayed training-mode dropout through a float64 restatement, and the bench-scale graphs (960 x 100 nodes, width 300)."""
import numpy as np
import pytest
import torch

from tests.util import _gat64, _gat_head64, _gcn64, bits_equal, build_from_contract, golden_ratio, load_golden, rel_close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0") if torch.cuda.is_available() else None


def _load(golden_dir, name):
    return load_golden(golden_dir, name, "encoder_contract.json")


def _cases(z, meta, kinds):
    for name in kinds:
        for kind in meta["adj_kinds"]:
            yield name, kind, f"{name}/{kind}::"


def _build(z, key, contract):
    return build_from_contract(z, key, contract[key.split("/")[0]]).to(DEV).train(False)


def _run_golden(golden_dir, npz, kinds_key):
    z, meta, contract = _load(golden_dir, npz)
    n_cases = 0
    for name, kind, key in _cases(z, meta, meta[kinds_key]):
        m = _build(z, key, contract)
        x = torch.from_numpy(z[key + "x"]).to(DEV).requires_grad_(True)
        adj = torch.from_numpy(z[key + "adj"]).to(DEV)
        out = m(x, adj)
        golden_ratio(out, z[key + "out"], 1e-4, 1e-4, key + "out")
        (out * torch.from_numpy(z[key + "gout"]).to(DEV)).sum().backward()
        golden_ratio(x.grad, z[key + "grad::x"], 1e-5, 1e-4, key + "grad::x")
        for k, p in m.named_parameters():
            golden_ratio(p.grad, z[key + "grad::" + k], 1e-5, 1e-4, key + "grad::" + k)
        n_cases += 1
    return n_cases


def test_gat_matches_reference_goldens(golden_dir):
    """GraphAttentionLayer (concat True / False) and GAT (heads 1, 3; num_layers 1, 2) on convert_text graphs with
    padding nodes (uniform attention rows, the /L output) and on a mixed-sign asymmetric adjacency with isolated rows."""
    assert _run_golden(golden_dir, "g10_gat.npz", "gat_cases") == 12


def test_gcn_matches_reference_goldens(golden_dir):
    """GCN (num_layers 1, 2) on convert_text's normalised adjacency and on an asymmetric weighted one with zero rows."""
    assert _run_golden(golden_dir, "g11_gcn.npz", "gcn_cases") == 4


def _fwd_bwd(m, x, adj, gout):
    x = x.clone().requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    out = m(x, adj)
    (out * gout).sum().backward()
    return out.detach().clone(), x.grad.clone(), [p.grad.clone() for p in m.parameters()]


def _same(a, b):
    """Two (out, grad x, [parameter grads]) of _fwd_bwd: the same bits, none of them NaN."""
    for i, (u, v) in enumerate(zip([a[0], a[1], *a[2]], [b[0], b[1], *b[2]])):
        assert not bool(torch.isnan(u).any()), i
        bits_equal(u, v, f"tensor {i} of two runs")


def test_dense_and_packed_adjacency_are_bit_identical(golden_dir):
    from get_amd import ops
    z, meta, contract = _load(golden_dir, "g10_gat.npz")
    for name in meta["gat_cases"]:
        key = f"{name}/text::"
        m = _build(z, key, contract)
        x = torch.from_numpy(z[key + "x"]).to(DEV)
        dense = torch.from_numpy(z[key + "adj"]).to(DEV)
        tokens = torch.from_numpy(z[key + "tokens"]).to(DEV)
        lengths = torch.from_numpy(z[key + "lengths"]).to(DEV)
        packed, _, _ = ops.graph_build(tokens, lengths, meta["window"])
        probe = m(x, dense)
        gout = torch.randn(probe.shape, generator=torch.Generator().manual_seed(3)).to(DEV)
        _same(_fwd_bwd(m, x, dense, gout), _fwd_bwd(m, x, packed, gout))
        key = f"{name}/weighted::"
        m = _build(z, key, contract)
        x = torch.from_numpy(z[key + "x"]).to(DEV)
        dense = torch.from_numpy(z[key + "adj"]).to(DEV)
        _same(_fwd_bwd(m, x, dense, gout), _fwd_bwd(m, x, ops.PackedAdj.from_dense(dense), gout))
    # GCN: a dense tensor and its PackedAdj are the same operator; the native graph_build pattern (normalised mode)
    # gives the reference's result too
    z, meta, contract = _load(golden_dir, "g11_gcn.npz")
    for name in meta["gcn_cases"]:
        key = f"{name}/text::"
        m = _build(z, key, contract)
        x = torch.from_numpy(z[key + "x"]).to(DEV)
        dense = torch.from_numpy(z[key + "adj"]).to(DEV)
        gout = torch.from_numpy(z[key + "gout"]).to(DEV)
        _same(_fwd_bwd(m, x, dense, gout), _fwd_bwd(m, x, ops.PackedAdj.from_dense(dense), gout))
        packed, _, _ = ops.graph_build(torch.from_numpy(z[key + "tokens"]).to(DEV),
                                       torch.from_numpy(z[key + "lengths"]).to(DEV), meta["window"])
        out, gx, gp = _fwd_bwd(m, x, packed, gout)
        golden_ratio(out, z[key + "out"], 1e-4, 1e-4, key + "packed out")
        golden_ratio(gx, z[key + "grad::x"], 1e-5, 1e-4, key + "packed grad::x")


def _params64(m):
    return {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.named_parameters()}


def _check_grads(m, x_dev, gout, out_dev, x64, p64, out64, tol_out=1e-4, tol_g=1e-4):
    (out_dev * gout).sum().backward()
    (out64 * gout.double().cpu()).sum().backward()
    golden_ratio(out_dev, out64.detach(), tol_out, tol_out, "out")
    golden_ratio(x_dev.grad, x64.grad, tol_g, tol_g, "grad::x")
    for k, p in m.named_parameters():
        golden_ratio(p.grad, p64[k].grad, tol_g, tol_g, "grad::" + k)


def test_training_mode_dropout_replays(golden_dir):
    """Training mode: the input / mid dropout masks (ops.feat_dropout) and the attention dropout masks
    (ops.gat_dropout_mask), replayed into a float64 restatement, give the module's output and gradients."""
    from get_amd import modules, ops
    torch.manual_seed(5)
    B, L, din, hid, out_dim, heads, p = 4, 20, 12, 8, 6, 3, 0.3
    g = torch.Generator().manual_seed(9)
    x = torch.randn((B, L, din), generator=g)
    lengths = torch.tensor([20, 13, 6, 1])
    tokens = torch.randint(1, 12, (B, L), generator=g)
    tokens[torch.arange(L)[None, :] >= lengths[:, None]] = 0
    packed, _, _ = ops.graph_build(tokens.to(DEV), lengths.to(DEV), 3)
    adj = packed.to_dense()
    gat = modules.GAT(din, hid, out_dim, head_num=heads, num_layers=2, dropout=p, alpha=0.2).to(DEV).train(True)
    xd = x.to(DEV).requires_grad_(True)
    y = gat(xd, adj)
    s_in, s_att0, s_mid, s_att1 = gat.last_seeds
    n = B
    masks = {"in": torch.from_numpy(ops.dropout_mask_reference(s_in, B * L, din, p)).double().view(B, L, din),
             "mid": torch.from_numpy(ops.dropout_mask_reference(s_mid, B * L, hid * heads, p)).double().view(B, L, -1),
             "att": [torch.from_numpy(ops.gat_dropout_mask(s_att0, 0, heads, n, L, p)).double(),
                     torch.from_numpy(ops.gat_dropout_mask(s_att1, 1, heads, n, L, p)).double()]}
    p64 = _params64(gat)
    x64 = x.double().requires_grad_(True)
    y64 = _gat64(p64, x64, adj.double().cpu(), heads, 2, 0.2, masks, p)
    gout = torch.randn(y.shape, generator=g).to(DEV)
    _check_grads(gat, xd, gout, y, x64, p64, y64)
    # a lone layer with concat=False in training mode (its own attention dropout, layer key 0)
    lay = modules.GraphAttentionLayer(din, hid, dropout=p, alpha=0.1, concat=False).to(DEV).train(True)
    xd = x.to(DEV).requires_grad_(True)
    y = lay(xd, adj)
    m0 = torch.from_numpy(ops.gat_dropout_mask(lay.last_seed, 0, 1, n, L, p)).double()[0]
    p64 = _params64(lay)
    x64 = x.double().requires_grad_(True)
    y64 = _gat_head64(x64, adj.double().cpu(), p64["W"], p64["a"], 0.1, m0, p, "plain")
    gout = torch.randn(y.shape, generator=g).to(DEV)
    _check_grads(lay, xd, gout, y, x64, p64, y64)
    # GCN: the input dropout
    gcn = modules.GCN(din, hid, hid, num_layers=2, dropout=p).to(DEV).train(True)
    xd = x.to(DEV).requires_grad_(True)
    y = gcn(xd, packed)
    mask = torch.from_numpy(ops.dropout_mask_reference(gcn.last_seed, B * L, din, p)).double().view(B, L, din)
    p64 = _params64(gcn)
    x64 = x.double().requires_grad_(True)
    y64 = _gcn64(p64, x64, adj.double().cpu(), 2, mask, p)
    gout = torch.randn(y.shape, generator=g).to(DEV)
    _check_grads(gcn, xd, gout, y, x64, p64, y64)


# ----------------------------------------------------------------------------- bench scale
def _bench_graphs():
    from get_amd import ops
    from get_amd.synth import make_tokens
    rng = np.random.default_rng(2024)
    toks, lens = make_tokens(rng, 960, 100, 20000, 20, 100)
    packed, _, n_nodes = ops.graph_build(torch.from_numpy(toks).to(DEV), torch.from_numpy(lens).to(DEV), 5)
    return packed


def test_bench_scale_gat_and_gcn():
    """960 graphs x 100 nodes of gh_graph_build on synth tokens, width 300: GAT (3 heads, a hidden layer) and GCN
    forward + backward against float64 restatements; two runs bit-identical (no global atomics); no dense buffer.
    Among the 28.8 M outputs of a ReLU a few lie within fp32 rounding of 0, where fp32 and float64 can take different
    sides of the kink (one such flip moves an input gradient by |g| / L): the restatements take the ReLU decisions of
    the device run, everything else is recomputed in float64."""
    from get_amd import modules
    torch.manual_seed(11)
    packed = _bench_graphs()
    B, L, D, heads = 960, 100, 300, 3
    adj64 = packed.to_dense().double().cpu()
    x = torch.randn((B, L, D), generator=torch.Generator().manual_seed(1)) * 0.5
    gat = modules.GAT(D, D, D, head_num=heads, num_layers=2).to(DEV).train(False)
    gcn = modules.GCN(D, D, D, num_layers=2).to(DEV).train(False)
    relu_in = []
    for lin in gcn.Linear:
        lin.register_forward_hook(lambda mod, inp, out: relu_in.append((out.detach() > 0).double().cpu()))
    for m in (gat, gcn):
        gout = torch.randn((B, L, D), generator=torch.Generator().manual_seed(2)).to(DEV)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        r1 = _fwd_bwd(m, x.to(DEV), packed, gout)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        masks = list(relu_in)
        r2 = _fwd_bwd(m, x.to(DEV), packed, gout)
        _same(r1, r2)
        # the reference's dense normalisation alone needs (B*L)^2 floats (36.9 GB); the feature-sized tensors of the
        # two layers (up to 900 columns) and their gradients take ~3 GB
        assert peak < (B * L) ** 2 * 4 / 8, peak
        out, gx, gp = r1
        p64 = _params64(m)
        x64 = x.double().requires_grad_(True)
        if m is gat:
            y64 = _gat64(p64, x64, adj64, heads, 2, 0.2, relu_mask=(out > 0).double().cpu())
        else:
            y64 = _gcn64(p64, x64, adj64, 2, relu_masks=masks[:2])
        (y64 * gout.double().cpu()).sum().backward()
        rel_close(out, y64, 1e-4, "out")
        rel_close(gx, x64.grad, 1e-4, "grad::x")
        for (k, _), g in zip(m.named_parameters(), gp):
            rel_close(g, p64[k].grad, 1e-4, "grad::" + k)


def test_gat_memory_holds_no_attention_matrix():
    """Attention over bit rows: at the bench graph count a narrow GAT (3 heads, a hidden layer) needs a fraction of what
    the reference's attention matrices alone take (one (B, L, L) fp32 buffer per head and layer, and it keeps several
    per head): its memory follows B*L*width, never B*L*L."""
    from get_amd import _lib, modules
    packed = _bench_graphs()
    B, L, D, heads = 960, 100, 4, 3
    gat = modules.GAT(D, D, D, head_num=heads, num_layers=2).to(DEV).train(False)
    x = torch.randn((B, L, D), device=DEV)
    gout = torch.randn((B, L, D), device=DEV)
    _lib.ensure_workspace(DEV)            # the split-K scratch of the weight gradients is allocated once per stream
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    _fwd_bwd(gat, x, packed, gout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    attention = 2 * heads * B * L * L * 4
    assert peak < attention / 4, (peak, attention)


def test_encoders_reject_oversized_graphs():
    from get_amd import modules
    adj = torch.zeros((1, 300, 300), device=DEV)
    adj[0, 0, 1] = 1.0
    x = torch.randn((1, 300, 4), device=DEV)
    with pytest.raises(RuntimeError, match="r=300"):
        modules.GAT(4, 4, 4, head_num=1).to(DEV)(x, adj)
    with pytest.raises(RuntimeError, match="r=300"):
        modules.GCN(4, 4, 4).to(DEV)(x, adj)


@pytest.mark.parametrize("h", [4, 8])
def test_spmm_rows_of_one_and_two_float4_columns(h):
    """GCN layers of width 4 or 8 aggregate rows of one or two float4 columns: one column group per row in the edge-list
    kernel (its magic-number division by 1)."""
    from get_amd import ops
    rng = np.random.default_rng(h)
    for r, n in ((12, 3), (100, 40)):
        a = rng.standard_normal((n, r, r)) * (rng.random((n, r, r)) < 0.3)
        A = torch.from_numpy(a).float().to(DEV)
        x = torch.from_numpy(rng.standard_normal((n, r, h)).astype(np.float32)).to(DEV).requires_grad_(True)
        y = ops.spmm(ops.PackedAdj.from_dense(A), x)
        ref = A @ x.detach()
        assert (y.detach() - ref).abs().max().item() <= 2e-6 * max(1.0, ref.abs().max().item())
        g = torch.randn_like(y)
        (y * g).sum().backward()
        refg = A.transpose(1, 2) @ g
        assert (x.grad - refg).abs().max().item() <= 2e-6 * max(1.0, refg.abs().max().item())

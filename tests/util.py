"""Shared helpers for the parity tests (fixtures, gradient summaries, tolerances)."""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def load(name):
    z = np.load(os.path.join(GOLDEN, name))
    meta = json.loads(bytes(z["meta"]).decode())
    return z, meta


def summary(g):
    """Same summary oracle/make_golden.py stores for large gradients."""
    g = np.asarray(g, dtype=np.float64)
    flat = g.reshape(g.shape[0], -1) if g.ndim > 1 else g.reshape(1, -1)
    return dict(head=flat[:4, :64], sum=g.sum(), abssum=np.abs(g).sum(), sqsum=(g * g).sum())


def check_grad(z, key, got, rtol=1e-3, atol=1e-5, what=""):
    """Compare ``got`` with the fixture entry ``key`` (full tensor or summary form)."""
    got = np.asarray(got, dtype=np.float64)
    if key in z.files:
        exp = z[key].astype(np.float64)
        scale = max(np.abs(exp).max(), 1e-6)
        err = np.abs(got.reshape(exp.shape) - exp).max()
        assert err <= atol + rtol * scale, f"{what}{key}: max err {err:.3e} vs scale {scale:.3e}"
        return
    s = summary(got)
    exp_head = z[key + "::head"]
    scale = max(np.sqrt(float(z[key + "::sqsum"]) / max(got.size, 1)), 1e-6)   # rms of the reference gradient
    err = np.abs(s["head"] - exp_head).max()
    assert err <= atol + rtol * max(scale, np.abs(exp_head).max()), f"{what}{key} head: {err:.3e} (rms {scale:.3e})"
    for k in ("abssum", "sqsum"):
        e = float(z[f"{key}::{k}"])
        assert abs(s[k] - e) <= 2e-3 * abs(e) + atol, f"{what}{key} {k}: {s[k]} vs {e}"
    e = float(z[key + "::sum"])
    assert abs(s["sum"] - e) <= 1e-3 * float(z[key + "::abssum"]) + atol, f"{what}{key} sum: {s['sum']} vs {e}"


def dense_from_coo(z, idx, fixed_length):
    a = np.zeros((fixed_length, fixed_length), np.float64)
    a[z[f"c{idx}_rows"].astype(int), z[f"c{idx}_cols"].astype(int)] = z[f"c{idx}_vals"]
    return a


def golden_ratio(got, want, atol, rtol, what):
    """Assert |got - want| <= atol + rtol |want| elementwise (the golden tests' bound); returns the worst ratio of it."""
    got = torch.as_tensor(np.asarray(got.detach().cpu() if torch.is_tensor(got) else got)).double()
    want = torch.as_tensor(np.asarray(want)).double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs()
    tol = atol + rtol * want.abs()
    worst = (err / tol).max().item()
    assert bool(torch.isfinite(got).all()) and bool((err <= tol).all()), \
        f"{what}: max err {err.max().item():.3e} ({worst:.2f} x bound)"
    return worst


# ----------------------------------------------------------------------------- path-by-path parity (tests/test_gpu_*_paths.py)
TOL = 1e-4                       # of the largest entry of the float64 result (the project's bound for restatements)
WORST = {}                       # family -> worst observed err / scale, printed with every case


def _rel(got, want, what, fam, floor=None):
    """Finite and max error <= TOL of the float64 result's largest entry; prints and records the ratio.  `floor`: where
    the float64 result is identically 0 because its terms cancel (the softmax over a single element has a zero
    Jacobian), the size of the cancelling terms, which is what a rounding error is relative to."""
    got = got.detach().double().cpu()
    want = want.detach().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements not written / not finite"
    scale = want.abs().max().item() + 1e-12
    if floor is not None and scale <= 1e-12:      # only ever in place of a result that is identically 0
        scale = float(floor)
    err = (got - want).abs().max().item()
    WORST[fam] = max(WORST.get(fam, 0.0), err / scale)
    print(f"{what}: max err {err:.3e} over scale {scale:.3e} = {err / scale:.3e} (worst {fam}: {WORST[fam]:.3e})")
    assert err <= TOL * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _same(a, b, what):
    for i, (u, v) in enumerate(zip(a, b)):
        if u is not None:
            assert torch.equal(u.view(torch.int32), v.view(torch.int32)), f"{what}: output {i} differs between two calls"


# ----------------------------------------------------------------------------- float64 restatements (tests only)
# Plain torch statements of the attention and encoder operations, evaluated in float64 by the GPU parity tests and
# checked on their own against the reference's goldens by tests/test_attention_cpu.py and tests/test_encoders_cpu.py.
def _query64(q, right, mask):
    s = (right @ q.unsqueeze(-1)).squeeze(-1).masked_fill(mask == 0, float("-inf"))
    w = torch.softmax(s, dim=1)
    return (right * w.unsqueeze(-1)).sum(1), w


def _tanh64(pre, u, w2, mask, values):
    t = torch.tanh(pre if u is None else pre + u.unsqueeze(1))
    e = (t @ w2.t()).masked_fill((mask == 0).unsqueeze(-1), float("-inf"))
    w = torch.softmax(e, dim=1)
    return w.transpose(1, 2) @ values, w


def _module64(cls, p, inputs, mask):
    """The five classes in float64 on plain torch ops; p: parameters by name, inputs in forward order."""
    if cls == "Dot":
        return _query64(inputs[0], inputs[1], mask)
    if cls == "BiLinear":
        return _query64(inputs[0] @ p["W.weight"].t() + p["W.bias"], inputs[1], mask)
    if cls == "BiLinearTanh":
        pre = inputs[0] @ p["left_linear.weight"].t() + p["left_linear.bias"]
        att, w = _tanh64(pre, inputs[1] @ p["right_linear.weight"].t(), p["combine.weight"], mask, inputs[0])
        return att[:, 0], w[:, :, 0]
    if cls == "SelfAttentionICLR2017":
        att, _ = _tanh64(inputs[0] @ p["linear1.weight"].t(), None, p["linear2.weight"], mask, inputs[0])
        return att[:, 0], None
    return _tanh64(inputs[1] @ p["linear1.weight"].t(), None, p["linear2.weight"], mask, inputs[0])


def _gat_head64(x, adj, W, a, alpha, att_mask, p, mode):
    """One head of wrapper.py:27-53 in float64; att_mask (B,L,L) bool of kept attention entries or None."""
    h = x @ W
    f = W.shape[1]
    e = F.leaky_relu(h @ a[:f] + (h @ a[f:]).transpose(1, 2), alpha)
    att = torch.softmax(torch.where(adj > 0, e, torch.full_like(e, -9e15)), dim=2)
    if att_mask is not None:
        att = att * att_mask / (1.0 - p)
    hp = att @ h
    return F.elu(hp) if mode == "elu" else hp


def _gat64(params, x, adj, heads, layers, alpha, masks=None, p=0.0, relu_mask=None):
    """GAT.forward (wrapper.py:99-110) in float64; masks: replayed (input, [per layer (H,B,L,L)], pre-output, output);
    relu_mask: the final ReLU's decisions taken from the device run (see test_bench_scale_gat_and_gcn)."""
    L = x.shape[1]
    if masks is not None:
        x = x * masks["in"] / (1.0 - p)
    for li in range(layers - 1):
        att = masks["att"][li] if masks is not None else None
        x = torch.cat([_gat_head64(x, adj, params[f"layer_{li}_{j}.W"], params[f"layer_{li}_{j}.a"], alpha,
                                   att[j] if att is not None else None, p, "elu") for j in range(heads)], dim=2)
    if masks is not None:
        x = x * masks["mid"] / (1.0 - p)
    att = masks["att"][layers - 1] if masks is not None else None
    y = sum([_gat_head64(x, adj, params[f"out_att.{j}.W"], params[f"out_att.{j}.a"], alpha,
                         att[j] if att is not None else None, p, "plain") for j in range(heads)]) / L
    return F.relu(y) if relu_mask is None else y * relu_mask


def _gcn64(params, x, adj, layers, in_mask=None, p=0.0, relu_masks=None):
    if in_mask is not None:
        x = x * in_mask / (1.0 - p)
    d = adj.sum(-1).pow(-0.5)
    d[torch.isinf(d)] = 0.0
    a_hat = d[:, :, None] * adj * d[:, None, :]
    for k in range(layers):
        x = (a_hat @ x) @ params[f"Linear.{k}.linear.weight"].t() + params[f"Linear.{k}.linear.bias"]
        x = F.relu(x) if relu_masks is None else x * relu_masks[k]
    return x

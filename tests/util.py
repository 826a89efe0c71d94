"""Shared helpers for the parity tests (fixtures, gradient summaries, tolerances)."""
import json
import os
import subprocess
import sys

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


# ----------------------------------------------------------------------------- comparisons (every parity and golden test)
TOL = 1e-4                       # of the largest entry of the float64 result (the project's bound for restatements)
WORST = {}                       # family -> worst observed err / scale, printed with every case


def _f64(t):
    """A tensor on any device, or anything numpy can read, as a float64 CPU tensor."""
    return t.detach().double().cpu() if torch.is_tensor(t) else torch.as_tensor(np.asarray(t)).double()


def golden_ratio(got, want, atol, rtol, what):
    """Equal shapes, `got` finite and |got - want| <= atol + rtol |want| elementwise (the golden tests' bound); prints and
    returns the worst fraction of that bound."""
    got, want = _f64(got), _f64(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements not written / not finite"
    err = (got - want).abs()
    tol = atol + rtol * want.abs()
    worst = (err / tol).max().item()
    print(f"{what}: max err {err.max().item():.3e}, {worst:.3f} of the bound")
    assert bool((err <= tol).all()), f"{what}: max err {err.max().item():.3e} ({worst:.2f} x bound)"
    return worst


def rel_close(got, want, tol, what, floor=None, fam=None, floor_replaces_zero=False):
    """Equal shapes, `got` finite and max |got - want| <= tol * scale, scale = max |want| + 1e-12; prints the ratio and, with
    `fam`, records it in WORST[fam].  `floor`: where the float64 result is identically 0 because its terms cancel (the
    softmax over a single element has a zero Jacobian), the size of the cancelling terms, which is what a rounding error is
    relative to.  It replaces the scale only where the scale is <= 1e-12, and is ignored otherwise; a caller that knows the
    result to be a cancellation passes floor_replaces_zero=True, which ASSERTS scale <= 1e-9 floor and then uses floor."""
    got, want = _f64(got), _f64(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} elements not written / not finite"
    scale = want.abs().max().item() + 1e-12
    if floor is not None and floor_replaces_zero:
        assert scale <= 1e-9 * float(floor), (what, scale, floor)
        scale = float(floor)
    elif floor is not None and scale <= 1e-12:
        scale = float(floor)
    err = (got - want).abs().max().item()
    note = ""
    if fam is not None:
        WORST[fam] = max(WORST.get(fam, 0.0), err / scale)
        note = f" (worst {fam}: {WORST[fam]:.3e})"
    print(f"{what}: max err {err:.3e} over scale {scale:.3e} = {err / scale:.3e}, {err / scale / tol:.3f} of the bound {tol:.0e}{note}")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"
    return err / scale


def _rel(got, want, what, fam, floor=None):
    """rel_close at the path tests' bound TOL, recorded under `fam` (tests/test_gpu_*_paths.py)."""
    rel_close(got, want, TOL, what, floor=floor, fam=fam)


def bits_equal(a, b, what):
    """Same shape and the same 32-bit patterns: tells +0.0 from -0.0 and accepts equal NaN patterns."""
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), what + " differs"


def _same(a, b, what):
    for i, (u, v) in enumerate(zip(a, b)):
        if u is not None:
            bits_equal(u, v, f"{what}: output {i} of two calls")


# ----------------------------------------------------------------------------- golden fixtures
_LOADED = {}


def load_golden(golden_dir, npz_name, contract_name=None):
    """(archive as a dict of arrays, its decoded meta or None, the contract or None), read once per file and shared by every
    test that asks again: nobody writes into what this returns."""
    key = (golden_dir, npz_name, contract_name)
    if key not in _LOADED:
        with np.load(os.path.join(golden_dir, npz_name)) as f:
            z = {k: f[k] for k in f.files}
        meta = json.loads(bytes(z["meta"]).decode()) if "meta" in z else None
        contract = None
        if contract_name is not None:
            with open(os.path.join(golden_dir, contract_name)) as fh:
                contract = json.load(fh)
        _LOADED[key] = (z, meta, contract)
    return _LOADED[key]


def build_from_contract(z, key_prefix, contract_entry, module_cls=None):
    """The get_amd.modules class of a contract entry ("class", or `module_cls` where the contract names none) built from its
    "kwargs", with every key_prefix + "param::*" array of the archive loaded into it (strict)."""
    from get_amd import modules
    m = (module_cls or getattr(modules, contract_entry["class"]))(**contract_entry["kwargs"])
    pre = key_prefix + "param::"
    m.load_state_dict({k[len(pre):]: torch.from_numpy(z[k]) for k in z if k.startswith(pre)}, strict=True)
    return m


def run_in_fresh_interpreter(tmp_path, body, packages=("thirdparty",)):
    """get_amd.install() in a new interpreter that finds empty `packages` under tmp_path, followed by `body` (the imports
    from the reference's module paths and the assertions on what they give)."""
    for pkg in packages:
        os.makedirs(os.path.join(tmp_path, pkg), exist_ok=True)
        open(os.path.join(tmp_path, pkg, "__init__.py"), "w").close()
    code = "import sys\nsys.path.insert(0, %r)\nsys.path.insert(0, %r)\nimport get_amd\nM = get_amd.install()\n%s\nprint('ok')\n" % (
        ROOT, str(tmp_path), body)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


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


# ----------------------------------------------------------------------------- graph restatements (numpy / float64, tests only)
# Plain statements of what csrc/graph_ops.hip computes, used as the references of tests/test_gpu_graph_paths.py and
# checked on their own, without any kernel, against the reference's goldens by tests/test_graph_restatements_cpu.py.
def g_words(r):
    return (r + 63) // 64


def g_pack_bits(mask):
    """bool (..., R) -> int64 (..., W) bit words, bit j & 63 of word j >> 6 = mask[..., j]; bits >= R are zero."""
    mask = np.asarray(mask, dtype=bool)
    r = mask.shape[-1]
    out = np.zeros(mask.shape[:-1] + (g_words(r),), dtype=np.uint64)
    for j in range(r):
        out[..., j >> 6] |= mask[..., j].astype(np.uint64) << np.uint64(j & 63)
    return out.view(np.int64)


def g_unpack_bits(words, r):
    """int64 / uint64 (..., W) -> bool (..., R); also returns whether any bit >= R is set."""
    w = np.ascontiguousarray(words).view(np.uint64)
    out = np.zeros(w.shape[:-1] + (r,), dtype=bool)
    for j in range(r):
        out[..., j] = ((w[..., j >> 6] >> np.uint64(j & 63)) & np.uint64(1)).astype(bool)
    spare = np.zeros(w.shape[:-1], dtype=bool)
    for j in range(r, 64 * w.shape[-1]):
        spare |= ((w[..., j >> 6] >> np.uint64(j & 63)) & np.uint64(1)).astype(bool)
    return out, bool(spare.any())


def g_dinv(pattern):
    """float32(1 / sqrt(float64(row degree))) of a bool pattern (..., R, R), 0 for rows without an edge."""
    deg = np.asarray(pattern, dtype=bool).sum(-1).astype(np.float64)
    with np.errstate(divide="ignore"):
        return np.where(deg > 0, 1.0 / np.sqrt(deg), 0.0).astype(np.float32)


def g_text_graphs(tokens, lengths, r, window, convert_text):
    """Word graphs of a batch of texts from the oracle's convert_text (lengths clamped into [0, r] as gh_graph_build does):
    node_ids int32 (n, r), n_nodes int32 (n,), pattern bool (n, r, r), dinv float32 (n, r), adj float64 (n, r, r)."""
    n = len(tokens)
    ids, nn = np.zeros((n, r), np.int32), np.zeros((n,), np.int32)
    adj = np.zeros((n, r, r), np.float64)
    for g in range(n):
        ln = min(max(int(lengths[g]), 0), r)
        i_, a_, k_ = convert_text([int(t) for t in tokens[g]], r, ln, window)
        ids[g], adj[g], nn[g] = np.asarray(i_), a_, k_
    pattern = adj != 0
    return ids, nn, pattern, g_dinv(pattern), adj


def g_dense_pattern(a):
    """Pattern a dense hand-over is packed to: A's non-zeros (after the cast to fp32) united with A^T's."""
    nz = np.asarray(a).astype(np.float32) != 0
    return nz | np.swapaxes(nz, -1, -2)


def g_refined64(pattern, keep=None, dinv=None, vals=None, transpose=False):
    """float64 (n, r, r) adjacency the aggregation multiplies with: entry (i, j) is on iff pattern[i][j] and (no keep-set or
    keep[i] or keep[j]); its value is dinv[i] dinv[j] (normalised mode) or vals[i][j] (weighted mode; A^T when `transpose`)."""
    on = np.asarray(pattern, dtype=bool)
    if keep is not None:
        keep = np.asarray(keep, dtype=bool)
        on = on & (keep[..., :, None] | keep[..., None, :])
    if vals is not None:
        v = np.asarray(vals, dtype=np.float32).astype(np.float64)
        v = np.swapaxes(v, -1, -2) if transpose else v
    else:
        d = np.asarray(dinv, dtype=np.float32).astype(np.float64)
        v = d[..., :, None] * d[..., None, :]
    return np.where(on, v, 0.0)


def g_topk(score, k):
    """bool keep-set of the k best per row of score (..., R): descending score, ties to the lower index (-0.0 == 0.0)."""
    s = np.asarray(score)
    r = s.shape[-1]
    order = np.argsort(-s.astype(np.float64), axis=-1, kind="stable")
    keep = np.zeros(s.shape, dtype=bool)
    kk = min(max(int(k), 0), r)
    np.put_along_axis(keep, order[..., :kk], True, axis=-1)
    return keep


def g_scorer64(adj64, xproj, gate):
    """The word scorer GGNN(h -> 1) after its projection, in float64: xproj (n, r) = proj(dropout(feat)), one aggregation
    with the UNREFINED adjacency adj64 (n, r, r), the six 1x1 gates gate[12] = {wz0,bz0,wz1,bz1,wr0,br0,wr1,br1,wh0,bh0,wh1,bh1}."""
    x = np.asarray(xproj, dtype=np.float64)
    g = np.asarray(gate, dtype=np.float64)
    a = np.einsum("nij,nj->ni", np.asarray(adj64, dtype=np.float64), x)
    sig = lambda t: 1.0 / (1.0 + np.exp(-t))
    z = sig((g[0] * a + g[1]) + (g[2] * x + g[3]))
    rr = sig((g[4] * a + g[5]) + (g[6] * x + g[7]))
    hh = np.tanh((g[8] * a + g[9]) + (g[10] * (rr * x) + g[11]))
    return hh * z + x * (1.0 - z)


def g_plan(n_nodes, r, node_ids=None):
    """Node-compact plan: goff (n + 1,), rowg / src (n r,), and with node_ids cids / maskf (n r,).  Real node j of graph g is
    row goff[g] + j; its padding nodes follow the real rows of the whole batch, graph by graph, in node order."""
    nn = np.clip(np.asarray(n_nodes, dtype=np.int64), 0, r)
    n = len(nn)
    goff = np.zeros(n + 1, np.int32)
    goff[1:] = np.cumsum(nn)
    rowg, src = np.zeros(n * r, np.int32), np.zeros(n * r, np.int32)
    pad = int(goff[n])
    for g in range(n):
        for j in range(r):
            if j < nn[g]:
                row = goff[g] + j
            else:
                row, pad = pad, pad + 1
            rowg[row], src[row] = g, g * r + j
    out = dict(goff=goff, rowg=rowg, src=src)
    if node_ids is not None:
        cids = np.asarray(node_ids, dtype=np.int32).reshape(-1)[src]
        out.update(cids=cids, maskf=(cids >= 1).astype(np.float32))
    return out


def g_depad(counts, n_max, r, ids, adj):
    """The fitter's de-padding as a loop over the claims: for every slot j < clamp(counts[c], 0, n_max), in claim order, the
    ids narrowed to int32, the number of real nodes (id >= 1), the packed pattern, dinv, the fp32 values and the two flags
    `bad` (ids not prefix-shaped, or an edge on a padding node) and `weighted` (not D^-1/2 A D^-1/2 of its own pattern to
    4e-7 relative, or an entry present on one side only)."""
    out = dict(ids=[], n_nodes=[], pattern=[], dinv=[], vals=[], bad=[], weighted=[])
    for c, cnt in enumerate(np.asarray(counts).tolist()):
        for j in range(min(max(int(cnt), 0), n_max)):
            i_ = np.asarray(ids[c, j]).astype(np.int64)
            a32 = np.asarray(adj[c, j], dtype=np.float64).astype(np.float32)
            real = i_ >= 1
            nn = int(real.sum())
            pat = (a32 != 0) | (a32.T != 0)
            dinv = g_dinv(pat)
            bad = bool((real != (np.arange(r) < nn)).any()) or bool((pat.any(-1) & ~real).any())
            e = (dinv[:, None] * dinv[None, :]).astype(np.float32)           # the fp32 product, as the kernel forms it
            tol = (np.float32(4e-7) * e).astype(np.float32)
            weighted = bool((pat & ~(np.abs(a32 - e) <= tol)).any())
            for key, v in zip(("ids", "n_nodes", "pattern", "dinv", "vals", "bad", "weighted"),
                              (i_.astype(np.int32), nn, pat, dinv, a32, bad, weighted)):
                out[key].append(v)
    return out

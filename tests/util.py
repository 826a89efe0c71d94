"""Shared helpers for the parity tests (fixtures, gradient summaries, tolerances)."""
import json
import math
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


# ----------------------------------------------------------------------------- fenced operands, poisoned workspace
# (shared by the direct-ABI path tests: tests/test_gpu_gemm_paths.py, test_gpu_concat_att_paths.py, test_gpu_ragged_paths.py)
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
NAN = float("nan")
FENCE = 64                       # floats of NaN on either side of every operand, at the least


def _ops():
    from get_amd import _lib, ops
    _lib.ensure_workspace(DEV)
    return _lib, ops


class _Fenced:
    """Tensors placed inside NaN-filled allocations of their own; check() asserts that every fence is still all NaN."""

    def __init__(self):
        self.items = []

    def put(self, name, src=None, shape=None, mis=False, dtype=torch.float32):
        """A contiguous device tensor of `shape` (default: src's) holding `src` (None: NaN) with >= FENCE floats of NaN
        before and after it, 16-byte aligned (mis: 4 bytes past a 16-byte boundary)."""
        shape = tuple(src.shape if shape is None else shape)
        n = math.prod(shape)
        es = torch.empty((), dtype=dtype).element_size()
        pad = FENCE * 4 // es
        buf = torch.full((n + 2 * pad + 16,), NAN, device=DEV, dtype=dtype)
        off = pad
        while (buf.data_ptr() + off * es) % 16 != (4 if mis else 0):
            off += 1
        v = buf[off:off + n].view(shape)
        if src is not None:
            v.copy_(src.to(dtype))
        assert v.is_contiguous() and v.data_ptr() % 16 == (4 if mis else 0)
        assert off * es >= FENCE * 4 and (buf.numel() - off - n) * es >= FENCE * 4
        self.items.append((name, buf, off, n))
        return v

    def check(self, what):
        for name, buf, off, n in self.items:
            ok = torch.isnan(buf[:off]).all() & torch.isnan(buf[off + n:]).all()
            assert bool(ok), f"{what}: the NaN fence around {name} was written"


_SMALL_WS = []                   # the 1 MiB workspace while a small-workspace case runs


def _poison():
    """NaN into every float of the registered workspace: split-K partial tiles and the column-sum tail."""
    _lib, _ = _ops()
    _lib.ensure_workspace(DEV).fill_(NAN)
    for t in _SMALL_WS:
        t.fill_(NAN)


_WS_MODE = ["default"]           # default | none | small: what is registered for the stream right now


def _ws_written():
    """(partial tiles written, column-sum partials written) since _poison().  make_workspace (csrc/gemm_ops.hip) gives the
    last 1/16 of the buffer, 16-byte aligned, to the column sums and the rest to the tiles, both filled from their start.
    Without a workspace, or with the small one, the default buffer must not have been touched at all.
    (Probing the first float of either area relies on today's layout: Batch::flush, nt_split_plan and launch_colsum3
    each hand out their area from its start, so problem 0's chunk 0 / row block 0 lands there.  A plan that starts
    elsewhere needs another probe.)"""
    _lib, _ = _ops()
    default = _lib.ensure_workspace(DEV)
    if _WS_MODE[0] != "default":
        assert bool(torch.isnan(default).all()), "the default workspace was written while it was not registered"
    if _WS_MODE[0] == "none":
        return False, False
    ws = default if _WS_MODE[0] == "default" else _SMALL_WS[0]
    nbytes = ws.numel() * 4
    cs = ((nbytes - ((nbytes // 16) & ~15)) & ~15) // 4
    return not bool(torch.isnan(ws[0])), not bool(torch.isnan(ws[cs]))


class _workspace:
    """with _workspace(None): no workspace for the current stream; _workspace(1): a 1 MiB one.  The default workspace
    is registered again on the way out."""

    def __init__(self, mib):
        self.mib = mib

    def __enter__(self):
        _lib, _ = _ops()
        if self.mib is None:
            _lib.call("gh_set_stream_workspace", _lib.stream(), None, 0)
            _WS_MODE[0] = "none"
        else:
            small = torch.empty(self.mib << 18, device=DEV, dtype=torch.float32)
            _SMALL_WS.append(small)
            _lib.call("gh_set_stream_workspace", _lib.stream(), small.data_ptr(), small.numel() * 4)
            _WS_MODE[0] = "small"

    def __exit__(self, *exc):
        from get_amd import _lib
        torch.cuda.synchronize()
        _WS_MODE[0] = "default"
        _SMALL_WS.clear()
        _lib._workspaces.clear()          # the next ensure_workspace registers a default-sized buffer again
        _lib.ensure_workspace(DEV)
        return False


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
# Plain statements of what csrc/graph_build_ops.hip, spmm_ops.hip, gsl_ops.hip and the node-compact plan of ragged_ops.hip compute,
# used as the references of tests/test_gpu_graph_paths.py and
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


# ----------------------------------------------------------------------------- GGNN cell restatement (float64, tests only)
# What gh_ggnn_cell_fwd saves and gh_ggnn_cell_bwd computes (csrc/cell_ops.hip), written out: the reference of
# tests/test_gpu_cell_paths.py and tests/test_gpu_cell_bwd_nodx.py, checked on its own against autograd through the oracle's cell
# and against the reference's golden by tests/test_cell_restatement_cpu.py.
CELL_W = ("p", "z0", "z1", "r0", "r1", "h0", "h1")
CELL_B = ("z0", "z1", "r0", "r1", "h0", "h1")
CELL_SAVED = ("xp", "a", "z", "rr", "rx", "hh")
CELL_SCRATCH = ("dhp", "dzp", "drp", "dxp", "da")


def cell_forward_f64(adj, x, w, b):
    """adj (N,R,R), x (N,R,din) the masked input rows, w / b: the seven weights and six biases by CELL_W / CELL_B name ->
    dict of the saved streams xp, a, z, rr, rx, hh and `out` (wrapper.py:188-208), float64."""
    W = {k: v.double() for k, v in w.items()}
    B = {k: v.double() for k, v in b.items()}
    adj, x = adj.double(), x.double()
    xp = x @ W["p"].t()
    a = adj @ xp
    z = torch.sigmoid(a @ W["z0"].t() + B["z0"] + xp @ W["z1"].t() + B["z1"])
    rr = torch.sigmoid(a @ W["r0"].t() + B["r0"] + xp @ W["r1"].t() + B["r1"])
    rx = rr * xp
    hh = torch.tanh(a @ W["h0"].t() + B["h0"] + rx @ W["h1"].t() + B["h1"])
    return dict(xp=xp, a=a, z=z, rr=rr, rx=rx, hh=hh, out=hh * z + xp * (1 - z))


def cell_backward_f64(adj, x, g, w, b, saved=None, scratch=None):
    """adj (N,R,R), x (N,R,din) the masked input rows, g (N,R,h): every gradient of the cell, by hand, in float64 ->
    (dw by CELL_W name, db by CELL_B name, dx).  saved: the forward's streams to start from (default: cell_forward_f64 of
    the same inputs); scratch: a dict that receives the five scratch streams as the written-out chain leaves them (dhp, dzp,
    drp; dxp after every term including A_hat^T da; da summed over the three gates)."""
    W = {k: v.double() for k, v in w.items()}
    adj, x, g = adj.double(), x.double(), g.double()
    s = cell_forward_f64(adj, x, w, b) if saved is None else {k: saved[k].double() for k in CELL_SAVED}
    xp, a, z, r, rx, hh = (s[k] for k in CELL_SAVED)
    dhp = g * z * (1 - hh * hh)
    dzp = g * (hh - xp) * z * (1 - z)
    dxp = g * (1 - z)
    da = dhp @ W["h0"]
    drx = dhp @ W["h1"]
    drp = drx * xp * r * (1 - r)
    dxp = dxp + drx * r
    da = da + dzp @ W["z0"] + drp @ W["r0"]
    dxp = dxp + dzp @ W["z1"] + drp @ W["r1"]
    dxp = dxp + adj.transpose(1, 2) @ da
    tn = lambda p, q: torch.einsum("nri,nrj->ij", p, q)
    dw = {"p": tn(dxp, x), "z0": tn(dzp, a), "z1": tn(dzp, xp), "r0": tn(drp, a), "r1": tn(drp, xp), "h0": tn(dhp, a),
          "h1": tn(dhp, rx)}
    col = lambda p: p.sum((0, 1))
    db = {"z0": col(dzp), "z1": col(dzp), "r0": col(drp), "r1": col(drp), "h0": col(dhp), "h1": col(dhp)}
    if scratch is not None:
        scratch.update(dhp=dhp, dzp=dzp, drp=drp, dxp=dxp, da=da)
    return dw, db, dxp @ W["p"]


# ----------------------------------------------------------------------------- concat attention restatement (float64, tests only)
# What gh_concat_att_fwd computes and saves, as plain torch ops; the reference of tests/test_gpu_concat_att_paths.py, checked
# on its own against the oracle and the reference's goldens by tests/test_concat_restatement_cpu.py.
def _concat64(left, right, mask, w1, w2):
    """left (b, xl) or None, right (b, l, dr), mask (b, l) with 0 = padded, w1 (ha, xl + dr), w2 (heads, ha) ->
    u (b, ha), t (b, l, ha), e (b, l, heads), weights (b, l, heads), attended (b, dr, heads).  A pair whose rows are all
    masked has NaN weights and NaN attended, as the softmax of an all -inf column has."""
    xl = 0 if left is None else left.shape[1]
    u = left @ w1[:, :xl].t() if left is not None else right.new_zeros((right.shape[0], w1.shape[0]))
    t = torch.tanh(right @ w1[:, xl:].t() + u.unsqueeze(1))
    e = t @ w2.t()
    w = torch.softmax(e.masked_fill((mask == 0).unsqueeze(-1), float("-inf")), dim=1)
    attended = torch.einsum("bld,blc->bdc", right, w)
    return u, t, e, w, attended


# ----------------------------------------------------------------------------- ragged restatements (numpy, tests only)
# Plain statements of what csrc/ragged_ops.hip computes: the references of tests/test_gpu_ragged_paths.py, checked against the
# oracle's pad_left / pad_right by tests/test_concat_restatement_cpu.py.
def r_seg_offsets(counts, b1):
    """offsets int32 (b + 1,), pair2claim int32 (b1,), has float32 (b,): pairs beyond sum(counts) map to claim 0, pairs
    beyond b1 do not exist."""
    counts = np.asarray(counts, dtype=np.int64)
    offsets = np.zeros(len(counts) + 1, np.int32)
    offsets[1:] = np.cumsum(counts)
    p2c = np.zeros(b1, np.int32)
    full = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    n = min(b1, len(full))
    p2c[:n] = full[:n]
    return offsets, p2c, (counts > 0).astype(np.float32)


def r_seg_sum(src, offsets):
    """float64 (b, x): the sum of rows [offsets[c], offsets[c + 1]) of src, exact zeros for an empty claim."""
    src = np.asarray(src, dtype=np.float64)
    out = np.zeros((len(offsets) - 1, src.shape[1]), np.float64)
    for c in range(len(offsets) - 1):
        out[c] = src[offsets[c]:offsets[c + 1]].sum(0)
    return out


def r_seg_pad(src, offsets, n_max):
    """(b, n_max, x): the first min(count, n_max) rows of every claim, zeros behind them."""
    src = np.asarray(src)
    out = np.zeros((len(offsets) - 1, n_max, src.shape[1]), src.dtype)
    for c in range(len(offsets) - 1):
        k = min(int(offsets[c + 1] - offsets[c]), n_max)
        out[c, :k] = src[offsets[c]:offsets[c] + k]
    return out


def r_seg_unpad(padded, offsets, dst0):
    """dst0 (b1, x) with rows offsets[c] + j, j < min(count, n_max), replaced by padded[c][j]; the other rows untouched."""
    padded = np.asarray(padded)
    out = np.array(dst0, copy=True)
    for c in range(len(offsets) - 1):
        k = min(int(offsets[c + 1] - offsets[c]), padded.shape[1])
        out[offsets[c]:offsets[c] + k] = padded[c, :k]
    return out


def r_masked_mean(hid, ids, lens):
    """float64 (b, h): sum over the tokens with id > 0 of hid, divided by lens."""
    hid = np.asarray(hid, dtype=np.float64)
    live = (np.asarray(ids) > 0).astype(np.float64)
    return (hid * live[:, :, None]).sum(1) / np.asarray(lens, dtype=np.float64)[:, None]


def r_masked_mean_bwd(g, ids, lens):
    """float64 (b, l, h): g / lens on the rows of tokens with id > 0, exact zeros elsewhere."""
    g = np.asarray(g, dtype=np.float64)
    live = (np.asarray(ids) > 0).astype(np.float64)
    return live[:, :, None] * (g / np.asarray(lens, dtype=np.float64)[:, None])[:, None, :]


def r_clamp_sources(sources, table_rows):
    """(row of the table every slot reads, number of ids the kernel counts as clamped): -1 is the padding id (row 0, not
    counted), every other id outside [0, table_rows) goes to the nearest row and is counted once."""
    s = np.asarray(sources, dtype=np.int64)
    return np.clip(s, 0, table_rows - 1), int(((s < -1) | (s >= table_rows)).sum())


def r_evd_assemble(avg, offsets, table, sources, document, n_max):
    """right (b, n_max, xa + ds) and mask (b, n_max) float32, and the clamped-id count; table None: ds = 0."""
    avg = np.asarray(avg, dtype=np.float32)
    right = r_seg_pad(avg, offsets, n_max)
    clamped = 0
    if table is not None:
        rows, clamped = r_clamp_sources(sources, table.shape[0])
        right = np.concatenate([right, np.asarray(table, dtype=np.float32)[rows]], axis=-1)
    mask = (np.asarray(document, dtype=np.int64).sum(-1) >= 1).astype(np.float32)
    return right, mask, clamped


def r_evd_assemble_bwd(g, offsets, sources, table_rows, xa, d_table0):
    """d_avg float32 (b1, xa): the slot rows of g[:, :, :xa], zeros for a claim's pairs beyond n_max; d_table float64 =
    d_table0 + the scatter-add of g[:, :, xa:] over the REAL slots (slot < min(count, n_max)) by clamped source id."""
    g = np.asarray(g)
    b, n_max = g.shape[:2]
    d_avg = np.zeros((int(offsets[-1]), xa), np.float32)
    d_table = None if d_table0 is None else np.array(d_table0, dtype=np.float64)
    rows = r_clamp_sources(sources, table_rows)[0] if d_table is not None else None
    for c in range(b):
        k = min(int(offsets[c + 1] - offsets[c]), n_max)
        d_avg[offsets[c]:offsets[c] + k] = g[c, :k, :xa]
        for j in range(k if d_table is not None else 0):
            d_table[rows[c, j]] += g[c, j, xa:].astype(np.float64)
    return d_avg, d_table


# ----------------------------------------------------------------------------- the whole model (GPU tests)
def build_model(cfg, seed):
    from get_amd import modules
    from get_amd.synth import make_embeddings, make_state_dict
    emb, art, clm = make_embeddings(cfg, seed)
    model = modules.Graph_basedSemantiStructure(cfg.model_params(emb, art, clm))
    full = model.state_dict()
    full.update({k: torch.from_numpy(v) for k, v in make_state_dict(cfg, seed).items()})
    model.load_state_dict(full, strict=True)
    return model.to(DEV).train(False)


def to_dev(kargs):
    out = {}
    for k, v in kargs.items():
        if torch.is_tensor(v):
            out[k] = v.to(DEV)
        elif isinstance(v, tuple):
            out[k] = tuple(t.to(DEV) if torch.is_tensor(t) else t for t in v)
        else:
            out[k] = v
    return out


def run_model(cfg, seed, native_graphs=False, int32_inputs=False):
    """One forward of the drop-in model on the synthetic batch of (cfg, seed): reference-API inputs, graphs built on the
    device (native_graphs) or the node-compact plan on top (native_graphs == "compact")."""
    from get_amd.synth import make_raw_batch
    from oracle import get_oracle as O
    from oracle.assemble import assemble_inputs, reference_kargs
    model = build_model(cfg, seed)
    raw = make_raw_batch(cfg, seed)
    inp = assemble_inputs(raw, cfg, O.convert_text)
    kargs = to_dev(reference_kargs(inp, torch, output_ranking=True))
    query = torch.from_numpy(inp["query"]).to(DEV)
    document = torch.from_numpy(inp["document"]).to(DEV)
    if native_graphs:
        from get_amd import ops
        qa, q_ids, q_n = ops.graph_build(torch.from_numpy(raw["claim_tokens"]).to(DEV),
                                         torch.from_numpy(raw["claim_len"]).to(DEV), cfg.window)
        da, d_ids, d_n = ops.graph_build(torch.from_numpy(raw["evd_tokens"]).to(DEV),
                                         torch.from_numpy(raw["evd_len"]).to(DEV), cfg.window)
        assert np.array_equal(q_ids.cpu().numpy(), inp["query"]) and np.array_equal(d_ids.cpu().numpy(), inp["doc_ids"])
        assert np.array_equal(q_n.cpu().numpy(), inp["query_lens"])
        if native_graphs == "compact":     # node-compact fast path (ops.RaggedPlan): padding nodes skipped where inert
            da = da.with_plan(ops.RaggedPlan(d_n, d_ids, int(inp["doc_lens"].sum()) if "doc_lens" in inp else int(d_n.sum().item())))
        kargs["query_adj"], kargs["docs_adj"] = qa, da
    if int32_inputs:       # the evaluation path hands int32 ids/lens (char_man_fitter_query_repr1.py:298-316)
        query, document = query.int(), document.int()
        for k in ("query_lens", "doc_content_without_padding_evidences", "doc_sources", "query_sources"):
            kargs[k] = kargs[k].int()
    phi, (ww, ew) = model(query, document, **kargs)
    loss = torch.nn.functional.cross_entropy(phi, torch.from_numpy(inp["labels"]).to(DEV))
    return cfg, model, inp, phi, ww, ew, loss


def composite_vs_modules(cfg, seed, native, oracle=False):
    """get_amd/fused.py (gh_get_forward / gh_get_backward: the whole model in one library call each) against the
    module-by-module path on the same inputs: equal keep-sets, logits / weights / scores within 2e-6 max(1, scale), every
    gradient within 2e-5 of its scale.  oracle: the composite run also against oracle.get_oracle.model_forward at the model
    tests' bounds (logits 1e-4, weights 1e-5, gradients 1e-3 of their scale + 1e-5)."""
    from get_amd import fused
    res = {}
    was = fused.ENABLED
    try:
        for on in (False, True):
            fused.ENABLED = on
            cfg, model, inp, phi, ww, ew, loss = run_model(cfg, seed, native_graphs=native)
            assert (getattr(model, "_gh_binding", None) is not None) == on, "the wrong path ran"
            loss.backward()
            torch.cuda.synchronize()
            res[on] = dict(phi=phi.detach().clone(), ww=ww.detach().clone(), ew=ew.detach().clone(),
                           score=model.ggnn_with_gsl.last_score.clone(), keep=model.ggnn_with_gsl.last_keep.clone(),
                           grads={k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    finally:
        fused.ENABLED = was
    a, b = res[False], res[True]
    assert torch.equal(a["keep"], b["keep"])
    for k in ("phi", "ww", "ew", "score"):
        scale = max(1.0, float(a[k].abs().max()))
        err = float((a[k] - b[k]).abs().max())
        WORST["composite-vs-module"] = max(WORST.get("composite-vs-module", 0.0), err / scale)
        assert err <= 2e-6 * scale, k
    assert set(a["grads"]) == set(b["grads"])
    for k, g in a["grads"].items():
        scale = max(float(g.abs().max()), 1e-8)
        err = float((g - b["grads"][k]).abs().max())
        WORST["composite-vs-module"] = max(WORST.get("composite-vs-module", 0.0), err / scale)
        assert err <= 2e-5 * scale, k
    print(f"composite vs modules (seed {seed}, native={native}): worst err / scale so far {WORST['composite-vs-module']:.3e}")
    if oracle:
        _model_vs_oracle(cfg, seed, inp, b)
    return res


def _model_vs_oracle(cfg, seed, inp, got):
    from get_amd.synth import make_embeddings, make_state_dict
    from oracle import get_oracle as O
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    emb, art, _ = make_embeddings(cfg, seed)
    p = {k: T(v).requires_grad_(True) for k, v in make_state_dict(cfg, seed).items()}
    p["embedding.weight"], p["article_source_embs.weight"] = T(emb), T(art)
    phi, ww, ew = O.model_forward(p, cfg.__dict__, T(inp["query"]), T(inp["document"]), T(inp["query_adj"]), T(inp["doc_ids"]),
                                  T(inp["doc_adj"]), T(inp["query_lens"]), inp["evd_counts"], T(inp["doc_sources"]),
                                  T(inp["query_sources"]))
    O.cross_entropy(phi, T(inp["labels"])).backward()
    assert float((got["phi"].cpu() - phi.detach()).abs().max()) <= 1e-4, "logits against the oracle"
    assert float((got["ww"].cpu() - ww.detach()).abs().max()) <= 1e-5, "word weights against the oracle"
    assert float((got["ew"].cpu() - ew.detach()).abs().max()) <= 1e-5, "evidence weights against the oracle"
    n = 0
    for k, g in got["grads"].items():
        if k in p and p[k].grad is not None:
            want = p[k].grad.double()
            scale = max(float(want.abs().max()), 1e-6)
            err = float((g.double().cpu() - want).abs().max())
            assert err <= 1e-5 + 1e-3 * scale, f"{k} against the oracle: {err:.3e} vs scale {scale:.3e}"
            n += 1
    assert n >= 10, n

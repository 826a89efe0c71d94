"""Plain-torch restatements of the matchzoo/modules family (tests only): the five ops of csrc/match_ops.hip and the seven
modules built on them, evaluated in float64 by the GPU parity tests (tests/test_gpu_match.py) and checked on their own
against the reference's goldens by tests/test_match_cpu.py.  Nothing here imports the reference or the kernels."""
import numpy as np
import torch
import torch.nn.functional as F


# ----------------------------------------------------------------------------- the five ops
def soft_align64(q, k, v, key_fill, row_zero=None, fill=-1e-7, fuse=False):
    """(out, weights): S = q k^T with the columns of key_fill REPLACED by `fill` (they keep a weight), softmax over the keys,
    o = weights v with the rows of row_zero zeroed; out = o, or [q, o, q - o, q * o] with fuse."""
    s = (q @ k.transpose(1, 2)).masked_fill(key_fill.bool().unsqueeze(1), fill)
    a = torch.softmax(s, dim=2)
    o = a @ v
    if row_zero is not None:
        o = o.masked_fill(row_zero.bool().unsqueeze(2), 0.0)
    return (torch.cat([q, o, q - o, q * o], dim=2) if fuse else o), a


def lin_att64(x, w, mode=0):
    """The reference's two comparisons read literally: mask = (s != m); masked_fill(mask == m, -inf); softmax.  mode 0 / 1 are
    m == 0 / m == 1, mode 2 stands for any other m (m = 2 here)."""
    s = x @ w.reshape(-1)
    m = (0, 1, 2)[mode]
    mask = (s != m)
    return torch.softmax(s.masked_fill(mask == m, -float("inf")), dim=-1)


def match_dot64(x, y, normalize=False):
    if normalize:
        x, y = F.normalize(x, p=2, dim=-1), F.normalize(y, p=2, dim=-1)
    return torch.einsum("bld,brd->blr", x, y)


def match_bcast64(x, y, op):
    xe, ye = x.unsqueeze(2).expand(-1, -1, y.shape[1], -1), y.unsqueeze(1).expand(-1, x.shape[1], -1, -1)
    if op == "mul":
        return xe * ye
    if op == "plus":
        return xe + ye
    if op == "minus":
        return xe - ye
    assert op == "concat", op
    return torch.cat((xe, ye), dim=3)


def gauss_kernel64(x, mu, sigma):
    return torch.exp(-0.5 * ((x - mu) ** 2) / (sigma ** 2))


# ----------------------------------------------------------------------------- recurrences (torch's gate orders)
def _lstm_dir64(x, w_ih, w_hh, b_ih, b_hh, reverse):
    B, L, _ = x.shape
    H = w_hh.shape[1]
    h, c = x.new_zeros(B, H), x.new_zeros(B, H)
    out = [None] * L
    for t in (range(L - 1, -1, -1) if reverse else range(L)):
        i, f, g, o = (x[:, t] @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh).chunk(4, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        out[t] = h
    return torch.stack(out, dim=1)


def _gru_dir64(x, w_ih, w_hh, b_ih, b_hh, reverse):
    B, L, _ = x.shape
    H = w_hh.shape[1]
    h = x.new_zeros(B, H)
    out = [None] * L
    for t in (range(L - 1, -1, -1) if reverse else range(L)):
        xr, xz, xn = (x[:, t] @ w_ih.t() + b_ih).chunk(3, dim=1)
        hr, hz, hn = (h @ w_hh.t() + b_hh).chunk(3, dim=1)
        r, z = torch.sigmoid(xr + hr), torch.sigmoid(xz + hz)
        n = torch.tanh(xn + r * hn)
        h = (1 - z) * n + z * h
        out[t] = h
    return torch.stack(out, dim=1)


def _drop(x, keep, p):
    """x with the replayed mask `keep` (bool, True = kept, any shape that views to x's) scaled by 1 / (1 - p)."""
    return x * torch.as_tensor(keep).to(x.dtype).reshape(x.shape) / (1.0 - p)


# ----------------------------------------------------------------------------- the seven modules; p: parameters by name
def attention64(p, x, mask=0):
    return lin_att64(x, p["linear.weight"], 0 if mask == 0 else (1 if mask == 1 else 2))


def bidirectional_attention64(v1, v1_mask, v2, v2_mask):
    return soft_align64(v1, v2, v2, v2_mask, v1_mask)[0], soft_align64(v2, v1, v1, v1_mask, v2_mask)[0]


def match_module64(p, v1, v2, v2_mask, keep=None, drop_p=0.0, relu_mask=None):
    """relu_mask: the ReLU's decisions taken from another run (bool, True = passed) instead of the sign of the pre-activation."""
    proj_v2 = v2 @ p["v2_proj.weight"].t() + p["v2_proj.bias"]
    fusion = soft_align64(v1, proj_v2, v2, v2_mask != 0, fuse=True)[0]
    pre = fusion @ p["proj.weight"].t() + p["proj.bias"]
    match = torch.relu(pre) if relu_mask is None else pre * relu_mask.to(pre.dtype)
    return match if keep is None else _drop(match, keep, drop_p)


def matching64(x, y, normalize=False, matching_type="dot"):
    return match_dot64(x, y, normalize) if matching_type == "dot" else match_bcast64(x, y, matching_type)


def rnn_dropout64(x, keep=None, drop_p=0.0):
    """keep: the replayed (B, D) mask, shared by every position; None = eval mode."""
    return x if keep is None else x * (torch.as_tensor(keep).to(x.dtype) / (1.0 - drop_p)).unsqueeze(1)


def stacked_brnn64(p, x, num_layers, rnn_type="LSTM", concat_layers=False, keeps=None, drop_p=0.0, keep_out=None):
    """keeps: one replayed input mask per layer (or None), keep_out: the replayed output mask (dropout_output) or None."""
    step = _lstm_dir64 if rnn_type == "LSTM" else _gru_dir64
    outputs, inp = [], x
    for i in range(num_layers):
        if keeps is not None and keeps[i] is not None:
            inp = _drop(inp, keeps[i], drop_p)
        dirs = [step(inp, *(p[f"rnns.{i}.{k}_l0{sfx}"] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")), rev)
                for sfx, rev in (("", False), ("_reverse", True))]
        inp = torch.cat(dirs, dim=2)
        outputs.append(inp)
    out = torch.cat(outputs, dim=2) if concat_layers else outputs[-1]
    return out if keep_out is None else _drop(out, keep_out, drop_p)


# ----------------------------------------------------------------------------- the golden cases (tests/golden/g17_match.npz)
# What tests/test_match_cpu.py (these restatements) and tests/test_gpu_match.py (the drop-ins) share: the forward arguments
# of a case, the restatement of its class, and the comparison at the golden bounds.
MAX_SCALED = ("bidir", "match")      # gradients bounded by TOL of the largest entry of their tensor, elementwise elsewhere


def golden_args(z, key):
    """The forward arguments of case `key` = '<family>::<shape>' in order, as (name, fp32 tensor or bool mask,
    differentiable); ``dotn`` runs on the inputs stored under ``dot``."""
    family = key.split("::")[0]
    src = key.replace("dotn::", "dot::")

    def arr(n):
        return torch.from_numpy(z[f"{src}::{n}"].astype(np.float32))

    def mask(n, length):
        return torch.arange(length)[None, :] >= torch.from_numpy(z[f"{key}::{n}"].astype(np.int64))[:, None]
    if family == "bidir":
        v1, v2 = arr("v1"), arr("v2")
        return [("v1", v1, True), ("v1_mask", mask("len1", v1.shape[1]), False), ("v2", v2, True),
                ("v2_mask", mask("len2", v2.shape[1]), False)]
    if family == "match":
        v1, v2 = arr("v1"), arr("v2")
        return [("v1", v1, True), ("v2", v2, True), ("v2_mask", mask("len2", v2.shape[1]), False)]
    if family in ("att", "gauss"):
        return [("x", arr("x"), True)]
    if family == "brnn":
        x = arr("x")
        return [("x", x, True), ("x_mask", torch.zeros(x.shape[:2], dtype=torch.bool), False)]
    return [("x", arr("x"), True), ("y", arr("y"), True)]


def golden_params(z, key):
    pre = f"{key}::param::"
    return {k[len(pre):]: torch.from_numpy(z[k].astype(np.float32)) for k in z if k.startswith(pre)}


def restate64(family, kwargs, p, args):
    """The class of `family` with the contract's kwargs on float64 `args` and parameters `p`, in eval mode: a tuple of outputs."""
    if family == "bidir":
        return bidirectional_attention64(*args)
    if family == "match":
        return (match_module64(p, *args),)
    if family == "att":
        return (attention64(p, args[0], kwargs["mask"]),)
    if family == "gauss":
        return (gauss_kernel64(args[0], kwargs["mu"], kwargs["sigma"]),)
    if family == "brnn":
        return (stacked_brnn64(p, args[0], kwargs["num_layers"], kwargs["rnn_type"], kwargs["concat_layers"]),)
    return (matching64(args[0], args[1], kwargs["normalize"], kwargs["matching_type"]),)


def check_golden(z, key, outs, grads):
    """`outs` (tuple) and `grads` (by input / parameter name) of case `key` at the golden bounds: outputs 1e-4 + 1e-4 |want|
    and gradients 1e-5 + 1e-4 |want| elementwise; the gradients of MAX_SCALED families within TOL of their tensor's largest
    entry.  A gradient stored as every n-th row ('::rows<n>') is compared on those rows.  Returns the number of gradients."""
    from tests.util import TOL, golden_ratio, rel_close
    family = key.split("::")[0]
    for i, o in enumerate(outs):
        golden_ratio(o, z[f"{key}::out{i}"], 1e-4, 1e-4, f"{key}::out{i}")
    assert f"{key}::out{len(outs)}" not in z
    pre = f"{key}::grad::"
    names = [k[len(pre):] for k in z if k.startswith(pre)]
    for name in names:
        want = z[pre + name]
        base, _, rows = name.partition("::rows")
        got = grads[base].detach()
        if rows:
            got = got[::int(rows)]
        if family in MAX_SCALED:
            rel_close(got, want, TOL, pre + name, fam="match_golden")
        else:
            golden_ratio(got, want, 1e-5, 1e-4, pre + name)
    return len(names)

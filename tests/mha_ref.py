"""Plain-torch restatements of the multi-head query/key/value attention family (tests only): evaluated in float64 by
tests/test_gpu_mha.py and checked on their own against the reference's goldens by tests/test_mha_cpu.py.  The conventions
of the kernels are stated here without a NaN detour: masked weights are exact zeros and a fully masked row is all zero."""
import torch


def sdpa64(q, k, v, mask, heads):
    """q (B,Lq,H*dk), k (B,Lk,H*dk), v (B,Lk,H*dv), mask (B,Lq,Lk) bool, True = masked -> out (B,Lq,H*dv),
    weights (H*B,Lq,Lk) head-major.  softmax(q_h k_h^T) over the unmasked keys, no temperature."""
    b, lq, _ = q.shape
    lk = k.shape[1]
    qh = q.reshape(b, lq, heads, -1).permute(2, 0, 1, 3)
    kh = k.reshape(b, lk, heads, -1).permute(2, 0, 1, 3)
    vh = v.reshape(b, lk, heads, -1).permute(2, 0, 1, 3)
    s = (qh @ kh.transpose(-1, -2)).masked_fill(mask.unsqueeze(0), float("-inf"))
    top = s.amax(-1, keepdim=True)
    e = torch.exp(s - torch.where(torch.isfinite(top), top, torch.zeros_like(top)))      # exp(-inf) = 0 at masked keys
    den = e.sum(-1, keepdim=True)
    w = e / torch.where(den > 0, den, torch.ones_like(den))
    out = (w @ vh).permute(1, 2, 0, 3).reshape(b, lq, -1)
    return out, w.reshape(heads * b, lq, lk)


def layernorm64(x, gamma, beta, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma + beta


def tanh_concat64(p, query, key, value, pad, prefix=""):
    """ConcatNotEqualSelfAttTransFormer: query (B,1,X), key (B,L,D), value (B,L,Dv), pad (B,L) bool, True = pad ->
    attended (B,Dv,1), weights (B,L,1)."""
    w1, w2 = p[prefix + "linear1.weight"], p[prefix + "linear2.weight"]
    x = query.shape[-1]
    t = torch.tanh(key @ w1[:, x:].t() + query @ w1[:, :x].t())
    e = (t @ w2.t()).masked_fill(pad.unsqueeze(-1), float("-inf"))
    w = torch.softmax(e, dim=1)
    return value.transpose(1, 2) @ w, w


def module64(cls, kwargs, p, args, mask, keep=None):
    """The four classes on plain torch ops; p: parameters by state_dict name, args: the forward's positional tensors.
    keep (a dict, MultiHeadAttentionOriginal only) receives the projected keys "kp" with their gradient retained."""
    lin = lambda x, n: x @ p[n + ".weight"].t() + p[n + ".bias"]
    if cls == "ScaledDotProductAttention":
        return sdpa64(args[0], args[1], args[2], mask, 1)
    if cls == "MultiHeadAttentionOriginal":
        q, k, v = args
        kp = lin(k, "w_ks")
        if keep is not None:
            kp.retain_grad()
            keep["kp"] = kp
        out, _ = sdpa64(lin(q, "w_qs"), kp, lin(v, "w_vs"), mask, kwargs["n_head"])
        return layernorm64(lin(out, "fc") + q, p["layer_norm.weight"], p["layer_norm.bias"]), None
    if cls == "ConcatNotEqualSelfAttTransFormer":
        return tanh_concat64(p, args[0], args[1], args[2], mask.reshape(args[1].shape[0], args[1].shape[1]))
    assert cls == "MultiHeadAttentionSimple", cls
    left, right = args
    h, (b, l, d) = kwargs["num_heads"], right.shape
    heads = lambda x, rows: x.reshape(b, rows, h, d).permute(2, 0, 1, 3).reshape(h * b, rows, d)
    att, w = tanh_concat64(p, heads(lin(left, "w_qs"), 1), heads(lin(right, "w_ks"), l), heads(lin(right, "w_vs"), l),
                           (mask == 0).repeat(h, 1), prefix="attention_func.")
    out = lin(att.reshape(h, b, 1, d).permute(1, 2, 0, 3).reshape(b, 1, h * d), "fc")
    if kwargs.get("use_layer_norm"):
        out = layernorm64(out, p["layer_norm.weight"], p["layer_norm.bias"])
    return out, w

"""Float64 restatement of the BERT encoder (tests only): the embedding sum + LayerNorm, the self-attention with its additive
key bias and dropout from a given keep mask, one encoder layer and the pooler, written from the formulas in plain torch.  The
GPU tests compare the kernels with it (tests/test_gpu_bert.py, tests/test_gpu_bert_paths.py); tests/test_bert_cpu.py checks it
on its own against the reference's goldens.  Everything is differentiable, so autograd supplies the float64 gradients."""
import math

import torch


def layer_norm(x, weight, bias, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * weight + bias


def dropout(x, keep, p):
    """x . keep / (1 - p); keep None = no dropout."""
    return x if keep is None else x * keep.to(x.dtype) / (1.0 - p)


def gelu(x):
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def attention(q, k, v, bias, heads, scale, keep=None, p=0.0):
    """q (B,Lq,H*dh), k, v (B,Lk,H*dh), bias (B,Lk) or None, keep (B,H,Lq,Lk) bool or None ->
    out (B,Lq,H*dh) = (softmax(scale q_h k_h^T + bias) . keep / (1 - p)) v_h and lse (B,H,Lq)."""
    b, lq, w = q.shape
    lk, dh = k.shape[1], w // heads
    split = lambda t, l: t.reshape(b, l, heads, dh).permute(0, 2, 1, 3)
    s = scale * (split(q, lq) @ split(k, lk).transpose(-1, -2))
    if bias is not None:
        s = s + bias[:, None, None, :]
    probs = dropout(torch.softmax(s, dim=-1), keep, p)
    out = (probs @ split(v, lk)).permute(0, 2, 1, 3).reshape(b, lq, w)
    return out, torch.logsumexp(s, dim=-1)


def embed(p, ids, pos_ids, type_ids, eps, prefix="embeddings."):
    """sum = word[ids] + pos[pos_ids] + type[type_ids] (pos_ids None: the column index; type_ids None: row 0) and its LayerNorm."""
    b, l = ids.shape
    if pos_ids is None:
        pos_ids = torch.arange(l).unsqueeze(0).expand(b, l)
    if type_ids is None:
        type_ids = torch.zeros_like(ids)
    # (padding_idx=0: row 0 of the word table is looked up like any other and receives no gradient)
    s = (torch.nn.functional.embedding(ids.long(), p[prefix + "word_embeddings.weight"], padding_idx=0)
         + p[prefix + "position_embeddings.weight"][pos_ids.long()] + p[prefix + "token_type_embeddings.weight"][type_ids.long()])
    return s, layer_norm(s, p[prefix + "LayerNorm.weight"], p[prefix + "LayerNorm.bias"], eps)


def linear(p, name, x):
    return x @ p[name + ".weight"].t() + p[name + ".bias"]


def layer(p, prefix, x, bias, heads, eps, act="gelu", masks=None, p_hidden=0.0, p_att=0.0):
    """One encoder layer; masks: {"att": (B,H,L,L), "att_out": (B,L,H), "out": (B,L,H)} keep masks or None."""
    masks = masks or {}
    dh = x.shape[-1] // heads
    a = prefix + "attention."
    ctx, _ = attention(linear(p, a + "self.query", x), linear(p, a + "self.key", x), linear(p, a + "self.value", x), bias, heads,
                       1.0 / math.sqrt(dh), masks.get("att"), p_att)
    h = dropout(linear(p, a + "output.dense", ctx), masks.get("att_out"), p_hidden)
    att = layer_norm(h + x, p[a + "output.LayerNorm.weight"], p[a + "output.LayerNorm.bias"], eps)
    i = linear(p, prefix + "intermediate.dense", att)
    i = gelu(i) if act == "gelu" else torch.relu(i)
    o = dropout(linear(p, prefix + "output.dense", i), masks.get("out"), p_hidden)
    return layer_norm(o + att, p[prefix + "output.LayerNorm.weight"], p[prefix + "output.LayerNorm.bias"], eps)


def pooler(p, seq):
    return torch.tanh(linear(p, "pooler.dense", seq[:, 0]))


def model(p, config, ids, type_ids=None, mask=None, pos_ids=None, masks=None):
    """BertModel.forward in float64: p = parameters by state_dict name (float64), config = dict of the BertConfig fields,
    mask (B,L) float or None, masks = {"emb": (B,L,H), "layers": [per layer dict as `layer` takes]} keep masks (training mode) or
    None (eval) -> (sequence_output, pooled_output, hidden states incl. the embedding output)."""
    eps, heads = config["layer_norm_eps"], config["num_attention_heads"]
    p_h, p_a = config["hidden_dropout_prob"], config["attention_probs_dropout_prob"]
    bias = None if mask is None else (1.0 - mask.double()) * -10000.0
    _, x = embed(p, ids, pos_ids, type_ids, eps)
    x = dropout(x, masks["emb"] if masks else None, p_h)
    hidden = [x]
    for n in range(config["num_hidden_layers"]):
        x = layer(p, f"encoder.layer.{n}.", x, bias, heads, eps, config["hidden_act"], masks["layers"][n] if masks else None, p_h, p_a)
        hidden.append(x)
    return x, pooler(p, x), hidden

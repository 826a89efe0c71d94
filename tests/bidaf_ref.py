"""Plain-torch restatement (tests only) of Models/BiDAF/bidaf_model.py: the attention-flow layer in closed form (no q_len
loop, no squeeze), the highway layer and the whole model, with tests/rnn_ref.py for the two encoders.  Evaluated in float64
by the GPU tests (tests/test_gpu_bidaf.py) and checked on its own against the reference's goldens by
tests/test_bidaf_cpu.py."""
import torch

from tests.rnn_ref import lstm64


def att_flow64(c, q, w_c, w_q, w_cq, bias=0.0):
    """c (B,Lc,D), q (B,Lq,D), w_* (D,), bias = b_c + b_q + b_cq -> x (B,Lc,4D) and the argmax (B,Lc) of torch.max over the
    scores' last axis (the lowest index among ties).  No mask: every row of c and q takes part."""
    s = (c @ w_c).unsqueeze(2) + (q @ w_q).unsqueeze(1) + (c * w_cq) @ q.transpose(1, 2) + bias
    a = torch.softmax(s, dim=2)
    c2q = a @ q
    m, am = torch.max(s, dim=2)
    beta = torch.softmax(m, dim=1)
    q2c = (beta.unsqueeze(2) * c).sum(1, keepdim=True)
    return torch.cat([c, c2q, c * c2q, c * q2c], dim=-1), am


def highway64(x, h_pre, g_pre):
    g = torch.sigmoid(g_pre)
    return g * torch.relu(h_pre) + (1 - g) * x


def _sub(params, prefix):
    return {k[len(prefix):]: v for k, v in params.items() if k.startswith(prefix)}


def bidaf64(params, query, document, q_lens, c_lens, drop_masks=None, p=0.0):
    """params: tensors by the model's state_dict names; query (B,L), document (B,R) integer ids; lengths (B,).  drop_masks:
    the kept entries of the three input dropouts (context encoder on the document (B,Tc,D), on the query (B,Tq,D), modeling
    encoder (B,Tc,8H)), None in eval mode.  Returns the logits (B,1)."""
    q_lens, c_lens = torch.as_tensor(q_lens).long(), torch.as_tensor(c_lens).long()
    masks = drop_masks or (None, None, None)

    def lin(x, name):
        return x @ params[name + ".weight"].t() + params[name + ".bias"]

    def highway(x):
        for i in range(2):
            x = highway64(x, lin(x, f"highway_linear{i}.0.linear"), lin(x, f"highway_gate{i}.0.linear"))
        return x

    emb = params["word_emb.weight"]
    c = highway(emb[document.long()])
    q = highway(emb[query.long()])
    ctx = _sub(params, "context_LSTM.")
    Tc, Tq = int(c_lens.max()), int(q_lens.max())
    c = lstm64(ctx, c[:, :Tc], c_lens, Tc, 1, True, masks[0], p)[0]
    q = lstm64(ctx, q[:, :Tq], q_lens, Tq, 1, True, masks[1], p)[0]
    w = [params[f"att_weight_{n}.linear.weight"].reshape(-1) for n in ("c", "q", "cq")]
    bias = sum(params[f"att_weight_{n}.linear.bias"] for n in ("c", "q", "cq"))
    g, _ = att_flow64(c, q, w[0], w[1], w[2], bias)
    m = lstm64(_sub(params, "modeling_LSTM1."), g, c_lens, Tc, 1, True, masks[2], p)[1]
    return lin(m, "last_linear")

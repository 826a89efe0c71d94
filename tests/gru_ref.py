"""Plain-torch restatement (tests only) of the GRU sequence encoder of Models/BiDAF/wrapper.py:279-327: torch.nn.GRU's
cell equations written out per step, sequences masked by their lengths, no nn.GRU, no packing.  Evaluated in float64 by the
GPU tests (tests/test_gpu_gru.py) and checked on its own against the reference's goldens by tests/test_gru_cpu.py."""
import torch


def gru64(params, x, lens, T, num_layers=1, bidirectional=False, drop_mask=None, p=0.0):
    """params: tensors by nn.GRU's names (``weight_ih_l0`` ..., an ``rnn.`` prefix is accepted); x (B,L,D); lens (B,) integers
    (clamped into [0, min(L, T)]); T: length of the output.  drop_mask (B,L,D) of kept entries: the input dropout replayed.
    Returns y (B,T,dirs*H), zero at t >= len, and h (B, layers*dirs*H): the state after each direction's last step,
    layer-major, zero for an empty sequence."""
    params = {(k[4:] if k.startswith("rnn.") else k): v for k, v in params.items()}
    B = x.shape[0]
    lens = torch.as_tensor(lens).long().clamp(0, min(x.shape[1], T))
    inp = x if drop_mask is None else x * drop_mask / (1.0 - p)
    states = []
    for layer in range(num_layers):
        outs = []
        for sfx in ("", "_reverse") if bidirectional else ("",):
            w_ih, w_hh = params[f"weight_ih_l{layer}{sfx}"], params[f"weight_hh_l{layer}{sfx}"]
            b_ih, b_hh = params[f"bias_ih_l{layer}{sfx}"], params[f"bias_hh_l{layer}{sfx}"]
            H = w_hh.shape[1]
            h = torch.zeros(B, H, dtype=x.dtype)
            y = [torch.zeros(B, H, dtype=x.dtype) for _ in range(T)]
            steps = range(min(inp.shape[1], T))
            for t in (reversed(steps) if sfx else steps):
                live = (t < lens).unsqueeze(1)
                gx_r, gx_z, gx_n = (inp[:, t] @ w_ih.t() + b_ih).chunk(3, dim=1)
                a_r, a_z, a_n = (h @ w_hh.t() + b_hh).chunk(3, dim=1)      # b_hn stays inside the product with r
                r = torch.sigmoid(gx_r + a_r)
                z = torch.sigmoid(gx_z + a_z)
                n = torch.tanh(gx_n + r * a_n)
                h_new = (1.0 - z) * n + z * h
                h = torch.where(live, h_new, h)
                y[t] = torch.where(live, h_new, torch.zeros_like(h_new))
            outs.append(torch.stack(y, dim=1))
            states.append(h)
        inp = torch.cat(outs, dim=2)
    return inp, torch.cat(states, dim=1)

"""Plain-torch restatement (tests only) of the two sequence encoders of Models/BiDAF/wrapper.py (LSTM :229-276, GRU :279-327):
torch.nn.LSTM's and torch.nn.GRU's cell equations written out per step, sequences masked by their lengths, no nn.LSTM, no
nn.GRU, no packing.  One driver (layers, directions, masking, the replayed input dropout), one function per cell.  Evaluated
in float64 by the GPU tests (tests/test_gpu_rnn.py, tests/test_gpu_bidaf.py through tests/bidaf_ref.py) and checked on its own
against the reference's goldens by tests/test_rnn_cpu.py."""
from collections import namedtuple

import torch


def _lstm_cell(x_t, state, w_ih, w_hh, b_ih, b_hh):
    h, c = state
    pre = x_t @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
    i, f, g, o = pre.chunk(4, dim=1)
    c_new = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    h_new = torch.sigmoid(o) * torch.tanh(c_new)
    return h_new, c_new


def _gru_cell(x_t, state, w_ih, w_hh, b_ih, b_hh):
    h, = state
    gx_r, gx_z, gx_n = (x_t @ w_ih.t() + b_ih).chunk(3, dim=1)
    a_r, a_z, a_n = (h @ w_hh.t() + b_hh).chunk(3, dim=1)      # b_hn stays inside the product with r
    r = torch.sigmoid(gx_r + a_r)
    z = torch.sigmoid(gx_z + a_z)
    n = torch.tanh(gx_n + r * a_n)
    return ((1.0 - z) * n + z * h,)


def _encoder(cell, n_state, params, x, lens, T, num_layers, bidirectional, drop_mask, p):
    """cell(x_t, state, w_ih, w_hh, b_ih, b_hh) -> the new state, a tuple of `n_state` (B,H) tensors whose first is h."""
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
            state = tuple(torch.zeros(B, H, dtype=x.dtype) for _ in range(n_state))
            y = [torch.zeros(B, H, dtype=x.dtype) for _ in range(T)]
            steps = range(min(inp.shape[1], T))
            for t in (reversed(steps) if sfx else steps):
                live = (t < lens).unsqueeze(1)
                new = cell(inp[:, t], state, w_ih, w_hh, b_ih, b_hh)
                state = tuple(torch.where(live, a, b) for a, b in zip(new, state))
                y[t] = torch.where(live, new[0], torch.zeros_like(new[0]))
            outs.append(torch.stack(y, dim=1))
            states.append(state[0])
        inp = torch.cat(outs, dim=2)
    return inp, torch.cat(states, dim=1)


def lstm64(params, x, lens, T, num_layers=1, bidirectional=False, drop_mask=None, p=0.0):
    """params: tensors by nn.LSTM's names (``weight_ih_l0`` ..., an ``rnn.`` prefix is accepted); x (B,L,D); lens (B,) integers
    (clamped into [0, min(L, T)]); T: length of the output.  drop_mask (B,L,D) of kept entries: the input dropout replayed.
    Returns y (B,T,dirs*H), zero at t >= len, and h (B, layers*dirs*H): the state after each direction's last step,
    layer-major, zero for an empty sequence."""
    return _encoder(_lstm_cell, 2, params, x, lens, T, num_layers, bidirectional, drop_mask, p)


def gru64(params, x, lens, T, num_layers=1, bidirectional=False, drop_mask=None, p=0.0):
    """The same for nn.GRU's names and cell."""
    return _encoder(_gru_cell, 1, params, x, lens, T, num_layers, bidirectional, drop_mask, p)


# what the tests of the two encoders are parametrised over: the drop-in's class name in get_amd.modules, its golden archive
# and contract under tests/golden/, its restatement above, its gate count
Cell = namedtuple("Cell", "module archive contract ref64 gates")
CELLS = {"lstm": Cell("LSTM", "g14_lstm.npz", "lstm_contract.json", lstm64, 4),
         "gru": Cell("GRU", "g16_gru.npz", "gru_contract.json", gru64, 3)}

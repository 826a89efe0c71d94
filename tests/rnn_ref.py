"""Plain-torch restatement (tests only) of the two sequence encoders of Models/BiDAF/wrapper.py (LSTM :229-276, GRU :279-327):
torch.nn.LSTM's and torch.nn.GRU's cell equations written out per step, sequences masked by their lengths, no nn.LSTM, no
nn.GRU, no packing.  One driver (layers, directions, masking, the replayed input dropout), one function per cell.  Evaluated
in float64 by the GPU tests (tests/test_gpu_rnn.py, tests/test_gpu_bidaf.py through tests/bidaf_ref.py) and checked on its own
against the reference's goldens by tests/test_rnn_cpu.py."""
from collections import namedtuple
from types import SimpleNamespace

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


# ----------------------------------------------------------------------------- one layer at the kernels' interface
# (include/get_hip.h gh_lstm_seq_* / gh_gru_seq_*): the per-step restatement that also returns the saved streams and, by
# autograd, the raw gradient streams.  Compared with the four entries by tests/test_gpu_rnn_paths.py, with lstm64 / gru64
# above and with its own fp32 evaluation by tests/test_rnn_cpu.py.
def _steps(G, gx, w_hh, b_hh, lens, t_in, t_out, g_y, g_hn, backward):
    dirs, (n, _, hg), dt = len(gx), gx[0].shape, gx[0].dtype
    h = hg // G
    assert dirs in (1, 2) and all(g.shape == (n, t_in, G * h) for g in gx) and all(w.shape == (G * h, h) for w in w_hh)
    cap = min(t_in, t_out)
    lens = torch.as_tensor(lens).long().clamp(0, cap)                      # the header's clamp
    gx = [g.detach().clone().requires_grad_(backward) for g in gx]
    w = [v.detach().clone().to(dt).requires_grad_(backward) for v in w_hh]
    b = [v.detach().clone().to(dt).requires_grad_(backward) for v in b_hh] if b_hh is not None else None
    # the GRU's zero probe: added to a = h W_hh^T + b_hh, its gradient is the header's `da`
    probe = [torch.zeros(n, t_in, G * h, dtype=dt, requires_grad=backward) for _ in range(dirs)] if b is not None else None
    nan = lambda *s: torch.full(s, float("nan"), dtype=dt)
    y = [[torch.zeros(n, h, dtype=dt) for _ in range(t_out)] for _ in range(dirs)]
    gates, aux, hprev = nan(dirs, n, t_in, G * h), nan(dirs, n, t_in, h), torch.zeros(dirs, n, t_in, h, dtype=dt)
    hn, cn = [], []
    for d in range(dirs):
        hs, cs = torch.zeros(n, h, dtype=dt), torch.zeros(n, h, dtype=dt)
        for t in (range(cap - 1, -1, -1) if d else range(cap)):            # the reverse direction walks len - 1 .. 0
            live = (t < lens).unsqueeze(1)
            rec = hs @ w[d].t()
            if b is None:                                                   # LSTM: i, f, g, o
                i, f, g, o = (gx[d][:, t] + rec).chunk(4, dim=1)
                i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
                c_new = f * cs + i * g
                h_new = o * torch.tanh(c_new)
                row, extra = torch.cat([i, f, g, o], dim=1), c_new
                cs = torch.where(live, c_new, cs)
            else:                                                           # GRU: r, z, n
                a_r, a_z, a_n = (rec + b[d] + probe[d][:, t]).chunk(3, dim=1)
                x_r, x_z, x_n = gx[d][:, t].chunk(3, dim=1)
                r, z = torch.sigmoid(x_r + a_r), torch.sigmoid(x_z + a_z)
                nn_ = torch.tanh(x_n + r * a_n)
                h_new = (1.0 - z) * nn_ + z * hs
                row, extra = torch.cat([r, z, nn_], dim=1), a_n
            m = live.squeeze(1)
            gates[d, m, t], aux[d, m, t], hprev[d, m, t] = row.detach()[m], extra.detach()[m], hs.detach()[m]
            y[d][t] = torch.where(live, h_new, torch.zeros_like(h_new))
            hs = torch.where(live, h_new, hs)
        hn.append(hs)
        cn.append(cs)
    y = torch.cat([torch.stack(v, dim=1) for v in y], dim=2)
    hn, cn = torch.stack(hn), torch.stack(cn)
    out = dict(y=y.detach(), h_n=hn.detach(), gates=gates, h_prev=hprev, lens=lens)
    out["c_n" if b is None else "_"] = cn.detach()
    out["c" if b is None else "an"] = aux
    out.pop("_", None)
    if backward:
        loss = 0.0
        if g_y is not None:
            loss = loss + (y * g_y.to(dt)).sum()
        if g_hn is not None:
            loss = loss + (hn * g_hn.to(dt)).sum()
        if torch.is_tensor(loss):
            loss.backward()
        grad = lambda ts: [t.grad if t.grad is not None else torch.zeros_like(t) for t in ts]
        out["dgates" if b is None else "dgx"] = torch.stack(grad(gx))
        out["dw"] = grad(w)
        if b is not None:
            out["da"], out["db"] = torch.stack(grad(probe)), grad(b)
    return out


def lstm_steps64(gx, w_hh, lens, t_in, t_out, g_y=None, g_hn=None, backward=False):
    """One LSTM layer as gh_lstm_seq_fwd / _bwd state it, in the dtype of gx (float64 for a reference).  gx, w_hh: one tensor
    per direction, (n, t_in, 4h) and (4h, h); lens (n,) integers, clamped into [0, min(t_in, t_out)].  Returns a dict: y
    (n, t_out, dirs h), h_n, c_n (dirs, n, h); the saved streams in the header's layout -- gates (dirs, n, t_in, 4h), c and
    h_prev (dirs, n, t_in, h), gates and c NaN where the header says "not written" (t >= len), h_prev zero there.  With
    backward=True, by autograd of sum(y g_y) + sum(h_n g_hn) (either may be None): dgates (dirs, n, t_in, 4h), the gradient
    of gx, and dw, the gradient of each w_hh."""
    return _steps(4, gx, w_hh, None, lens, t_in, t_out, g_y, g_hn, backward)


def gru_steps64(gx, w_hh, b_hh, lens, t_in, t_out, g_y=None, g_hn=None, backward=False):
    """The same for gh_gru_seq_fwd / _bwd: gx (n, t_in, 3h) is x W_ih^T + b_ih alone, b_hh (3h,) per direction.  Saved streams:
    gates (r, z, n), an (a_n, b_hn included), h_prev.  Backward: dgx, the gradient of gx; da, the gradient of a zero probe
    added to a = h W_hh^T + b_hh; dw and db, the gradients of each w_hh and b_hh."""
    return _steps(3, gx, w_hh, b_hh, lens, t_in, t_out, g_y, g_hn, backward)


STEPS = {"lstm": lstm_steps64, "gru": gru_steps64}
FWD_STREAMS = {"lstm": ("y", "h_n", "c_n", "gates", "c", "h_prev"), "gru": ("y", "h_n", "gates", "an", "h_prev")}
BWD_STREAMS = {"lstm": ("dgates",), "gru": ("dgx", "da")}


# ----------------------------------------------------------------------------- the cases of tests/test_gpu_rnn_paths.py
# They live here so that the CPU suite can evaluate the restatement in fp32 at every one of them (tests/test_rnn_cpu.py) and
# check the width table against the kernels' constants (tests/test_rnn_paths_cpu.py).
def P(h, **kw):
    """A case.  n, t_in, t_out (None: t_in), dirs; lens: mixed | dev (0, -3 and t_in + 5 among them) | empty16 (16 live
    sequences, every other one empty); order: sorted | none | identity | skip (sorted, its last two entries -1 and n); pitch:
    ldgx, ldy, ldgy above their rows; mis: gx, y and g_y 4 bytes past a 16-byte boundary; save: the saved pointers given; gy, ghn:
    the gradients given; sat: gx of +-100."""
    d = dict(h=h, n=17, t_in=5, t_out=None, dirs=2, lens="mixed", order="sorted", pitch=False, mis=False, save=True, gy=True,
             ghn=True, sat=False, tag="")
    d.update(kw)
    d["t_out"] = d["t_in"] if d["t_out"] is None else d["t_out"]
    return SimpleNamespace(**d)


def case_name(c):
    return f"h{c.h}" + (f"-{c.tag}" if c.tag else "")


# h -> what the width reaches (rnn_ops.hip; tests/test_rnn_paths_cpu.py derives the classes from the RNN_* constants)
WIDTHS = (1, 5, 6, 30, 16, 17, 32, 33, 129, 255, 256, 257, 258, 300, 511, 513, 768, 1023)
WIDTH_CASES = [P(h, n=3, t_in=3) if h == 1023 else P(h) for h in WIDTHS]


def arg_cases(h):
    return [P(h, pitch=True, tag="pitch"), P(h, mis=True, tag="mis"), P(h, dirs=1, tag="dirs1"),
            P(h, order="none", tag="order-null"), P(h, order="identity", tag="order-identity"), P(h, order="skip", tag="order-skip"),
            P(h, t_in=5, t_out=7, tag="tout+2"), P(h, t_in=6, t_out=4, tag="tout-2"), P(h, lens="dev", tag="devlens"),
            P(h, n=33, lens="empty16", tag="empty-tile"),
            P(h, n=1, tag="n1"), P(h, n=16, tag="n16"), P(h, n=17, tag="n17"), P(h, n=32, tag="n32"), P(h, n=37, tag="n37"),
            P(h, save=False, tag="inference"), P(h, gy=False, tag="gy-null"), P(h, ghn=False, tag="ghn-null"),
            P(h, gy=False, ghn=False, tag="both-null"), P(h, sat=True, tag="saturated")]


ARG_CASES = arg_cases(6) + arg_cases(300)
CHAIN_CASES = [P(6, t_in=7, tag="chain"), P(300, t_in=7, tag="chain"), P(513, t_in=7, tag="chain")]

_INPUTS, _REFS = {}, {}


def _input_key(c):
    return (c.h, c.n, c.t_in, c.t_out, c.lens, c.sat)


def case_inputs(kind, c):
    """The numbers of a case, fp32 on the CPU, both directions whatever c.dirs (one direction takes the first of each): gx per
    direction, w_hh = randn / sqrt(h), b_hh = 0.3 randn, the raw device lengths, g_y, g_hn.  The same for every order, pitch,
    alignment and set of pointers, so that two such cases can be compared bit for bit."""
    k = (kind,) + _input_key(c)
    if k not in _INPUTS:
        G = CELLS[kind].gates
        gen = torch.Generator().manual_seed(1009 * c.h + 31 * c.n + 7 * c.t_in + c.t_out + (G if c.sat else 0))
        rn = lambda *s: torch.randn(*s, generator=gen)
        if c.lens == "empty16":
            lens = [1 + (i * 3) % c.t_in if i < 32 and i % 2 == 0 else 0 for i in range(c.n)]
            lens[0], lens[2] = c.t_in, 1
        else:
            lens = [int(v) for v in torch.randint(1, c.t_in + 1, (c.n,), generator=gen)]
            lens[0] = c.t_in
            if c.n > 1:
                lens[1] = 1
            if c.lens == "dev":
                lens[2], lens[3], lens[4] = 0, -3, c.t_in + 5
        gx = [rn(c.n, c.t_in, G * c.h) for _ in range(2)]
        if c.sat:
            gx = [100.0 * torch.sign(g) for g in gx]
        _INPUTS[k] = dict(gx=gx, w=[rn(G * c.h, c.h) / c.h ** 0.5 for _ in range(2)], b=[0.3 * rn(G * c.h) for _ in range(2)],
                          lens=torch.tensor(lens, dtype=torch.int32), g_y=rn(c.n, c.t_out, 2 * c.h), g_hn=rn(2, c.n, c.h))
    return _INPUTS[k]


def case_reference(kind, c, dtype=torch.float64):
    """The restatement's streams of a case in `dtype`, forward and backward, computed once."""
    k = (kind, dtype, c.dirs, c.gy, c.ghn) + _input_key(c)
    if k not in _REFS:
        inp, d = case_inputs(kind, c), c.dirs
        g_y = inp["g_y"][:, :, :d * c.h] if c.gy else None
        g_hn = inp["g_hn"][:d] if c.ghn else None
        args = [[g.to(dtype) for g in inp["gx"][:d]], inp["w"][:d]] + ([inp["b"][:d]] if kind == "gru" else [])
        _REFS[k] = STEPS[kind](*args, inp["lens"], c.t_in, c.t_out, g_y, g_hn, backward=True)
    return _REFS[k]

"""Float64 restatements, in plain torch and numpy, of what csrc/pair_ops.hip computes (tests only): the references of
tests/test_gpu_pair.py, checked on their own against the upstream reference's goldens by tests/test_pair_cpu.py."""
import numpy as np
import torch


def l2_inner64(a, b):
    """(A2 - 2 a.b) + B2 of a (B,L,D), b (B,R,D) in float64."""
    a, b = a.double(), b.double()
    return ((a * a).sum(-1).unsqueeze(-1) - 2 * (a @ b.transpose(1, 2))) + (b * b).sum(-1).unsqueeze(1)


def pair_l2_64(a, b, eps=1e-10):
    return torch.sqrt(torch.abs(l2_inner64(a, b)) + eps)


def pair_l2_grads64(a, b, g, eps=1e-10):
    """(out, da, db) of sum(out * g) from the closed form: w = g 0.5 / out sign(inner), da = 2 a rowsum(w) - 2 w b."""
    a, b, g = a.double(), b.double(), g.double()
    inner = l2_inner64(a, b)
    out = torch.sqrt(inner.abs() + eps)
    w = g * 0.5 / out * torch.sign(inner)
    da = 2 * a * w.sum(2, keepdim=True) - 2 * (w @ b)
    db = 2 * b * w.sum(1).unsqueeze(-1) - 2 * (w.transpose(1, 2) @ a)
    return out, da, db


def pair_l1_64(a, b):
    return (a.double().unsqueeze(2) - b.double().unsqueeze(1)).abs().sum(-1)


def pair_l1_grads64(a, b, g):
    """(out, da, db): da = sum_r g sign(a - b), db = -sum_l g sign(a - b), sign(0) = 0."""
    a, b, g = a.double(), b.double(), g.double()
    diff = a.unsqueeze(2) - b.unsqueeze(1)
    s = torch.sign(diff) * g.unsqueeze(-1)
    return diff.abs().sum(-1), s.sum(2), -s.sum(1)


def window_out_len(l, w, left=0, right=0):
    return max(l + left + right - w + 1, 0)


def window_mean64(x, w, left=0, right=0, mask=None):
    """x (B,L,D) -> (B,L_out,D): every window summed directly over the zero-padded sequence."""
    x = x.double()
    bn, l, d = x.shape
    lo = window_out_len(l, w, left, right)
    y = torch.zeros((bn, left + l + right, d), dtype=torch.float64)
    y[:, left:left + l] = x
    out = torch.zeros((bn, lo, d), dtype=torch.float64)
    for k in range(w if lo else 0):
        out += y[:, k:k + lo]
    out = out / w
    return out if mask is None else out * mask.double().unsqueeze(-1)


def window_mean_bwd64(g, l, w, left=0, right=0, mask=None):
    """dx (B,L,D) from g (B,L_out,D): row t of the masked g / w goes to the rows t - left .. t - left + w - 1 that exist."""
    g = g.double()
    if mask is not None:
        g = g * mask.double().unsqueeze(-1)
    bn, lo, d = g.shape
    dy = torch.zeros((bn, left + l + right, d), dtype=torch.float64)
    for k in range(w if lo else 0):
        dy[:, k:k + lo] += g / w
    return dy[:, left:left + l]


def hist_scaled64(table, ids_left, ids_right, bins):
    """float64 (Lq, Lr) scaled values (v + 1) / 2 * (bins - 1) of one pair; table (V,D) as the kernel reads it."""
    t = np.asarray(table, dtype=np.float64)
    v = t[np.asarray(ids_left, dtype=np.int64)] @ t[np.asarray(ids_right, dtype=np.int64)].T
    return (v + 1.) / 2. * (bins - 1.)


def hist_bins(scaled, bins):
    """int((v + 1) / 2 (bins - 1)): truncation toward zero, clamped into [0, bins - 1]."""
    return np.clip(np.trunc(np.asarray(scaled, dtype=np.float64)).astype(np.int64), 0, bins - 1)


def hist_counts(bin_idx, bins):
    """(Lq, bins) int64: 1 plus the number of entries of every row that fall into the bin."""
    bin_idx = np.asarray(bin_idx)
    out = np.ones((bin_idx.shape[0], bins), np.int64)
    for i in range(bin_idx.shape[0]):
        out[i] += np.bincount(bin_idx[i].reshape(-1), minlength=bins)[:bins]
    return out


def hist_mode(counts, mode):
    c = np.asarray(counts, dtype=np.float64)
    if mode == "NH":
        return c / c.sum(axis=1, keepdims=True)
    if mode == "LCH":
        return np.log(c)
    assert mode == "CH", mode
    return c


def match_hist64(table, ids_left, ids_right, len_right, bins, mode):
    """(B, Lq, bins) float64 of a batch: right ids at or beyond len_right are ignored."""
    out = []
    for il, ir, n in zip(np.asarray(ids_left), np.asarray(ids_right), np.asarray(len_right)):
        n = int(min(max(int(n), 0), len(ir)))
        out.append(hist_mode(hist_counts(hist_bins(hist_scaled64(table, il, ir[:n], bins), bins), bins), mode))
    return np.stack(out)


def normalize_table64(table):
    t = np.asarray(table, dtype=np.float64)
    return t / np.sqrt((t * t).sum(axis=1))[:, None]

"""Plain restatements of the embedding table gradient (include/get_hip.h, gh_embed_bwd) for the tests:

``embed_bwd_ordered``  the order contract in numpy float32, addition by addition -- chunks of EMBED_CHUNK sorted positions, the
                       rows of a run added one after the other from the run's first row, the partials of a run that spans
                       several chunks combined in chunk order, one addition into the table.  The kernel must give these bits.
``embed_bwd_f64``      the same sums in float64 through np.add.at, in no particular order.
``embed_bwd_bound``    the element-wise fp32 bound of any summation order against the exact sum.
"""
import numpy as np

EMBED_CHUNK = 128          # GH_EMBED_CHUNK; tests/test_embed_cpu.py holds the header and get_amd.ops to it


def _live(t, vocab, padding_idx):
    return 0 <= t < vocab and t != padding_idx


def embed_bwd_ordered(dx, ids, dtable0, padding_idx=-1, chunk=EMBED_CHUNK):
    """dx (m,d) float32, ids (m,) integers, dtable0 (V,d) float32 -> the table after gh_embed_bwd, bit for bit."""
    dx = np.asarray(dx, np.float32)
    ids = np.asarray(ids).astype(np.int64).reshape(-1)
    out = np.array(dtable0, np.float32, copy=True)
    vocab = out.shape[0]
    m = ids.shape[0]
    order = np.argsort(ids, kind="stable")          # ascending (id, row)
    sid = ids[order]
    pos = 0
    while pos < m:
        t = int(sid[pos])
        end = pos
        while end < m and sid[end] == t:
            end += 1
        if _live(t, vocab, padding_idx):
            total = None
            p = pos
            while p < end:
                stop = min(end, (p // chunk + 1) * chunk)
                part = dx[order[p]].copy()                      # a run's sum starts from its first row
                for s in range(p + 1, stop):
                    part = (part + dx[order[s]]).astype(np.float32)
                total = part if total is None else (total + part).astype(np.float32)
                p = stop
            out[t] = (out[t] + total).astype(np.float32)
        pos = end
    return out


def embed_bwd_f64(dx, ids, dtable0, padding_idx=-1):
    """The exact sums (float64): dtable0 + the rows of dx added at their ids; dead ids (outside the table, padding) add nothing."""
    ids = np.asarray(ids).astype(np.int64).reshape(-1)
    out = np.array(dtable0, np.float64, copy=True)
    live = (ids >= 0) & (ids < out.shape[0]) & (ids != padding_idx)
    np.add.at(out, ids[live], np.asarray(dx, np.float64)[live])
    return out


def embed_bwd_bound(dx, ids, dtable0, padding_idx=-1):
    """|result - exact| <= (n_t + 1) 2^-23 (|dtable0[t]| + sum_i |dx_i|), element-wise, n_t = rows with id t.
    Summing n_t + 1 fp32 terms in ANY order of pairwise additions takes n_t roundings, each at most 2^-24 of a partial sum
    that is itself at most sum |terms| (1 + n_t 2^-24): n_t 2^-24 (1 + ..) sum |terms| <= (n_t + 1) 2^-23 sum |terms| for every
    n_t below 2^22.  Derived, not measured; a dropped or doubled row misses it by the size of the row."""
    ids = np.asarray(ids).astype(np.int64).reshape(-1)
    mag = np.abs(np.asarray(dtable0, np.float64))
    live = (ids >= 0) & (ids < mag.shape[0]) & (ids != padding_idx)
    np.add.at(mag, ids[live], np.abs(np.asarray(dx, np.float64))[live])
    n_t = np.bincount(ids[live], minlength=mag.shape[0]).astype(np.float64)
    return (n_t[:, None] + 1.0) * 2.0 ** -23 * mag

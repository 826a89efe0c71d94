"""The width table of tests/test_gpu_rnn_paths.py (tests/rnn_ref.py WIDTHS) against the constants of csrc/rnn_ops.hip.  The
RNN_* constants are read out of the kernel file; from them each width's class follows -- forward loads 16 bytes or single
floats, backward loads 8 bytes or single floats, unit tiles of the forward and live columns of the last one, chunks of the
backward and rows of the last one, live column groups and live units of the last one -- and every class the table's comments
claim must be there.  Whoever changes a constant is told here, without a GPU, which width to add."""
import os
import re

import pytest

from tests.rnn_ref import WIDTH_CASES, WIDTHS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "get_amd", "csrc", "rnn_ops.hip")).read()


def _constants():
    env = {}
    for name, expr in re.findall(r"constexpr int (RNN_\w+) = ([^;]+);", SRC):
        env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))            # integer expressions over earlier constants
    return env


K = _constants()
TILE, GW, CHUNK, MAX_H, WAVES = K["RNN_TILE"], K["RNN_GW"], K["RNN_CHUNK"], K["RNN_MAX_H"], K["RNN_WAVES"]
KSTEP = 4 * K["RNN_BWD_PF"]                                  # k rows of W_hh one block of the backward product fetches


def width_class(h):
    ceil = lambda a, b: -(-a // b)
    tiles, chunks, groups = ceil(h, TILE), ceil(h, CHUNK), ceil(h, GW)
    return dict(fwd_vec=h % 4 == 0, bwd_vec=h % 2 == 0, tiles=tiles, tile_cols=h - TILE * (tiles - 1), chunks=chunks,
                chunk_rows=h - CHUNK * (chunks - 1), groups=groups, group_units=h - GW * (groups - 1))


def test_constants_are_the_ones_the_table_was_written_for():
    """The loaders' vector conditions are not constants: the table relies on h % 4 (forward) and h % 2 (backward)."""
    assert K["RNN_THREADS"] == 64 * WAVES and CHUNK == GW * WAVES and K["RNN_BWD_NP"] * CHUNK == MAX_H
    assert len(re.findall(r"const bool vec = \(h & 3\) == 0;", SRC)) == 2, "the forward kernels' 16-byte condition changed"
    assert len(re.findall(r"const bool vec = \(h & 1\) == 0;", SRC)) == 2, "the backward kernels' 8-byte condition changed"
    assert (TILE, GW, CHUNK, MAX_H, K["RNN_MAX_T"]) == (16, 32, 256, 1024, 4096), \
        "a constant of rnn_ops.hip changed: the refusals of tests/test_gpu_rnn_paths.py name h = 1025 and t_in = 4097"


REQUIRED = [
    ("scalar loads both ways, one unit tile", lambda c: not c["fwd_vec"] and not c["bwd_vec"] and c["tiles"] == 1, 1),
    ("forward scalar, backward 8 bytes", lambda c: not c["fwd_vec"] and c["bwd_vec"], 6),
    ("forward scalar, backward 8 bytes, two unit tiles", lambda c: not c["fwd_vec"] and c["bwd_vec"] and c["tiles"] == 2, GW - 2),
    ("exactly one full unit tile", lambda c: c["tiles"] == 1 and c["tile_cols"] == TILE, TILE),
    ("a second unit tile with one live column", lambda c: c["tiles"] == 2 and c["tile_cols"] == 1, TILE + 1),
    ("the second column group starts at h", lambda c: c["groups"] == 1 and c["group_units"] == GW, GW),
    ("a second column group with one live unit", lambda c: c["groups"] == 2 and c["group_units"] == 1, GW + 1),
    ("more unit tiles than waves, odd", lambda c: c["tiles"] > WAVES and c["chunks"] == 1 and not c["bwd_vec"], CHUNK // 2 + 1),
    ("one chunk, one row short, odd", lambda c: c["chunks"] == 1 and c["chunk_rows"] == CHUNK - 1, CHUNK - 1),
    ("exactly one chunk", lambda c: c["chunks"] == 1 and c["chunk_rows"] == CHUNK, CHUNK),
    ("a second chunk of one row", lambda c: c["chunks"] == 2 and c["chunk_rows"] == 1, CHUNK + 1),
    ("a second chunk of two rows", lambda c: c["chunks"] == 2 and c["chunk_rows"] == 2, CHUNK + 2),
    ("a second chunk that ends inside a block of k steps, 16-byte loads",
     lambda c: c["chunks"] == 2 and c["fwd_vec"] and c["chunk_rows"] % KSTEP not in (0, 1, 2), 300),
    ("a full odd tail", lambda c: c["chunks"] == 2 and c["chunk_rows"] == CHUNK - 1, 2 * CHUNK - 1),
    ("a third chunk of one row", lambda c: c["chunks"] == 3 and c["chunk_rows"] == 1, 2 * CHUNK + 1),
    ("three full chunks", lambda c: c["chunks"] == 3 and c["chunk_rows"] == CHUNK, 3 * CHUNK),
    ("every chunk a wave can own, scalar loads", lambda c: c["chunks"] == MAX_H // CHUNK and not c["bwd_vec"], MAX_H - 1),
]


@pytest.mark.parametrize("what,pred,suggest", REQUIRED, ids=[r[0] for r in REQUIRED])
def test_the_width_table_reaches(what, pred, suggest):
    have = [h for h in WIDTHS if pred(width_class(h))]
    assert have, f"no width of tests/rnn_ref.py WIDTHS reaches '{what}' with today's RNN_* constants: add h = {suggest}"
    assert pred(width_class(suggest)), f"the suggestion {suggest} itself does not reach '{what}'"


def test_every_chunk_count_and_every_width_is_a_case():
    for k in range(1, MAX_H // CHUNK + 1):
        assert any(width_class(h)["chunks"] == k for h in WIDTHS), f"no width with {k} chunks: add h = {k * CHUNK}"
    assert all(1 <= h <= MAX_H for h in WIDTHS) and 300 in WIDTHS
    assert [c.h for c in WIDTH_CASES] == list(WIDTHS) and len(set(WIDTHS)) == len(WIDTHS)
    assert all(c.t_in <= 7 and c.n <= 37 for c in WIDTH_CASES)

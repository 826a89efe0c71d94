"""The pairwise interaction helpers of the reference under their own names, on csrc/pair_ops.hip:

    cosine_distance, l1_distance, moving_average, _get_doc_context_copacrr     torch_utils.py:292-376
    MovingAverage                                                              layers.py:42-66
    MatchingHistogram                                                          matchzoo/preprocessors/units/matching_histogram.py

``torch_utils``, ``layers`` and ``matchzoo.preprocessors.units`` hold far more than these names and the reference's driver
imports them as they are, so ``get_amd.install()`` does not shim those module paths.  ``patch()`` instead sets the drop-ins on
reference modules the caller has already imported.

Quirks of the reference that are kept:
  * ``cosine_distance`` is the Euclidean distance sqrt(|A2 - 2 a.b + B2| + 1e-10).
  * ``moving_average`` and ``MovingAverage`` take the cumulative sum along ``dimension`` but subtract and slice along dim 1
    whatever it says: only ``dimension`` 1 (or -2) on a 3-d tensor is a moving average, anything else is refused here.
  * ``MatchingHistogram`` starts every bin from 1.
One that is not: a zero-norm embedding row with ``normalize=True`` gives NaN in the reference, which then fails in ``int()``
on the first pair that meets it; here the constructor refuses it.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from . import ops


def cosine_distance(a: torch.Tensor, b: torch.Tensor):
    """a (B,L,D), b (B,R,D) -> (B,L,R); torch_utils.py:311-329."""
    assert len(a.size()) == len(b.size()) == 3
    return ops.pair.pair_l2(a, b, 1e-10)


def l1_distance(a: torch.Tensor, b: torch.Tensor):
    """a (B,L,D), b (B,R,D) -> (B,L,R) without the (B,L,R,D) difference tensor; torch_utils.py:332-348."""
    assert len(a.size()) == len(b.size()) == 3
    return ops.pair.pair_l1(a, b)


def _check_dimension(input_tensor, dimension, who):
    if input_tensor.dim() != 3 or dimension not in (1, -2):
        raise ValueError(f"{who}: the reference subtracts and slices along dim 1 whatever `dimension` says, so only dimension 1 "
                         f"(or -2) of a (B,L,D) tensor is a moving average; got dimension {dimension} on a {input_tensor.dim()}-d tensor")


def moving_average(input_tensor: torch.Tensor, window_size: int, dimension: int):
    """(B,L,D) -> (B, L - window_size + 1, D), (B,0,D) where the window is longer than the sequence; torch_utils.py:292-308."""
    _check_dimension(input_tensor, dimension, "moving_average")
    return ops.pair.window_mean(input_tensor, window_size)


def _get_doc_context_copacrr(doc: torch.Tensor, doc_mask: torch.Tensor, context_window_size: int) -> torch.Tensor:
    """doc (B,R,D), doc_mask (B,R) -> (B,R,D): the mean over the window of context_window_size rows around every token (zeros
    beyond the ends), exact zeros at the masked tokens; torch_utils.py:351-376."""
    left = context_window_size // 2
    right = context_window_size - left - 1
    return ops.pair.window_mean(doc, context_window_size, left, right, doc_mask)


class MovingAverage(nn.Module):
    """layers.py:42-66."""

    def __init__(self, window_size: int, dimension: int):
        super(MovingAverage, self).__init__()
        self.window_size = window_size
        self.dimension = dimension

    def forward(self, input_tensor: torch.Tensor):
        _check_dimension(input_tensor, self.dimension, "MovingAverage")
        return ops.pair.window_mean(input_tensor, self.window_size)


class MatchingHistogram:
    """matchzoo/preprocessors/units/matching_histogram.py: the same constructor and ``transform([left, right])`` for one pair,
    and ``transform_batch`` on device tensors in place of data_generator/callbacks/histogram.py's pair-by-pair loop.  The
    table is normalised (in float64, as the reference does) and uploaded once, here."""

    def __init__(self, bin_size: int = 30, embedding_matrix=None, normalize=True, mode: str = 'LCH'):
        if embedding_matrix is None:
            raise ValueError("MatchingHistogram: an embedding matrix (V,D) is required")
        if mode not in ops.pair.HIST_MODES:
            raise ValueError("MatchingHistogram: mode %r is not one of %s" % (mode, list(ops.pair.HIST_MODES)))
        table = embedding_matrix.detach().cpu().numpy() if torch.is_tensor(embedding_matrix) else np.asarray(embedding_matrix)
        if table.ndim != 2 or table.shape[0] < 1 or table.shape[1] < 1:
            raise ValueError(f"MatchingHistogram: an embedding matrix (V,D) is expected, got {table.shape}")
        if not 1 <= int(bin_size) <= ops.pair.HIST_MAX_BINS:
            raise ValueError(f"MatchingHistogram: bin_size {bin_size} is outside 1 .. {ops.pair.HIST_MAX_BINS}")
        table = table.astype(np.float64)
        if normalize:
            l2_norm = np.sqrt((table * table).sum(axis=1))
            if not (l2_norm > 0).all():
                raise ValueError("MatchingHistogram: embedding rows %s have norm 0 and cannot be normalised"
                                 % np.flatnonzero(~(l2_norm > 0))[:8].tolist())
            table = table / l2_norm[:, np.newaxis]
        self._hist_bin_size = int(bin_size)
        self._mode = mode
        self._embedding_matrix = table
        self._device = torch.device("cuda", torch.cuda.current_device())
        self._table = torch.from_numpy(table.astype(np.float32)).to(self._device)

    def transform_batch(self, ids_left, ids_right, len_right):
        """ids_left (B,Lq), ids_right (B,Ld), len_right (B) integers (device tensors, or host arrays, which are uploaded) ->
        (B,Lq,bins) fp32 on the device."""
        up = lambda t: (t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))).to(self._device)
        return ops.pair.match_hist(self._table, None, up(ids_left), up(ids_right), up(len_right), self._hist_bin_size, self._mode)

    def transform(self, input_: list) -> list:
        """[text_left, text_right] of one pair -> the nested list the reference returns."""
        text_left, text_right = input_
        left = torch.as_tensor(np.asarray(text_left, dtype=np.int64).reshape(1, -1))
        right = torch.as_tensor(np.asarray(text_right, dtype=np.int64).reshape(1, -1))
        return self.transform_batch(left, right, torch.tensor([right.shape[1]]))[0].cpu().tolist()


_TORCH_UTILS = {"cosine_distance": cosine_distance, "l1_distance": l1_distance, "moving_average": moving_average,
                "_get_doc_context_copacrr": _get_doc_context_copacrr}


def patch(torch_utils=None, layers=None, units=None):
    """Set the drop-ins on reference modules the caller has already imported: ``torch_utils`` (the four functions), ``layers``
    (MovingAverage), ``units`` (``matchzoo.preprocessors.units``: MatchingHistogram, also on its ``matching_histogram``
    submodule where that is loaded).  Returns the names it replaced, as 'module.attribute'."""
    done = []

    def put(mod, name, obj):
        setattr(mod, name, obj)
        done.append(f"{getattr(mod, '__name__', type(mod).__name__)}.{name}")

    if torch_utils is not None:
        for name, fn in _TORCH_UTILS.items():
            put(torch_utils, name, fn)
    if layers is not None:
        put(layers, "MovingAverage", MovingAverage)
    if units is not None:
        put(units, "MatchingHistogram", MatchingHistogram)
        sub = getattr(units, "matching_histogram", None)
        if sub is not None and hasattr(sub, "MatchingHistogram"):
            put(sub, "MatchingHistogram", MatchingHistogram)
    return done

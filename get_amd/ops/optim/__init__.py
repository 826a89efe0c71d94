"""Front of csrc/optim_ops.hip: the global gradient norm and AdamW under a segment table on a flat bucket
(pytorch_transformers/optimization.py), and the pure-host builders of the block map and the table.

The table changes every step (the schedule and the bias correction move), so it travels through a ring of pinned staging
buffers with an asynchronous copy: a step never synchronises the device and never builds a device tensor from a Python list."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from ..._lib import call, ptr, stream
from ..weights import _bump_trainer_epoch

ADAMW_BLOCK = 64             # GH_ADAMW_BLOCK
MAX_SEGMENTS = 65535         # GH_ADAMW_MAX_SEGMENTS
NORM_CHUNK = 32768           # GH_NORM_CHUNK
SKIP_SEGMENT = 0             # entry 0 of every table the builders make: padding blocks point at it
# gh_adamw_seg of include/get_hip.h
SEG_DTYPE = np.dtype([("step_size", "<f4"), ("lr_wd", "<f4"), ("beta1", "<f4"), ("beta2", "<f4"), ("eps", "<f4"),
                      ("one_minus_beta1", "<f4"), ("one_minus_beta2", "<f4"), ("skip", "<i4")])
assert SEG_DTYPE.itemsize == 32


# ---------------------------------------------------------------------------- pure host
def adamw_block_map(offsets, sizes, total: int) -> np.ndarray:
    """uint16 [total / 64]: the segment of every 64-element block of a bucket whose slot i holds `sizes[i]` elements from
    `offsets[i]` (a multiple of 64) on.  Slot i is segment i + 1, in bucket order; a block no slot touches -- padding between
    slots -- is SKIP_SEGMENT.  The spare elements behind a slot's last element share its last block: they are zero in p, g, m
    and v and stay zero under the update."""
    if total % ADAMW_BLOCK:
        raise ValueError(f"get_amd: a bucket of {total} elements is no whole number of {ADAMW_BLOCK}-element blocks")
    if len(offsets) != len(sizes) or len(sizes) + 1 > MAX_SEGMENTS:
        raise ValueError(f"get_amd: {len(offsets)} offsets for {len(sizes)} slots (at most {MAX_SEGMENTS - 1})")
    out = np.full(total // ADAMW_BLOCK, SKIP_SEGMENT, dtype=np.uint16)
    end = 0
    for i, (off, n) in enumerate(zip(offsets, sizes)):
        off, n = int(off), int(n)
        if off % ADAMW_BLOCK or off < end or n < 0 or off + n > total:
            raise ValueError(f"get_amd: slot {i} (offset {off}, {n} elements) is misaligned, overlaps its predecessor or leaves "
                             f"the bucket of {total}")
        blocks = (n + ADAMW_BLOCK - 1) // ADAMW_BLOCK
        out[off // ADAMW_BLOCK: off // ADAMW_BLOCK + blocks] = i + 1
        end = off + blocks * ADAMW_BLOCK
    return out


def adamw_segment(lr, betas, eps, weight_decay, correct_bias, step):
    """The table entry of one parameter at its `step`-th update (>= 1), computed in double (optimization.py:170-174, :187):
    (step_size, lr_wd, beta1, beta2, eps, 1 - beta1, 1 - beta2, skip = 0)."""
    b1, b2 = float(betas[0]), float(betas[1])
    step_size = float(lr)
    if correct_bias:
        step_size = step_size * math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)
    return (step_size, float(lr) * float(weight_decay), b1, b2, float(eps), 1.0 - b1, 1.0 - b2, 0)


_SKIP_ENTRY = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1)


def adamw_segment_table(hypers, out: np.ndarray = None) -> np.ndarray:
    """SEG_DTYPE [len(hypers) + 1]: entry 0 the skip segment, entry i + 1 = adamw_segment(*hypers[i]), or a skipped one where
    hypers[i] is None (a parameter without a gradient this step).  `out`: the array to fill (a pinned staging buffer)."""
    n = len(hypers) + 1
    if n > MAX_SEGMENTS:
        raise ValueError(f"get_amd: {n} segments, the 16-bit block ids name at most {MAX_SEGMENTS}")
    if out is None:
        out = np.zeros(n, dtype=SEG_DTYPE)
    assert out.dtype == SEG_DTYPE and out.shape == (n,)
    out[0] = _SKIP_ENTRY
    for i, h in enumerate(hypers):
        out[i + 1] = _SKIP_ENTRY if h is None else adamw_segment(*h)
    return out


# ---------------------------------------------------------------------------- device side
def grad_norm_partials(count: int) -> int:
    """How many doubles of scratch gh_flat_grad_norm takes for `count` elements (host arithmetic, no device call)."""
    out = ctypes.c_int64(-1)
    call("gh_flat_grad_norm_partials", int(count), ctypes.addressof(out))
    return out.value


def grad_norm_flat(g: torch.Tensor, grad_scale: float = 1.0, partials: torch.Tensor = None, out: torch.Tensor = None) -> torch.Tensor:
    """grad_scale * ||g||_2 of a flat fp32 gradient as a 0-dim device tensor: no atomics, the same bits on every call, no
    host synchronisation.  partials (float64, >= grad_norm_partials(g.numel())) and out (fp32, one element) are allocated when
    not given."""
    assert g.dtype == torch.float32 and g.dim() == 1, "grad_norm_flat: a flat fp32 gradient"
    need = grad_norm_partials(g.numel())
    if partials is None:
        partials = torch.empty(max(need, 1), device=g.device, dtype=torch.float64)
    if out is None:
        out = torch.empty(1, device=g.device, dtype=torch.float32)
    assert partials.dtype == torch.float64 and out.dtype == torch.float32 and out.numel() == 1
    call("gh_flat_grad_norm", ptr(g), g.numel(), float(grad_scale), ptr(partials), partials.numel(), ptr(out), stream())
    return out.view(())


class SegmentTable:
    """The device copy of a segment table of `n_seg` entries and the ring of pinned staging buffers it is refreshed through.
    upload(hypers) fills the next staging buffer on the host and enqueues one asynchronous copy on the current stream, behind
    the previous step's kernel; the host waits only for the copy that used the same staging buffer `depth` uploads ago."""

    def __init__(self, n_seg: int, device, depth: int = 4):
        self.n_seg = int(n_seg)
        self.dev = torch.zeros(self.n_seg * 8, device=device, dtype=torch.float32)
        self._ring = [torch.zeros(self.n_seg * 8, dtype=torch.float32).pin_memory() for _ in range(depth)]
        self._host = [r.numpy().view(SEG_DTYPE) for r in self._ring]
        self._events = [None] * depth
        self._next = 0

    def upload(self, hypers):
        i = self._next
        self._next = (i + 1) % len(self._ring)
        if self._events[i] is None:
            self._events[i] = torch.cuda.Event()
        else:
            self._events[i].synchronize()
        adamw_segment_table(hypers, out=self._host[i])
        self.dev.copy_(self._ring[i], non_blocking=True)
        self._events[i].record()
        return self.dev


def adamw_step_flat(p, g, m, v, block_seg: torch.Tensor, table: torch.Tensor, grad_scale: float = 1.0, norm: torch.Tensor = None,
                    max_norm: float = None):
    """One AdamW step on flat fp32 buffers in one launch (gh_adamw_step).  block_seg: the device copy of adamw_block_map (two
    bytes per block); table: the device copy of adamw_segment_table (eight 32-bit words per entry); norm: the device scalar
    grad_norm_flat returned, with max_norm, or None for no clipping."""
    assert block_seg.element_size() == 2 and table.element_size() == 4 and table.numel() % 8 == 0
    assert block_seg.numel() * ADAMW_BLOCK == p.numel() == g.numel() == m.numel() == v.numel(), "adamw_step_flat: one id per 64 elements"
    assert (norm is None) == (max_norm is None), "adamw_step_flat: norm and max_norm go together"
    call("gh_adamw_step", ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(block_seg), ptr(table), table.numel() // 8,
         float(grad_scale), ptr(norm), float(max_norm) if max_norm is not None else 0.0, stream())
    _bump_trainer_epoch()


class FlatAdamW:
    """What dist.FlatTrainer and optim.AdamW share: the block map of a bucket on its device, the segment table with its
    staging ring, and the scratch of the norm.  step(hypers) is the optional norm (two launches) and the update (one)."""

    def __init__(self, flat_p, flat_g, flat_m, flat_v, offsets, sizes):
        if not flat_p.is_cuda:
            raise RuntimeError("get_amd: the optimiser step runs on a ROCm device (cuda:N); there is no CPU path")
        self.p, self.g, self.m, self.v = flat_p, flat_g, flat_m, flat_v
        bmap = adamw_block_map(offsets, sizes, flat_p.numel())
        self.block_seg = torch.from_numpy(bmap.view(np.int16)).to(flat_p.device)
        self.table = SegmentTable(len(sizes) + 1, flat_p.device)
        self.partials = torch.empty(max(grad_norm_partials(flat_p.numel()), 1), device=flat_p.device, dtype=torch.float64)
        self.norm = torch.zeros(1, device=flat_p.device, dtype=torch.float32)

    def step(self, hypers, grad_scale: float = 1.0, max_grad_norm: float = None):
        table = self.table.upload(hypers)
        norm = None
        if max_grad_norm is not None:
            norm = grad_norm_flat(self.g, grad_scale, self.partials, self.norm)
        adamw_step_flat(self.p, self.g, self.m, self.v, self.block_seg, table, grad_scale, norm, max_grad_norm)
        return norm

"""The auxiliary HIP stream of each device and the bookkeeping that joins it back at the end of a backward pass.  The three
flags are read at call time as ``streams.X`` and are NOT re-exported by the package: who patches them patches this module."""
import os

import torch

from .. import _lib

# GET_AMD_CLAIM_STREAM=0 keeps the claim branch on the caller's stream (modules.Graph_basedSemantiStructure.forward)
CLAIM_SIDE_STREAM = os.environ.get("GET_AMD_CLAIM_STREAM", "1") != "0"
# Weight gradients of the few-row layers (evidence-level attention, head) leave the critical path of backward: with a
# FlatTrainer (gradients accumulate straight into the flat bucket) they are issued on the auxiliary stream and joined
# at the end of the backward pass (and before any all-reduce).  GET_AMD_WGRAD_STREAM=0 keeps them in line.
WGRAD_SIDE_STREAM = os.environ.get("GET_AMD_WGRAD_STREAM", "1") != "0"
WGRAD_FEW_ROWS = 4096
_SIDE_STREAMS: dict = {}
_side_pending: set = set()


def _index(device) -> int:
    dev = torch.device(device)
    return dev.index if dev.index is not None else torch.cuda.current_device()


def side_stream(device) -> "torch.cuda.Stream":
    """One auxiliary HIP stream per device for work that is independent of the main chain of launches."""
    idx = _index(device)
    s = _SIDE_STREAMS.get(idx)
    if s is None:
        s = torch.cuda.Stream(device=idx)
        _SIDE_STREAMS[idx] = s
    return s


def side_join():
    """Make the current stream wait for everything issued on the auxiliary stream so far (no-op when nothing is)."""
    for idx in list(_side_pending):
        torch.cuda.current_stream(idx).wait_stream(_SIDE_STREAMS[idx])
        _side_pending.discard(idx)


def pending_side_stream():
    """The auxiliary stream of the current device if work of the running backward pass is pending on it, else None."""
    idx = torch.cuda.current_device() if torch.cuda.is_available() else None
    return _SIDE_STREAMS.get(idx) if idx in _side_pending else None


def _mark_pending(idx: int, join: bool):
    """Work of the running backward pass is on the auxiliary stream of device `idx`: pending_side_stream() now reports it,
    and with `join` side_join is queued for the end of the pass -- once, however many callers mark the device."""
    if idx not in _side_pending:
        _side_pending.add(idx)
        if join:
            torch.autograd.Variable._execution_engine.queue_callback(side_join)


def side_mark_backward(device):
    """Called from inside a backward pass when work of that pass runs (or is about to run) on the auxiliary stream -- the
    claim branch's backward, which autograd replays on its forward stream: marks the device pending and queues the join
    for the end of the pass.  With a FlatTrainer the branch's backward returns no gradients to autograd (they land in
    the flat bucket directly), so the engine itself never learns about the side stream and would not join it."""
    idx = _index(device)
    if idx in _SIDE_STREAMS:
        _mark_pending(idx, True)


def _side_wgrad(dev, tensors, launch):
    """Run `launch()` (weight-gradient launches only) on the auxiliary stream after the current stream's work;
    `tensors` are the operands it reads.  The join is queued for the end of the running backward pass."""
    idx = _index(dev)
    side = side_stream(dev)
    main = torch.cuda.current_stream(idx)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        _lib.ensure_workspace(dev)
        launch()
    for t in tensors:
        if t is not None:
            t.record_stream(side)
    _mark_pending(idx, True)

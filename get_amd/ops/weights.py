"""What is derived from the weights and kept across steps: k-major transposes, bf16 twins, small packed values.

ONE validity rule (`_valid`): an entry holds while each tensor it was made from is the same object (weak reference) at the
same `data_ptr()` and in-place `_version`, and the weight epoch has not moved on -- a frozen entry ignores the epoch.  Never
by address or `id` alone: both are recycled.  A raw `w.data += 1` moves none of these, hence `bump_weight_epoch`."""
import ctypes
import weakref
from collections import namedtuple

import torch

from .. import _lib
from .._lib import call, ptr, stream
from ._util import _f32

_WEIGHT_EPOCH = 0
_FROZEN = -1                 # stands in for the epoch of an entry whose sources no optimiser touches
# srcs: (weak reference, data_ptr, _version) of every source tensor when `value` was made; epoch: the weight epoch then
_Entry = namedtuple("_Entry", "srcs epoch value")
_WT_CACHE: dict = {}         # id(w) -> _Entry of Wt
_BF16_CACHE: dict = {}       # id(w) -> _Entry of (bf16 W, bf16 Wt)
_DERIVED_CACHE: dict = {}    # (tag, id(t), ...) -> _Entry of what fn() returned
# persistent buffers, one set per parameter object, rewritten in place: their addresses are part of the composite entry
# points' cached descriptor (get_amd/fused.py) and the key of the library's pre-split images (gemm mode "fp32x3p")
_WT_PERSIST: dict = {}       # id(w) -> _Entry of (Wt,), its source the weak reference alone, no epoch
_BF16_PERSIST: dict = {}     # id(w) -> _Entry of (bf16 W, bf16 Wt), likewise
_X3P_SIG: dict = {}          # id(module) -> _Entry of the signature of the module's parameters, likewise


def _entry(tensors, epoch, value):
    return _Entry(tuple((weakref.ref(t), t.data_ptr(), t._version) for t in tensors), epoch, value)


def _valid(e, tensors, epoch) -> bool:
    """Is `e` still the value of `tensors` at `epoch` (the current weight epoch, or _FROZEN)?"""
    if e.epoch != epoch:
        return False
    i = 0
    for ref, dptr, version in e.srcs:      # (no zip, no generator: this runs once per linear forward)
        t = tensors[i]
        i += 1
        if ref() is not t or dptr != t.data_ptr() or version != t._version:
            return False
    return True


def _sweep(table: dict):
    """Every table, before it grows past 512 entries: drop those whose source objects are gone.  A dead
    entry can never hit, it only holds memory and an id that will be recycled."""
    if len(table) > 512:
        for k in [k for k, v in table.items() if any(src[0]() is None for src in v.srcs)]:
            del table[k]


def _persistent(table: dict, w: torch.Tensor, twin: bool = False):
    """The persistent buffers of parameter `w`: (Wt,) in fp32, or with `twin` (W, Wt) in bf16.  Reused while the parameter is
    the same object of the same shape on the same device."""
    hit = table.get(id(w))
    tshape = (w.shape[1], w.shape[0])
    if hit is None or hit.srcs[0][0]() is not w or hit.value[-1].shape != tshape or hit.value[-1].device != w.device:
        _sweep(table)
        shapes, dtype = ((tuple(w.shape), tshape), torch.bfloat16) if twin else ((tshape,), torch.float32)
        bufs = tuple(torch.empty(s, device=w.device, dtype=dtype) for s in shapes)
        hit = table[id(w)] = _Entry(((weakref.ref(w),),), None, bufs)
    return hit.value


# ---- the two doors to the library (a CPU test replaces them with torch stand-ins)
def _transpose(ws, wts, twins=None):
    """wts[i] <- ws[i]^T on the current stream.  twins None: one matrix on its own (gh_transpose); else ONE launch for all
    of them, in which the (bf16 W, bf16 Wt) buffers twins[i] are filled too where they are not None."""
    if twins is None:
        return call("gh_transpose", ptr(ws[0]), ptr(wts[0]), ws[0].shape[0], ws[0].shape[1], stream())
    n = len(ws)
    arr = lambda ctype, vals: ctypes.cast((ctype * n)(*vals), ctypes.c_void_p)
    ptrs = lambda ts: arr(ctypes.c_void_p, [t.data_ptr() if t is not None else None for t in ts])
    rows, cols = (arr(ctypes.c_int, [w.shape[i] for w in ws]) for i in (0, 1))
    if any(t is not None for t in twins):
        w16, t16 = ([t[i] if t is not None else None for t in twins] for i in (0, 1))
        call("gh_weights_refresh", n, ptrs(ws), ptrs(wts), ptrs(w16), ptrs(t16), rows, cols, stream())
    else:
        call("gh_transpose_batch", n, ptrs(ws), ptrs(wts), rows, cols, stream())


def _notify(name: str):
    """The library's pre-split weight images (gemm mode "fp32x3p"): gh_weights_changed marks every image stale (re-made by
    the launch that meets it), gh_fp32x3_refresh re-makes the stale ones now in one launch, gh_fp32x3_clear drops them."""
    call(name, *((stream(),) if name == "gh_fp32x3_refresh" else ()))


def bump_weight_epoch():
    """Invalidate EVERY cached derivative of the weights (transposes, bias sums, packed scalar gates, bf16 twins).  The
    public invalidation API: call it after writing parameters through `.data` / raw pointers (EMA swaps, hand-written
    optimisers) -- such writes do not bump `_version`, so nothing else can notice them."""
    global _WEIGHT_EPOCH
    _WEIGHT_EPOCH += 1
    _WT_CACHE.clear()
    _BF16_CACHE.clear()
    _DERIVED_CACHE.clear()
    if _lib.gemm_mode() == "fp32x3p":       # the library's pre-split weight images: drop them (weights may have been replaced)
        _notify("gh_fp32x3_clear")


def _bump_trainer_epoch():
    """FlatTrainer.step's own invalidation: the fused optimiser rewrites exactly the parameters of its bucket, so entries
    derived from tensors OUTSIDE the bucket (`frozen`: the never-trained GSL scorer's packed gates, the bf16 twin of a
    frozen embedding table) stay valid."""
    global _WEIGHT_EPOCH
    _WEIGHT_EPOCH += 1
    _WT_CACHE.clear()
    _BF16_CACHE.clear()
    for k in [k for k, e in _DERIVED_CACHE.items() if e.epoch != _FROZEN]:
        del _DERIVED_CACHE[k]
    if _lib.gemm_mode() == "fp32x3p":       # every image stale; refresh_transposes re-makes them all in one launch
        _notify("gh_weights_changed")


def fp32x3p_guard(module):
    """gemm mode "fp32x3p" only: the library reads the weight operand of its activation-sized GEMMs from pre-split images
    and cannot see in-place updates by a torch optimiser.  Called at the top of the model's forward: when any parameter's
    `_version` or address moved since the last call, every image is marked stale (re-made by the launch that meets it).
    FlatTrainer rewrites parameters through raw pointers and tells the library itself (_bump_trainer_epoch)."""
    sig = 0
    for q in module.parameters():
        sig = (sig * 1000003 + q._version * 31 + q.data_ptr()) & 0xFFFFFFFFFFFF
    hit = _X3P_SIG.get(id(module))
    if hit is None or hit.srcs[0][0]() is not module or hit.value != sig:
        _sweep(_X3P_SIG)
        _X3P_SIG[id(module)] = _Entry(((weakref.ref(module),),), None, sig)
        _notify("gh_weights_changed")


def _direct(p) -> bool:
    """True when gradients of `p` may be accumulated by the kernels straight into `p.grad` (a live view of the trainer's flat
    bucket, see dist.FlatTrainer) instead of being returned to autograd, which would add them there with one extra elementwise
    kernel per parameter."""
    if not getattr(p, "_gh_direct_grad", False):      # (first: a non-leaf view of a weight has no .grad to ask for)
        return False
    g = getattr(p, "grad", None)
    return g is not None and g.dtype == torch.float32 and g.is_contiguous() and g.shape == p.shape


def transposed(w: torch.Tensor) -> torch.Tensor:
    """W[n_out][n_in] -> Wt[n_in][n_out], cached per parameter OBJECT (weak reference), storage address, in-place version
    and weight epoch -- never by address alone, which the caching allocator recycles."""
    hit = _WT_CACHE.get(id(w))
    if hit is not None and _valid(hit, (w,), _WEIGHT_EPOCH):
        return hit.value
    wc = _f32(w.detach())
    if _lib.gemm_mode() == "fp32x3p":
        # the library keys its pre-split images by operand address: keep the k-major copy in the parameter's persistent
        # buffer (as refresh_transposes does) so that the address stays, and mark the images stale
        wt, = _persistent(_WT_PERSIST, w)
        _notify("gh_weights_changed")
    else:
        wt = torch.empty((wc.shape[1], wc.shape[0]), device=w.device, dtype=torch.float32)
    _transpose([wc], [wt])
    _sweep(_WT_CACHE)
    _WT_CACHE[id(w)] = _entry((w,), _WEIGHT_EPOCH, wt)
    return wt


def bf16_twins(w: torch.Tensor):
    """(bf16(W) [n_out][n_in], bf16(W^T) [n_in][n_out]) of a weight matrix, cached per parameter object / storage address /
    in-place version / weight epoch; re-made together with the fp32 transpose in ONE launch (gh_weights_refresh), by
    refresh_transposes after the optimiser step or here on a miss."""
    hit = _BF16_CACHE.get(id(w))
    if hit is not None and _valid(hit, (w,), _WEIGHT_EPOCH):
        return hit.value
    _persistent(_BF16_PERSIST, w, twin=True)
    refresh_transposes([w])
    return _BF16_CACHE[id(w)].value


def derived(tag: str, tensors, fn, frozen: bool = False):
    """Small per-parameter-set cache for values derived from weights (bias sums, packed scalar gates): recomputed only
    when one of the source tensors was replaced, modified in place (``_version``) or the weight epoch moved on (the
    fused optimiser updates parameters through raw pointers).  Saves a dozen tiny elementwise launches per step."""
    key = (tag,) + tuple(id(t) for t in tensors)
    # frozen: the sources are never touched by the optimiser (requires_grad False), so the weight epoch does not matter
    epoch = _FROZEN if frozen else _WEIGHT_EPOCH
    hit = _DERIVED_CACHE.get(key)
    if hit is not None and _valid(hit, tensors, epoch):
        return hit.value
    with torch.no_grad():
        val = fn()
    _sweep(_DERIVED_CACHE)
    _DERIVED_CACHE[key] = _entry(tensors, epoch, val)
    return val


def refresh_transposes(weights):
    """Transpose many weight matrices in ONE launch and prime the cache (called by the trainer right
    after the optimiser step, so the next forward finds every k-major operand ready)."""
    ws = [w for w in weights if w.dim() == 2]
    if not ws:
        return
    wts = [_persistent(_WT_PERSIST, w)[0] for w in ws]
    # bf16 twins ride in the same launch for every matrix that has them (i.e. that a bf16-storage cell has asked for)
    twins = [_BF16_PERSIST.get(id(w)) for w in ws]
    twins = [t.value if (t is not None and t.srcs[0][0]() is w and t.value[0].device == w.device) else None for t, w in zip(twins, ws)]
    _transpose(ws, wts, twins)
    if _lib.gemm_mode() == "fp32x3p":
        _notify("gh_fp32x3_refresh")
    _sweep(_WT_CACHE)
    _sweep(_BF16_CACHE)
    for w, wt, t in zip(ws, wts, twins):
        _WT_CACHE[id(w)] = _entry((w,), _WEIGHT_EPOCH, wt)
        if t is not None:
            _BF16_CACHE[id(w)] = _entry((w,), _WEIGHT_EPOCH, t)

"""The BERT fine-tuning optimiser as drop-ins for pytorch_transformers/optimization.py: ``AdamW`` and the five ``LambdaLR``
schedules, with global-norm gradient clipping folded into the update.

``AdamW`` owns one flat fp32 bucket laid out like dist.FlatTrainer's (``param.data`` and ``param.grad`` are views into it), so
a step is at most three launches whatever the number of parameters: the gradient norm (two, only with ``max_grad_norm``) and
``gh_adamw_step``, which reads every parameter's hyperparameters from a small table (csrc/optim_ops.hip).  The reference's
step issues about eight elementwise launches per parameter, and ``clip_grad_norm_`` one norm per parameter and a host read.

Difference from ``torch.nn.utils.clip_grad_norm_``: the gradients are not rescaled in memory; the clip coefficient is applied
inside the update, and the norm comes back as a 0-dim device tensor that nothing reads on the host.
"""
from __future__ import annotations

import math

import torch
from torch.optim import Optimizer
from torch.optim.lr_scheduler import LambdaLR

from . import ops
from .dist import build_flat_bucket, forward_matrices

__all__ = ["AdamW", "ConstantLRSchedule", "WarmupConstantSchedule", "WarmupLinearSchedule", "WarmupCosineSchedule",
           "WarmupCosineWithHardRestartsSchedule", "constant_schedule", "warmup_constant_schedule", "warmup_linear_schedule",
           "warmup_cosine_schedule", "warmup_cosine_hard_restarts_schedule"]


# ---------------------------------------------------------------------------- schedules: the factor on the base lr at `step`
def _warmup(step, warmup_steps):
    return float(step) / float(max(1, warmup_steps))


def _progress(step, warmup_steps, t_total):
    return float(step - warmup_steps) / float(max(1, t_total - warmup_steps))


def constant_schedule(step, warmup_steps=0, t_total=0, cycles=0.0):
    """1 at every step (optimization.py:26-30)."""
    return 1.0


def warmup_constant_schedule(step, warmup_steps=0, t_total=0, cycles=0.0):
    """step / warmup_steps below warmup_steps, then 1 (optimization.py:33-45)."""
    return _warmup(step, warmup_steps) if step < warmup_steps else 1.0


def warmup_linear_schedule(step, warmup_steps=0, t_total=0, cycles=0.0):
    """The same warmup, then a straight line from 1 at warmup_steps to 0 at t_total, 0 beyond (optimization.py:48-61)."""
    if step < warmup_steps:
        return _warmup(step, warmup_steps)
    return max(0.0, float(t_total - step) / float(max(1, t_total - warmup_steps)))


def warmup_cosine_schedule(step, warmup_steps=0, t_total=0, cycles=0.5):
    """The same warmup, then (1 + cos(2 pi cycles x)) / 2 over the progress x from warmup_steps to t_total: half a cosine wave
    from 1 to 0 at the default cycles = 0.5 (optimization.py:64-81)."""
    if step < warmup_steps:
        return _warmup(step, warmup_steps)
    x = _progress(step, warmup_steps, t_total)
    return max(0.0, 0.5 * (1.0 + math.cos(2.0 * math.pi * float(cycles) * x)))


def warmup_cosine_hard_restarts_schedule(step, warmup_steps=0, t_total=0, cycles=1.0):
    """The same warmup, then `cycles` half cosine waves from 1 to 0, each restarting at 1; 0 from t_total on
    (optimization.py:84-103)."""
    if step < warmup_steps:
        return _warmup(step, warmup_steps)
    x = _progress(step, warmup_steps, t_total)
    if x >= 1.0:
        return 0.0
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((float(cycles) * x) % 1.0))))


class _Schedule(LambdaLR):
    _fn = staticmethod(constant_schedule)
    warmup_steps, t_total, cycles = 0, 0, 0.0

    def lr_lambda(self, step):
        return type(self)._fn(step, self.warmup_steps, self.t_total, self.cycles)


class ConstantLRSchedule(_Schedule):
    def __init__(self, optimizer, last_epoch=-1):
        super().__init__(optimizer, self.lr_lambda, last_epoch=last_epoch)


class WarmupConstantSchedule(_Schedule):
    _fn = staticmethod(warmup_constant_schedule)

    def __init__(self, optimizer, warmup_steps, last_epoch=-1):
        self.warmup_steps = warmup_steps
        super().__init__(optimizer, self.lr_lambda, last_epoch=last_epoch)


class WarmupLinearSchedule(_Schedule):
    _fn = staticmethod(warmup_linear_schedule)

    def __init__(self, optimizer, warmup_steps, t_total, last_epoch=-1):
        self.warmup_steps, self.t_total = warmup_steps, t_total
        super().__init__(optimizer, self.lr_lambda, last_epoch=last_epoch)


class WarmupCosineSchedule(_Schedule):
    _fn = staticmethod(warmup_cosine_schedule)

    def __init__(self, optimizer, warmup_steps, t_total, cycles=.5, last_epoch=-1):
        self.warmup_steps, self.t_total, self.cycles = warmup_steps, t_total, cycles
        super().__init__(optimizer, self.lr_lambda, last_epoch=last_epoch)


class WarmupCosineWithHardRestartsSchedule(_Schedule):
    _fn = staticmethod(warmup_cosine_hard_restarts_schedule)

    def __init__(self, optimizer, warmup_steps, t_total, cycles=1., last_epoch=-1):
        self.warmup_steps, self.t_total, self.cycles = warmup_steps, t_total, cycles
        super().__init__(optimizer, self.lr_lambda, last_epoch=last_epoch)


# ---------------------------------------------------------------------------- AdamW
class AdamW(Optimizer):
    """Adam with decoupled weight decay as optimization.py:107-189 defines it: eps outside the bias correction, which
    ``correct_bias=False`` switches off (the BERT way), and the decay applied to the updated parameter with the group's lr.
    ``params`` and ``param_groups`` as for any torch optimiser, so a ``LambdaLR`` drives the groups' ``lr``.

    max_grad_norm: clip the global gradient norm to this value inside the update (see the module docstring); step() then
    returns the norm as a 0-dim device tensor.  model: the module the parameters belong to, so that its embedding tables
    are told apart from the matrices whose transposes the forward consumes (without it every matrix is refreshed).

    A parameter whose ``.grad`` is None at step() is skipped and its step count does not advance (:143-144).  A ``.grad``
    that is not the bucket's view (autograd made a new tensor after ``.grad`` was None) is copied into the view, and the
    view is attached again.

    Where this differs from the reference's rule: the constructor attaches a zero gradient view to every parameter of the
    bucket, so a parameter that no backward pass ever reaches (BERT's pooler when only ``sequence_output`` is used) has a
    ``.grad`` that is not None: it is updated with a zero gradient -- its step count advances and its weight decay applies --
    until its ``.grad`` is set to None (``zero_grad(set_to_none=True)`` or ``model.zero_grad()`` before the backward pass restore
    the reference's behaviour).  A parameter with ``requires_grad=False`` at construction is left out of the bucket and never
    updated.  ``add_param_group`` after construction is refused: the bucket is laid out once."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True, max_grad_norm=None,
                 model: torch.nn.Module = None):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[1]))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(eps))
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError("Invalid max_grad_norm: {} - should be > 0.0 or None".format(max_grad_norm))
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias))
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm = None          # 0-dim device tensor of the last clipped step, as FlatTrainer keeps it
        # a parameter that does not require a gradient stays out of the bucket, as in FlatTrainer: it is never updated
        self._params = [p for group in self.param_groups for p in group["params"] if p.requires_grad]
        if not self._params:
            raise ValueError("get_amd: AdamW got no parameter that requires a gradient")
        for p in self._params:
            if p.dtype != torch.float32 or p.device != self._params[0].device:
                raise ValueError("get_amd: AdamW takes fp32 parameters on one device")
        self.flat_p, self.flat_g, self.flat_m, self.flat_v, self._views, self._offsets = build_flat_bucket(self._params)
        self._moments = [(self.flat_m[off:off + p.numel()].view_as(p), self.flat_v[off:off + p.numel()].view_as(p))
                         for p, off in zip(self._params, self._offsets)]
        self._matrices = forward_matrices(model, self._params)
        self._slot = {id(p): i for i, p in enumerate(self._params)}
        self._flat_step = None
        self._built = True

    def add_param_group(self, param_group):
        """Only while the constructor runs: the bucket is laid out once, over the groups given there."""
        if getattr(self, "_built", False):
            raise RuntimeError("get_amd: AdamW lays its flat bucket out at construction; build a new optimiser over all the groups "
                               "instead of add_param_group()")
        super().add_param_group(param_group)

    def _state_of(self, i):
        """The reference's per-parameter state (:152-157), its moments being views of the bucket."""
        st = self.state[self._params[i]]
        if len(st) == 0:
            st["step"] = 0
            st["exp_avg"], st["exp_avg_sq"] = self._moments[i]
        return st

    @torch.no_grad()
    def step(self, closure=None):
        """One update of every parameter that has a gradient.  Returns the gradient norm (0-dim device tensor, also kept in
        ``last_grad_norm``) when max_grad_norm is set, else the closure's loss (None without a closure), as the reference does."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._flat_step is None:
            self._flat_step = ops.FlatAdamW(self.flat_p, self.flat_g, self.flat_m, self.flat_v, self._offsets,
                                            [p.numel() for p in self._params])
        hypers = [None] * len(self._params)
        for group in self.param_groups:
            for p in group["params"]:
                i = self._slot.get(id(p))
                if i is None:                    # requires_grad was False at construction: not in the bucket
                    continue
                gv = self._views[i]
                if p.grad is None:
                    if self.max_grad_norm is not None:
                        gv.zero_()               # a stale gradient must not count in the norm
                else:
                    if p.grad.data_ptr() != gv.data_ptr():
                        if p.grad.is_sparse:
                            raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                        gv.copy_(p.grad)
                        p.grad = gv
                    st = self._state_of(i)
                    st["step"] += 1
                    hypers[i] = (group["lr"], tuple(group["betas"]), group["eps"], group["weight_decay"], group["correct_bias"],
                                 st["step"])
        norm = self.last_grad_norm = self._flat_step.step(hypers, grad_scale=1.0, max_grad_norm=self.max_grad_norm)
        ops.refresh_transposes(self._matrices)     # k-major copies for the next forward, one launch
        return norm if self.max_grad_norm is not None else loss

    def zero_grad(self, set_to_none: bool = False):
        """One memset of the flat gradient; the views stay attached (set_to_none=True detaches them instead: the next step
        then skips every parameter that has received no gradient since)."""
        if set_to_none:
            for p in self._params:
                p.grad = None
            return
        self.flat_g.zero_()
        for p, gv in zip(self._params, self._views):
            if p.grad is None or p.grad.data_ptr() != gv.data_ptr():
                p.grad = gv

    def state_dict(self):
        """torch's layout with the reference's state keys (step, exp_avg, exp_avg_sq per parameter); the moments are copies."""
        sd = super().state_dict()
        sd["state"] = {k: {n: (t.detach().clone() if torch.is_tensor(t) else t) for n, t in st.items()} for k, st in sd["state"].items()}
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """Copies the loaded moments into the bucket: the views stay attached."""
        super().load_state_dict(state_dict)
        for i, p in enumerate(self._params):
            m, v = self._moments[i]
            st = self.state.get(p)
            if st:
                m.copy_(st["exp_avg"])
                v.copy_(st["exp_avg_sq"])
                st["exp_avg"], st["exp_avg_sq"] = m, v
                st["step"] = int(st["step"])
            else:
                m.zero_()
                v.zero_()

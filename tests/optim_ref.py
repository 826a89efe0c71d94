"""float64 numpy restatement of the BERT fine-tuning optimiser (tests only): the AdamW update, the clip coefficient of
clip_grad_norm_, the five schedules, and a small driver that runs a whole recipe (groups, schedule, clipping, parameters
without a gradient); and the two kernels' own arithmetic in fp32, operation by operation in the order include/get_hip.h fixes,
which says what bits they must give.  Checked on its own against the reference's golden vectors by tests/test_optim_cpu.py; the reference of
tests/test_gpu_optim.py and tests/test_gpu_optim_paths.py."""
import math

import numpy as np


# ---------------------------------------------------------------------------- schedules
def schedule(name, step, warmup_steps=0, t_total=0, cycles=None):
    """The factor on the base learning rate at `step` for the schedule class `name`."""
    if name == "ConstantLRSchedule":
        return 1.0
    if step < warmup_steps:
        return step / max(1, warmup_steps)
    if name == "WarmupConstantSchedule":
        return 1.0
    rest = max(1, t_total - warmup_steps)
    if name == "WarmupLinearSchedule":
        return max(0.0, (t_total - step) / rest)
    x = (step - warmup_steps) / rest
    if name == "WarmupCosineSchedule":
        c = 0.5 if cycles is None else cycles
        return max(0.0, (1.0 + math.cos(2.0 * math.pi * c * x)) / 2.0)
    if name == "WarmupCosineWithHardRestartsSchedule":
        c = 1.0 if cycles is None else cycles
        if x >= 1.0:
            return 0.0
        return max(0.0, (1.0 + math.cos(math.pi * math.fmod(c * x, 1.0))) / 2.0)
    raise KeyError(name)


# ---------------------------------------------------------------------------- clipping
def global_norm(grads):
    """sqrt of the sum of the squares of every element of every gradient, in float64."""
    return math.sqrt(sum(float((np.asarray(g, dtype=np.float64) ** 2).sum()) for g in grads))


def clip_coef(norm, max_norm, one_at_or_below=False):
    """min(1, max_norm / (norm + 1e-6)), clip_grad_norm_'s coefficient.  one_at_or_below: exactly 1 whenever norm <= max_norm,
    the rule of gh_adamw_step (the two differ by at most 1e-6 / max_norm, for norms within 1e-6 of max_norm)."""
    if one_at_or_below and norm <= max_norm:
        return 1.0
    return min(1.0, max_norm / (norm + 1e-6))


# ---------------------------------------------------------------------------- the update
def adamw_update(p, g, m, v, lr, betas, eps, weight_decay, correct_bias, step, clip=1.0, grad_scale=1.0):
    """One AdamW update of one parameter at its `step`-th update (>= 1) -> (p, m, v), float64."""
    p, g, m, v = (np.asarray(t, dtype=np.float64) for t in (p, g, m, v))
    b1, b2 = betas
    gr = g * grad_scale * clip
    m = b1 * m + (1.0 - b1) * gr
    v = b2 * v + (1.0 - b2) * gr * gr
    step_size = lr
    if correct_bias:
        step_size = lr * math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)
    p = p - step_size * m / (np.sqrt(v) + eps)
    if weight_decay > 0.0:
        p = p - lr * weight_decay * p
    return p, m, v


# ---------------------------------------------------------------------------- the kernels' own arithmetic, in fp32
def adamw_update_f32(p, g, m, v, entry, grad_scale=1.0, clip=1.0):
    """gh_adamw_step's update of the elements of one segment, operation by operation in fp32 as include/get_hip.h states it
    (numpy rounds every float32 operation once; its sqrt and division are correctly rounded) -> (p, m, v) with the bits the
    kernel must give.  entry: the segment's row of ops.adamw_segment_table (fp32 fields); clip: the fp32 coefficient."""
    f = np.float32
    p, g, m, v = (np.asarray(t, dtype=f) for t in (p, g, m, v))
    e = {k: f(entry[k]) for k in ("step_size", "lr_wd", "beta1", "beta2", "eps", "one_minus_beta1", "one_minus_beta2")}
    gr = (g * f(grad_scale)) * f(clip)
    m = e["beta1"] * m + e["one_minus_beta1"] * gr
    v = e["beta2"] * v + (e["one_minus_beta2"] * gr) * gr
    denom = np.sqrt(v) + e["eps"]
    p1 = p - (e["step_size"] * m) / denom
    p = p1 - e["lr_wd"] * p1 if e["lr_wd"] > 0 else p1
    assert p.dtype == m.dtype == v.dtype == f
    return p, m, v


def clip_coef_f32(norm, max_norm):
    """The coefficient gh_adamw_step forms from the fp32 norm: exactly 1 at or below max_norm."""
    f = np.float32
    norm, max_norm = f(norm), f(max_norm)
    return f(1.0) if norm <= max_norm else min(f(1.0), max_norm / (norm + f(1e-6)))


def flat_grad_norm_f32(g, grad_scale=1.0, chunk=32768, lanes=256):
    """gh_flat_grad_norm in the order include/get_hip.h fixes -> the fp32 value whose bits the kernel must give.  Padding the
    gradient with zeros up to whole chunks changes nothing: a lane sum is >= +0 and x + 0 * 0 = x."""
    f = np.float32
    g = np.asarray(g, dtype=f)
    n_chunks = (g.size + chunk - 1) // chunk
    x = np.zeros(n_chunks * chunk, dtype=f)
    x[:g.size] = g
    x = x.reshape(n_chunks, chunk // (4 * lanes), lanes, 4)
    acc = np.zeros((n_chunks, lanes), dtype=f)
    for r in range(x.shape[1]):                    # a lane's float4s in address order, their four squares in order
        for k in range(4):
            acc = acc + x[:, r, :, k] * x[:, r, :, k]
    s = acc.astype(np.float64).reshape(n_chunks, lanes // 64, 64)
    width = 64
    while width > 1:                               # the butterfly (xor 32, 16, .. 1): fold the upper half onto the lower
        width //= 2
        s = s[..., :width] + s[..., width:2 * width]
    w = s[..., 0]
    partials = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    per = (n_chunks + lanes - 1) // lanes if n_chunks else 0
    total = 0.0
    for t in range(lanes):                         # 256 contiguous runs in index order, then the runs in order
        run = 0.0
        for q in partials[t * per:(t + 1) * per]:
            run += float(q)
        total += run
    return f(float(f(grad_scale)) * math.sqrt(total))      # the scale arrives as fp32; product and root in double, rounded once


class Recipe:
    """A whole recipe in float64: parameters in groups (group_of[i] = index into `groups`, each a dict of lr, betas, eps,
    weight_decay, correct_bias), an optional schedule (name, kwargs) scaling every group's lr by schedule(completed steps), an
    optional max_norm.  step(grads) takes one gradient per parameter, None for a parameter that is skipped."""

    def __init__(self, params, group_of, groups, sched=None, max_norm=None, one_at_or_below=False):
        self.p = [np.asarray(t, dtype=np.float64).copy() for t in params]
        self.m = [np.zeros_like(t) for t in self.p]
        self.v = [np.zeros_like(t) for t in self.p]
        self.steps = [0] * len(self.p)
        self.group_of, self.groups, self.sched, self.max_norm = list(group_of), groups, sched, max_norm
        self.one_at_or_below = one_at_or_below
        self.done = 0
        self.last_norm, self.last_lr = None, None

    def lrs(self):
        f = 1.0 if self.sched is None else schedule(self.sched[0], self.done, **self.sched[1])
        return [g["lr"] * f for g in self.groups]

    def step(self, grads):
        lrs = self.lrs()
        clip = 1.0
        self.last_norm = None
        if self.max_norm is not None:
            self.last_norm = global_norm([g for g in grads if g is not None])
            clip = clip_coef(self.last_norm, self.max_norm, self.one_at_or_below)
        for i, g in enumerate(grads):
            if g is None:
                continue
            self.steps[i] += 1
            h = self.groups[self.group_of[i]]
            self.p[i], self.m[i], self.v[i] = adamw_update(self.p[i], g, self.m[i], self.v[i], lrs[self.group_of[i]], h["betas"],
                                                           h["eps"], h["weight_decay"], h["correct_bias"], self.steps[i], clip)
        self.last_lr = lrs
        self.done += 1

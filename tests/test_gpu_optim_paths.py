"""Every path of the optimiser entries of csrc/optim_ops.hip (gh_adamw_step, gh_flat_grad_norm), called through the C-ABI on
NaN-fenced buffers and compared with the float64 restatement of tests/optim_ref.py; and, since the header fixes the order and
the rounding of every fp32 operation, bit for bit with its fp32 restatements (adamw_update_f32 on 2 097 216 elements,
flat_grad_norm_f32 at every count).

gh_adamw_step.  p, m, v and g sit in NaN-fenced allocations; after every call the fences are intact and g holds the bits it
held before.  The grid is capped at ADAMW_GRID_CAP = 2048 workgroups of 256 lanes, a float4 per lane (csrc/optim_ops.hip), so one
pass of the grid-stride loop covers 2048 * 256 * 4 = 2 097 152 elements: the over-one-pass bucket has one 64-element block more.

Bound of the update, TOL_STEP = 2e-6 of the float64 result's largest entry.  m and v are four resp. five fp32 roundings of terms no
larger than the result's scale (<= 5 * 2^-24 = 3e-7 of it); p adds the rounding of step_size * m / (sqrt(v) + eps), an update of
about lr = 1e-3 .. 1e-2 of p's scale whose relative error stays below 1e-4 even where v is at its smallest here (5e-7 among two
million uniform draws, sqrt 7e-4, against an error of 3e-7 in m), and the table's fp32 rounding of step_size and lr_wd (6e-8 of
the update).  2e-6 is six times the sum.

Bound of the norm.  clip_grad_norm_ in fp32 on the CPU against float64, measured on this test's own gradients (one thread):
5.5e-8, 3.6e-9, 5.1e-8, 3.6e-8, 1.2e-7 for the five counts up to 32 832 and 2.8e-5 for the 2 097 216-element one.  Ten times the
largest of the first five, TOL_NORM = 1.2e-6, is held at EVERY count: for the large bucket that is 230 times tighter than ten
times torch's own error there."""
import numpy as np
import pytest
import torch

from tests import optim_ref
from tests.util import DEV, NAN, _Fenced, _ops, bits_equal, rel_close

pytestmark = pytest.mark.gpu

GRID_CAP = 2048                                  # ADAMW_GRID_CAP of csrc/optim_ops.hip
ONE_PASS = GRID_CAP * 256 * 4
NORM_CHUNK = 32768                               # GH_NORM_CHUNK of include/get_hip.h
TOL_STEP = 2e-6
TOL_NORM = 1.2e-6                                # 10 x 1.2e-7, see the module docstring
H1 = (1e-3, (0.9, 0.999), 1e-6, 0.01, True, 3)
H2 = (5e-3, (0.8, 0.99), 1e-8, 0.0, True, 1)
H3 = (1e-2, (0.9, 0.999), 1e-6, 0.1, False, 5)


def _data(count, seed=0):
    g = torch.Generator().manual_seed(1000 + count + seed)
    return (torch.randn(count, generator=g), torch.randn(count, generator=g), torch.randn(count, generator=g) * 0.5,
            torch.rand(count, generator=g))


class _Step:
    """One gh_adamw_step call on fenced buffers: block ids `ids` (one per 64 elements), `hypers` as ops.adamw_segment_table takes
    them.  norm: the value placed in the device scalar, or None for a NULL pointer."""

    def __init__(self, data, ids, hypers, grad_scale=1.0, norm=None, max_norm=0.0, n_seg=None, mis=None, count=None, expect_error=None):
        _lib, ops = _ops()
        p, g, m, v = data
        n = p.numel()
        self.F = F = _Fenced()
        self.p, self.g, self.m, self.v = (F.put(k, t, mis=(mis == k)) for k, t in zip("pgmv", (p, g, m, v)))
        tab = ops.adamw_segment_table(hypers)
        self.tab = F.put("table", torch.from_numpy(tab.view(np.float32).copy()))
        self.ids = torch.from_numpy(np.asarray(ids, dtype=np.uint16).view(np.int16).copy()).to(DEV)
        self.norm = F.put("norm", torch.tensor([norm], dtype=torch.float32)) if norm is not None else None
        before = [t.clone() for t in (self.p, self.g, self.m, self.v)]
        args = (self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), n if count is None else count,
                self.ids.data_ptr(), self.tab.data_ptr(), len(tab) if n_seg is None else n_seg, grad_scale,
                self.norm.data_ptr() if self.norm is not None else None, max_norm, _lib.stream())
        if expect_error is not None:
            with pytest.raises(RuntimeError, match=expect_error):
                _lib.call("gh_adamw_step", *args)
            torch.cuda.synchronize()
            for k, a, b in zip("pgmv", (self.p, self.g, self.m, self.v), before):
                bits_equal(a, b, f"refused call: {k}")
        else:
            _lib.call("gh_adamw_step", *args)
            torch.cuda.synchronize()
            bits_equal(self.g, before[1], "g after the step")
        F.check(f"adamw_step n={n}")


def _want(data, ids, hypers, grad_scale=1.0, clip=1.0):
    """float64 through optim_ref.adamw_update, block by block; a skipped block (hypers None, id 0 or id beyond the table) keeps
    its inputs."""
    p, g, m, v = (t.double().numpy().copy() for t in data)
    owner = np.repeat(np.asarray(ids), 64)
    for sid in sorted(set(ids)):
        h = hypers[sid - 1] if 1 <= sid <= len(hypers) else None
        if h is None:
            continue
        s = owner == sid
        lr, betas, eps, wd, cb, step = h
        p[s], m[s], v[s] = optim_ref.adamw_update(p[s], g[s], m[s], v[s], lr, betas, eps, wd, cb, step, clip, grad_scale)
    return p, m, v


def _check(run, want, what):
    for k, got, w in zip("pmv", (run.p, run.m, run.v), want):
        rel_close(got, w, TOL_STEP, f"{what}: {k}", fam="adamw_step")


def test_one_block():
    data = _data(64)
    _check(_Step(data, [1], [H1]), _want(data, [1], [H1]), "count=64")


@pytest.mark.parametrize("how", ["skip flag", "segment 0", "id beyond the table"])
def test_skipped_middle_block_keeps_its_bits_even_nan(how):
    p, g, m, v = _data(192)
    for t in (p, m, v):
        t[64:128] = NAN
        t[70] = 1.5
    data = (p, g, m, v)
    ids, hypers = {"skip flag": ([1, 2, 3], [H1, None, H2]), "segment 0": ([1, 0, 2], [H1, H2]),
                   "id beyond the table": ([1, 3, 2], [H1, H2])}[how]
    run = _Step(data, ids, hypers)
    for k, got, src in zip("pmv", (run.p, run.m, run.v), (p, m, v)):
        bits_equal(got[64:128].cpu(), src[64:128], f"{how}: {k} of the skipped block")
    want = _want(data, ids, hypers)
    for k, got, w in zip("pmv", (run.p, run.m, run.v), want):
        keep = np.r_[0:64, 128:192]
        rel_close(got.cpu()[keep], w[keep], TOL_STEP, f"{how}: {k} of the live blocks", fam="adamw_step")


def test_two_segment_boundaries_inside_one_wave():
    data = _data(256)
    ids, hypers = [1, 1, 2, 3], [H1, H2, H3]
    _check(_Step(data, ids, hypers), _want(data, ids, hypers), "three segments in 256 elements")


def test_one_block_more_than_a_full_grid_pass():
    n = ONE_PASS + 64
    data = _data(n)
    ids = [1 + (b // 3) % 2 for b in range(n // 64 - 1)] + [3]      # the block of the second pass has a segment of its own
    hypers = [H1, H2, H3]
    _check(_Step(data, ids, hypers), _want(data, ids, hypers), "one pass + 64")


def test_bits_of_the_update_against_the_fp32_restatement():
    """The header fixes the order and the rounding of every operation, so optim_ref.adamw_update_f32 -- the same operations in
    numpy's float32 -- must give the kernel's bits on all 2 097 216 elements: three segments (two with weight decay), an active
    clip and a grad_scale that is no power of two.  That this can tell a contracted multiply-add from two roundings is asserted
    below: the fused form of the m update alone differs in more than a thousand elements here."""
    _, ops = _ops()
    n = ONE_PASS + 64
    data = _data(n, seed=5)
    ids = np.array([1 + (b // 3) % 2 for b in range(n // 64 - 1)] + [3])
    hypers = [H1, (5e-3, (0.8, 0.99), 1e-8, 0.02, True, 1), H3]
    scale, norm, max_norm = 1.0 / 3.0, 37.5, 2.0
    run = _Step(data, ids, hypers, grad_scale=scale, norm=norm, max_norm=max_norm)
    tab = ops.adamw_segment_table(hypers)
    clip = optim_ref.clip_coef_f32(norm, max_norm)
    assert 0 < clip < 0.06
    owner = np.repeat(ids, 64)
    want = [t.numpy().copy() for t in (data[0], data[2], data[3])]
    fused_differs = 0
    for sid in (1, 2, 3):
        s = owner == sid
        p, g, m, v = (t.numpy()[s] for t in data)
        want[0][s], want[1][s], want[2][s] = optim_ref.adamw_update_f32(p, g, m, v, tab[sid], scale, clip)
        gr = (g * np.float32(scale)) * clip
        fused = (np.float64(tab[sid]["beta1"]) * m + np.float64(tab[sid]["one_minus_beta1"] * gr)).astype(np.float32)
        fused_differs += int((fused != want[1][s]).sum())
    assert fused_differs > 1000, fused_differs
    for k, got, w in zip("pmv", (run.p, run.m, run.v), want):
        bits_equal(got.cpu(), torch.from_numpy(w), f"{k} against the fp32 restatement")


def test_clipping_null_inactive_and_active():
    data = _data(320)
    ids, hypers = [1, 2, 2, 1, 2], [H1, H2]
    plain = _Step(data, ids, hypers)
    for norm in (0.25, 2.0):                                         # below and exactly at max_norm: the unclipped step, bit for bit
        same = _Step(data, ids, hypers, norm=norm, max_norm=2.0)
        for k, a, b in zip("pmv", (plain.p, plain.m, plain.v), (same.p, same.m, same.v)):
            bits_equal(a, b, f"norm {norm} <= max_norm 2: {k}")
    active = _Step(data, ids, hypers, norm=37.5, max_norm=2.0)
    clip = optim_ref.clip_coef(37.5, 2.0)
    assert clip < 0.06
    _check(active, _want(data, ids, hypers, clip=clip), "norm 37.5, max_norm 2")
    assert not torch.equal(active.m, plain.m)


@pytest.mark.parametrize("scale", [0.25, 1.0 / 3.0])
def test_grad_scale(scale):
    data = _data(128, seed=1)
    ids, hypers = [1, 2], [H1, H2]
    _check(_Step(data, ids, hypers, grad_scale=scale), _want(data, ids, hypers, grad_scale=scale), f"grad_scale {scale}")
    clipped = _Step(data, ids, hypers, grad_scale=scale, norm=10.0, max_norm=1.0)
    _check(clipped, _want(data, ids, hypers, grad_scale=scale, clip=optim_ref.clip_coef(10.0, 1.0)), f"grad_scale {scale}, clipped")


def test_bias_correction_off():
    data = _data(128, seed=2)
    off, on = list(H3), list(H3)
    on[4] = True
    r_off, r_on = _Step(data, [1, 1], [tuple(off)]), _Step(data, [1, 1], [tuple(on)])
    _check(r_off, _want(data, [1, 1], [tuple(off)]), "correct_bias off")
    _check(r_on, _want(data, [1, 1], [tuple(on)]), "correct_bias on")
    bits_equal(r_off.m, r_on.m, "m does not depend on the bias correction")
    assert not torch.equal(r_off.p, r_on.p)


def test_without_weight_decay_p_is_p1_bit_for_bit():
    data = _data(192, seed=3)
    decayed, plain = H1, (H1[0], H1[1], H1[2], 0.0, H1[4], H1[5])
    r0, r1 = _Step(data, [1, 1, 1], [plain]), _Step(data, [1, 1, 1], [decayed])
    bits_equal(r0.m, r1.m, "m")
    bits_equal(r0.v, r1.v, "v")
    p1 = r0.p.cpu()
    lr_wd = torch.tensor(np.float32(H1[0] * H1[3]))
    bits_equal(r1.p.cpu(), p1 - lr_wd * p1, "p = p1 - lr_wd * p1, each rounded once")
    _check(r0, _want(data, [1, 1, 1], [plain]), "lr_wd = 0")


@pytest.mark.parametrize("what", ["count", "p", "g", "m", "v", "table", "max_norm"])
def test_refused_calls_leave_the_buffers_untouched(what):
    data = _data(128, seed=4)
    kw = {"count": dict(count=96, expect_error="multiple of 64"), "table": dict(n_seg=65536, expect_error="16-bit"),
          "max_norm": dict(norm=3.0, max_norm=0.0, expect_error="max_norm")}.get(what) or dict(mis=what, expect_error="16-byte aligned")
    _Step(data, [1, 1], [H1], **kw)


# ---------------------------------------------------------------------------- gh_flat_grad_norm
def _norm(g_host, grad_scale=1.0, calls=1):
    _lib, ops = _ops()
    n = g_host.numel()
    need = ops.grad_norm_partials(n)
    assert need == (n + NORM_CHUNK - 1) // NORM_CHUNK
    F = _Fenced()
    g = F.put("g", g_host)
    partials = F.put("partials", shape=(need + 3,), dtype=torch.float64)
    outs = []
    for _ in range(calls):
        out = F.put("norm", shape=(1,))
        _lib.call("gh_flat_grad_norm", g.data_ptr(), n, grad_scale, partials.data_ptr(), need + 3, out.data_ptr(), _lib.stream())
        outs.append(out)
    torch.cuda.synchronize()
    bits_equal(g.cpu(), g_host, "g after the norm")
    assert bool(torch.isfinite(partials[:need]).all()) and bool(torch.isnan(partials[need:]).all()), "exactly `need` partials are written"
    F.check(f"flat_grad_norm n={n}")
    return [o.cpu() for o in outs]


@pytest.mark.parametrize("count", [64, 192, NORM_CHUNK - 64, NORM_CHUNK, NORM_CHUNK + 64, ONE_PASS + 64])
def test_grad_norm_against_float64(count):
    g = torch.randn(count, generator=torch.Generator().manual_seed(count))
    want = float(g.double().pow(2).sum().sqrt())
    a, b = _norm(g, calls=2)
    bits_equal(a, b, "two calls")
    rel = abs(float(a) - want) / want
    print(f"flat_grad_norm count={count}: relative error {rel:.3e} (bound {TOL_NORM:.1e})")
    assert rel <= TOL_NORM
    bits_equal(a, torch.from_numpy(np.array([optim_ref.flat_grad_norm_f32(g.numpy())])), "the norm against the fp32 restatement")
    s, = _norm(g, grad_scale=0.125)
    assert float(s) == float(a) * 0.125                                        # a power of two scales exactly
    t, = _norm(g, grad_scale=1.0 / 3.0)
    bits_equal(t, torch.from_numpy(np.array([optim_ref.flat_grad_norm_f32(g.numpy(), 1.0 / 3.0)])), "the scaled norm against the fp32 restatement")


def test_grad_norm_of_zeros_is_exactly_zero_and_partials_are_refused_when_short():
    _lib, ops = _ops()
    z, = _norm(torch.zeros(NORM_CHUNK + 64))
    assert float(z) == 0.0 and not np.signbit(float(z))
    g = torch.ones(NORM_CHUNK + 64, device=DEV)
    out = torch.full((1,), NAN, device=DEV)
    partials = torch.full((1,), NAN, device=DEV, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="partials"):
        _lib.call("gh_flat_grad_norm", g.data_ptr(), g.numel(), 1.0, partials.data_ptr(), 1, out.data_ptr(), _lib.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(partials).all())
    n, = _norm(torch.ones(67))                                                  # a count that is no multiple of 4
    assert abs(float(n) - 67 ** 0.5) <= TOL_NORM * 67 ** 0.5
    g67 = torch.randn(67, generator=torch.Generator().manual_seed(67))          # the short last float4 adds in the same order
    n, = _norm(g67)
    bits_equal(n, torch.from_numpy(np.array([optim_ref.flat_grad_norm_f32(g67.numpy())])), "count 67 against the fp32 restatement")
    assert ops.grad_norm_partials(0) == 0 and float(ops.grad_norm_flat(torch.zeros(0, device=DEV))) == 0.0

"""The BiDAF drop-in on the GPU (csrc/bidaf_ops.hip, ops.att_flow / ops.highway, modules.BiDAF): the reference's goldens,
every tiling path of the attention-flow kernels against the float64 restatement of tests/bidaf_ref.py, zero rows and ties,
in-place operands, determinism, the highway gate, the replayed training-mode dropout, the limits, and the whole model at
the project's widths.  The ratios the tests print are the ones quoted in DESIGN.md 4.11."""
import numpy as np
import pytest
import torch

from tests.bidaf_ref import att_flow64, bidaf64, highway64
from tests.test_bidaf_cpu import CASES, KEYS, model_params, params_of
from tests.util import TOL, bits_equal, golden_ratio, load_golden, rel_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
WNAMES = ("w_c", "w_q", "w_cq")


def _archive(golden_dir):
    return load_golden(golden_dir, "g15_bidaf.npz", "bidaf_contract.json")


def _model(z, contract, name):
    from get_amd import modules
    m = modules.BiDAF(model_params(z, contract, name))
    m.load_state_dict(params_of(z, name), strict=True)
    return m.to(DEV).eval()


def _forward(m, z, name):
    idx = {k: torch.from_numpy(z[f"{name}::{k}_indices"]) for k in ("q_new", "q_restoring", "d_new", "d_restoring")}
    return m(torch.from_numpy(z[name + "::query"]).to(DEV), torch.from_numpy(z[name + "::document"]).to(DEV),
             query_lens_indices=(idx["q_new"], idx["q_restoring"], torch.from_numpy(z[name + "::q_lens"])),
             doc_lens_indices=(idx["d_new"], idx["d_restoring"], torch.from_numpy(z[name + "::c_lens"])))


@pytest.mark.parametrize("name", CASES)
def test_bidaf_matches_reference_goldens(golden_dir, name):
    """Logits within 1e-4 + 1e-4 |want|, every gradient within 1e-5 + 1e-4 |want| of the reference's fp32 results,
    elementwise; the three attention bias gradients are present and exactly zero."""
    z, _, contract = _archive(golden_dir)
    m = _model(z, contract, name)
    logits = _forward(m, z, name)
    (logits * torch.from_numpy(z[name + "::g_logits"]).to(DEV)).sum().backward()
    worst = golden_ratio(logits, z[name + "::logits"], 1e-4, 1e-4, f"{name}::logits")
    grads = dict(m.named_parameters())
    for k in KEYS:
        if f"{name}::grad::{k}" in z:
            worst = max(worst, golden_ratio(grads[k].grad, z[f"{name}::grad::{k}"], 1e-5, 1e-4, f"{name}::grad::{k}"))
    print(f"{name}: worst ratio of the golden bound {worst:.3f}")
    for n in ("c", "q", "cq"):
        g = grads[f"att_weight_{n}.linear.bias"].grad
        assert g is not None and g.shape == (1,) and float(g.abs().max()) == 0.0
    assert m.last_seeds == [None, None, None]


def _inputs(b, lc, lq, d, seed):
    g = torch.Generator().manual_seed(seed)
    c, q = torch.randn(b, lc, d, generator=g), torch.randn(b, lq, d, generator=g)
    w = [torch.randn(d, generator=g) / d ** 0.5 for _ in range(3)]
    bias = [0.3 * torch.randn(1, generator=g) for _ in range(3)]
    gx = torch.randint(-16, 17, (b, lc, 4 * d), generator=g).float() / 16
    return c, q, w, bias, gx


def _run(c, q, w, bias, gx, out=None):
    """ops.att_flow forward + backward on the device: x and the gradients of c, q, w_c, w_q, w_cq (c and q are used as given,
    so that column slices stay column slices)."""
    from get_amd import ops
    c, q = c.requires_grad_(True), q.requires_grad_(True)
    w = [t.to(DEV).requires_grad_(True) for t in w]
    bias = [t.to(DEV).requires_grad_(True) for t in bias]
    x = ops.att_flow(c, q, w[0], w[1], w[2], bias[0], bias[1], bias[2], out=out)
    saved = x.grad_fn.saved_tensors
    x.backward(gx)
    torch.cuda.synchronize()
    for t in bias:
        assert t.grad is not None and float(t.grad.abs().max()) == 0.0
    return x.detach(), [c.grad, q.grad] + [t.grad for t in w], saved


def _want(c, q, w, bias, gx):
    c64, q64 = c.double().requires_grad_(True), q.double().requires_grad_(True)
    w64 = [t.double().requires_grad_(True) for t in w]
    x64, am = att_flow64(c64, q64, w64[0], w64[1], w64[2], sum(t.double() for t in bias))
    (x64 * gx.double()).sum().backward()
    return x64.detach(), [c64.grad, q64.grad] + [t.grad for t in w64], am


SHAPES = [(2, 5, 3, 6),           # everything below one tile, depth not a multiple of 4
          (3, 21, 9, 10),         # two row tiles: beta crosses tiles
          (2, 37, 35, 70),        # three row tiles, three column tiles, ragged tails
          (4, 100, 30, 600),      # the project's shape
          (2, 19, 20, 700),       # two depth / column blocks of 640
          (1, 1024, 1024, 8)]     # the length limits


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_att_flow_against_float64(shape):
    """x and dc, dq, dw_c, dw_q, dw_cq within 1e-4 of the largest float64 entry of each tensor."""
    c, q, w, bias, gx = _inputs(*shape, seed=sum(shape))
    x, grads, _ = _run(c.to(DEV), q.to(DEV), w, bias, gx.to(DEV))
    x64, g64, _ = _want(c, q, w, bias, gx)
    tag = "x".join(map(str, shape))
    rel_close(x, x64, TOL, f"att_flow {tag} x", fam="att_flow")
    for name, got, want in zip(("dc", "dq") + tuple("d" + n for n in WNAMES), grads, g64):
        rel_close(got, want, TOL, f"att_flow {tag} {name}", fam="att_flow")


def test_zero_rows_take_part_and_ties_go_to_the_lowest_index():
    """Trailing zero rows in c and q, and q_j.w_q < 0 for every real j: each row's maximum sits on the tied zero rows of q.
    The saved argmax is the lowest of them, the gradient of the maximum reaches only that row, and nothing is NaN."""
    b, lc, lq, d, lc_real, lq_real = 2, 21, 9, 10, 17, 5
    c, q, w, bias, gx = _inputs(b, lc, lq, d, seed=77)
    c[:, lc_real:] = 0
    q = -q.abs()
    q[:, lq_real:] = 0
    w[1] = w[1].abs() + 0.5          # q_j . w_q < 0 for the real rows
    w[2] = 0.01 * w[2]               # and the trilinear term cannot outweigh it
    x64, g64, am64 = _want(c, q, w, bias, gx)
    assert bool((q[:, :lq_real] @ w[1] < 0).all()) and bool((am64 == lq_real).all())      # float64 argmax: the first zero row
    x, grads, saved = _run(c.to(DEV), q.to(DEV), w, bias, gx.to(DEV))
    amax = [t for t in saved if t.dtype == torch.int32][0]
    assert amax.shape == (b, lc) and bool((amax == lq_real).all())
    rel_close(x, x64, TOL, "ties x", fam="att_flow")
    for name, got, want in zip(("dc", "dq") + tuple("d" + n for n in WNAMES), grads, g64):
        rel_close(got, want, TOL, f"ties {name}", fam="att_flow")
    # the other tied rows get no share of the maximum's gradient: among themselves they are equal (q_j = 0 alike), and they
    # differ from the row that owns the maximum
    dq = grads[1].cpu()
    rel_close(dq[:, lq_real + 1:], g64[1][:, lq_real + 1:], TOL, "ties dq at the other tied rows", fam="att_flow")
    assert bool((dq[:, lq_real + 1] == dq[:, lq_real + 2]).all()) and not bool((dq[:, lq_real] == dq[:, lq_real + 1]).all())
    # zero rows of c still score q_j . w_q + bias: their attention is not uniform
    a = [t for t in saved if t.shape == (b, lc, lq)][0]
    assert float((a[:, lc_real:, 0] - a[:, lc_real:, lq - 1]).abs().min()) > 1e-3


def test_operands_are_read_and_written_in_place():
    """c and q as column slices of wider tensors whose base is not 16-byte aligned, x written into a column slice of a wider
    buffer: bit-identical to contiguous copies (single-float accesses against 16 bytes per lane), nothing outside the slice is
    written."""
    b, lc, lq, d = 2, 37, 35, 12
    c, q, w, bias, gx = _inputs(b, lc, lq, d, seed=9)
    ref_x, ref_g, _ = _run(c.to(DEV), q.to(DEV), w, bias, gx.to(DEV))

    def wide(t, extra, off):
        n, l, wd = t.shape
        flat = torch.full((n * l * (wd + extra) + 1,), 7.0, device=DEV)
        v = flat[1:].view(n, l, wd + extra)[:, :, off:off + wd]
        v.copy_(t)
        assert v.data_ptr() % 16 != 0 and not v.is_contiguous()
        return v
    cw, qw = wide(c, 3, 1), wide(q, 5, 2)
    buf = torch.full((b, lc, 4 * d + 6), -3.0, device=DEV)
    x, g, _ = _run(cw.detach(), qw.detach(), w, bias, gx.to(DEV), out=buf[:, :, 2:2 + 4 * d])
    assert x.data_ptr() == buf[:, :, 2:].data_ptr()
    bits_equal(x, ref_x, "x in place")
    assert bool((buf[:, :, :2] == -3.0).all()) and bool((buf[:, :, 2 + 4 * d:] == -3.0).all())
    for name, u, v in zip(("dc", "dq") + WNAMES, g, ref_g):
        bits_equal(u, v, name + " in place")


def test_two_runs_are_bit_identical():
    c, q, w, bias, gx = _inputs(2, 37, 35, 70, seed=4)
    runs = [_run(c.clone().to(DEV), q.clone().to(DEV), w, bias, gx.to(DEV)) for _ in range(2)]
    bits_equal(runs[0][0], runs[1][0], "x of two runs")
    for name, u, v in zip(("dc", "dq") + WNAMES, runs[0][1], runs[1][1]):
        bits_equal(u, v, name + " of two runs")


@pytest.mark.parametrize("rows,d", [(7, 6), (33, 70), (96000, 300)])
def test_highway_against_float64(rows, d):
    """y and the three gradients within 1e-4 of the largest float64 entry; pre-activations of +-100 give exact 1 / 0 gates."""
    from get_amd import ops
    g = torch.Generator().manual_seed(rows + d)
    x, h, gp = (torch.randn(rows, d, generator=g) for _ in range(3))
    x = x + torch.sign(x)          # |x| >= 1: an exact-0 gate returns x itself
    gp[0, :] = 100.0
    gp[1, :] = -100.0
    gy = torch.randint(-16, 17, (rows, d), generator=g).float() / 16
    dev = [t.to(DEV).requires_grad_(True) for t in (x, h, gp)]
    y = ops.highway(*dev)
    y.backward(gy.to(DEV))
    c64 = [t.double().requires_grad_(True) for t in (x, h, gp)]
    y64 = highway64(*c64)
    (y64 * gy.double()).sum().backward()
    rel_close(y, y64, TOL, f"highway {rows}x{d} y", fam="highway")
    for name, u, v in zip(("dx", "dh_pre", "dg_pre"), dev, c64):
        rel_close(u.grad, v.grad, TOL, f"highway {rows}x{d} {name}", fam="highway")
    yc = y.detach().cpu()
    bits_equal(yc[0], torch.relu(h[0]), "gate exactly 1")
    bits_equal(yc[1], x[1], "gate exactly 0")
    assert float(dev[2].grad[:2].abs().max()) <= 1e-30 and bool((dev[0].grad[0] == 0).all())


def test_training_mode_replays_the_three_dropouts(golden_dir):
    """One training-mode forward + backward of the second golden case's model (dropout 0.2): the three input-dropout masks
    rebuilt from BiDAF.last_seeds through the float64 restatement; logits and every gradient within 1e-4."""
    from get_amd import ops
    name = "v60_h16"
    z, _, contract = _archive(golden_dir)
    m = _model(z, contract, name).train(True)
    p = contract[name]["params"]["dropout"]
    logits = _forward(m, z, name)
    g_logits = torch.from_numpy(z[name + "::g_logits"])
    (logits * g_logits.to(DEV)).sum().backward()
    seeds = m.last_seeds
    assert all(s is not None for s in seeds) and len(set(seeds)) == 3
    (B, L), R = z[name + "::query"].shape, z[name + "::document"].shape[1]
    D, H = contract[name]["params"]["word_dim"], contract[name]["params"]["hidden_size"]
    Tc, Tq = int(z[name + "::c_lens"].max()), int(z[name + "::q_lens"].max())
    masks = (torch.from_numpy(ops.dropout_mask_reference(seeds[0], B * R, D, p)).double().view(B, R, D)[:, :Tc],
             torch.from_numpy(ops.dropout_mask_reference(seeds[1], B * L, D, p)).double().view(B, L, D)[:, :Tq],
             torch.from_numpy(ops.dropout_mask_reference(seeds[2], B * Tc, 8 * H, p)).double().view(B, Tc, 8 * H))
    assert all(0 < float(k.mean()) < 1 for k in masks)
    p64 = {k: v.double().requires_grad_(True) for k, v in params_of(z, name).items()}
    want = bidaf64(p64, torch.from_numpy(z[name + "::query"]), torch.from_numpy(z[name + "::document"]), z[name + "::q_lens"],
                   z[name + "::c_lens"], masks, p)
    (want * g_logits.double()).sum().backward()
    rel_close(logits, want, TOL, "training logits", fam="bidaf_train")
    for k, prm in m.named_parameters():
        if k.startswith("att_weight") and k.endswith("bias"):      # mathematically zero: exact zeros here
            assert float(prm.grad.abs().max()) == 0.0 and float(p64[k].grad.abs().max()) <= 1e-9
            continue
        rel_close(prm.grad, p64[k].grad, TOL, "training grad " + k, fam="bidaf_train")


def test_limits_are_refused_and_nothing_is_written():
    from get_amd import ops
    bias = torch.zeros(1, device=DEV)
    for (lc, lq, d), limit in (((1025, 3, 4), "1024"), ((3, 1025, 4), "1024"), ((3, 3, 2049), "2048")):
        wd = torch.zeros(d, device=DEV)
        out = torch.full((1, lc, 4 * d), 5.0, device=DEV)
        with pytest.raises(RuntimeError, match=limit):
            ops.att_flow(torch.zeros(1, lc, d, device=DEV), torch.zeros(1, lq, d, device=DEV), wd, wd, wd, bias, bias, bias, out=out)
        torch.cuda.synchronize()
        assert bool((out == 5.0).all())


def test_whole_model_at_the_projects_widths():
    """B = 37, L = 30, R = 100, D = 300, H = 150 against the float64 restatement: logits and every gradient within 1e-4 of the
    largest float64 entry of each tensor."""
    from get_amd import modules
    B, L, R, D, H, V = 37, 30, 100, 300, 150, 200
    g = torch.Generator().manual_seed(21)
    emb = (0.5 * torch.randn(V, D, generator=g)).numpy()
    torch.manual_seed(21)
    m = modules.BiDAF(dict(embedding=emb, embedding_freeze=False, word_dim=D, hidden_size=H, dropout=0.2)).eval()
    with torch.no_grad():
        for k, prm in m.named_parameters():
            if "bias" in k:
                prm.copy_(0.1 * torch.randn(prm.shape, generator=g))
    p64 = {k: v.detach().clone().double().requires_grad_(True) for k, v in m.state_dict().items()}
    m = m.to(DEV)
    query, document = torch.randint(0, V, (B, L), generator=g), torch.randint(0, V, (B, R), generator=g)
    q_lens, c_lens = torch.randint(1, L + 1, (B,), generator=g), torch.randint(1, R + 1, (B,), generator=g)
    q_lens[3], c_lens[5], q_lens[0], c_lens[1] = L, R, 1, 1
    g_logits = torch.randint(-16, 17, (B, 1), generator=g).float() / 16
    idx = []
    for lens in (q_lens, c_lens):
        new = torch.sort(lens, descending=True, stable=True)[1]
        idx.append((new, torch.argsort(new), lens))
    logits = m(query.to(DEV), document.to(DEV), query_lens_indices=idx[0], doc_lens_indices=idx[1])
    assert logits.shape == (B, 1)
    (logits * g_logits.to(DEV)).sum().backward()
    want = bidaf64(p64, query, document, q_lens, c_lens)
    (want * g_logits.double()).sum().backward()
    rel_close(logits, want, TOL, "project logits", fam="bidaf_model")
    for k, prm in m.named_parameters():
        if k.startswith("att_weight") and k.endswith("bias"):      # mathematically zero: exact zeros here
            assert float(prm.grad.abs().max()) == 0.0 and float(p64[k].grad.abs().max()) <= 1e-9
            continue
        rel_close(prm.grad, p64[k].grad, TOL, "project grad " + k, fam="bidaf_model")
    # predict(): eval mode, indices by descending length, a flat numpy result; numpy and tensor lengths alike
    from get_amd.keywords import KeyWordSettings as K
    for lens in ((q_lens.numpy(), c_lens.numpy()), (q_lens, c_lens.to(DEV))):
        out = m.predict(query.to(DEV), document.to(DEV), **{K.Query_lens: lens[0], K.Doc_lens: lens[1]})
        assert isinstance(out, np.ndarray) and out.shape == (B,)
        rel_close(out, want.detach().flatten(), TOL, "predict", fam="bidaf_model")

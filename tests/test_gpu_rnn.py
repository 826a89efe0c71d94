"""GPU checks of the two sequence encoders (get_amd.modules.LSTM / GRU, ops.lstm_seq / gru_seq, csrc/rnn_ops.hip), every test
once per cell: against the reference's captured outputs and gradients (tests/golden/g14_lstm.npz, g16_gru.npz), the padding
conventions, the processing order, run-to-run determinism, the project's width against the float64 restatement of
tests/rnn_ref.py, the replayed input dropout, the documented limits and -- for the LSTM -- the model's two encoders."""
import pytest
import torch

from tests.rnn_ref import CELLS
from tests.util import bits_equal, build_from_contract, golden_ratio, load_golden, rel_close

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0") if torch.cuda.is_available() else None

CASES = ["bi_b5", "bi_b5_max25", "uni_h5", "two_layers", "bi_b37", "bi_l70", "bi_b5_saturated"]


@pytest.fixture(params=list(CELLS))
def cell(request):
    return CELLS[request.param]


def _cls(cell):
    from get_amd import modules
    return getattr(modules, cell.module)


def _golden(golden_dir, cell):
    z, _, contract = load_golden(golden_dir, cell.archive, cell.contract)
    return z, contract


def _module(cell, z, contract, name):
    return build_from_contract(z, name + "::", contract[name], _cls(cell)).to(DEV).eval()


def _pair(lens):
    new = torch.sort(torch.as_tensor(lens).long().cpu(), descending=True, stable=True)[1]
    return new, torch.argsort(new)


def _run(m, x, lens, pair, max_len, gy, gh, return_h=True):
    """Forward + backward of sum(y gy) + sum(h gh) with fresh gradients; returns y, h and every gradient by name."""
    m.zero_grad(set_to_none=True)
    xd = x.detach().clone().to(DEV).requires_grad_(True)
    y, h = m((xd, lens, pair[0], pair[1]), return_h=return_h, max_len=max_len)
    ((y * gy.to(DEV)).sum() + (h * gh.to(DEV)).sum()).backward()
    grads = {"x": xd.grad}
    grads.update({k: p.grad for k, p in m.named_parameters()})
    return y.detach(), h.detach(), grads


@pytest.mark.parametrize("name", CASES)
def test_matches_reference_goldens(golden_dir, cell, name):
    """y, h and every gradient (x and all parameters) within 1e-5 + 1e-4 |want| of the reference's fp32 results, elementwise.
    GRU: the gradient of bias_hh is also checked third by third: its n third is where a bias folded into gx or a missing factor
    r shows (the gradient of gx_n is not the gradient of a_n).  Achieved on the MI355X: see DESIGN.md 4.10 and 4.12."""
    z, contract = _golden(golden_dir, cell)
    m = _module(cell, z, contract, name)
    g = lambda k: torch.from_numpy(z[f"{name}::{k}"])
    pair = (g("new_indices"), g("restoring_indices"))
    y, h, grads = _run(m, g("x"), g("lens"), pair, contract[name]["max_len"], g("gy"), g("gh"))
    golden_ratio(y, g("y"), 1e-5, 1e-4, name + "::y")
    golden_ratio(h, g("h"), 1e-5, 1e-4, name + "::h")
    assert set(grads) == {"x"} | {k for k, _ in contract[name]["state_dict"]}
    for k, got in grads.items():
        assert got is not None, k
        golden_ratio(got, g("grad::" + k), 1e-5, 1e-4, f"{name}::grad::{k}")
        if cell.module == "GRU" and "bias_hh" in k:
            H = contract[name]["kwargs"]["hidden_size"]
            want = g("grad::" + k)
            assert got.shape == (3 * H,)
            for j, third in enumerate("rzn"):
                assert bool((want[j * H:(j + 1) * H] != 0).any()), (k, third)
                golden_ratio(got[j * H:(j + 1) * H], want[j * H:(j + 1) * H], 1e-5, 1e-4, f"{name}::grad::{k}[{third}]")
            # the two biases' gradients differ in the n third only (there by the factor r)
            gi = g("grad::" + k.replace("bias_hh", "bias_ih"))
            assert not torch.equal(gi[2 * H:], want[2 * H:])
    if name == "bi_b37":      # return_h=False: the raw (layers * dirs, B, H) state in the sorted order
        with torch.no_grad():
            y2, raw = m((g("x").to(DEV), g("lens"), pair[0], pair[1]), return_h=False)
        bits_equal(y2, y, "y of return_h=False")
        golden_ratio(raw, g("h_raw"), 1e-5, 1e-4, name + "::h_raw")


def test_padding_never_reaches_a_result(golden_dir, cell):
    """Other finite values (+-1e3) in x at t >= len leave y, h and every gradient bit-identical; y and the gradient of x are
    exact zeros at t >= len, rows [L, max_len) of y are zero; a device length of 0 gives zero rows, a zero state and finite
    gradients, and leaves the sequence next to it untouched to the bit."""
    z, contract = _golden(golden_dir, cell)
    name = "bi_b5_max25"
    m = _module(cell, z, contract, name)
    g = lambda k: torch.from_numpy(z[f"{name}::{k}"])
    x, lens, pair = g("x"), g("lens"), (g("new_indices"), g("restoring_indices"))
    L = x.shape[1]
    dead = torch.arange(L)[None, :] >= lens[:, None]
    x2 = x.clone()
    x2[dead] = torch.where(torch.arange(int(dead.sum()) * x.shape[2]).view(-1, x.shape[2]) % 2 == 0, 1e3, -1e3)
    assert bool(dead.any()) and not torch.equal(x, x2)
    y, h, grads = _run(m, x, lens, pair, 25, g("gy"), g("gh"))
    y2, h2, grads2 = _run(m, x2, lens, pair, 25, g("gy"), g("gh"))
    bits_equal(y, y2, "y")
    bits_equal(h, h2, "h")
    for k in grads:
        bits_equal(grads[k], grads2[k], "grad " + k)
    dead_t = torch.arange(25)[None, :] >= lens[:, None]
    assert y.shape == (5, 25, 16) and bool((y.cpu()[dead_t] == 0).all()) and bool((y[:, L:] == 0).all())
    assert bool((grads["x"].cpu()[dead] == 0).all())
    # a length of 0 on the device (the host check cannot see it): zero rows, zero state, finite gradients
    lens0 = lens.clone()
    lens0[1] = 0
    y0, h0, grads0 = _run(m, x, lens0.to(DEV), _pair(lens0), 25, g("gy"), g("gh"))
    assert bool((y0[1] == 0).all()) and bool((h0[1] == 0).all()) and bool((grads0["x"][1] == 0).all())
    assert all(bool(torch.isfinite(v).all()) for v in grads0.values())
    bits_equal(y0[0], y[0], "an untouched sequence next to an empty one")
    bits_equal(h0[0], h[0], "the state of an untouched sequence next to an empty one")
    bits_equal(grads0["x"][0], grads["x"][0], "the gradient of an untouched sequence next to an empty one")
    # host lengths outside [1, T] raise as the reference's pack / pad functions do
    with pytest.raises(ValueError):
        m((x.to(DEV), lens0, pair[0], pair[1]), max_len=25)
    with pytest.raises(ValueError):
        m((x.to(DEV), lens, pair[0], pair[1]), max_len=20)


def test_processing_order_does_not_change_a_bit(golden_dir, cell):
    """The same batch with the identity pair and with the sorted pair.  Bitwise equality applies: a sequence's arithmetic does
    not depend on its position in a 16-sequence tile (each output element of the MFMA is its own k-ordered fma chain), and the
    weight-gradient GEMMs sum over rows in memory order, which the processing order does not touch."""
    z, contract = _golden(golden_dir, cell)
    name = "bi_b37"
    m = _module(cell, z, contract, name)
    g = lambda k: torch.from_numpy(z[f"{name}::{k}"])
    ident = (torch.arange(37), torch.arange(37))
    lens = g("lens").to(DEV)          # on the device: no host check of the order
    y, h, grads = _run(m, g("x"), lens, (g("new_indices"), g("restoring_indices")), 20, g("gy"), g("gh"))
    y2, h2, grads2 = _run(m, g("x"), lens, ident, 20, g("gy"), g("gh"))
    bits_equal(y, y2, "y")
    bits_equal(h, h2, "h")
    for k in grads:
        bits_equal(grads[k], grads2[k], "grad " + k)


def test_two_runs_are_bit_identical(golden_dir, cell):
    z, contract = _golden(golden_dir, cell)
    for name in ("bi_b37", "two_layers"):
        m = _module(cell, z, contract, name)
        g = lambda k: torch.from_numpy(z[f"{name}::{k}"])
        args = (g("x"), g("lens"), (g("new_indices"), g("restoring_indices")), None, g("gy"), g("gh"))
        y, h, grads = _run(m, *args)
        y2, h2, grads2 = _run(m, *args)
        bits_equal(y, y2, "y")
        bits_equal(h, h2, "h")
        for k in grads:
            bits_equal(grads[k], grads2[k], "grad " + k)


def _against_float64(cell, m, x, lens, T, seed, what, drop_mask=None, p=0.0):
    gen = torch.Generator().manual_seed(seed)
    H, dirs, layers = m.rnn.hidden_size, 2 if m.rnn.bidirectional else 1, m.rnn.num_layers
    gy, gh = torch.randn(x.shape[0], T, dirs * H, generator=gen), torch.randn(x.shape[0], layers * dirs * H, generator=gen)
    p64 = {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.named_parameters()}
    x64 = x.double().requires_grad_(True)
    y64, h64 = cell.ref64(p64, x64, lens, T, layers, dirs == 2, drop_mask, p)
    ((y64 * gy.double()).sum() + (h64 * gh.double()).sum()).backward()
    return gy, gh, y64.detach(), h64.detach(), {"x": x64.grad, **{k: v.grad for k, v in p64.items()}}


def test_project_width_against_float64(cell):
    """B=37, L=100, D=H=300, bidirectional, unsorted lengths including 1 and 100, against tests/rnn_ref.py in float64:
    max |got - want| <= 2e-5 max |want| per tensor (the project's float64 bound of its GEMM tests; torch's own fp32 nn.GRU is
    at most 2.6e-6 from float64 at this shape).  Two 256-unit chunks of the backward, the second partial, and three tiles.
    (An elementwise bound is not used at this shape: the reference's own fp32 LSTM result misses 1e-5 + 1e-4 |want| on the
    weight_ih gradients there, through cancellation.)"""
    torch.manual_seed(11)
    m = _cls(cell)(300, 300, bidirectional=True).to(DEV).eval()
    gen = torch.Generator().manual_seed(12)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "bias" in k:
                p.copy_(0.3 * torch.randn(p.shape, generator=gen))
    lens = torch.randint(2, 100, (37,), generator=gen)
    lens[5], lens[20], lens[36] = 1, 100, 100
    x = torch.randn(37, 100, 300, generator=gen)
    gy, gh, y64, h64, g64 = _against_float64(cell, m, x, lens, 100, 13, "h300")
    y, h, grads = _run(m, x, lens, _pair(lens), 100, gy, gh)
    rel_close(y, y64, 2e-5, "h300 y")
    rel_close(h, h64, 2e-5, "h300 h")
    for k in grads:
        rel_close(grads[k], g64[k], 2e-5, "h300 grad " + k)


def test_input_dropout_is_replayed_from_its_seed(golden_dir, cell):
    """Training mode: the input dropout's mask, rebuilt from last_seed by ops.dropout_mask_reference, through the float64
    restatement, at the golden bound; eval mode records no seed."""
    from get_amd import ops
    z, contract = _golden(golden_dir, cell)
    name = "bi_b5"
    m = _module(cell, z, contract, name)
    g = lambda k: torch.from_numpy(z[f"{name}::{k}"])
    x, lens, pair = g("x"), g("lens"), (g("new_indices"), g("restoring_indices"))
    _run(m, x, lens, pair, None, g("gy"), g("gh"))
    assert m.last_seed is None
    m.zero_grad(set_to_none=True)
    m.train(True)
    p = m.dropout.p
    xd = x.to(DEV).requires_grad_(True)
    y, h = m((xd, lens, pair[0], pair[1]))
    assert m.last_seed is not None
    B, L, D = x.shape
    mask = torch.from_numpy(ops.dropout_mask_reference(m.last_seed, B * L, D, p)).double().view(B, L, D)
    assert 0 < float(mask.mean()) < 1
    gy, gh, y64, h64, g64 = _against_float64(cell, m, x, lens, 21, 17, "dropout", mask, p)
    ((y * gy.to(DEV)).sum() + (h * gh.to(DEV)).sum()).backward()
    golden_ratio(y, y64, 1e-5, 1e-4, "dropout y")
    golden_ratio(h, h64, 1e-5, 1e-4, "dropout h")
    golden_ratio(xd.grad, g64["x"], 1e-5, 1e-4, "dropout grad x")
    for k, q in m.named_parameters():
        golden_ratio(q.grad, g64[k], 1e-5, 1e-4, "dropout grad " + k)


def test_limits_and_the_models_encoders(cell):
    """h = 1025 and t_in = 4097 are refused with the limit in the message; h = 1024 (every 256-unit chunk of the backward) and
    t_in = 4096 run, the former also checked against float64 at the project's bound; LSTM: the model's bilstm runs."""
    cls = _cls(cell)
    one = (torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long))
    torch.manual_seed(5)
    with pytest.raises(RuntimeError, match="1024"):
        cls(4, 1025).to(DEV).eval()((torch.zeros(1, 3, 4, device=DEV), torch.tensor([3]), *one))
    with pytest.raises(RuntimeError, match="4096"):
        cls(4, 4).to(DEV).eval()((torch.zeros(1, 4097, 4, device=DEV), torch.tensor([4097]), *one))
    m = cls(4, 1024, bidirectional=True).to(DEV).eval()
    gen = torch.Generator().manual_seed(6)
    x, lens = torch.randn(1, 3, 4, generator=gen), torch.tensor([3])
    gy, gh, y64, h64, g64 = _against_float64(cell, m, x, lens, 3, 7, "h1024")
    y, h, grads = _run(m, x, lens, one, 3, gy, gh)
    rel_close(y, y64, 2e-5, "h1024 y")
    rel_close(h, h64, 2e-5, "h1024 h")
    for k in grads:
        rel_close(grads[k], g64[k], 2e-5, "h1024 grad " + k)
    m = cls(4, 4).to(DEV).eval()
    x, lens = torch.randn(1, 4096, 4, generator=gen), torch.tensor([4096])
    y, h, grads = _run(m, x, lens, one, 4096, torch.ones(1, 4096, 4), torch.ones(1, 4))
    assert y.shape == (1, 4096, 4) and all(bool(torch.isfinite(v).all()) for v in [y, h, *grads.values()])
    assert bool((y[0, -1] == h[0]).all())
    if cell.module != "LSTM":
        return
    # the model's recurrent encoders (graph_based_semantic_structure.py:127-142 calls them with max_len)
    from get_amd import modules
    from get_amd.synth import make_embeddings
    from oracle.cases_model import MODEL_CASES
    cfg, seed = MODEL_CASES["small"]
    emb, art, clm = make_embeddings(cfg, seed)
    model = modules.Graph_basedSemantiStructure(cfg.model_params(emb, art, clm)).to(DEV).eval()
    D, H = model.bilstm.rnn.input_size, model.bilstm.rnn.hidden_size
    lens = torch.tensor([7, 100, 31])
    y, h = model.bilstm((torch.randn(3, 100, D, generator=gen).to(DEV), lens, *_pair(lens)), max_len=100)
    assert y.shape == (3, 100, 2 * H) and h.shape == (3, 2 * H) and bool(torch.isfinite(y).all())
    assert bool((y[0, 7:] == 0).all()) and bool((y[0, 6, :H] == h[0, :H]).all()) and bool((y[0, 0, H:] == h[0, H:]).all())

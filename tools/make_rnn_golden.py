"""Golden vectors of the two sequence encoders (Models/BiDAF/wrapper.py: LSTM :229-276, GRU :279-327), captured from the
upstream reference in the build container -- never on the GPU machine, and no test reads the reference.

    python tools/make_rnn_golden.py --cell lstm|gru

Loads the reference's ``Models/BiDAF/wrapper.py`` (it imports only torch) from the directory ``oracle/_refshim.py`` points
at, runs every case in fp32 on the CPU in eval() mode, and writes

    --cell lstm   tests/golden/g14_lstm.npz   tests/golden/lstm_contract.json
    --cell gru    tests/golden/g16_gru.npz    tests/golden/gru_contract.json

(the archive: every case below; the contract: constructor kwargs and state_dict key / shape lists of every configuration).

The reference's ``GRU.__init__`` raises as written: ``reset_params`` ends with ``bias_hh.chunk(4)[1].fill_(1)`` in place on a
leaf parameter that requires grad.  ``GRU.forward`` is fine.  The generator defines a subclass at run time that runs the
reference's ``reset_params`` unchanged inside ``torch.no_grad()`` -- the one-line repair any user of the class makes -- and
asserts what it leaves in ``bias_hh`` (ones on elements [ceil(3H/4), 2 ceil(3H/4)), zeros elsewhere) before the biases are
reseeded.

Cases (RNN = LSTM or GRU; B sequences of padded length L; the index pair is the stable argsort by descending length and its
inverse):
  bi_b5            RNN(12, 8, bidirectional=True), B=5, L=21, lengths [21, 9, 9, 1, 14] (a length of 1, a duplicate), max_len=None
  bi_b5_max25      the same with max_len=25: rows [21, 25) of y are a zero tail beyond L
  uni_h5           RNN(6, 5), B=3, L=7: no width is a multiple of 4
  two_layers       RNN(12, 8, num_layers=2, bidirectional=True), B=4, L=10
  bi_b37           RNN(10, 12, bidirectional=True), B=37, L=20, unsorted lengths: two full 16-sequence tiles and a partial one;
                   also ``h_raw``, the second value with return_h=False
  bi_l70           RNN(8, 8, bidirectional=True), B=2, L=70: crosses 64 steps
  bi_b5_saturated  bi_b5 with x scaled by 30: saturated gates

Weights keep the reference's init (orthogonal / kaiming-normal); bias_ih and bias_hh are seeded, non-zero and distinct, so a
dropped bias shows.  Per case ``<case>::``: ``x``, ``lens``, ``new_indices``, ``restoring_indices``, every parameter
(``param::<name>``), ``y``, ``h``, the seeded upstream gradients ``gy`` / ``gh`` of the loss sum(y * gy) + sum(h * gh), and the
gradients of x (``grad::x``) and of every parameter (``grad::<name>``).

Every case also runs in float64, and the reference's own fp32 result must lie within one tenth of the tolerance the tests
apply (1e-5 + 1e-4 |want| elementwise), so the fixture never eats the test's margin.  The exceptions, printed on every run: the
weight_ih gradients of bi_b5_saturated are sums of products with the 30-fold inputs that cancel, and the reference's own fp32
result sits at 0.37 (LSTM; 0.3 - 0.54 over seven other seeds of the inputs, so no seed helps) and 0.27 (GRU) of the bound
there; the GRU's of bi_b37 are sums over 37 x 20 rows that sit at 0.11.  For these groups of tensors (``capped`` below) the
generator asserts <= 0.6 of the bound, and a tenth for everything else.  The tests' bound is the same for all tensors.
"""
import argparse
import json
import os
import zlib

import numpy as np
import torch

from golden_common import OUT, load_reference, margin, to_numpy, write_contract, write_npz

B37_LENS = [7, 20, 3, 12, 1, 16, 9, 9, 20, 5, 14, 2, 18, 11, 6, 20, 4, 13, 8, 17, 10, 1, 15, 19, 3, 12, 7, 20, 6, 9, 2, 16, 11, 5, 14, 8,
            13]
BI_B5 = dict(kw=dict(input_size=12, hidden_size=8, bidirectional=True), L=21, lens=[21, 9, 9, 1, 14])
CASES = {
    "bi_b5": dict(BI_B5, max_len=None),
    "bi_b5_max25": dict(BI_B5, max_len=25),
    "uni_h5": dict(kw=dict(input_size=6, hidden_size=5), L=7, lens=[7, 3, 5], max_len=None),
    "two_layers": dict(kw=dict(input_size=12, hidden_size=8, num_layers=2, bidirectional=True), L=10, lens=[10, 4, 7, 2], max_len=None),
    "bi_b37": dict(kw=dict(input_size=10, hidden_size=12, bidirectional=True), L=20, lens=B37_LENS, max_len=None, raw=True),
    "bi_l70": dict(kw=dict(input_size=8, hidden_size=8, bidirectional=True), L=70, lens=[66, 70], max_len=None),
    "bi_b5_saturated": dict(BI_B5, max_len=None, scale=30.0, seed_as="bi_b5"),
}
TOL = (1e-5, 1e-4)      # the tests' bound: atol + rtol |want|, elementwise, outputs and gradients alike


def runnable_gru(ref):
    """The reference's GRU with its reset_params run unchanged under no_grad (as written, its in-place fill of a view of a leaf
    parameter raises).  Defined at run time: no reference text lives here."""
    class G(ref.GRU):
        def reset_params(self):
            with torch.no_grad():
                super().reset_params()
    return G


def gru_biases_as_reset(m, H):
    """What the reference's reset_params leaves in the GRU's biases."""
    q = -(-3 * H // 4)
    for k, p in m.named_parameters():
        if "bias_hh" in k:
            want = torch.zeros(3 * H)
            want[q:2 * q] = 1
            assert torch.equal(p.detach(), want), k
        elif "bias_ih" in k:
            assert bool((p == 0).all()), k


# per cell: the reference class, the assertion on the constructed module's biases, the cases whose weight_ih gradients get the
# 0.6 cap, the files written
CELLS = {
    "lstm": dict(cls=lambda ref: ref.LSTM, check=lambda m, H: None, capped=("bi_b5_saturated",),
                 npz="g14_lstm.npz", contract="lstm_contract.json"),
    "gru": dict(cls=runnable_gru, check=gru_biases_as_reset, capped=("bi_b5_saturated", "bi_b37"),
                npz="g16_gru.npz", contract="gru_contract.json"),
}


def run(cell, ref, name, spec, dtype):
    seed = zlib.crc32(spec.get("seed_as", name).encode())
    torch.manual_seed(seed)
    m = cell["cls"](ref)(**spec["kw"])
    cell["check"](m, spec["kw"]["hidden_size"])
    g = torch.Generator().manual_seed(seed ^ 0x5EED)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if "bias" in k:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
    m = m.to(dtype).eval()
    lens = torch.tensor(spec["lens"], dtype=torch.int64)
    B, L = len(spec["lens"]), spec["L"]
    x = (torch.randn(B, L, spec["kw"]["input_size"], generator=g) * spec.get("scale", 1.0)).to(dtype).requires_grad_(True)
    new = torch.sort(lens, descending=True, stable=True)[1]
    restoring = torch.argsort(new)
    y, h = m((x, lens, new, restoring), max_len=spec["max_len"])
    # upstream gradients on a grid of sixteenths in [-1, 1] (they compress; the archive stays below 300 KB)
    gy = torch.randint(-16, 17, y.shape, generator=g).float() / 16
    gh = torch.randint(-16, 17, h.shape, generator=g).float() / 16
    ((y * gy.to(dtype)).sum() + (h * gh.to(dtype)).sum()).backward()
    res = {"x": x, "lens": lens.numpy().astype(np.int32), "new_indices": new.numpy(), "restoring_indices": restoring.numpy(),
           "y": y, "h": h, "gy": gy, "gh": gh, "grad::x": x.grad}
    for k, p in m.named_parameters():
        res["param::" + k] = p
        res["grad::" + k] = p.grad
    if spec.get("raw"):
        with torch.no_grad():
            res["h_raw"] = m((x, lens, new, restoring), return_h=False, max_len=spec["max_len"])[1]
    return m, to_numpy(res)


def bound(k, want):
    return TOL[0] + TOL[1] * np.abs(want)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", choices=sorted(CELLS), required=True)
    cell = CELLS[ap.parse_args().cell]
    ref = load_reference("Models/BiDAF/wrapper.py", "ref_bidaf_wrapper")
    torch.set_num_threads(1)
    store, contract = {}, {}
    for name, spec in CASES.items():
        m, r32 = run(cell, ref, name, spec, torch.float32)
        _, r64 = run(cell, ref, name, spec, torch.float64)
        cancelling = [k for k in r32 if k.startswith("grad::rnn.weight_ih")] if name in cell["capped"] else []
        checked = [k for k in r32 if k in ("y", "h", "h_raw") or k.startswith("grad::")]
        worst = margin(r32, r64, [k for k in checked if k not in cancelling], bound)
        print(f"{name}: fp32 reference at {worst:.3f} of a tenth of the bound")
        assert worst <= 1.0, (name, worst)
        if cancelling:
            w = 0.1 * margin(r32, r64, cancelling, bound)
            print(f"{name}: weight_ih gradients (long cancelling sums): fp32 reference at {w:.3f} of the bound")
            assert w <= 0.6, (name, w)
        assert all(np.isfinite(v).all() for v in r32.values())
        contract[name] = {"kwargs": spec["kw"], "max_len": spec["max_len"],
                          "state_dict": [[k, list(v.shape)] for k, v in m.state_dict().items()]}
        for k, v in r32.items():
            store[f"{name}::{k}"] = v
    store["meta"] = np.frombuffer(json.dumps({"cases": list(CASES)}).encode(), dtype=np.uint8)
    write_npz(os.path.join(OUT, cell["npz"]), store)
    write_contract(os.path.join(OUT, cell["contract"]), contract)
    for f in (cell["npz"], cell["contract"]):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")
    assert os.path.getsize(os.path.join(OUT, cell["npz"])) < 300 * 1024


if __name__ == "__main__":
    main()

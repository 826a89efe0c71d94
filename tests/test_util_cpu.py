"""The comparison and fixture helpers of tests/util.py themselves: a check that cannot fail hides every other failure, so
each one is shown to pass just inside its bound and to raise just outside it, on a NaN, on an inf and on a shape mismatch."""
import os

import pytest
import torch

from tests import util
from tests.util import bits_equal, golden_ratio, load_golden, rel_close

ATOL, RTOL = 1e-5, 1e-4


def _at(fraction, index=None):
    """(got, want) of shape 3 x 5 with every element, or only the one at `index`, at `fraction` of its elementwise bound."""
    want = torch.linspace(-2.0, 3.0, 15, dtype=torch.float64).reshape(3, 5)
    step = fraction * (ATOL + RTOL * want.abs())
    if index is not None:
        only = torch.zeros_like(want)
        only[index] = 1.0
        step = step * only
    return want + step, want


def test_golden_ratio_passes_inside_the_bound_and_returns_the_fraction():
    got, want = _at(0.99)
    assert golden_ratio(got, want, ATOL, RTOL, "inside") == pytest.approx(0.99, rel=1e-6)
    assert golden_ratio(want.numpy(), want.numpy(), ATOL, RTOL, "numpy operands") == 0.0


@pytest.mark.parametrize("bad", ["outside", "nan", "inf", "shape"])
def test_golden_ratio_raises(bad):
    got, want = _at(1.01, (1, 3)) if bad == "outside" else _at(0.0)
    if bad == "nan":
        got[2, 0] = float("nan")
    elif bad == "inf":
        got[0, 4] = float("inf")
    elif bad == "shape":
        got = got[:, :4]
    with pytest.raises(AssertionError):
        golden_ratio(got, want, ATOL, RTOL, bad)


def test_rel_close_bound_and_floor():
    want = torch.tensor([[0.5, -4.0], [2.0, 0.0]], dtype=torch.float64)
    off = torch.zeros_like(want)
    off[1, 1] = 1e-3 * 4.0          # tol * max |want|, placed on the smallest entry: the bound is per tensor
    assert rel_close(want + 0.99 * off, want, 1e-3, "inside") == pytest.approx(0.99e-3, rel=1e-6)
    with pytest.raises(AssertionError):
        rel_close(want + 1.01 * off, want, 1e-3, "outside")
    with pytest.raises(AssertionError):                                  # a floor does not widen a non-zero scale
        rel_close(want + 1.01 * off, want, 1e-3, "floor ignored", floor=1e6)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(AssertionError):
            rel_close(torch.full_like(want, bad), want, 1e-3, "not finite")
    with pytest.raises(AssertionError):
        rel_close(want[:1], want, 1e-3, "shape")
    # an identically zero result: only the floor gives an error something to be relative to
    zero = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(AssertionError):
        rel_close(zero + 1e-9, zero, 1e-3, "zero, no floor")
    rel_close(zero + 0.99e-3, zero, 1e-3, "zero, floor", floor=1.0)
    with pytest.raises(AssertionError):
        rel_close(zero + 1.01e-3, zero, 1e-3, "zero, floor", floor=1.0)
    # the guarded mode refuses a floor for a result that is not numerically zero
    rel_close(zero + 0.99e-3, zero, 1e-3, "guarded", floor=1.0, floor_replaces_zero=True)
    with pytest.raises(AssertionError):
        rel_close(want, want, 1e-3, "guarded, non-zero", floor=1e6, floor_replaces_zero=True)


def test_rel_close_records_the_ratio_of_a_family():
    fam = "test_util_cpu"
    util.WORST.pop(fam, None)
    want = torch.tensor([1.0, -2.0], dtype=torch.float64)
    rel_close(want + torch.tensor([0.0, 2e-6]), want, 1e-4, "first", fam=fam)
    assert util.WORST[fam] == pytest.approx(1e-6, rel=1e-6)
    rel_close(want, want, 1e-4, "second", fam=fam)
    assert util.WORST[fam] == pytest.approx(1e-6, rel=1e-6)          # the worst so far, not the last
    util._rel(want + torch.tensor([4e-6, 0.0]), want, "through _rel", fam)
    assert util.WORST.pop(fam) == pytest.approx(2e-6, rel=1e-6)
    with pytest.raises(AssertionError):
        util._rel(want + 1.01 * util.TOL * 2.0, want, "outside TOL", fam)
    util.WORST.pop(fam)


def test_bits_equal_tells_the_zeros_apart():
    a = torch.tensor([[0.0, 1.5], [-3.0, float("nan")]])
    bits_equal(a, a.clone(), "same bits")
    bits_equal(a.t(), a.t().clone(), "not contiguous")
    b = a.clone()
    b[0, 0] = -0.0
    assert b[0, 0] == a[0, 0]
    with pytest.raises(AssertionError):
        bits_equal(a, b, "+0.0 and -0.0")
    with pytest.raises(AssertionError):
        bits_equal(a, a[:1], "shape")
    with pytest.raises(AssertionError):
        util._same([None, a], [None, b], "through _same")
    util._same([None, a], [b, a.clone()], "an output that is not there is skipped")


def test_load_golden_reads_a_file_once():
    golden_dir = os.path.join(util.ROOT, "tests", "golden")
    first = load_golden(golden_dir, "g11_gcn.npz", "encoder_contract.json")
    again = load_golden(golden_dir, "g11_gcn.npz", "encoder_contract.json")
    z, meta, contract = first
    assert again[0] is z and again[1] is meta and again[2] is contract
    assert isinstance(z, dict) and "meta" in z and meta["gcn_cases"] and set(meta["gcn_cases"]) <= set(contract)
    assert load_golden(golden_dir, "g11_gcn.npz")[2] is None

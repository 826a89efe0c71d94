"""The CPU-side checks of the GRU encoder under the test ids this file always had.  The checks themselves live once, for both
cells, in tests/test_rnn_cpu.py."""
import pytest

from tests import test_rnn_cpu as rnn
from tests.rnn_ref import CELLS

CELL = CELLS["gru"]


def test_gru_golden_archive_is_complete(golden_dir):
    rnn.test_golden_archive_is_complete(golden_dir, CELL)


@pytest.mark.parametrize("name", rnn.CASES)
def test_float64_restatement_reproduces_the_gru_goldens(golden_dir, name):
    rnn.test_float64_restatement_reproduces_the_goldens(golden_dir, CELL, name)


def test_gru_state_dicts_match_the_reference_contract(golden_dir):
    rnn.test_state_dicts_match_the_reference_contract(golden_dir, CELL)


def test_header_declares_and_binding_matches_the_gru_entries():
    rnn.test_header_declares_and_binding_matches_the_entries(CELL)


def test_gru_refuses_cpu_tensors_and_bad_lengths():
    rnn.test_refuses_cpu_tensors_and_bad_lengths(CELL)

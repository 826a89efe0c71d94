"""The GRU encoder against the reference's goldens under the test ids this file always had.  The check itself lives once, for
both cells, in tests/test_gpu_rnn.py, with the other GPU checks of the two encoders."""
import pytest

from tests import test_gpu_rnn as rnn
from tests.rnn_ref import CELLS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", rnn.CASES)
def test_gru_matches_reference_goldens(golden_dir, name):
    rnn.test_matches_reference_goldens(golden_dir, CELLS["gru"], name)

"""tests/test_front_end_cpu.py with the model on the GPU: the calls that refuse a CPU model get past the device check here, and the record
holds what they hand to the engine (labels drawn, self.rng seeded, seeds and parameters spread).  The engine is a stub: no kernel runs."""
import pytest

from tests import frontcases

pytestmark = pytest.mark.gpu


def test_front_end_gpu():
    outcomes, _ = frontcases.record('cuda')
    same, moved = frontcases.compare('gpu', outcomes)
    print(same, 'cases as recorded,', moved, 'in UNIFIED')

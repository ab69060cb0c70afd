"""The F(4x4,3x3) input-transform pass writing V with non-temporal stores, on the MI355X: the checks of tests/_fir_v_checks.py
(shared with the CPU-emulated suite, tests/test_fir_v_cpu.py) -- V bit for bit that of plain stores and within rounding of fp64."""
import pytest

import _fir_v_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("prologue", K.PROLOGUES)
@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c[0])
def test_streamed_v_keeps_the_bits(case, prologue):
    K.check_streamed_v("cuda", case, prologue)


def test_pass_entry_refusals():
    K.check_entry_refusals("cuda")

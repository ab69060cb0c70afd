"""The F(4x4,3x3) input-transform pass writing V with non-temporal stores, under the test-only CPU emulator (tests/emu/): V bit
for bit that of plain stores and within rounding of fp64, and the shape of the lowered CIFAR-10 program.  Same checks as
tests/test_fir_v_gpu.py; see tests/_fir_v_checks.py for what is compared and the bounds."""
import pytest

import emu
import _fir_v_checks as K

needs_emu = pytest.mark.skipif(not emu.available(), reason="emulator needs x86-64 + ROCm's clang++")


def test_cifar_program_keeps_its_shape(monkeypatch):
    K.check_cifar_program_shape(monkeypatch)


@needs_emu
@pytest.mark.parametrize("prologue", K.PROLOGUES)
@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c[0])
def test_streamed_v_keeps_the_bits(case, prologue):
    with emu.emulated():
        K.check_streamed_v("cpu", case, prologue)


@needs_emu
def test_pass_entry_refusals():
    with emu.emulated():
        K.check_entry_refusals("cpu")

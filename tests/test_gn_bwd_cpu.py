"""GroupNorm backward of the 4-channel-multiple path and ssde_prologue_bwd (CPU): the kernels of backward.hip under the test-only
emulator (tests/emu/) against fp64 autograd at wide groups, straddled concat boundaries, ragged pixel counts and ragged runs of
groups, with and without dropout, on the one-pass kernel and on the three kernels.  See tests/_gn_bwd_checks.py."""
import pytest

import emu
import _gn_bwd_checks as K

needs_emu = pytest.mark.skipif(not emu.available(), reason="emulator needs x86-64 + ROCm's clang++")


@pytest.fixture
def emulated():
    with emu.emulated():
        yield


@needs_emu
@pytest.mark.parametrize("case", K.GN_CASES, ids=K.case_id)
def test_gn_backward_against_fp64(emulated, case):
    K.check_gn_backward("cpu", case)


@needs_emu
@pytest.mark.parametrize("case", K.CALL_FORM_CASES, ids=K.case_id)
def test_gn_backward_call_forms(emulated, case):
    K.check_gn_call_forms("cpu", case)


@needs_emu
@pytest.mark.parametrize("dropout", [False, True], ids=["no-dropout", "dropout"])
@pytest.mark.parametrize("case", K.PROLOGUE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_prologue_bwd_alone(emulated, case, dropout):
    K.check_prologue_bwd("cpu", case, dropout)

"""GroupNorm backward of the 4-channel-multiple path and ssde_prologue_bwd on the MI355X: the kernels of backward.hip against
fp64 autograd at wide groups, straddled concat boundaries, ragged pixel counts and ragged runs of groups, with and without
dropout, on the one-pass kernel and on the three kernels.  Every test runs in both matrix modes (tests/conftest.py); these
kernels take no matrix mode.  Checks: tests/_gn_bwd_checks.py."""
import pytest

import _gn_bwd_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", K.GN_CASES, ids=K.case_id)
def test_gn_backward_against_fp64(case):
    K.check_gn_backward("cuda", case)


@pytest.mark.parametrize("case", K.CALL_FORM_CASES, ids=K.case_id)
def test_gn_backward_call_forms(case):
    K.check_gn_call_forms("cuda", case)


@pytest.mark.parametrize("dropout", [False, True], ids=["no-dropout", "dropout"])
@pytest.mark.parametrize("case", K.PROLOGUE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_prologue_bwd_alone(case, dropout):
    K.check_prologue_bwd("cuda", case, dropout)

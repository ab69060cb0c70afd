"""The 3x3 convolution routes and the weight-gradient routes on irregular maps, on the MI355X: every route of ssde_conv2d and
every SSDE_WGRADF_* form against fp64 at rectangular maps, partial tile columns and rows, several images per workgroup with a
ragged batch tail, strides, end padding, crops, explicit splits; GroupNorm partials against the fp64 statistics of the fp64
reference output.  Every test runs in both matrix modes (tests/conftest.py).  Checks: tests/_conv_shape_checks.py."""
import pytest

import _conv_shape_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", K.FWD_CASES, ids=K.fwd_id)
def test_forward_route_against_fp64(case):
    K.check_forward_case("cuda", case)


@pytest.mark.parametrize("case,word", K.REFUSALS, ids=lambda v: K.fwd_id(v) if isinstance(v, K.Fwd) else None)
def test_forward_plan_refuses_outside_the_limits(case, word):
    K.check_refusal(case, word)


@pytest.mark.parametrize("case", K.WGRAD_CASES, ids=K.wg_id)
def test_wgrad_route_against_fp64(case):
    K.check_wgrad("cuda", case)


@pytest.mark.parametrize("case", K.V_CASES, ids=K.v_id)
def test_forward_v_feeds_the_weight_gradient(case):
    K.check_v_handover("cuda", case)

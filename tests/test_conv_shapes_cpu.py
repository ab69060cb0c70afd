"""The 3x3 convolution routes and the weight-gradient routes on irregular maps (CPU): the kernels under the test-only emulator
(tests/emu/) against fp64 -- rectangular maps, partial tile columns and rows, several images per workgroup with a ragged batch
tail, strides, end padding, crops, explicit splits -- the refusals of the plans just outside each route's limits, and a seeded
sweep over the shapes the plans accept.  See tests/_conv_shape_checks.py."""
import pytest

import emu
import _conv_shape_checks as K

needs_emu = pytest.mark.skipif(not emu.available(), reason="emulator needs x86-64 + ROCm's clang++")


@pytest.fixture
def emulated():
    with emu.emulated():
        yield


def test_rows_hit_the_tiling_states_they_are_listed_for():
    K.check_table_states()


@needs_emu
@pytest.mark.parametrize("case", K.FWD_CASES, ids=K.fwd_id)
def test_forward_route_against_fp64(emulated, case):
    K.check_forward_case("cpu", case)


@needs_emu
@pytest.mark.parametrize("case,word", K.REFUSALS, ids=lambda v: K.fwd_id(v) if isinstance(v, K.Fwd) else None)
def test_forward_plan_refuses_outside_the_limits(emulated, case, word):
    K.check_refusal(case, word)


@needs_emu
def test_small_cout_route_hands_the_rest_to_the_direct_kernel(emulated):
    K.check_small_edges()


@needs_emu
@pytest.mark.parametrize("case", K.WGRAD_CASES, ids=K.wg_id)
def test_wgrad_route_against_fp64(emulated, case):
    K.check_wgrad("cpu", case)


@needs_emu
@pytest.mark.parametrize("case,word", K.WG_REFUSALS, ids=lambda v: K.wg_id(v) if isinstance(v, K.Wg) else None)
def test_wgrad_plan_refuses_outside_the_limits(emulated, case, word):
    K.check_wgrad_refusal(case, word)


@needs_emu
@pytest.mark.parametrize("case", K.V_CASES, ids=K.v_id)
def test_forward_v_feeds_the_weight_gradient(emulated, case):
    K.check_v_handover("cpu", case)


@needs_emu
def test_seeded_sweep_of_accepted_shapes(emulated):
    K.check_sweep("cpu")

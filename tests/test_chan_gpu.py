"""config.data.num_channels = C for any C >= 1 on the MI355X: the wide image-head launches of conv_small.hip against fp64 and
against the direct kernel, routing, whole forwards, gradients and the input gradient against the reference's, the PC sampler
(op by op and as hipGraph replays), inpainting with a mask over some channels, plans and one likelihood evaluation.
Checks: tests/_chan_checks.py."""
import pytest

import _chan_checks as K
import _chan_cases as CC

pytestmark = pytest.mark.gpu
source_id = lambda s: "%d+%d" % s       # noqa: E731


@pytest.mark.parametrize("source", K.HEAD_SOURCES, ids=source_id)
@pytest.mark.parametrize("cout", K.HEAD_COUTS)
def test_head_launches_against_fp64_and_the_direct_kernel(cout, source):
    K.check_head_launches("cuda", cout, source)


def test_head_routing_and_abi():
    K.check_head_routing("cuda")


@pytest.mark.parametrize("c", [6, 8, 13])
def test_lowering_of_wide_counts(c):
    K.check_lowering_wide_counts(c)


@pytest.mark.parametrize("case", list(CC.FORWARD_CASES))
def test_forward_against_the_reference(case):
    K.check_forward("cuda", case)


@pytest.mark.parametrize("wino", ["0", "4"])       # direct kernels everywhere, F(4x4,3x3) wherever legal (the default: above)
@pytest.mark.parametrize("case", ["ffhq_c8", "ncsnpp_c13"])
def test_forward_against_the_reference_on_every_route(case, wino, monkeypatch):
    monkeypatch.setenv("SSDE_WINOGRAD", wino)
    K.check_forward("cuda", case)


@pytest.mark.parametrize("case", list(CC.TRAIN_CASES))
def test_loss_and_gradients_against_the_reference(case):
    K.check_loss_and_gradients("cuda", case)


@pytest.mark.parametrize("case", list(CC.TRAIN_CASES))
def test_input_gradient_against_the_reference(case):
    K.check_input_gradient("cuda", case)


def test_sampler():
    K.check_sampler("cuda", B=2)


def test_inpainting_with_a_mask_over_some_channels():
    K.check_inpainting("cuda", B=2)


def test_colorizer_refuses_six_channels_before_any_launch():
    K.check_refusals()


@pytest.mark.parametrize("case", ["ncsnpp_c6", "ffhq_c8"])       # C = 6; and a head per level with the output pyramid at C = 8
def test_unet_plan_round_trip(case):
    K.check_unet_plan_round_trip("cuda", case)


def test_train_plan_round_trip():
    K.check_train_plan_round_trip("cuda")


def test_sampler_plan_with_inpainting_round_trip():
    K.check_sampler_plan_round_trip("cuda")


def test_ode_plan_round_trip():
    K.check_ode_plan_round_trip("cuda")


def test_likelihood():
    K.check_likelihood("cuda")

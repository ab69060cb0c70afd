"""config.data.num_channels = C for any C >= 1 (CPU): state-dict names against the reference's, the refusals, dry lowering, and --
under the test-only emulator (tests/emu/) -- the wide image-head launches of conv_small.hip against fp64, whole forwards,
gradients and the input gradient against the reference's, the PC sampler and inpainting, plans and one likelihood evaluation.
See tests/_chan_checks.py."""
import pytest

import emu
import _chan_checks as K
import _chan_cases as CC

needs_emu = pytest.mark.skipif(not emu.available(), reason="emulator needs x86-64 + ROCm's clang++")
source_id = lambda s: "%d+%d" % s       # noqa: E731


@pytest.fixture
def emulated():
    with emu.emulated():
        yield


@pytest.mark.parametrize("case", list(CC.FORWARD_CASES))
def test_state_dict_names_equal_the_reference(case):
    K.check_state_dict_names(case)


def test_refusals():
    K.check_refusals()


@needs_emu
@pytest.mark.parametrize("source", K.HEAD_SOURCES, ids=source_id)
@pytest.mark.parametrize("cout", K.HEAD_COUTS)
def test_head_launches_against_fp64_and_the_direct_kernel(emulated, cout, source):
    K.check_head_launches("cpu", cout, source)


@needs_emu
def test_head_routing_and_abi(emulated):
    K.check_head_routing("cpu")


@needs_emu
@pytest.mark.parametrize("c", [1, 3, 4])
def test_lowering_of_small_counts_is_unchanged(emulated, c):
    K.check_lowering_small_counts(c)


@needs_emu
@pytest.mark.parametrize("c", [6, 8, 13])
def test_lowering_of_wide_counts(emulated, c):
    K.check_lowering_wide_counts(c)


@needs_emu
@pytest.mark.parametrize("case", list(CC.FORWARD_CASES))
def test_forward_against_the_reference(emulated, case):
    K.check_forward("cpu", case, batch=1 if CC.family(case) == "ddpm" else None)     # (nf = 128: one image on the emulator)


@needs_emu
@pytest.mark.parametrize("case", list(CC.TRAIN_CASES))
def test_loss_and_gradients_against_the_reference(emulated, case):
    K.check_loss_and_gradients("cpu", case)


@needs_emu
@pytest.mark.parametrize("case", list(CC.TRAIN_CASES))
def test_input_gradient_against_the_reference(emulated, case):
    K.check_input_gradient("cpu", case)


@needs_emu
def test_sampler(emulated):
    K.check_sampler("cpu", B=1)


@needs_emu
def test_inpainting_with_a_mask_over_some_channels(emulated):
    K.check_inpainting("cpu", B=1)


@needs_emu
@pytest.mark.parametrize("case", ["ncsnpp_c6", "ffhq_c8"])       # C = 6; and a head per level with the output pyramid at C = 8
def test_unet_plan_round_trip(emulated, case):
    K.check_unet_plan_round_trip("cpu", case)


@needs_emu
def test_train_plan_round_trip(emulated):
    K.check_train_plan_round_trip("cpu", n_steps=1)       # (a second step only repeats the first on the emulator; the GPU suite runs two)


@needs_emu
def test_sampler_plan_with_inpainting_round_trip(emulated):
    K.check_sampler_plan_round_trip("cpu", B=1)


@needs_emu
def test_ode_plan_round_trip(emulated):
    K.check_ode_plan_round_trip("cpu")


@needs_emu
def test_likelihood(emulated):
    K.check_likelihood("cpu")

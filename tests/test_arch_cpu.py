"""NCSN++ with DDPM residual blocks, the 'cat' combine and the residual input pyramid without FIR (CPU): the constructor, dry
lowering, and -- under the test-only emulator (tests/emu/) -- the concatenation launch, its program op and its adjoint bit for bit,
its refusals, whole forwards against the reference, gradients and the input gradient against the reference's, the PC sampler and
plans.  See tests/_arch_checks.py."""
import pytest

import emu
import _arch_checks as A

needs_emu = pytest.mark.skipif(not emu.available(), reason="emulator needs x86-64 + ROCm's clang++")
shape_id = lambda s: "%dx%dx%d+%d" % s       # noqa: E731


@pytest.fixture
def emulated():
    with emu.emulated():
        yield


@pytest.mark.parametrize("case", list(A.CASES))
def test_state_dict_names_equal_the_reference(case):
    A.check_state_dict_names(case)


def test_constructor_refusals():
    A.check_constructor_refusals()


@needs_emu
def test_lowering_shapes(emulated):
    A.check_lowering_shapes()


@needs_emu
def test_abi_unchanged(emulated):
    A.check_abi_unchanged()


@needs_emu
@pytest.mark.parametrize("shape", A.CONCAT_SHAPES, ids=shape_id)
def test_concat_launch(emulated, shape):
    A.check_concat_launch("cpu", shape)


@needs_emu
@pytest.mark.parametrize("shape", A.CONCAT_SHAPES, ids=shape_id)
def test_concat_program(emulated, shape):
    A.check_concat_program("cpu", shape)


@needs_emu
@pytest.mark.parametrize("shape", A.CONCAT_SHAPES, ids=shape_id)
def test_concat_adjoint(emulated, shape):
    A.check_concat_adjoint("cpu", shape)


@needs_emu
def test_concat_refusals(emulated):
    A.check_concat_refusals("cpu")


@needs_emu
@pytest.mark.parametrize("case", list(A.CASES))
def test_forward_against_the_reference(emulated, case):
    A.check_forward("cpu", case)


@needs_emu
@pytest.mark.parametrize("case", list(A.TRAIN_CASES))
def test_loss_and_gradients_against_the_reference(emulated, case):
    A.check_loss_and_gradients("cpu", case)


@needs_emu
@pytest.mark.parametrize("case", list(A.TRAIN_CASES))
def test_input_gradient_against_the_reference(emulated, case):
    A.check_input_gradient("cpu", case)


@needs_emu
def test_sampler(emulated):
    A.check_sampler("cpu", B=1)


@needs_emu
def test_unet_plan_round_trip(emulated):
    A.check_unet_plan_round_trip("cpu")


@needs_emu
def test_train_plan_round_trip(emulated):
    A.check_train_plan_round_trip("cpu", n_steps=1)       # (a second step only repeats the first on the emulator; the GPU suite runs two)

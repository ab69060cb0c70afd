"""NCSN++ / DDPM++ with elu, relu and lrelu (CPU): the constructor, dry lowering, and -- under the test-only emulator
(tests/emu/) -- the apply launch and its adjoint with src.act against fp64, the activation alone, the refusals of the other
entry points, whole forwards against the reference, ELU gradients and training steps against the reference's run, and plans.
See tests/_act_checks.py."""
import pytest

import emu
import _act_checks as A

needs_emu = pytest.mark.skipif(not emu.available(), reason="emulator needs x86-64 + ROCm's clang++")


@pytest.fixture
def emulated():
    with emu.emulated():
        yield


def test_constructor():
    A.check_constructor()


def test_same_program_for_every_activation():
    A.check_same_program_for_every_activation()


@needs_emu
@pytest.mark.parametrize("side", A.KERNEL_MAPS)
@pytest.mark.parametrize("shape", A.KERNEL_SHAPES, ids=lambda s: "%d+%d_in_%d" % s)
@pytest.mark.parametrize("act", A.ACTS)
def test_kernels_against_fp64(emulated, act, shape, side):
    A.check_kernels("cpu", act, *shape, side)


@needs_emu
@pytest.mark.parametrize("shape", A.ACT_ONLY_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("act", ("swish",) + A.ACTS)
def test_activation_only(emulated, act, shape):
    A.check_act_only("cpu", act, shape)


@needs_emu
@pytest.mark.parametrize("shape", A.ACT_ONLY_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_activation_only_silu_is_the_fused_prologue(emulated, shape):
    A.check_act_only_silu_is_the_fused_prologue("cpu", shape)


@needs_emu
def test_refusals(emulated):
    A.check_refusals("cpu")


@needs_emu
@pytest.mark.parametrize("wino", ["0", "1", "4"])
@pytest.mark.parametrize("name", list(A.FORWARD_CASES))
def test_forward_against_the_reference(emulated, name, wino, monkeypatch):
    # 2e-6 on the emulator's exact-fp32 arithmetic where the existing emulator tests ask that (the direct kernels and the default
    # routes, tests/test_gn_width_cpu.py); F(4x4,3x3) everywhere rounds about five times coarser -- 2.5e-6 to 1.3e-5 on a whole
    # network (engine.Lowering.conv3_route) -- and keeps the whole-forward bound of its own emulator test
    # (tests/test_emulated_kernels.py::test_unet_forward_winograd_f4x4_kernel)
    monkeypatch.setenv("SSDE_WINOGRAD", wino)
    A.check_forward("cpu", name, tol=A.TOL_FWD if wino == "4" else 2e-6)


@needs_emu
def test_elu_loss_and_gradients_against_the_reference(emulated):
    A.check_loss_and_gradients("cpu")


@needs_emu
def test_elu_three_steps_against_the_reference_run(emulated, monkeypatch):
    """step_fn itself under the emulator: the product asks losses._on_device whether a tensor is HIP memory"""
    from score_sde_pytorch_amd import losses
    monkeypatch.setattr(losses, "_on_device", lambda t: True)
    A.check_train_steps_against_reference_run("cpu")


@needs_emu
def test_unet_plan_round_trip(emulated):
    A.check_unet_plan_round_trip("cpu")


@needs_emu
def test_train_plan_round_trip(emulated):
    A.check_train_plan_round_trip("cpu", n_steps=1)       # (a second step only repeats the first on the emulator; the GPU suite runs two)


@needs_emu
def test_pc_plan_matches_pc_engine(emulated):
    A.check_pc_plan("cpu", B=1)

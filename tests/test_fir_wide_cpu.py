"""FIR resampling with any kernel under the test-only CPU emulator (tests/emu/): ssde_upfirdn2d with up to 16 x 16 taps and
negative pads on all three kernels, score_sde_pytorch_amd.op.upfirdn2d, and networks with a 3-tap / 6-tap fir_kernel against
the reference's forwards and training run.  Same checks as tests/test_fir_wide_gpu.py; see tests/_fir_wide_checks.py for what
is compared and the bounds."""
import pytest
import torch

import emu
import _fir_util as FU
import _fir_wide_checks as K

needs_emu = pytest.mark.skipif(not emu.available(), reason="emulator needs x86-64 + ROCm's clang++")


def test_the_grid_skips_less_than_a_quarter():
    skipped, total = K.check_grid_is_mostly_runnable()
    assert total == 300


def test_dry_lowering_of_cifar_with_six_taps():
    K.check_dry_lowering_cifar()


def test_seventeen_tap_fir_kernel_is_refused_at_lowering():
    K.check_too_long_fir_kernel_raises()


@needs_emu
@pytest.mark.parametrize("taps", K.TAPS, ids=lambda t: "%dx%d" % t)
def test_op_grid(taps):
    with emu.emulated():
        K.check_op_grid("cpu", taps)


@needs_emu
def test_op_grid_four_taps_with_pads_whose_gradient_pads_are_negative():
    with emu.emulated():
        K.check_op_grid("cpu", (4, 4), pad55=True)


@needs_emu
def test_prologue_dual_output_and_accumulate():
    with emu.emulated():
        K.check_prologue_dual_accumulate("cpu")


@needs_emu
def test_refusals():
    with emu.emulated():
        K.check_refusals("cpu")


@needs_emu
def test_op_package():
    import score_sde_pytorch_amd.op as op
    assert op.upfirdn2d.__defaults__ == (1, 1, (0, 0))
    with pytest.raises(ValueError):
        op.upfirdn2d(torch.zeros(1, 3, 4, 4, device="meta"), torch.ones(17, 17))
    # the package refuses CPU tensors; under the emulator host memory is the device
    with emu.emulated():
        K.check_op_package("cpu", lambda input, kernel, up=1, down=1, pad=(0, 0):
                           op.UpFirDn2d.apply(input, kernel.to(torch.float32), up, down, (pad[0], pad[1])))


@needs_emu
@pytest.mark.parametrize("net", list(FU.FORWARD_NETS))
@pytest.mark.parametrize("fir", list(FU.FIR_KERNELS))
def test_forward_matches_reference_golden(fir, net):
    with emu.emulated():
        K.check_forward_golden("cpu", fir, net)


@needs_emu
def test_unet_plan_round_trip():
    with emu.emulated():
        K.check_unet_plan_round_trip("cpu")


@pytest.fixture
def host_is_device(monkeypatch):
    """step_fn itself under the emulator: the product asks losses._on_device whether a tensor is HIP memory"""
    from score_sde_pytorch_amd import losses
    monkeypatch.setattr(losses, "_on_device", lambda t: True)


@needs_emu
def test_training_loss_and_gradients_match_reference(host_is_device):
    with emu.emulated():
        FU.check_training_loss_and_gradients("cpu", FU.train_gold(), FU.TRAIN_NAME, FU.TRAIN_CASE)


@needs_emu
def test_step_fn_matches_the_reference_run(host_is_device):
    with emu.emulated():
        FU.check_step_fn_against_reference_run("cpu", FU.train_gold(), FU.TRAIN_NAME, FU.TRAIN_CASE)

"""FIR resampling with any kernel on the MI355X: the checks of tests/_fir_wide_checks.py (shared with the CPU-emulated suite,
tests/test_fir_wide_cpu.py) -- ssde_upfirdn2d with up to 16 x 16 taps and negative pads on all three kernels,
score_sde_pytorch_amd.op.upfirdn2d, and networks with a 3-tap / 6-tap fir_kernel against the reference's forwards, its
training run, and through exported plans."""
import pytest

import _fir_util as FU
import _fir_wide_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("taps", K.TAPS, ids=lambda t: "%dx%d" % t)
def test_op_grid(taps):
    K.check_op_grid("cuda", taps)


def test_op_grid_four_taps_with_pads_whose_gradient_pads_are_negative():
    K.check_op_grid("cuda", (4, 4), pad55=True)


def test_prologue_dual_output_and_accumulate():
    K.check_prologue_dual_accumulate("cuda")


def test_refusals():
    K.check_refusals("cuda")


def test_op_package():
    import score_sde_pytorch_amd.op as op
    K.check_op_package("cuda", op.upfirdn2d)


@pytest.mark.parametrize("wino", ["0", "2"])
@pytest.mark.parametrize("net", list(FU.FORWARD_NETS))
@pytest.mark.parametrize("fir", list(FU.FIR_KERNELS))
def test_forward_matches_reference_golden(fir, net, wino, monkeypatch):
    monkeypatch.setenv("SSDE_WINOGRAD", wino)
    K.check_forward_golden("cuda", fir, net)


def test_unet_plan_round_trip():
    K.check_unet_plan_round_trip("cuda")


def test_pc_sampler_plan_matches_python_sampler():
    K.check_pc_plan_matches_python_sampler()


def test_training_loss_and_gradients_match_reference():
    FU.check_training_loss_and_gradients("cuda", FU.train_gold(), FU.TRAIN_NAME, FU.TRAIN_CASE)


def test_step_fn_matches_the_reference_run():
    FU.check_step_fn_against_reference_run("cuda", FU.train_gold(), FU.TRAIN_NAME, FU.TRAIN_CASE)

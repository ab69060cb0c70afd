"""The input-gradient launches of the backward lowering (CPU): forward convolution kernels under the test-only emulator
(tests/emu/) on the output gradient, with the weights WeightStore.derived packs for them, written into NaN and accumulated in
place, against fp64 autograd -- every 3x3 route at stride 1, the transposed stride-2 form, the derived 1x1 matrices.
See tests/_dgrad_checks.py."""
import pytest

import emu
import _dgrad_checks as K

pytestmark = pytest.mark.skipif(not emu.available(), reason="emulator needs x86-64 + ROCm's clang++")


@pytest.fixture(autouse=True)
def _emulated():
    with emu.emulated():
        yield


@pytest.mark.parametrize("case", K.stride1_cases(), ids=K.stride1_id)
def test_stride1_input_gradient_on_every_route(case):
    K.check_stride1("cpu", case)


@pytest.mark.parametrize("case", K.STRIDE2_CASES, ids=K.stride2_id)
def test_stride2_input_gradient_by_zero_insertion_and_crop(case):
    K.check_stride2("cpu", case)


@pytest.mark.parametrize("case", K.MATRIX_CASES, ids=K.matrix_id)
def test_1x1_input_gradient_with_the_derived_matrix(case):
    K.check_matrix("cpu", case)

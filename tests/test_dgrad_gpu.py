"""The input-gradient launches of the backward lowering on the MI355X: forward convolution kernels on the output gradient,
with the weights WeightStore.derived packs for them on the device (ssde_pack_weights), written into NaN and accumulated in
place, against fp64 autograd -- every 3x3 route at stride 1, the transposed stride-2 form, the derived 1x1 matrices.  Every
test runs in both matrix modes (tests/conftest.py).  Checks: tests/_dgrad_checks.py."""
import pytest

import _dgrad_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", K.stride1_cases(), ids=K.stride1_id)
def test_stride1_input_gradient_on_every_route(case):
    K.check_stride1("cuda", case)


@pytest.mark.parametrize("case", K.STRIDE2_CASES, ids=K.stride2_id)
def test_stride2_input_gradient_by_zero_insertion_and_crop(case):
    K.check_stride2("cuda", case)


@pytest.mark.parametrize("case", K.MATRIX_CASES, ids=K.matrix_id)
def test_1x1_input_gradient_with_the_derived_matrix(case):
    K.check_matrix("cuda", case)

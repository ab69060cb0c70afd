"""Attention at 256 tokens and below on the MI355X: the single-tile kernels of attention.hip against fp64 at ragged and wide
shapes, the engine's forward -> backward chain, inert padding, bit reproducibility, a transposed-operand check of forward and
backward, ties and a dominated row.  Every test runs in both matrix modes (tests/conftest.py).  Checks:
tests/_attn_tile_checks.py."""
import pytest

import _attn_tile_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", K.CASES, ids=lambda s: "%dx%dx%d" % s)
def test_kernels_against_fp64(shape, monkeypatch):
    K.check_shape("cuda", *shape, monkeypatch)


@pytest.mark.parametrize("shape", K.CHAIN_CASES, ids=lambda s: "%dx%dx%d" % s)
def test_backward_of_the_kernels_own_forward(shape):
    K.check_chain("cuda", *shape)


def test_padding_is_inert():
    K.check_padding_is_inert("cuda")


def test_two_runs_agree_to_the_bit():
    K.check_reproducible("cuda")


def test_transpose_detecting():
    K.check_transpose_detecting("cuda")


def test_ties_and_a_dominated_row():
    K.check_ties_and_dominated_row("cuda")

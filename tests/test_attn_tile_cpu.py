"""Attention at 256 tokens and below (CPU): the single-tile kernels of attention.hip under the test-only emulator (tests/emu/)
against fp64 at ragged and wide shapes, the engine's forward -> backward chain, inert padding, bit reproducibility, a
transposed-operand check of forward and backward, ties and a dominated row.  See tests/_attn_tile_checks.py."""
import pytest

import emu
import _attn_tile_checks as K

needs_emu = pytest.mark.skipif(not emu.available(), reason="emulator needs x86-64 + ROCm's clang++")


@pytest.fixture
def emulated():
    with emu.emulated():
        yield


def _id(p):
    return "%dx%dx%d-%s" % (p[0] + (p[1],))


# every shape in f32 mode (all of them on attn_kernel); in bf16x6 mode only the shapes whose route differs (attn_x6_kernel: the
# backward takes no matrix mode, and the other shapes run the same kernels again)
SWEEP = [(s, "f32") for s in K.CASES] + [(s, "bf16x6") for s in K.CASES if s in K.X6_CASES]


@needs_emu
@pytest.mark.parametrize("case", SWEEP, ids=_id)
def test_kernels_against_fp64(emulated, case, monkeypatch):
    shape, matrix = case
    monkeypatch.setenv("SSDE_MATRIX", matrix)
    K.check_shape("cpu", *shape, monkeypatch)


# (2, 256, 256) takes attn_x6_kernel in bf16x6 mode, and the emulator adds the 16 products of a bf16 MFMA to the accumulator one
# at a time (test_emulated_kernels.py), so its forward error -- which this chain passes into D = dO . O -- is not the hardware's:
# the chain through attn_x6_kernel is held to the tolerance on the GPU only
@needs_emu
@pytest.mark.parametrize("shape", K.CHAIN_CASES, ids=lambda s: "%dx%dx%d" % s)
def test_backward_of_the_kernels_own_forward(emulated, shape, monkeypatch):
    monkeypatch.setenv("SSDE_MATRIX", "f32")
    K.check_chain("cpu", *shape)


@needs_emu
def test_padding_is_inert(emulated):
    K.check_padding_is_inert("cpu")


@needs_emu
def test_two_runs_agree_to_the_bit(emulated):
    K.check_reproducible("cpu")


def test_transpose_detecting_inputs_select_about_half():
    """the reference alone: the softened backward inputs give a largest softmax weight inside 0.3 .. 0.7"""
    _, _, wmax = K.transpose_backward_inputs()
    assert 0.3 < wmax < 0.7, wmax


@needs_emu
def test_transpose_detecting(emulated):
    K.check_transpose_detecting("cpu")


@needs_emu
def test_ties_and_a_dominated_row(emulated):
    K.check_ties_and_dominated_row("cpu")

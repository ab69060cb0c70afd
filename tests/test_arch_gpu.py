"""NCSN++ with DDPM residual blocks, the 'cat' combine and the residual input pyramid without FIR on the MI355X: the
concatenation launch, its program op and its adjoint bit for bit, its refusals, whole forwards against the reference (the 'cat'
network on every 3x3 route), gradients and the input gradient against the reference's, training steps as one hipGraph and as
program runs, the PC sampler and plans.  Checks: tests/_arch_checks.py."""
import pytest
import torch

import _arch_checks as A

pytestmark = pytest.mark.gpu
shape_id = lambda s: "%dx%dx%d+%d" % s       # noqa: E731


def test_abi_unchanged():
    A.check_abi_unchanged()


@pytest.mark.parametrize("shape", A.CONCAT_SHAPES, ids=shape_id)
def test_concat_launch(shape):
    A.check_concat_launch("cuda", shape)


@pytest.mark.parametrize("shape", A.CONCAT_SHAPES, ids=shape_id)
def test_concat_program(shape):
    A.check_concat_program("cuda", shape)


@pytest.mark.parametrize("shape", A.CONCAT_SHAPES, ids=shape_id)
def test_concat_adjoint(shape):
    A.check_concat_adjoint("cuda", shape)


def test_concat_refusals():
    A.check_concat_refusals("cuda")


ROUTE_CASES = ["cat", "ddpmblk_fir"]


@pytest.mark.parametrize("case", [c for c in A.CASES if c not in ROUTE_CASES])
def test_forward_against_the_reference(case):
    A.check_forward("cuda", case)


@pytest.mark.parametrize("wino", ["0", "1", "4"])       # direct kernels everywhere, the default routes, F(4x4,3x3) wherever legal
@pytest.mark.parametrize("case", ROUTE_CASES)
def test_forward_against_the_reference_on_every_route(case, wino, monkeypatch):
    monkeypatch.setenv("SSDE_WINOGRAD", wino)
    A.check_forward("cuda", case)


@pytest.mark.parametrize("case", list(A.TRAIN_CASES))
def test_loss_and_gradients_against_the_reference(case):
    A.check_loss_and_gradients("cuda", case)


@pytest.mark.parametrize("case", list(A.TRAIN_CASES))
def test_input_gradient_against_the_reference(case):
    A.check_input_gradient("cuda", case)


@pytest.mark.parametrize("case", list(A.TRAIN_CASES))
def test_train_steps_as_one_graph_and_as_program_runs(case, monkeypatch):
    monkeypatch.setenv("SSDE_TRAIN_GRAPH", "1")
    loss_g, params_g = A.run_train_steps("cuda", case)
    monkeypatch.setenv("SSDE_TRAIN_GRAPH", "0")
    loss_p, params_p = A.run_train_steps("cuda", case)
    assert loss_g == loss_p and all(torch.equal(a, b) for a, b in zip(params_g, params_p))


def test_sampler():
    A.check_sampler("cuda")


def test_unet_plan_round_trip():
    A.check_unet_plan_round_trip("cuda")


def test_train_plan_round_trip():
    A.check_train_plan_round_trip("cuda")

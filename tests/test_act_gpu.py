"""NCSN++ / DDPM++ with elu, relu and lrelu on the MI355X: the apply launch and its adjoint with src.act against fp64, the
activation alone, the refusals of the other entry points, whole forwards against the reference, ELU gradients and training
steps against the reference's run (as one hipGraph and as program runs), and plans.  Checks: tests/_act_checks.py."""
import pytest
import torch

import _act_checks as A

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("side", A.KERNEL_MAPS)
@pytest.mark.parametrize("shape", A.KERNEL_SHAPES, ids=lambda s: "%d+%d_in_%d" % s)
@pytest.mark.parametrize("act", A.ACTS)
def test_kernels_against_fp64(act, shape, side):
    A.check_kernels("cuda", act, *shape, side)


@pytest.mark.parametrize("shape", A.ACT_ONLY_SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("act", ("swish",) + A.ACTS)
def test_activation_only(act, shape):
    A.check_act_only("cuda", act, shape)


@pytest.mark.parametrize("shape", A.ACT_ONLY_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_activation_only_silu_is_the_fused_prologue(shape):
    A.check_act_only_silu_is_the_fused_prologue("cuda", shape)


def test_refusals():
    A.check_refusals("cuda")


@pytest.mark.parametrize("wino", ["0", "1", "4"])
@pytest.mark.parametrize("name", list(A.FORWARD_CASES))
def test_forward_against_the_reference(name, wino, monkeypatch):
    monkeypatch.setenv("SSDE_WINOGRAD", wino)
    A.check_forward("cuda", name, tol=A.TOL_FWD)


def test_elu_loss_and_gradients_against_the_reference():
    A.check_loss_and_gradients("cuda")


@pytest.mark.parametrize("graph", ["1", "0"])       # the whole step as one hipGraph replay / as program runs
def test_elu_three_steps_against_the_reference_run(graph, monkeypatch):
    monkeypatch.setenv("SSDE_TRAIN_GRAPH", graph)
    first, model = A.check_train_steps_against_reference_run("cuda")
    params = [p.detach().clone() for p in model.parameters()]
    again, model2 = A.check_train_steps_against_reference_run("cuda")
    assert first == again and all(torch.equal(a, b.detach()) for a, b in zip(params, model2.parameters()))


def test_unet_plan_round_trip():
    A.check_unet_plan_round_trip("cuda")


def test_train_plan_round_trip():
    A.check_train_plan_round_trip("cuda")


def test_pc_plan_matches_pc_engine():
    A.check_pc_plan("cuda")

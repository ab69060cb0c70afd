"""Controllable generation from plan blobs on the MI355X (`-m gpu`): the prepare launch against fp64, the blob of an
inpainter's / colorizer's engine through plan_export.LoadedPlan -- op by op and as a replayed hipGraph -- against the
Python-driven engine and against the reference, tests/c_host/control_host.c linked with libssde_hip.so as one child process,
and the refusals.  Cases, bounds and the reasons for them: _plan_control_checks.py."""
import numpy as np
import pytest
import torch

import _util
import _plan_control_checks as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [(2, 1, 7), (2, 4, 64)])
def test_project_prepare_identity_form_is_the_reference_expression(shape):
    P.check_prepare_identity("cuda", *shape)


@pytest.mark.parametrize("own_mask", [False, True])
@pytest.mark.parametrize("n,hw", [(3, 25), (5, 64)])
def test_project_prepare_colour_form_against_fp64(n, hw, own_mask):
    P.check_prepare_colour("cuda", n, hw, own_mask)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("task", ["inpaint", "colorize"])
def test_plan_reproduces_python_driven_engine(task, use_graph):
    x_py, xm_py = P.python_run(task, "cuda")
    x, xm = P.plan_run(task, "cuda", use_graph=use_graph)
    assert torch.isfinite(x).all() and torch.equal(x, x_py) and torch.equal(xm, xm_py)


def test_known_pixels_come_back_bit_for_bit():
    """VE inpainting: on mask == 1 the last projection writes x_mean = x * 0 + data * 1"""
    s = P.setup(P.BITWISE["inpaint"], "cuda")
    _, xm = P.plan_run("inpaint", "cuda", use_graph=True)
    known = s.mask.cpu() == 1
    assert known.any() and not known.all() and torch.equal(xm[known], s.data.cpu()[known])


@pytest.mark.parametrize("name", list(_util.CONTROLLABLE_CASES))
def test_plan_with_injected_noise_matches_reference(name):
    P.assert_matches_reference(name, P.reference_run(name, "cuda"))


@pytest.mark.parametrize("task", ["inpaint", "colorize"])
def test_control_host_c_matches_loaded_plan(task, tmp_path):
    exe = P.build_c_host(tmp_path)
    out = P.run_c_host(exe, task, "cuda", tmp_path, use_graph=True, timeout=120)
    assert np.array_equal(out, P.plan_run(task, "cuda", use_graph=True)[1].numpy())


def test_refusals_name_their_entry_point():
    P.check_refusals("cuda")

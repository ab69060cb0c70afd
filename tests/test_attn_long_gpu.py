"""Attention over more than 256 tokens on the MI355X: the streaming kernels against fp64, the forced streaming forward at
16 x 16 and below, the small nets with attention at 32 x 32 against the reference's forward, oracle autograd and the
reference's three optimizer steps, a captured PC run and the plan round trip through the plain-C host.  Every test runs in
both matrix modes (tests/conftest.py).  Checks: tests/_attn_long_checks.py."""
import os
import subprocess

import pytest
import torch

import _util
import _attn_long_checks as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", K.KERNEL_CASES + K.KERNEL_CASES_GPU_ONLY, ids=lambda s: "%dx%dx%d" % s)
def test_kernels_against_fp64(shape):
    K.check_kernel("cuda", *shape)


@pytest.mark.parametrize("shape", K.FORCED_CASES, ids=lambda s: "%dx%dx%d" % s)
def test_forced_streaming_forward(shape, monkeypatch):
    K.check_forced_stream("cuda", *shape, monkeypatch)


def test_rescale_in_both_directions_and_ties():
    K.check_rescale_directions("cuda")


def test_transpose_detecting_across_the_block_boundary():
    K.check_transpose_detecting("cuda")


def test_padding_is_inert():
    K.check_padding_is_inert("cuda")


@pytest.mark.parametrize("wino", ["0", "1", "4"])
def test_small_net_forward_against_the_reference(wino, monkeypatch):
    monkeypatch.setenv("SSDE_WINOGRAD", wino)
    K.check_net_forward("cuda")


def test_small_ddpm_net_forward_against_the_reference():
    K.check_net_forward("cuda", family="ddpm")


@pytest.mark.parametrize("wino", ["0", "1", "4"])
def test_small_net_gradients_against_oracle_autograd(wino, monkeypatch):
    monkeypatch.setenv("SSDE_WINOGRAD", wino)
    K.check_net_grads("cuda")


@pytest.mark.parametrize("graph", ["1", "0"])       # the whole step as one hipGraph replay / as program runs
def test_three_steps_against_the_reference_run(graph, monkeypatch):
    monkeypatch.setenv("SSDE_TRAIN_GRAPH", graph)
    first, model = K.check_train_steps_against_reference_run("cuda")
    params = [p.detach().clone() for p in model.parameters()]
    again, model2 = K.check_train_steps_against_reference_run("cuda")
    assert first == again and all(torch.equal(a, b.detach()) for a, b in zip(params, model2.parameters()))


def test_captured_pc_run_is_finite_and_repeatable():
    """10 iterations of the captured predictor-corrector loop on the net with attention at 32 x 32"""
    from score_sde_pytorch_amd import sde_lib, sampling
    cfg, model, _ = K.small_model("cuda")
    N, B = 10, 2
    sde = sde_lib.VESDE(sigma_min=0.01, sigma_max=50, N=N)
    sampler = sampling.get_pc_sampler(sde, (B, 3, 32, 32), sampling.ReverseDiffusionPredictor, sampling.LangevinCorrector,
                                      lambda v: v, snr=0.16, n_steps=1, continuous=True, denoise=False, eps=1e-5, device="cuda")
    x_T = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(3)) * 50
    a, _ = sampler(model, x_init=x_T, seed=77, use_graph=True)
    a = a.clone()
    b, _ = sampler(model, x_init=x_T, seed=77, use_graph=True)
    assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    assert torch.equal(a, b)


def test_plan_round_trip_through_the_c_host(tmp_path):
    from score_sde_pytorch_amd import _lib as L

    def link(exe):
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_host", "plan_host.c")
        libdir = os.path.dirname(L.LIB_PATH)
        r = subprocess.run(["gcc", "-O1", "-std=c11", "-I", os.path.join(_util.ROOT, "include"), "-I", "/opt/rocm/include", src, "-o", exe,
                            L.LIB_PATH, "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return exe
    K.check_plan_round_trip("cuda", tmp_path, link)

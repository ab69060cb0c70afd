"""Attention over more than 256 tokens (CPU): the route query without a device, unchanged programs, the dry lowering that
refuses a token count beyond SSDE_ATTN_L_MAX, and -- under the test-only emulator (tests/emu/) -- the streaming kernels
against fp64, the small nets with attention at 32 x 32 against the reference's forward, oracle autograd and the reference's
three optimizer steps, and the plan round trip through the plain-C host.  See tests/_attn_long_checks.py."""
import ctypes as C
import os
import subprocess

import pytest
import torch

import emu
import _util
import _attn_long_checks as K

needs_emu = pytest.mark.skipif(not emu.available(), reason="emulator needs x86-64 + ROCm's clang++")


@pytest.fixture
def emulated():
    with emu.emulated():
        yield


def test_route_query_matches_the_dispatch():
    K.check_routes()


# op count of ve/cifar10_ncsnpp_continuous at batch 2 (CPU dry lowering, SSDE_WINOGRAD=1), recorded from commit 88405c2 (the
# parent of this change): 108 conv, 9 upfirdn, 6 attention, 95 GroupNorm finalize, embed, 2 boundary ops
CIFAR_OPS_AT_88405C2 = 221


@pytest.mark.parametrize("matrix", ["f32", "bf16x6"])
def test_programs_of_the_shipped_config_are_unchanged(matrix, monkeypatch):
    from score_sde_pytorch_amd import configs, engine as E, _lib as L
    from score_sde_pytorch_amd.models import utils as mutils
    monkeypatch.setenv("SSDE_WINOGRAD", "1")
    monkeypatch.setenv("SSDE_MATRIX", matrix)
    monkeypatch.delenv("SSDE_ATTN_STREAM", raising=False)
    cfg = configs.get_config("ve/cifar10_ncsnpp_continuous")
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(cfg)
    eng = E.UNetEngine(model, 2, 32, 32, "cpu")
    eng.validate_plans()
    kinds = [int(eng.program.ops[i].kind) for i in range(eng.program.n)]
    assert len(kinds) == CIFAR_OPS_AT_88405C2
    assert (kinds.count(L.OP_CONV), kinds.count(L.OP_UPFIRDN), kinds.count(L.OP_ATTN), kinds.count(L.OP_GN_FINALIZE)) == (108, 9, 6, 95)
    attn = K.attention_ops(eng.program)
    assert sorted((a.l, a.c) for a in attn) == [(16, 256)] + [(256, 256)] * 5
    for a in attn:
        assert a.flags == (L.ATTNF_BF16X6 if matrix == "bf16x6" else 0)
        assert L.load().ssde_attention_route(C.byref(a)) == K.parent_route(a.l, a.c, a.flags)


def test_lowering_refuses_a_token_count_beyond_the_limit():
    """attention at 160 x 160 = 25600 tokens > SSDE_ATTN_L_MAX: refused by validate_plans, before any launch"""
    from score_sde_pytorch_amd import engine as E, _lib as L
    from score_sde_pytorch_amd.models import utils as mutils
    cfg = _util.small_config("ncsnpp", image_size=160, attn=(160,))
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(cfg)
    eng = E.UNetEngine(model, 1, 160, 160, "cpu")
    with pytest.raises(L.SsdeError, match="token count 25600 outside"):
        eng.validate_plans()


def test_lowering_accepts_attention_at_32_and_16_dry():
    from score_sde_pytorch_amd import engine as E, backward as B
    cfg, model, _ = K.small_model("cpu")
    eng = E.UNetEngine(model, 2, 32, 32, "cpu")
    assert all(v > 0 for v in eng.validate_plans())
    assert sorted(a.l for a in K.attention_ops(eng.program)) == [256, 256, 256, 1024, 1024]      # down, bottleneck and up at 16 x 16; down and up at 32 x 32
    B.TrainEngine(model, 2, 32, 32, "cpu")


@needs_emu
@pytest.mark.parametrize("shape", K.KERNEL_CASES, ids=lambda s: "%dx%dx%d" % s)
def test_kernels_against_fp64(emulated, shape):
    K.check_kernel("cpu", *shape)


@needs_emu
@pytest.mark.parametrize("shape", K.FORCED_CASES, ids=lambda s: "%dx%dx%d" % s)
def test_forced_streaming_forward(emulated, shape, monkeypatch):
    K.check_forced_stream("cpu", *shape, monkeypatch)


@needs_emu
def test_rescale_in_both_directions_and_ties(emulated):
    K.check_rescale_directions("cpu")


@needs_emu
def test_transpose_detecting_across_the_block_boundary(emulated):
    K.check_transpose_detecting("cpu")


@needs_emu
def test_padding_is_inert(emulated):
    K.check_padding_is_inert("cpu")


@needs_emu
@pytest.mark.parametrize("wino", ["0", "1", "4"])
def test_small_net_forward_against_the_reference(emulated, wino, monkeypatch):
    monkeypatch.setenv("SSDE_WINOGRAD", wino)
    K.check_net_forward("cpu")


@needs_emu
def test_small_ddpm_net_forward_against_the_reference(emulated):
    K.check_net_forward("cpu", family="ddpm")


@needs_emu
def test_small_net_gradients_against_oracle_autograd(emulated):
    K.check_net_grads("cpu")


@needs_emu
def test_three_steps_against_the_reference_run(emulated, monkeypatch):
    from score_sde_pytorch_amd import losses
    monkeypatch.setattr(losses, "_on_device", lambda t: True)       # (the step function asks whether a tensor is HIP memory)
    first, model = K.check_train_steps_against_reference_run("cpu")
    params = [p.detach().clone() for p in model.parameters()]
    again, model2 = K.check_train_steps_against_reference_run("cpu")
    assert first == again and all(torch.equal(a, b.detach()) for a, b in zip(params, model2.parameters()))


@needs_emu
def test_plan_round_trip_through_the_c_host(emulated, tmp_path):
    emu_lib = emu.build_emu.build()

    def link(exe):
        src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_host", "plan_host.c")
        r = subprocess.run(["gcc", "-O1", "-std=c11", "-DHOST_IS_DEVICE", "-I", os.path.join(_util.ROOT, "include"), src, "-o", exe,
                            emu_lib, "-lm", "-Wl,-rpath," + os.path.dirname(emu_lib)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return exe
    K.check_plan_round_trip("cpu", tmp_path, link)

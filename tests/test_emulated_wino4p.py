"""The position-batched F(4x4,3x3) convolution (conv_wino4p.hip, SSDE_TILE_WINOGRAD4P) under the CPU emulator (tests/emu):
the op through the C ABI against fp64 torch, the host packer against fp64 G g G^T, and the lowering rule at the BASELINE
sampler's shape.  Checks: tests/_wino4p_checks.py."""
import ctypes as C

import pytest
import torch

import _util
import _wino4p_checks as W
import emu


@pytest.fixture()
def ops():
    if not emu.available():
        pytest.skip("emulator needs x86-64 + ROCm's clang++")
    from score_sde_pytorch_amd import hipops
    with emu.emulated():
        yield hipops


@pytest.mark.parametrize("ks", [1, 2, 4])
@pytest.mark.parametrize("resid_post", [0, 1])
def test_concat_source_gn_prologue_epilogue_and_splits(ops, ks, resid_post):
    """4x4 maps, 64 + 64 channels -> 96 (a cout tile that is not full), GroupNorm + SiLU prologue, every epilogue term"""
    W.run_case("cpu", ops, 3, 64, 64, 96, 4, True, resid_post, ks, seed=ks + 10 * resid_post)


def test_larger_map_several_tiles_per_image(ops):
    """8x8 maps (four tiles per image, four GroupNorm slices), plain source"""
    W.run_case("cpu", ops, 2, 32, 0, 64, 8, False, 0, 1, seed=5)


def test_splits_agree_with_each_other(ops):
    d1, _ = W.run_case("cpu", ops, 2, 128, 0, 64, 4, True, 0, 1, seed=9)
    d4, _ = W.run_case("cpu", ops, 2, 128, 0, 64, 4, True, 0, 4, seed=9)
    assert _util.rel_err(d4, d1) < W.TOL


def test_host_packer():
    W.check_packer()


def test_cifar_sampler_lowering_puts_every_4x4_layer_on_the_position_batched_form(monkeypatch):
    """CIFAR NCSN++ at batch 256 (the bench's shape), the production heuristic: every stride-1 3x3 convolution on the 4x4 maps
    without a fused 1x1 source takes SSDE_TILE_WINOGRAD4P with its own workspace and leaves wino_v unset; nothing else does"""
    from score_sde_pytorch_amd import engine as E, _lib as L
    from score_sde_pytorch_amd.models import utils as mutils
    monkeypatch.setenv("SSDE_WINOGRAD", "1")
    model = mutils.get_model("ncsnpp")(_util.cfgs.get_config("ve/cifar10_ncsnpp_continuous"))
    eng = E.UNetEngine(model, 256, 32, 32, torch.device("cpu"))
    lib = L.load()
    at4 = [f for k, f, _, _ in eng.b.specs
           if k == L.OP_CONV and f["ksize"] == 3 and f["h_out"] == 4 and f["stride"] == 1 and f["aux"]["p0"] is None]
    assert len(at4) == 18
    for f in at4:
        assert f["tile"] == L.TILE_WINOGRAD4P and f["wino_v"] is None
        assert f["wino_ws"] is not None and f["wino_ws"].numel == f["wino_ws_floats"]
    others = [f for k, f, _, _ in eng.b.specs if k == L.OP_CONV and all(f is not g for g in at4)]
    assert not [f for f in others if f["tile"] == L.TILE_WINOGRAD4P or f.get("wino_ws") is not None]
    ops = [eng.program.ops[i].u.conv for i in range(eng.program.n) if eng.program.ops[i].kind == L.OP_CONV]
    p4 = [c for c in ops if c.tile == L.TILE_WINOGRAD4P]
    assert len(p4) == 18 and all(not c.wino_v and c.wino_ws and c.wino_ws_floats == lib.ssde_conv_ws_floats(C.byref(c)) for c in p4)
    assert min(eng.validate_plans()) > 0
    monkeypatch.setenv("SSDE_WINOGRAD", "2")
    assert not [1 for k, f, _, _ in E.UNetEngine(model, 256, 32, 32, torch.device("cpu")).b.specs
                if k == L.OP_CONV and f["tile"] == L.TILE_WINOGRAD4P]

"""The position-batched F(4x4,3x3) convolution (conv_wino4p.hip, SSDE_TILE_WINOGRAD4P) on the MI355X: the emulator suite's op
cases at the sampler's and the training step's shapes, and the device weight re-pack after an optimizer step.
Checks: tests/_wino4p_checks.py."""
import pytest
import torch

import _wino4p_checks as W

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ks", [1, 2, 4])
@pytest.mark.parametrize("resid_post", [0, 1])
def test_concat_source_gn_prologue_epilogue_and_splits(ks, resid_post):
    from score_sde_pytorch_amd import hipops as ops
    W.run_case("cuda", ops, 3, 64, 64, 96, 4, True, resid_post, ks, seed=ks + 10 * resid_post)


@pytest.mark.parametrize("n,c0,c1,cout", [(256, 256, 256, 256), (256, 256, 0, 256), (128, 256, 0, 256), (37, 256, 512, 256)])
def test_sampler_and_training_shapes(n, c0, c1, cout):
    from score_sde_pytorch_amd import hipops as ops
    for ks in (1, 2, 4):
        W.run_case("cuda", ops, n, c0, c1, cout, 4, True, 0, ks, seed=n + ks)


def test_larger_map_several_tiles_per_image():
    from score_sde_pytorch_amd import hipops as ops
    W.run_case("cuda", ops, 5, 96, 32, 64, 8, True, 1, 2, seed=5)


def test_device_repack_matches_host_pack_after_an_optimizer_step():
    """ssde_pack_weights with SSDE_PACK_WINO4P, forward and input-gradient images, after torch.optim.SGD changed the weight"""
    from score_sde_pytorch_amd import engine as E
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(3)
    w = torch.nn.Parameter((torch.randn(256, 512, 3, 3, generator=g) / 70).to(dev))
    ws = E.WeightStore(dev)
    fwd = ws.conv3(w, route=E.F4P)
    dgrad = lambda t: E.pack_wino4p_weight(t.permute(1, 0, 2, 3).flip(2, 3))  # noqa: E731
    bwd = ws.derived(fwd, E.F4P)
    ws.refresh()
    opt = torch.optim.SGD([w], lr=0.5)
    w.grad = torch.randn(w.shape, generator=g).to(dev)
    opt.step()
    fwd.fill_(7.0)
    bwd.fill_(7.0)
    ws.refresh()                                   # a stale source: the device re-pack
    assert float((fwd - E.pack_wino4p_weight(w.detach())).abs().max()) < 1e-6
    assert float((bwd - dgrad(w.detach())).abs().max()) < 1e-6

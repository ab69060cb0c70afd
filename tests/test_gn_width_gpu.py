"""GroupNorm groups of any width on the MI355X: the new kernels against fp64, the nf = 16 network against the reference's
forward, oracle autograd and the reference's three optimizer steps, a deep nf = 16 network against the CPU oracle, and one
evaluation of the 1024-px preset.  Checks: tests/_gn_width_checks.py."""
import pytest
import torch

import _util
import _gn_width_checks as K
import _gn_width_util as W

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("side", K.KERNEL_MAPS)
@pytest.mark.parametrize("shape", K.KERNEL_SHAPES, ids=lambda s: "%d+%d_in_%d" % s)
def test_kernels_against_fp64(shape, side):
    K.check_kernels("cuda", *shape, side)


def test_any_width_statistics_kernel_has_the_quad_kernels_bits():
    K.check_any_width_kernel_has_the_quad_kernels_bits("cuda")


@pytest.mark.parametrize("wino", ["0", "1", "4"])
def test_small_net_forward_against_the_reference(wino, monkeypatch):
    monkeypatch.setenv("SSDE_WINOGRAD", wino)
    K.check_small_net_forward("cuda", tol=K.TOL_FWD)


def test_small_net_gradients_against_oracle_autograd():
    K.check_small_net_grads("cuda")


def test_small_net_dropout_through_the_apply_launch():
    K.check_small_net_dropout("cuda")


@pytest.mark.parametrize("graph", ["1", "0"])       # the whole step as one hipGraph replay / as program runs
def test_three_steps_against_the_reference_run(graph, monkeypatch):
    monkeypatch.setenv("SSDE_TRAIN_GRAPH", graph)
    first, model = K.check_train_steps_against_reference_run("cuda")
    params = [p.detach().clone() for p in model.parameters()]
    again, model2 = K.check_train_steps_against_reference_run("cuda")
    assert first == again and all(torch.equal(a, b.detach()) for a, b in zip(params, model2.parameters()))


def test_plan_round_trip():
    K.check_plan_round_trip("cuda")


def test_deep_nf16_net_against_the_cpu_oracle():
    """nf = 16 under ch_mult (1, 2, 4, 8, 16, 32) at 128 px, batch 2: the lowest map is 4x4, attention and the 6-wide groups sit
    at 16x16, and the top level concatenates 16 + 16 channels.  (The CPU oracle takes 0.5 s on it with 16 threads.)"""
    from oracle import unet_oracle
    from score_sde_pytorch_amd import engine as E, _lib as L
    cfg = W.small_config(image_size=128, ch_mult=(1, 2, 4, 8, 16, 32))
    cfg, model, sd = K.small_model("cuda", cfg=cfg)
    x, sig = W.forward_inputs(cfg)
    with torch.no_grad():
        ref = unet_oracle.ncsnpp_forward(cfg, sd, x, sig)
    eng = E.UNetEngine(model, x.shape[0], 128, 128, torch.device("cuda"))
    kinds, fused = K.program_facts(eng.program)
    assert kinds.count(L.OP_GN_APPLY) >= 1 and all(w % 4 == 0 for w in fused)
    y = eng.forward(x.cuda(), sig.cuda())
    err = _util.rel_err(y, ref)
    print("deep nf16 net, 128 px: rel err %.3g" % err)
    assert err < K.TOL_FWD, err


def test_ffhq_1024_preset_one_forward():
    """ve/ffhq_ncsnpp_continuous as published, batch 1: finite, and two evaluations agree to the bit (no parity claim here: its
    routes are those of the deep net above and of the dry lowering)"""
    from score_sde_pytorch_amd import configs, engine as E
    from score_sde_pytorch_amd.models import utils as mutils
    cfg = configs.get_config("ve/ffhq_ncsnpp_continuous")
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(cfg)
    _util.load_seeded(model, seed=1)
    model = model.to("cuda").eval()
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(1, 3, 1024, 1024, generator=g) * 20).cuda()
    sig = torch.tensor([7.0]).cuda()
    eng = E.UNetEngine(model, 1, 1024, 1024, torch.device("cuda"))
    y1 = eng.forward(x, sig)
    y2 = eng.forward(x, sig)
    assert bool(torch.isfinite(y1).all()) and float(y1.abs().max()) > 0
    assert torch.equal(y1, y2)

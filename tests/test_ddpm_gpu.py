"""The `ddpm` model family on the MI355X: forward, ancestral sampler and training step against what the REFERENCE computed
(tests/golden/*ddpm*.npz, written by tools/gen_golden_ddpm.py), and the 256-px church configuration against the restatement
of the forward (tests/_ddpm_oracle.py, pinned to the same goldens by tests/test_ddpm_cpu.py).

Tolerances are the suite's own: test_unet_gpu.TOL_FWD (1e-4, twice that per sample) for forwards, _util.assert_trajectory_close
for sampler states, _train_checks.TOL_OP / TOL_GRAD and the bounds of _train_checks._compare_with_reference_step for training.
The conftest runs every test in both matrix modes.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _util
import _ddpm_util as D
import _ddpm_oracle
import _train_checks as T
from _util import rel_err

pytestmark = pytest.mark.gpu

TOL_FWD = 1e-4          # tests/test_unet_gpu.py
WINO_MODES = ["0", "1", "4"]


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _model(cfg):
    from score_sde_pytorch_amd.models import utils as mutils
    torch.manual_seed(0)
    model = mutils.get_model("ddpm")(cfg)
    sd = {k: v.clone() for k, v in _util.load_seeded(model, seed=1).items()}
    sd["sigmas"] = model.sigmas.clone()
    return model, sd


@pytest.mark.parametrize("wino", WINO_MODES)
@pytest.mark.parametrize("case", D.FORWARD_CASES)
def test_forward_matches_reference_golden(case, wino, monkeypatch):
    monkeypatch.setenv("SSDE_WINOGRAD", wino)
    gold = np.load(os.path.join(_util.GOLDEN, "unet_%s.npz" % case))
    model, _ = _model(D.forward_config(case))
    model = model.cuda().eval()
    with torch.no_grad():
        y = model(torch.from_numpy(gold["x"]).cuda(), torch.from_numpy(gold["cond"]).cuda())
    y_ref = torch.from_numpy(gold["y"])
    e, ps = rel_err(y, y_ref), _util.per_sample_err(y, y_ref)
    print("ddpm forward %s SSDE_WINOGRAD=%s: rel err %.3g, per sample %.3g" % (case, wino, e, ps))
    assert e < TOL_FWD, e
    assert ps < 2 * TOL_FWD, ps


def test_forward_church_256_full_architecture():
    """configs/vp/ddpm/church.py: six resolutions from 256x256 down to 8x8, five end-padded Downsample launches, batch 1"""
    cfg = _util.cfgs.get_config("vp/ddpm/church")
    model, sd = _model(cfg)
    x, labels = D.forward_inputs(cfg, batch=1, seed=5)
    with torch.no_grad():
        ref = _ddpm_oracle.ddpm_forward(cfg, sd, x, labels)
        y = model.cuda().eval()(x.cuda(), labels.cuda())
    print("ddpm church 256: rel err %.3g" % rel_err(y, ref))
    assert rel_err(y, ref) < TOL_FWD


def test_forward_without_resampling_convolutions():
    cfg = D.small_config(resamp_with_conv=False)
    model, sd = _model(cfg)
    x, labels = D.forward_inputs(cfg, batch=3, seed=6)
    with torch.no_grad():
        ref = _ddpm_oracle.ddpm_forward(cfg, sd, x, labels)
        y = model.cuda().eval()(x.cuda(), labels.cuda())
    assert rel_err(y, ref) < TOL_FWD


def test_cpu_tensor_fails_loudly():
    model, _ = _model(D.small_config())
    model = model.cuda().eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(torch.zeros(1, 3, 16, 16), torch.zeros(1))


# n, c0, c1, cout, h, w, GroupNorm + SiLU prologue: odd and even maps, a concatenated source, the CIFAR Downsample shapes
PAD_END_CASES = [(2, 32, 0, 64, 8, 8, False), (1, 16, 0, 40, 7, 9, False), (2, 32, 32, 64, 6, 10, True), (3, 8, 0, 32, 16, 16, True),
                 (4, 128, 0, 128, 32, 32, False), (4, 256, 0, 256, 16, 16, True), (16, 256, 0, 256, 8, 8, False)]


@pytest.mark.parametrize("n,c0,c1,cout,h,w,gn", PAD_END_CASES)
def test_end_padded_conv_and_weight_gradient(n, c0, c1, cout, h, w, gn):
    """ssde_conv2d / ssde_conv_wgrad with pad_end = 1, stride 2 against fp64 F.pad + conv2d and its autograd"""
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    g = torch.Generator().manual_seed(70 + h)
    x1 = torch.randn(n, c0, h, w, generator=g) + 0.3
    x2 = torch.randn(n, c1, h, w, generator=g) if c1 else None
    C_ = c0 + c1
    wt = torch.randn(cout, C_, 3, 3, generator=g) / np.sqrt(9 * C_)
    bias = torch.randn(cout, generator=g)
    G = max(1, C_ // 8)
    gamma, beta = 1 + 0.1 * torch.randn(C_, generator=g), 0.1 * torch.randn(C_, generator=g)
    gout = torch.randn(n, cout, h // 2, w // 2, generator=g)
    xc = (torch.cat([x1, x2], 1) if c1 else x1).double()
    w64 = wt.double().requires_grad_()
    u = F.silu(F.group_norm(xc, G, gamma.double(), beta.double(), 1e-6)) if gn else xc
    ref = F.conv2d(F.pad(u, (0, 1, 0, 1)), w64, bias.double(), stride=2)
    ref.backward(gout.double())
    a1, a2 = nhwc(x1).cuda(), (nhwc(x2).cuda() if c1 else None)
    gnt = None
    if gn:
        mean, rstd = ops.groupnorm_stats(a1, G, 1e-6, x2=a2)
        gnt = (mean, rstd, gamma.cuda(), beta.cuda(), G)
    pro = L.PRO_GN_SILU if gn else L.PRO_NONE
    y = ops.conv2d(a1, wt, bias.cuda(), stride=2, pad=0, pad_end=1, x2=a2, pro=pro, gn=gnt)
    assert tuple(y.shape) == (n, h // 2, w // 2, cout)
    assert rel_err(nchw(y), ref.detach()) < T.TOL_OP
    dw = torch.zeros(cout, C_, 3, 3, device="cuda")
    ops.conv_wgrad(a1, nhwc(gout).cuda(), 3, dw, stride=2, pad=0, pad_end=1, x2=a2, pro=pro, gn=gnt, scale=0.5)
    assert rel_err(dw, 0.5 * w64.grad) < T.TOL_OP
    with pytest.raises(L.SsdeError, match="pad_end"):
        ops.conv2d(a1, wt, None, stride=1, pad=1, pad_end=1, x2=a2, tile=L.TILE_WINOGRAD, out_hw=(h, w))


@pytest.mark.parametrize("wino", WINO_MODES)
def test_ancestral_sampling_trajectory_matches_reference(wino, monkeypatch):
    """vp/ddpm/cifar10's own sampler (ancestral sampling, no corrector, discrete labels), 10 steps, injected noise"""
    from score_sde_pytorch_amd import sde_lib, sampling
    monkeypatch.setenv("SSDE_WINOGRAD", wino)
    pc = D.PC_CASE
    gold = np.load(os.path.join(_util.GOLDEN, "pc_cifar_ddpm_n10.npz"))
    model, _ = _model(_util.cfgs.get_config(pc["config"]))
    model = model.cuda().eval()
    B, N = pc["batch"], pc["sde_kwargs"]["N"]
    sde = sde_lib.VPSDE(**pc["sde_kwargs"])
    sampler = sampling.get_pc_sampler(sde, (B, 3, 32, 32), sampling.AncestralSamplingPredictor, sampling.NoneCorrector,
                                      lambda v: v, snr=0.16, n_steps=1, probability_flow=False, continuous=False,
                                      denoise=pc["denoise"], eps=pc["eps"], device="cuda")
    x_T, noises = D.pc_inputs()
    samples, nfe = sampler(model, x_init=x_T, noises=noises)
    assert sampler.last_path == "fused-eager"
    _util.assert_trajectory_close(samples, torch.from_numpy(gold["samples"]), "samples")
    for k in pc["steps_kept"]:
        sampler(model, x_init=x_T, noises=noises, max_steps=k + 1)
        x_k = sampler.engine.x.view(B, 3, 32, 32).cpu()
        _util.assert_trajectory_close(x_k, torch.from_numpy(gold["x_step%d" % k]), "x_step%d" % k)


def test_training_loss_and_gradients_match_reference():
    D.check_training_loss_and_gradients("cuda")


@pytest.mark.parametrize("graph", ["1", "0"])       # the whole step as one hipGraph replay / as program runs
def test_step_fn_matches_the_reference_run(graph, monkeypatch):
    monkeypatch.setenv("SSDE_TRAIN_GRAPH", graph)
    D.check_step_fn_against_reference_run("cuda", graph_expected=graph == "1")


def test_whole_network_gradients_against_the_restatement():
    """every parameter gradient and the input gradient of the small network (end-padded Downsample, NIN shortcut, nearest
    Upsample + 3x3) against autograd through the restatement"""
    from score_sde_pytorch_amd import backward as B
    cfg = D.small_config()
    model, sd = _model(cfg)
    x, labels = D.forward_inputs(cfg, batch=3, seed=9)
    g = torch.Generator().manual_seed(8)
    gout = torch.randn(x.shape, generator=g)
    sd_req = {k: (v.clone().requires_grad_() if k != "sigmas" else v) for k, v in sd.items()}
    xr = x.clone().requires_grad_()
    y_ref = _ddpm_oracle.ddpm_forward(cfg, sd_req, xr, labels)
    y_ref.backward(gout)
    ref = {k: v.grad for k, v in sd_req.items() if k != "sigmas"}
    model = model.cuda()
    eng = B.TrainEngine(model, 3, 16, 16, torch.device("cuda"), input_grad=True, dropout=False)
    y = eng.forward_train(x.cuda(), labels.cuda()).clone()
    assert rel_err(y, y_ref.detach()) < TOL_FWD
    eng.backward(gout.cuda())
    assert rel_err(eng.gx_view(), xr.grad) < T.TOL_GRAD
    T.compare_param_grads(model, eng.flat, ref)


@pytest.mark.parametrize("case", [c for c in T.RECT_EMULATED + T.RECT_GPU_ONLY if c[0] == "ddpm"], ids=T.rect_id)
def test_whole_network_gradients_on_a_rectangular_image(case):
    """h != w against the fp64 restatement: attention on a rectangular map; at 12x20 the end-padded stride-2 launch and its
    cropped transposed gradient on the 6x10 -> 3x5 step (tests/_train_checks.py: RECT_*)"""
    T.check_rect_grads("cuda", case)

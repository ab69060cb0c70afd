"""The `ddpm` model family without a GPU: parameter naming against the reference's own list, the restatement of the forward
(tests/_ddpm_oracle.py) against the reference's stored outputs, dry lowering of the full configs, and the end-padded
convolution (ssde_conv_args.pad_end / ssde_wgrad_args.pad_end, ABI 12) run under the kernel emulator against fp64.

Tolerances: 2e-5 per contraction -- what tests/test_emulated_kernels.py asks of the direct kernel and tests/_train_checks.py
(TOL_OP) of the weight gradient; 2e-5 for the restatement (what oracle/gen_golden.py asks of unet_oracle).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _util
import _ddpm_util as D
import _ddpm_oracle
from _util import rel_err
from _train_checks import TOL_OP
import emu

needs_emu = pytest.mark.skipif(not emu.available(), reason="emulator needs x86-64 + ROCm's clang++")


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _model(cfg):
    from score_sde_pytorch_amd.models import utils as mutils
    torch.manual_seed(0)
    return mutils.get_model("ddpm")(cfg)


# --------------------------------------------------------------------------- parameters
@pytest.mark.parametrize("case", list(D.STATE_DICT_CASES))
def test_state_dict_names_and_shapes_equal_the_reference(case):
    with open(os.path.join(_util.GOLDEN, "ddpm_state_dict_names.json")) as f:
        ref = [(k, tuple(s)) for k, s in json.load(f)[case]]
    mine = [(k, tuple(v.shape)) for k, v in _model(D.STATE_DICT_CASES[case]()).state_dict().items()]
    assert mine == ref


def test_strict_round_trip_and_reference_inits():
    cfg = D.small_config()
    a, b = _model(cfg), _model(cfg)
    _util.load_seeded(a, seed=1)
    res = b.load_state_dict(a.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert all(torch.equal(v, b.state_dict()[k]) for k, v in a.state_dict().items())
    # init_scale = 0 (1e-10) on Conv_1 of every block, NIN_3 of every attention block and the head; everything else at scale 1 / 0.1
    fresh = _model(cfg)
    mods = list(fresh.all_modules)
    for m in mods:
        if getattr(m, "kind", "") == "res":
            assert float(m.Conv_1.weight.abs().max()) < 1e-4 < float(m.Conv_0.weight.abs().max())
            assert float(m.Conv_1.bias.abs().max()) == 0.0
        if getattr(m, "kind", "") == "attn":
            assert float(m.NIN_3.W.abs().max()) < 1e-4 < float(m.NIN_0.W.abs().max())
    assert float(mods[-1].weight.abs().max()) < 1e-4
    assert fresh.sigmas.shape == (cfg.model.num_scales,)


def test_unbuilt_variants_raise_at_construction():
    with pytest.raises(NotImplementedError, match="nonlinearity"):
        _model(D.small_config(nonlinearity="elu"))
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        _model(D.small_config(nf=64))
    from score_sde_pytorch_amd.models import ddpm
    with pytest.raises(NotImplementedError, match="conv_shortcut"):
        ddpm.ResnetBlockDDPM(128, 256, temb_dim=512, conv_shortcut=True)


def test_cpu_tensor_fails_loudly():
    model = _model(D.small_config())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(torch.zeros(1, 3, 16, 16), torch.zeros(1))


def test_presets():
    from score_sde_pytorch_amd import configs
    for name in ("cifar10", "cifar10_continuous", "cifar10_unconditional", "church", "bedroom", "celebahq"):
        cfg = configs.get_config("vp/ddpm/" + name)
        assert cfg.model.name == "ddpm" and cfg.training.sde == "vpsde" and cfg.data.centered
    assert configs.get_config("vp/ddpm/cifar10_continuous").training.continuous
    assert not configs.get_config("vp/ddpm/cifar10_unconditional").model.conditional
    church, bedroom = configs.get_config("vp/ddpm/church"), configs.get_config("vp/ddpm/bedroom")
    assert tuple(church.model.ch_mult) == (1, 1, 2, 2, 4, 4) and church.data.image_size == 256
    assert church.model == bedroom.model and bedroom.data.category == "bedroom"
    assert configs.get_config("vp/ddpm/celebahq").data.dataset == "CelebAHQ"


# --------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", D.FORWARD_CASES)
def test_restatement_matches_reference_golden(case):
    gold = np.load(os.path.join(_util.GOLDEN, "unet_%s.npz" % case))
    cfg = D.forward_config(case)
    model = _model(cfg)
    sd = dict(_util.load_seeded(model, seed=1)); sd["sigmas"] = model.sigmas.clone()
    x, labels = D.forward_inputs(cfg)
    assert torch.equal(x, torch.from_numpy(gold["x"])) and torch.equal(labels, torch.from_numpy(gold["cond"]))
    with torch.no_grad():
        y = _ddpm_oracle.ddpm_forward(cfg, sd, x, labels)
    assert rel_err(y, torch.from_numpy(gold["y"])) < 2e-5


# --------------------------------------------------------------------------- dry lowering
def _conv_ops(eng):
    from score_sde_pytorch_amd import _lib as L
    prog = eng.program
    return [prog.ops[i].u.conv for i in range(prog.n) if prog.ops[i].kind == L.OP_CONV]


@pytest.mark.parametrize("name,batch", [("vp/ddpm/cifar10", 2), ("vp/ddpm/church", 1)])
@pytest.mark.parametrize("wino", ["1", "2", "4"])
def test_dry_lowering_has_one_end_padded_launch_per_downsample(name, batch, wino, monkeypatch):
    from score_sde_pytorch_amd import configs, engine as E, _lib as L
    monkeypatch.setenv("SSDE_WINOGRAD", wino)
    cfg = configs.get_config(name)
    model = _model(cfg)
    R = cfg.data.image_size
    eng = E.UNetEngine(model, batch, R, R, "cpu")
    assert all(b > 0 for b in eng.validate_plans())
    padded = [c for c in _conv_ops(eng) if c.pad_end != 0]
    downs = [m for m in model.all_modules if getattr(m, "kind", "") == "down"]
    assert len(padded) == len(downs) == len(cfg.model.ch_mult) - 1
    for c, m, lvl in zip(padded, downs, range(len(downs))):
        assert (c.pad_end, c.stride, c.pad, c.ksize) == (1, 2, 0, 3)
        assert c.h_in == R >> lvl and c.h_out == c.h_in // 2 and c.c_out == m.channels
        assert c.tile < L.TILE_WINOGRAD, "an end-padded launch on a Winograd tile"
        assert c.gn_part, "the Downsample feeds a GroupNorm: its epilogue writes the partial statistics"
    # no padded copy anywhere: the only resamplers are the nearest x2 of the Upsample modules
    firs = [eng.program.ops[i].u.fir for i in range(eng.program.n) if eng.program.ops[i].kind == L.OP_UPFIRDN]
    assert len(firs) == len(downs) and all(f.up == 2 and f.down == 1 for f in firs)
    assert eng.cond_only_ops == 4


def test_unconditional_and_plain_resamplers_lower():
    from score_sde_pytorch_amd import configs, engine as E, backward as B, _lib as L
    cfg = configs.get_config("vp/ddpm/cifar10_unconditional")
    eng = E.UNetEngine(_model(cfg), 2, 32, 32, "cpu")
    assert eng.cond_only_ops == 0
    kinds = [int(eng.program.ops[i].kind) for i in range(eng.program.n)]
    assert L.OP_EMBED not in kinds and all(not c.chan_add for c in _conv_ops(eng))
    # resamp_with_conv=False: the 2x2 box down, the nearest box up, no end-padded launch
    eng = E.UNetEngine(_model(D.small_config(resamp_with_conv=False)), 2, 16, 16, "cpu")
    assert all(b > 0 for b in eng.validate_plans())
    assert not [c for c in _conv_ops(eng) if c.pad_end]
    firs = [eng.program.ops[i].u.fir for i in range(eng.program.n) if eng.program.ops[i].kind == L.OP_UPFIRDN]
    assert sorted((f.up, f.down) for f in firs) == [(1, 2), (2, 1)]
    # the training program carries pad_end into the weight gradient of every Downsample and keeps them off the Winograd routes
    t = B.TrainEngine(_model(D.small_config()), 2, 16, 16, "cpu", dropout=False)
    wg = [t.program.ops[i].u.wgrad for i in range(t.program.n) if t.program.ops[i].kind == L.OP_WGRAD]
    padded = [w for w in wg if w.pad_end]
    assert len(padded) == 1 and (padded[0].stride, padded[0].pad, padded[0].h_in, padded[0].h_out) == (2, 0, 16, 8)
    assert not L.load().ssde_wgrad_wants_winograd4(C.byref(padded[0]))


def test_pad_end_launches_stay_off_winograd_and_the_small_cout_kernel():
    """plan-only queries of the library (no device): naming a Winograd tile with pad_end is SSDE_EINVAL with a message; the
    weight-gradient route queries answer no; the same launch without pad_end is accepted where it was before"""
    from score_sde_pytorch_amd import _lib as L
    lib = L.load()
    a = L.ConvArgs()
    a.main.p0, a.main.c0, a.w_main, a.dst = 0x1000, 64, 0x1000, 0x1000
    a.n, a.h_in, a.w_in, a.h_out, a.w_out, a.c_out = 2, 16, 16, 16, 16, 64
    a.ksize, a.stride, a.pad, a.out_scale = 3, 1, 1, 1.0
    for tile in (L.TILE_WINOGRAD, L.TILE_WINOGRAD4, L.TILE_WINOGRAD4R, L.TILE_WINOGRAD4P):
        a.tile, a.pad_end = tile, 1
        assert lib.ssde_conv_lds_bytes(C.byref(a)) < 0
        assert b"pad_end" in lib.ssde_last_error()
        assert lib.ssde_conv_gn_slices(C.byref(a)) == 0
    a.tile, a.pad_end = L.TILE_WINOGRAD, 0
    assert lib.ssde_conv_lds_bytes(C.byref(a)) > 0
    # stride 2 / pad 0 on an even map: 7 output rows without the end padding, 8 with it
    a.tile, a.stride, a.pad, a.h_out, a.w_out = L.TILE_AUTO, 2, 0, 8, 8
    a.pad_end = 0
    assert lib.ssde_conv_lds_bytes(C.byref(a)) < 0
    a.pad_end = 1
    assert lib.ssde_conv_lds_bytes(C.byref(a)) > 0
    a.pad_end = 2
    assert lib.ssde_conv_lds_bytes(C.byref(a)) < 0
    w = L.WgradArgs()
    w.src.c0, w.g_ld, w.n, w.h_in, w.w_in, w.h_out, w.w_out = 128, 128, 64, 16, 16, 16, 16
    w.c_out, w.ksize, w.stride, w.pad, w.cin_store = 128, 3, 1, 1, 128
    w.flags = L.WGRADF_F4_FORCE
    assert lib.ssde_wgrad_wants_winograd4(C.byref(w))
    w.pad_end = 1
    assert not lib.ssde_wgrad_wants_winograd4(C.byref(w))


# --------------------------------------------------------------------------- the kernels under the emulator
@pytest.fixture()
def ops():
    from score_sde_pytorch_amd import hipops
    with emu.emulated():
        yield hipops


# n, c0, c1, cout, h, w, GroupNorm + SiLU prologue
PAD_END_CASES = [(2, 32, 0, 64, 8, 8, False),        # even map
                 (1, 16, 0, 40, 7, 9, False),        # odd map, ragged couts: the padded row / column is never read for h odd
                 (2, 32, 32, 64, 6, 10, True),       # concatenated source + prologue, non-square
                 (3, 8, 0, 32, 16, 16, True),        # several tiles per image
                 (1, 64, 0, 128, 32, 32, False)]     # the first CIFAR Downsample's map


def _pad_end_case(n, c0, c1, cout, h, w, gn, seed):
    g = torch.Generator().manual_seed(seed)
    x1 = torch.randn(n, c0, h, w, generator=g) + 0.3
    x2 = torch.randn(n, c1, h, w, generator=g) if c1 else None
    C_ = c0 + c1
    wt = torch.randn(cout, C_, 3, 3, generator=g) / np.sqrt(9 * C_)
    bias = torch.randn(cout, generator=g)
    G = max(1, C_ // 8)
    gamma, beta = 1 + 0.1 * torch.randn(C_, generator=g), 0.1 * torch.randn(C_, generator=g)
    ho, wo = (h + 1 - 3) // 2 + 1, (w + 1 - 3) // 2 + 1
    gout = torch.randn(n, cout, ho, wo, generator=g)
    return x1, x2, wt, bias, G, gamma, beta, gout


def _fp64_reference(x1, x2, wt, bias, G, gamma, beta, gn, gout=None):
    xc = (torch.cat([x1, x2], 1) if x2 is not None else x1).double()
    w64 = wt.double().requires_grad_()
    u = F.silu(F.group_norm(xc, G, gamma.double(), beta.double(), 1e-6)) if gn else xc
    # a zero row and column AFTER the prologue: the padding is of the convolution's input, not of the normalised tensor
    y = F.conv2d(F.pad(u, (0, 1, 0, 1)), w64, bias.double(), stride=2)
    if gout is not None:
        y.backward(gout.double())
    return y.detach(), w64.grad


@needs_emu
@pytest.mark.parametrize("n,c0,c1,cout,h,w,gn", PAD_END_CASES)
def test_emulated_end_padded_conv(ops, n, c0, c1, cout, h, w, gn):
    from score_sde_pytorch_amd import _lib as L
    x1, x2, wt, bias, G, gamma, beta, _ = _pad_end_case(n, c0, c1, cout, h, w, gn, seed=40 + h)
    ref, _ = _fp64_reference(x1, x2, wt, bias, G, gamma, beta, gn)
    a1, a2 = nhwc(x1), (nhwc(x2) if x2 is not None else None)
    gnt = None
    if gn:
        mean, rstd = ops.groupnorm_stats(a1, G, 1e-6, x2=a2)
        gnt = (mean, rstd, gamma, beta, G)
    y = ops.conv2d(a1, wt, bias, stride=2, pad=0, pad_end=1, x2=a2, pro=L.PRO_GN_SILU if gn else L.PRO_NONE, gn=gnt)
    assert tuple(y.shape) == (n, ref.shape[2], ref.shape[3], cout) == (n, h // 2, w // 2, cout)
    assert rel_err(nchw(y), ref) < 2e-5
    # without the end padding the same output size is refused on even maps (what the parent's kernels did with every such launch)
    if h % 2 == 0:
        with pytest.raises(L.SsdeError, match="larger than input"):
            ops.conv2d(a1, wt, bias, stride=2, pad=0, x2=a2, out_hw=(h // 2, w // 2))


@needs_emu
@pytest.mark.parametrize("n,c0,c1,cout,h,w,gn", PAD_END_CASES)
def test_emulated_end_padded_wgrad(ops, n, c0, c1, cout, h, w, gn):
    from score_sde_pytorch_amd import _lib as L
    x1, x2, wt, bias, G, gamma, beta, gout = _pad_end_case(n, c0, c1, cout, h, w, gn, seed=60 + h)
    _, dw_ref = _fp64_reference(x1, x2, wt, bias, G, gamma, beta, gn, gout)
    a1, a2 = nhwc(x1), (nhwc(x2) if x2 is not None else None)
    gnt = None
    if gn:
        mean, rstd = ops.groupnorm_stats(a1, G, 1e-6, x2=a2)
        gnt = (mean, rstd, gamma, beta, G)
    for splits in (0, 2):
        dw = torch.zeros(cout, c0 + c1, 3, 3)
        ops.conv_wgrad(a1, nhwc(gout), 3, dw, stride=2, pad=0, pad_end=1, x2=a2, pro=L.PRO_GN_SILU if gn else L.PRO_NONE, gn=gnt,
                       scale=0.5, splits=splits)
        assert rel_err(dw, 0.5 * dw_ref) < TOL_OP, splits


@needs_emu
def test_emulated_winograd_tile_refuses_end_padding(ops):
    from score_sde_pytorch_amd import _lib as L
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 8, 8, 32, generator=g)
    wt = torch.randn(64, 32, 3, 3, generator=g)
    for tile in (L.TILE_WINOGRAD, L.TILE_WINOGRAD4):
        with pytest.raises(L.SsdeError, match="pad_end"):
            ops.conv2d(x, wt, None, stride=1, pad=1, pad_end=1, tile=tile, out_hw=(8, 8))
    y = ops.conv2d(x, wt, None, stride=1, pad=1, tile=L.TILE_WINOGRAD)          # pad_end = 0: as before
    assert rel_err(nchw(y), F.conv2d(nchw(x), wt, padding=1)) < 2e-5


@needs_emu
def test_emulated_unconditional_forward():
    """conditional=False: no embedding, no temb addend, the labels are never read"""
    from score_sde_pytorch_amd import engine as E
    cfg = D.small_config(conditional=False)
    model = _model(cfg)
    sd = dict(_util.load_seeded(model, seed=1)); sd["sigmas"] = model.sigmas.clone()
    x, labels = D.forward_inputs(cfg)
    with torch.no_grad():
        ref = _ddpm_oracle.ddpm_forward(cfg, sd, x, labels)
    with emu.emulated():
        eng = E.UNetEngine(model, x.shape[0], 16, 16, torch.device("cpu"))
        y = eng.forward(x, labels)
    assert rel_err(y, ref) < 1e-4


@needs_emu
def test_emulated_small_network_forward_and_gradients():
    """the small DDPM network end to end under the emulator: forward against the reference golden, and every parameter
    gradient + the input gradient against autograd through the restatement"""
    from score_sde_pytorch_amd import backward as B
    from _train_checks import TOL_GRAD, compare_param_grads
    gold = np.load(os.path.join(_util.GOLDEN, "unet_small_ddpm.npz"))
    cfg = D.forward_config("small_ddpm")
    model = _model(cfg)
    sd = {k: v.clone() for k, v in _util.load_seeded(model, seed=1).items()}
    sd["sigmas"] = model.sigmas.clone()
    x, labels = D.forward_inputs(cfg)
    g = torch.Generator().manual_seed(8)
    gout = torch.randn(x.shape, generator=g)
    sd_req = {k: (v.clone().requires_grad_() if k != "sigmas" else v) for k, v in sd.items()}
    xr = x.clone().requires_grad_()
    _ddpm_oracle.ddpm_forward(cfg, sd_req, xr, labels).backward(gout)
    ref = {k: v.grad for k, v in sd_req.items() if k != "sigmas"}
    with emu.emulated():
        eng = B.TrainEngine(model, x.shape[0], 16, 16, torch.device("cpu"), input_grad=True, dropout=False)
        y = eng.forward_train(x, labels).clone()
        assert rel_err(y, torch.from_numpy(gold["y"])) < 1e-4
        eng.backward(gout)
        assert rel_err(eng.gx_view(), xr.grad) < TOL_GRAD
        compare_param_grads(model, eng.flat, ref)


@needs_emu
def test_emulated_whole_network_gradients_on_a_rectangular_image():
    """8x24, attention on 4x12 = 48 tokens, against the fp64 restatement (tests/_train_checks.py: RECT_EMULATED)"""
    import _train_checks as T
    (case,) = [c for c in T.RECT_EMULATED if c[0] == "ddpm"]
    with emu.emulated():
        T.check_rect_grads("cpu", case)


@needs_emu
def test_emulated_training_loss_and_gradients_match_reference(monkeypatch):
    """the fused loss head + backward program on a DDPM model under the emulator, against the reference's loss.backward()"""
    from score_sde_pytorch_amd import losses
    monkeypatch.setattr(losses, "_on_device", lambda t: True)
    with emu.emulated():
        D.check_training_loss_and_gradients("cpu")


@needs_emu
def test_emulated_step_fn_matches_the_reference_run(monkeypatch):
    """step_fn itself under the emulator (program runs; the graph-captured form is the GPU suite's), three steps + eval"""
    from score_sde_pytorch_amd import losses
    monkeypatch.setattr(losses, "_on_device", lambda t: True)
    with emu.emulated():
        D.check_step_fn_against_reference_run("cpu")


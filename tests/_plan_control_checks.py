"""Shared checks of controllable generation through plan blobs (include/ssde.h: ssde_project_prepare, ssde_pc_projection /
ssde_pc_set_known / ssde_pc_reset_known / ssde_pc_set_noise; controllable_generation's fn.engine; tests/c_host/control_host.c)
for the emulator tests (test_plan_control_cpu.py) and the device tests (test_plan_control_gpu.py).

Networks, SDEs, inputs and noise streams are those of _util.CONTROLLABLE_CASES / controllable_inputs(), the cases behind
tests/golden/controllable_small.npz: batch 4, 3 x 16 x 16, N = 6.  The two `*_ve_rd_langevin` entries are the setup of the
bit-for-bit checks: small NCSN++, VESDE, reverse diffusion + Langevin.  `dev` is "cpu" (kernels on the emulator; the caller
holds emu.emulated()) or "cuda".

Bounds:
  * ssde_project_prepare, identity form: torch.equal with the reference's expression (the kernel rounds every product and sum
    once, in torch's order).  Colour form, u = 2^-24: one mat3_apply (a product and two fused multiply-adds per output) has
    forward error <= gamma_3 sum_i |v_i| |M_ij| with gamma_3 = 3u / (1 - 3u) < 4u, so, elementwise and in fp64 from absolute values,
        e_known = 4u |data|^T |M|
        e_y     = e_known mask + 4u |prior (1 - mask)|^T |M| + u |y|          (one rounded sum; products by a 0 / 1 mask are exact)
        e_x     = 4u |y|^T |invM| + e_y^T |invM|
  * plan against the Python-driven engine: the same programs, the same kernels, the same seed word -> torch.equal.
  * plan against the reference: rel_err < 2e-4, the yardstick of tests/test_emulated_sampler.py and tests/test_sampler_gpu.py
    for exactly these cases; the prepare launch adds a few ulp to the start state (the bound above).
"""
import functools
import os
import re
import subprocess
import types

import numpy as np
import torch

import _util

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "c_host", "control_host.c")
INC = os.path.join(_util.ROOT, "include")

BATCH, SIZE, SEED = _util.PC_VARIANT_BATCH, _util.PC_VARIANT_SIZE, 77
BITWISE = {"inpaint": "inpaint_ve_rd_langevin", "colorize": "colorize_ve_rd_langevin"}
REFERENCE_TOL = 2e-4
U = 2.0 ** -24


def gold():
    return np.load(os.path.join(_util.GOLDEN, "controllable_small.npz"))


def matrices():
    """(M, invM) as the colorizer builds them, nine floats each"""
    from score_sde_pytorch_amd import controllable_generation as cg
    M = torch.tensor(cg._M)
    return M.flatten().tolist(), torch.inverse(M).flatten().tolist()


def _mode():
    """the matrix mode is read when a program is lowered: part of every cache key"""
    return os.environ.get("SSDE_MATRIX", "")


# ---- check 1: the prepare launch --------------------------------------------------------------------------------------
def prepare_inputs(n, c, hw, seed):
    g = torch.Generator().manual_seed(seed)
    data = torch.rand(n, c, hw, 1, generator=g)
    prior = torch.randn(n, c, hw, 1, generator=g) * 50.0
    mask = torch.randint(0, 2, (n, c, hw, 1), generator=g).float()
    return data, mask, prior


def check_prepare_identity(dev, n, c, hw):
    from score_sde_pytorch_amd import hipops
    data, mask, prior = (t.to(dev) for t in prepare_inputs(n, c, hw, 11 + hw))
    known, mask_out, x = hipops.project_prepare(data, mask, prior)
    assert torch.equal(x, data * mask + prior * (1. - mask))
    assert torch.equal(known, data) and torch.equal(mask_out, mask)
    known2, _, x2 = hipops.project_prepare(data, mask)                   # without a prior: known and mask only
    assert x2 is None and torch.equal(known2, data)


def check_prepare_colour(dev, n, hw, own_mask):
    from score_sde_pytorch_amd import hipops
    M, invM = matrices()
    data, mask, prior = prepare_inputs(n, 3, hw, 23 + hw)
    if own_mask:
        mask = torch.cat([torch.ones_like(data[:, :1]), torch.zeros_like(data[:, 1:])], dim=1)
    known, mask_out, x = hipops.project_prepare(data.to(dev), None if own_mask else mask.to(dev), prior.to(dev), M, invM)
    known, mask_out, x = known.cpu().double(), mask_out.cpu(), x.cpu().double()
    assert torch.equal(mask_out, mask)
    M64 = torch.tensor(M, dtype=torch.float32).double().view(3, 3)       # the fp32 values the kernel multiplies by
    I64 = torch.tensor(invM, dtype=torch.float32).double().view(3, 3)
    ap = lambda v, A: torch.einsum('bihw,ij->bjhw', v, A)               # noqa: E731
    d, m, p = data.double(), mask.double(), prior.double()
    known64 = ap(d, M64)
    e_known = 4 * U * ap(d.abs(), M64.abs())
    y64 = known64 * m + ap(p * (1 - m), M64)
    e_y = e_known * m + 4 * U * ap((p * (1 - m)).abs(), M64.abs()) + U * y64.abs()
    x64 = ap(y64, I64)
    e_x = 4 * U * ap(y64.abs(), I64.abs()) + ap(e_y, I64.abs())
    worst_k = float(((known - known64).abs() / e_known.clamp_min(1e-300)).max())
    worst_x = float(((x - x64).abs() / e_x.clamp_min(1e-300)).max())
    print("project_prepare colour n=%d hw=%d own_mask=%d: worst |err| / bound: known %.3f, x %.3f" % (n, hw, own_mask, worst_k, worst_x))
    assert bool(((known - known64).abs() <= e_known).all()), worst_k
    assert bool(((x - x64).abs() <= e_x).all()), worst_x


# ---- the cases ----------------------------------------------------------------------------------------------------------
def setup(name, dev):
    """model, SDE, the inpainter / colorizer, its engine and the inputs of one entry of _util.CONTROLLABLE_CASES"""
    return _setup(name, dev, _mode())


@functools.lru_cache(maxsize=None)
def _setup(name, dev, mode):
    from score_sde_pytorch_amd import sde_lib, sampling, controllable_generation as cg
    from score_sde_pytorch_amd.models import utils as mutils
    task, variant, pred, corr = _util.CONTROLLABLE_CASES[name]
    kind, sde_kind, kw, _, _, _, continuous, _, _, eps = _util.PC_VARIANTS[variant]
    cfg = _util.small_config(kind)
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(cfg).eval()
    _util.load_seeded(model, seed=1)
    model = model.to(dev)
    sde = {"vesde": sde_lib.VESDE, "vpsde": sde_lib.VPSDE, "subvpsde": sde_lib.subVPSDE}[sde_kind](**kw)
    make = cg.get_pc_inpainter if task == "inpaint" else cg.get_pc_colorizer
    fn = make(sde, sampling.get_predictor(pred), sampling.get_corrector(corr), lambda v: v, snr=0.16, n_steps=1,
              probability_flow=False, continuous=continuous, denoise=True, eps=eps)
    eng = fn.engine(model, (BATCH, 3, SIZE, SIZE), device="cpu" if dev == "cpu" else None)
    assert eng is not None
    data, mask, prior, noises = _util.controllable_inputs(name, BATCH, kw["N"], SIZE, kw.get("sigma_max", 1.0))
    return types.SimpleNamespace(name=name, task=task, pred=pred, corr=corr, N=kw["N"], model=model, sde=sde, fn=fn, eng=eng,
                                 data=data.to(dev).contiguous(), mask=mask.to(dev).contiguous(), prior=prior.to(dev).contiguous(),
                                 noises=noises.to(dev).contiguous(), given_mask=mask.to(dev).contiguous() if task == "inpaint" else None)


def blob_of(name, dev, with_rng):
    return _blob_of(name, dev, with_rng, _mode())


@functools.lru_cache(maxsize=None)
def _blob_of(name, dev, with_rng, mode):
    from score_sde_pytorch_amd import plan_export
    return plan_export.export_pc_plan(setup(name, dev).eng, with_rng=with_rng)


def load(name, dev, with_rng):
    """a fresh LoadedPlan (its known data not set)"""
    from score_sde_pytorch_amd import plan_export
    return plan_export.LoadedPlan(blob_of(name, dev, with_rng))


def unconditional_blob(dev):
    return _unconditional_blob(dev, _mode())


@functools.lru_cache(maxsize=None)
def _unconditional_blob(dev, mode):
    from score_sde_pytorch_amd import pc_engine, plan_export, sampling
    s = setup(BITWISE["inpaint"], dev)
    plan = pc_engine.plan_fused(s.sde, sampling.ReverseDiffusionPredictor, sampling.LangevinCorrector, s.model, True,
                                types.SimpleNamespace(is_cuda=True))      # only the device kind of x is inspected
    eng = pc_engine.FusedPCSampler(s.model, s.sde, plan, (BATCH, 3, SIZE, SIZE), snr=0.16, n_steps=1, probability_flow=False, eps=1e-5,
                                   device=torch.device(dev))
    return plan_export.export_pc_plan(eng)


def _side_stream(dev):
    """(stream object or None, its handle or None): graph capture needs a non-default stream"""
    if dev == "cpu":
        return None, None
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    return side, side.cuda_stream


# ---- check 2: the plan against the Python-driven engine ------------------------------------------------------------------
def python_run(task, dev):
    """(x, x_mean) of the engine driven from Python: start state of hipops.project_prepare, seed word SEED, launch by launch"""
    return _python_run(task, dev, _mode())


@functools.lru_cache(maxsize=None)
def _python_run(task, dev, mode):
    from score_sde_pytorch_amd import hipops
    s = setup(BITWISE[task], dev)
    M, invM = matrices() if task == "colorize" else (None, None)
    known, mask, x0 = hipops.project_prepare(s.data, s.given_mask, s.prior, M, invM)
    s.eng.set_projection_inputs(known, mask)
    x, x_mean = s.eng.run(x0, seed=SEED, use_graph=False)
    return x.cpu(), x_mean.cpu()


def plan_run(task, dev, use_graph=False):
    """(x, x_mean) of the same iterations through LoadedPlan, from the blob of the same engine"""
    return _plan_run(task, dev, bool(use_graph), _mode())


@functools.lru_cache(maxsize=None)
def _plan_run(task, dev, use_graph, mode):
    s = setup(BITWISE[task], dev)
    plan = load(s.name, dev, True)
    side, stream = _side_stream(dev)
    plan.pc_set_known(s.data, s.given_mask, stream=stream)
    plan.pc_reset_known(s.prior, SEED, stream=stream)
    plan.pc_run(s.N, use_graph=use_graph, stream=stream)
    x, x_mean = plan.pc_state(s.data, stream=stream)
    if side is not None:
        side.synchronize()
    plan.close()
    return x.cpu(), x_mean.cpu()


# ---- check 3: the plan against the reference -----------------------------------------------------------------------------
def reference_run(name, dev):
    """x_mean after N iterations of a plan exported with with_rng=False, fed the noise streams of the golden case"""
    s = setup(name, dev)
    plan = load(name, dev, False)
    stages = [k for k, have in enumerate((s.corr != "none", s.pred != "none", True, True)) if have]
    plan.pc_set_known(s.data, s.given_mask)
    plan.pc_reset_known(s.prior, 0)
    for i in range(s.N):
        for k in stages:
            plan.pc_set_noise(k, s.noises[i, k])
        plan.pc_run(1)
    _, x_mean = plan.pc_state(s.data)
    if dev != "cpu":
        torch.cuda.synchronize()
    plan.close()
    return x_mean.cpu()


def assert_matches_reference(name, x_mean):
    err = _util.rel_err(x_mean, torch.from_numpy(gold()[name]))
    print("controllable plan [%s]: rel_err against the reference %.3g (bound %.1g)" % (name, err, REFERENCE_TOL))
    assert err < REFERENCE_TOL, (name, err)


# ---- check 4: the plain-C host -------------------------------------------------------------------------------------------
def build_c_host(tmp_path, emu_lib=None):
    """control_host.c compiled with gcc: against the emulator library (-DHOST_IS_DEVICE) or libssde_hip.so + the HIP runtime"""
    from score_sde_pytorch_amd import _lib as L
    exe = str(tmp_path / ("control_host_emu" if emu_lib else "control_host"))
    if emu_lib:
        cmd = ["gcc", "-O1", "-std=c11", "-DHOST_IS_DEVICE", "-I", INC, SRC, "-o", exe, emu_lib, "-lm", "-Wl,-rpath," + os.path.dirname(emu_lib)]
    else:
        cmd = ["gcc", "-O1", "-std=c11", "-I", INC, "-I", "/opt/rocm/include", SRC, "-o", exe, L.LIB_PATH, "-L/opt/rocm/lib", "-lamdhip64",
               "-lm", "-Wl,-rpath," + os.path.dirname(L.LIB_PATH), "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def run_c_host(exe, task, dev, tmp_path, use_graph, timeout):
    """one child process on the blob of check 2: inpainting with its mask given, colorization with the mask left to the
    library; returns x_mean [B,C,H,W] as the host wrote it"""
    s = setup(BITWISE[task], dev)
    f = {k: str(tmp_path / (task + "_" + k)) for k in ("plan.blob", "data.f32", "mask.f32", "prior.f32", "x_mean.f32")}
    open(f["plan.blob"], "wb").write(blob_of(s.name, dev, True))
    for k, t in (("data.f32", s.data), ("prior.f32", s.prior)) + ((("mask.f32", s.given_mask),) if s.given_mask is not None else ()):
        t.cpu().numpy().astype(np.float32).tofile(f[k])
    cmd = [exe, f["plan.blob"], f["data.f32"], f["mask.f32"] if s.given_mask is not None else "-", f["prior.f32"], str(SEED), str(s.N),
           str(int(use_graph)), f["x_mean.f32"]]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    m = re.search(r"control_host: (inpainting|colorization), .* checksum (\S+)", r.stdout)
    assert m and m.group(1) == {"inpaint": "inpainting", "colorize": "colorization"}[task], r.stdout
    print(r.stdout.strip())
    out = np.fromfile(f["x_mean.f32"], dtype=np.float32).reshape(tuple(s.data.shape))
    assert abs(float(m.group(2)) - float(out.astype(np.float64).sum())) <= 1e-6 * float(np.abs(out).astype(np.float64).sum())
    return out


# ---- check 6: refusals ---------------------------------------------------------------------------------------------------
def check_refusals(dev):
    from score_sde_pytorch_amd import plan_export as X
    inp, col = setup(BITWISE["inpaint"], dev), setup(BITWISE["colorize"], dev)
    p = lambda t: t.data_ptr()                                           # noqa: E731

    def refused(lib, rc, *words):
        msg = lib.ssde_last_error() or b""
        assert rc != 0 and all(w.encode() in msg for w in words), (rc, msg, words)

    plain = X.LoadedPlan(unconditional_blob(dev))
    lib = plain.lib
    assert plain.pc_projection() == X.PC_PROJ_NONE == 0
    refused(lib, lib.ssde_pc_set_known(plain.handle, p(inp.data), p(inp.mask), None), "pc_set_known", "no projection")
    refused(lib, lib.ssde_pc_reset_known(plain.handle, p(inp.prior), 1, None), "pc_reset_known", "no projection")
    refused(lib, lib.ssde_pc_set_noise(plain.handle, 0, p(inp.prior), None), "pc_set_noise", "draws its own noise")
    plain.close()

    plan = load(inp.name, dev, True)
    assert plan.pc_projection() == X.PC_PROJ_MASK == 1
    refused(lib, lib.ssde_pc_reset_known(plan.handle, p(inp.prior), 1, None), "pc_reset_known", "never set")
    refused(lib, lib.ssde_pc_run(plan.handle, 1, 0, None), "pc_run", "never set")
    refused(lib, lib.ssde_pc_set_known(plan.handle, p(inp.data), None, None), "pc_set_known", "mask")      # no mask of its own
    refused(lib, lib.ssde_pc_reset_known(plan.handle, p(inp.prior), 1, None), "pc_reset_known", "never set")   # ... and nothing was set
    refused(lib, lib.ssde_pc_set_noise(plan.handle, 2, p(inp.prior), None), "pc_set_noise", "draws its own noise")
    plan.pc_set_known(inp.data, inp.mask)
    plan.pc_reset(inp.prior, 1)                                         # a host that composes the start state itself
    plan.close()

    plan = load(col.name, dev, True)
    assert plan.pc_projection() == X.PC_PROJ_COLOR == 2
    plan.close()

    name = "inpaint_vp_ancestral_none"                                   # no corrector: no buffer for its noise
    s = setup(name, dev)
    plan = load(name, dev, False)
    assert plan.pc_projection() == X.PC_PROJ_MASK
    refused(lib, lib.ssde_pc_set_noise(plan.handle, 0, p(s.prior), None), "pc_set_noise", "no corrector stage")
    refused(lib, lib.ssde_pc_set_noise(plan.handle, 4, p(s.prior), None), "pc_set_noise")
    for k in (1, 2, 3):
        plan.pc_set_noise(k, s.noises[0, k])
    plan.close()
    if dev != "cpu":
        torch.cuda.synchronize()
    unet = X.LoadedPlan(_unet_blob(dev, _mode()))
    rc = lib.ssde_pc_projection(unet.handle)
    assert rc < 0, rc
    refused(lib, rc, "pc_projection", "not a sampler plan")
    unet.close()


@functools.lru_cache(maxsize=None)
def _unet_blob(dev, mode):
    from score_sde_pytorch_amd import engine as E, plan_export
    s = setup(BITWISE["inpaint"], dev)
    return plan_export.export_unet_plan(E.UNetEngine(s.model, BATCH, SIZE, SIZE, torch.device(dev)))

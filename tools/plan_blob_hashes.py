#!/usr/bin/env python
"""Print `name size sha256` of the plan blobs the Python host exports, lowered on the CPU under the test-only emulator.

    python tools/plan_blob_hashes.py [name ...]          # no GPU needed; SSDE_* switches are read from the environment

A blob holds the op bytes, regions, relocations, parameter table and packed weights of a lowered program
(score_sde_pytorch_amd/plan_export.py), position independent, so two commits that print the same lines lower, compose,
pack and export identically.  Networks and cases are those of the tests (tests/_util.py and friends; seeded weights).
"""
import hashlib
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _util                                            # noqa: E402
import emu                                              # noqa: E402

CPU = torch.device("cpu")


def _model(cfg, family="ncsnpp"):
    from score_sde_pytorch_amd.models import utils as mutils
    torch.manual_seed(0)
    model = mutils.get_model(family)(cfg).eval()
    _util.load_seeded(model, seed=1)
    return model


def _unet(cfg, family="ncsnpp", batch=2):
    from score_sde_pytorch_amd import engine as E, plan_export
    R = cfg.data.image_size
    return plan_export.export_unet_plan(E.UNetEngine(_model(cfg, family), batch, R, R, CPU))


def _pc(projection):
    from score_sde_pytorch_amd import pc_engine, plan_export, sampling, sde_lib
    model = _model(_util.small_config("ncsnpp"))
    sde = sde_lib.VESDE(sigma_min=0.01, sigma_max=50, N=6)
    plan = pc_engine.plan_fused(sde, sampling.ReverseDiffusionPredictor, sampling.LangevinCorrector, model, True,
                                types.SimpleNamespace(is_cuda=True))      # only the device kind of x is inspected
    eng = pc_engine.FusedPCSampler(model, sde, plan, (2, 3, 16, 16), snr=0.16, n_steps=1, probability_flow=False, eps=1e-5,
                                   device=CPU, projection=projection)
    return plan_export.export_pc_plan(eng)


def _colorizer_matrices():
    from score_sde_pytorch_amd import controllable_generation as cg
    M = torch.tensor(cg._M)
    return dict(M=M.flatten().tolist(), invM=torch.inverse(M).flatten().tolist())


def _train():
    import _train_checks as T
    from score_sde_pytorch_amd import plan_export
    case = T._train_plan_case("cpu", dropout=0.1)
    opt, ema, fs = case[4], case[5], case[8]
    return plan_export.export_train_plan(fs, opt, ema)


def _ddpm():
    import _ddpm_util as D
    return _unet(D.small_config(), "ddpm", D.FORWARD_BATCH)


def _gn_width():
    import _gn_width_util as W
    return _unet(W.small_config(), batch=W.BATCH)


def _ode(kind):
    import _plan_ode_checks as P
    return P.rhs_of(kind, "cpu")[1]


PLANS = [("unet_ncsnpp", lambda: _unet(_util.small_config("ncsnpp"))),
         ("unet_ddpmpp", lambda: _unet(_util.small_config("ddpmpp"))),
         ("unet_ddpm", _ddpm),
         ("unet_gn_width", _gn_width),
         ("pc", lambda: _pc(None)),
         ("pc_projection", lambda: _pc(_colorizer_matrices())),
         ("ode_sample", lambda: _ode("sample")),
         ("ode_likelihood", lambda: _ode("likelihood")),
         ("train", _train)]


def main(names):
    unknown = set(names) - {n for n, _ in PLANS}
    if unknown:
        raise SystemExit("unknown plan(s) %s; known: %s" % (sorted(unknown), " ".join(n for n, _ in PLANS)))
    if not emu.available():
        raise SystemExit("the kernel emulator needs x86-64 and ROCm's clang++")
    with emu.emulated():
        for name, make in PLANS:
            if names and name not in names:
                continue
            blob = make()
            print("%s %d %s" % (name, len(blob), hashlib.sha256(blob).hexdigest()), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])

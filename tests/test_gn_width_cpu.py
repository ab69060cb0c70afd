"""GroupNorm groups of any width (CPU): dry lowering of every NCSN++ config of the reference, the two 1024-px presets, the new
kernels under the test-only emulator (tests/emu/) against fp64, the lowering of the nf = 16 network against the reference's
forward and oracle autograd, unchanged programs, and the plan round trip.  See tests/_gn_width_checks.py."""
import importlib.util
import os
import sys
import types

import pytest
import torch

import emu
import _util
import _gn_width_checks as K
import _gn_width_util as W

REF_CONFIGS = "/root/reference/configs"
needs_emu = pytest.mark.skipif(not emu.available(), reason="emulator needs x86-64 + ROCm's clang++")


@pytest.fixture
def emulated():
    with emu.emulated():
        yield


def _dry(cfg, batch=1):
    from score_sde_pytorch_amd import engine as E
    from score_sde_pytorch_amd.models import utils as mutils
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(cfg)
    R = cfg.data.image_size
    eng = E.UNetEngine(model, batch, R, R, "cpu")
    lds = eng.validate_plans()
    assert lds and all(v > 0 for v in lds)
    return eng


def _reference_configs():
    """every configs/**/*.py of the reference with model.name == 'ncsnpp', loaded with ml_collections or, where that package is
    not installed, with the few lines of ConfigDict the files use"""
    if "ml_collections" not in sys.modules and importlib.util.find_spec("ml_collections") is None:
        shim = types.ModuleType("ml_collections")

        class ConfigDict(dict):
            def __getattr__(self, k):
                try:
                    return self[k]
                except KeyError:
                    raise AttributeError(k)

            def __setattr__(self, k, v):
                self[k] = v
        shim.ConfigDict = ConfigDict
        sys.modules["ml_collections"] = shim
        added = True
    else:
        added = False
    out = {}
    sys.path.insert(0, os.path.dirname(REF_CONFIGS))
    try:
        for root, _, files in sorted(os.walk(REF_CONFIGS)):
            for f in sorted(files):
                if not f.endswith(".py") or f.startswith("default_") or f == "__init__.py":
                    continue
                rel = os.path.relpath(os.path.join(root, f), REF_CONFIGS)[:-3]
                spec = importlib.util.spec_from_file_location("_refcfg_" + rel.replace(os.sep, "_"), os.path.join(root, f))
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)
                cfg = mod.get_config()
                if cfg.model.name == "ncsnpp":
                    out[rel.replace(os.sep, "/")] = cfg
    finally:
        sys.path.pop(0)
        for k in [k for k in sys.modules if k == "configs" or k.startswith("configs.")]:
            del sys.modules[k]
        if added:
            del sys.modules["ml_collections"]
    return out


@pytest.mark.skipif(not os.path.isdir(REF_CONFIGS), reason="the reference's configs/ directory is not on this machine")
def test_every_ncsnpp_config_of_the_reference_lowers():
    from score_sde_pytorch_amd import configs
    refs = _reference_configs()
    assert len(refs) == 20, sorted(refs)
    for name, ref in sorted(refs.items()):
        _dry(configs.from_reference(ref))
    for name in ("ve/ffhq_ncsnpp_continuous", "ve/celebahq_ncsnpp_continuous"):
        ref, mine = refs[name], configs.get_config(name)
        for sec in ("training", "sampling", "eval", "data", "model", "optim"):
            for k, v in ref[sec].items():
                if k == "tfrecords_path":
                    continue
                mv = mine[sec][k]
                assert (tuple(v) == tuple(mv)) if isinstance(v, (list, tuple)) else (v == mv), (name, sec, k, v, mv)
        assert ref["seed"] == mine["seed"]


@pytest.mark.parametrize("name", ["ve/ffhq_ncsnpp_continuous", "ve/celebahq_ncsnpp_continuous"])
def test_1024_px_presets_lower(name):
    """the presets themselves (no reference needed): 1024 px, nf = 16, ch_mult (1, 2, 4, 8, 16, 32, 32, 32); batch 1 and the
    training batch the config names"""
    from score_sde_pytorch_amd import configs, _lib as L
    cfg = configs.get_config(name)
    assert (cfg.data.image_size, cfg.model.nf, tuple(cfg.model.ch_mult), cfg.model.num_res_blocks) == (1024, 16, (1, 2, 4, 8, 16, 32, 32, 32), 1)
    assert (cfg.training.batch_size, cfg.sampling.snr, cfg.model.sigma_max) == (8, 0.15, 1348)
    assert cfg.training.reduce_mean == (name == "ve/ffhq_ncsnpp_continuous")
    for batch in (1, cfg.training.batch_size):
        kinds, fused = K.program_facts(_dry(cfg, batch).program)
        assert kinds.count(L.OP_GN_APPLY) >= 1 and all(w % 4 == 0 for w in fused)


def test_small_failing_net_lowers_dry():
    """the issue's reproduction: batch 2, 32 px, nf = 16, ch_mult (1, 2, 4, 8)"""
    from score_sde_pytorch_amd import engine as E, backward as B, _lib as L
    from score_sde_pytorch_amd.models import utils as mutils
    cfg = W.small_config()
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(cfg)
    eng = E.UNetEngine(model, 2, 32, 32, "cpu")
    eng.validate_plans()
    assert K.program_facts(eng.program)[0].count(L.OP_GN_APPLY) >= 1
    tr = B.TrainEngine(model, 2, 32, 32, "cpu")
    kinds, fused = K.program_facts(tr.program)
    assert kinds.count(L.OP_GN_APPLY_BWD) >= 1 and all(w % 4 == 0 for w in fused)


# op count of ve/cifar10_ncsnpp_continuous at batch 2 (CPU dry lowering, the default route heuristic SSDE_WINOGRAD=1), recorded
# from commit 1e1aac0 (the parent of this change): 108 conv, 9 upfirdn, 6 attention, 95 GroupNorm finalize, embed, 2 boundary ops
CIFAR_OPS_AT_1E1AAC0 = 221


def test_programs_without_narrow_groups_are_unchanged(monkeypatch):
    from score_sde_pytorch_amd import configs, engine as E, _lib as L
    from score_sde_pytorch_amd.models import utils as mutils
    monkeypatch.setenv("SSDE_WINOGRAD", "1")
    cfg = configs.get_config("ve/cifar10_ncsnpp_continuous")
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(cfg)
    eng = E.UNetEngine(model, 2, 32, 32, "cpu")
    kinds, fused = K.program_facts(eng.program)
    assert L.OP_GN_APPLY not in kinds and L.OP_GN_APPLY_BWD not in kinds
    assert len(kinds) == CIFAR_OPS_AT_1E1AAC0
    assert (kinds.count(L.OP_CONV), kinds.count(L.OP_UPFIRDN), kinds.count(L.OP_ATTN), kinds.count(L.OP_GN_FINALIZE)) == (108, 9, 6, 95)
    assert fused and all(w % 4 == 0 for w in fused)
    for i in range(eng.program.n):
        op = eng.program.ops[i]
        if op.kind == L.OP_CONV:
            for s in (op.u.conv.main, op.u.conv.aux):
                assert not s.gn_groups or ((s.c0 + s.c1) // s.gn_groups) % 4 == 0


@needs_emu
@pytest.mark.parametrize("side", K.KERNEL_MAPS)
@pytest.mark.parametrize("shape", K.KERNEL_SHAPES, ids=lambda s: "%d+%d_in_%d" % s)
def test_kernels_against_fp64(emulated, shape, side):
    K.check_kernels("cpu", *shape, side)


@needs_emu
def test_any_width_statistics_kernel_has_the_quad_kernels_bits(emulated):
    K.check_any_width_kernel_has_the_quad_kernels_bits("cpu")


@needs_emu
def test_fused_prologues_still_refuse_a_narrow_group(emulated):
    """called directly through the C ABI the consumers refuse such a source, as before"""
    from score_sde_pytorch_amd import hipops as ops, _lib as L
    x = torch.randn(1, 8, 8, 48)
    mean, rstd = ops.groupnorm_stats(x, 8)                    # 6 per group: the statistics pass accepts it
    w = torch.randn(32, 48, 3, 3)
    with pytest.raises(L.SsdeError, match="channels-per-group"):
        ops.conv2d(x, w, None, pro=L.PRO_GN_SILU, gn=(mean, rstd, torch.ones(48), torch.zeros(48), 8))


@needs_emu
def test_small_net_forward_against_the_reference(emulated):
    K.check_small_net_forward("cpu", tol=2e-6)


@needs_emu
def test_small_net_gradients_against_oracle_autograd(emulated):
    K.check_small_net_grads("cpu")


@needs_emu
def test_small_net_dropout_through_the_apply_launch(emulated):
    K.check_small_net_dropout("cpu")


@needs_emu
def test_plan_round_trip(emulated):
    K.check_plan_round_trip("cpu")

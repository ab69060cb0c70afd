"""Controllable generation from plan blobs on the emulator (`-m "not gpu"`): the prepare launch against fp64, the blob of an
inpainter's / colorizer's engine through plan_export.LoadedPlan against the Python-driven engine and against the reference,
tests/c_host/control_host.c compiled with gcc against the emulator library, and the refusals.  The loader, the relocation
and the entry points of csrc/plan.hip run for real; the kernels run on the emulator.  Cases, bounds and the reasons for them:
_plan_control_checks.py."""
import numpy as np
import pytest
import torch

import _plan_control_checks as P


@pytest.fixture()
def emulated():
    import emu
    if not emu.available():
        pytest.skip("emulator needs x86-64 + ROCm's clang++")
    with emu.emulated():
        yield emu


@pytest.mark.parametrize("shape", [(2, 1, 7), (2, 4, 64)])
def test_project_prepare_identity_form_is_the_reference_expression(shape, emulated):
    P.check_prepare_identity("cpu", *shape)


@pytest.mark.parametrize("own_mask", [False, True])
@pytest.mark.parametrize("n,hw", [(3, 25), (5, 64)])
def test_project_prepare_colour_form_against_fp64(n, hw, own_mask, emulated):
    P.check_prepare_colour("cpu", n, hw, own_mask)


def test_project_prepare_refuses_what_it_cannot_do(emulated):
    from score_sde_pytorch_amd import hipops, _lib as L
    data, mask, prior = P.prepare_inputs(2, 4, 9, 5)
    with pytest.raises(L.SsdeError, match="mask == NULL"):
        hipops.project_prepare(data, None, prior)
    M, invM = P.matrices()
    with pytest.raises(L.SsdeError, match="3 channels"):
        hipops.project_prepare(data, mask, prior, M, invM)


def test_engine_of_the_returned_functions(emulated):
    """fn.engine: the cached engine a call uses (None where the generic loop runs), exportable without a GPU"""
    from score_sde_pytorch_amd import pc_engine, plan_export as X
    s = P.setup(P.BITWISE["inpaint"], "cpu")
    assert isinstance(s.eng, pc_engine.FusedPCSampler) and s.eng.projection is not None
    assert s.fn.engine(s.model, (P.BATCH, 3, P.SIZE, P.SIZE), device="cpu") is s.eng          # built once
    assert s.fn.engine(s.model, (P.BATCH, 3, P.SIZE, P.SIZE)) is None                         # a host model: the generic loop
    hdr = X.LoadedPlan(P.blob_of(s.name, "cpu", True)).header
    assert hdr.kind == X.PLAN_PC and hdr.sde_steps == s.N and hdr.nfe_per_iteration == 2
    assert (hdr.batch, hdr.channels, hdr.height, hdr.width) == (P.BATCH, 3, P.SIZE, P.SIZE)


def test_blob_of_an_engine_survives_flattening_of_its_model(emulated):
    """a training engine built later on the same model moves the parameters into one flat buffer (backward.FlatParams); the
    inference engine's blob stays what it was, byte for byte"""
    from score_sde_pytorch_amd import backward, engine as E, plan_export as X
    from score_sde_pytorch_amd.models import utils as mutils
    torch.manual_seed(0)
    model = mutils.get_model("ncsnpp")(P._util.small_config("ncsnpp")).eval()
    P._util.load_seeded(model, seed=1)
    eng = E.UNetEngine(model, 2, 16, 16, torch.device("cpu"))
    before = X.export_unet_plan(eng)
    trained = lambda: next(p for p in model.parameters() if p.requires_grad)   # noqa: E731
    assert trained().untyped_storage().nbytes() == trained().numel() * 4
    backward.flat_params_of(model, torch.device("cpu"))
    assert trained().untyped_storage().nbytes() > trained().numel() * 4
    assert X.export_unet_plan(eng) == before


@pytest.mark.parametrize("task", ["inpaint", "colorize"])
def test_plan_reproduces_python_driven_engine(task, emulated):
    x_py, xm_py = P.python_run(task, "cpu")
    x, xm = P.plan_run(task, "cpu")
    assert torch.isfinite(x).all() and torch.equal(x, x_py) and torch.equal(xm, xm_py)


def test_known_pixels_come_back_bit_for_bit(emulated):
    """VE inpainting: on mask == 1 the last projection writes x_mean = x * 0 + data * 1"""
    s = P.setup(P.BITWISE["inpaint"], "cpu")
    _, xm = P.plan_run("inpaint", "cpu")
    known = s.mask.cpu() == 1
    assert known.any() and not known.all() and torch.equal(xm[known], s.data.cpu()[known])


@pytest.mark.parametrize("name", ["inpaint_vp_ancestral_none", "colorize_ve_rd_langevin"])
def test_plan_with_injected_noise_matches_reference(name, emulated):
    P.assert_matches_reference(name, P.reference_run(name, "cpu"))


@pytest.mark.parametrize("task", ["inpaint", "colorize"])
def test_control_host_c_matches_loaded_plan(task, emulated, tmp_path):
    exe = P.build_c_host(tmp_path, emu_lib=emulated.build_emu.build())
    out = P.run_c_host(exe, task, "cpu", tmp_path, use_graph=False, timeout=900)
    assert np.array_equal(out, P.plan_run(task, "cpu")[1].numpy())


def test_refusals_name_their_entry_point(emulated):
    P.check_refusals("cpu")

"""The kernels between U-Net evaluations -- sampler, ODE, loss-head and optimizer launches -- on the emulator (`-m "not gpu"`)
against fp64: every case of _update_checks.py but the "large" ones (whose second grid-stride pass needs a million elements).
Cases, references, bounds and the reasons for them: _update_checks.py."""
import itertools

import pytest

import _update_checks as K


@pytest.fixture()
def emulated():
    import emu
    if not emu.available():
        pytest.skip("emulator needs x86-64 + ROCm's clang++")
    with emu.emulated():
        yield emu


@pytest.mark.parametrize("n", K.BATCHES)
def test_sumsq_per_sample(n, emulated):
    for per in K.PERS:
        K.check_sumsq("cpu", n, per)


@pytest.mark.parametrize("n", K.BATCHES)
def test_langevin_update(n, emulated):
    for per, (alpha_tab, step) in zip(K.PERS, itertools.cycle(K.LANGEVIN_MODES)):
        K.check_langevin("cpu", n, per, alpha_tab, step)
    for alpha_tab, step in K.LANGEVIN_MODES:
        K.check_langevin("cpu", n, 257, alpha_tab, step)


@pytest.mark.parametrize("with_z", [True, False])
def test_predictor_update(with_z, emulated):
    for numel, step in itertools.product(K.NUMELS, K.STEPS):
        K.check_predictor("cpu", numel, step, with_z)


@pytest.mark.parametrize("use_a,use_y,use_z", list(itertools.product([False, True], repeat=3)))
def test_sample_update_every_combination(use_a, use_y, use_z, emulated):
    for n, per in K.FEW_SHAPES:
        K.check_sample_update("cpu", n, per, use_a, use_y, use_z)


@pytest.mark.parametrize("n", K.BATCHES)
def test_sample_update_shapes(n, emulated):
    for per in K.PERS:
        K.check_sample_update("cpu", n, per, True, True, True)


def test_project_update_elementwise(emulated):
    for (n, c, hw), step in itertools.product(K.PROJECT_SHAPES, K.STEPS):
        K.check_project("cpu", n, c, hw, step)


@pytest.mark.parametrize("own_mask", [False, True])
def test_project_update_colour_form(own_mask, emulated):
    for hw, step in itertools.product(K.COLOUR_HW, K.STEPS):
        K.check_project_colour("cpu", 3, hw, step, own_mask)


@pytest.mark.parametrize("use_a", [False, True])
def test_perturb(use_a, emulated):
    for n, per in K.SHAPES:
        K.check_perturb("cpu", n, per, use_a)


@pytest.mark.parametrize("use_dyn", [False, True])
def test_pf_drift(use_dyn, emulated):
    for numel in K.NUMELS:
        K.check_pf_drift("cpu", numel, use_dyn)


@pytest.mark.parametrize("use_dyn,dst_off", [(False, 0), (False, 5), (True, 0), (True, 5)])
def test_hutch_div(use_dyn, dst_off, emulated):
    for n, per in K.SHAPES:
        K.check_hutch_div("cpu", n, per, use_dyn, dst_off)


@pytest.mark.parametrize("terms", sorted(K.RK_COEF))
def test_rk_combine_rows(terms, emulated):
    for n, n32 in itertools.product(K.NUMELS, K.N32_MODES):
        K.check_rk_combine("cpu", n, terms, None if n32 is None else min(n32, n - 1))


@pytest.mark.parametrize("pair", [0, 1])
def test_rk_error_norm_rows(pair, emulated):
    for n in K.NUMELS:
        K.check_rk_error("cpu", n, pair)
    if pair:
        K.check_rk_error("cpu", 257, 1, zero=True)
        K.check_rk_error("cpu", 257, 1, h_abs=0.0)


def test_rk_error_norm_refusals_name_their_entry_point(emulated):
    K.check_rk_error_refusals("cpu")


@pytest.mark.parametrize("reduce_mean,lw", list(itertools.product([False, True], repeat=2)))
def test_dsm_loss(reduce_mean, lw, emulated):
    for (n, per), (gs, want) in itertools.product(K.DSM_SHAPES, K.DSM_MODES):
        K.check_dsm_loss("cpu", n, per, reduce_mean, lw, grad_scale=gs, want_grad=want)


def test_sumsq_flat(emulated):
    for numel in K.FLAT_NUMELS:
        K.check_sumsq_flat("cpu", numel)


@pytest.mark.parametrize("name", sorted(K.ADAM_CASES))
def test_adam_clip_ema_updates(name, emulated):
    for numel, wd, use_ema in itertools.product(K.ADAM_NUMELS, (0.0, 0.01), (True, False)):
        K.check_adam("cpu", numel, wd=wd, use_ema=use_ema, **K.ADAM_CASES[name])


def test_layout_to_nhwc(emulated):
    for mode, c_pad in itertools.product((0, 1, 2), (3, 4, 8)):
        K.check_to_nhwc("cpu", 3, 3, 5, 9, c_pad, mode)


def test_layout_to_nchw(emulated):
    for mode, (alpha, acc) in itertools.product((0, 1, 2), K.NCHW_MODES):
        K.check_to_nchw("cpu", 3, 3, 5, 9, 8, mode, alpha, acc)


@pytest.mark.parametrize("act", [1, 3])
@pytest.mark.parametrize("use_bias", [False, True])
def test_fused_bias_act_forward_and_gradient_mode(act, use_bias, emulated):
    K.check_bias_act("cpu", (4, 6, 5, 7), act, use_bias)
    K.check_bias_act_empty("cpu")


@pytest.mark.parametrize("acc", [False, True])
def test_axpy(acc, emulated):
    for numel in K.NUMELS:
        K.check_axpy("cpu", numel, acc)


def test_fill_from_table_and_step_inc(emulated):
    K.check_fill_and_step("cpu")
    K.check_step_sequence("cpu")


def test_randn_reproducible_and_seed_word(emulated):
    K.check_randn_reproducible("cpu")


def test_randn_every_size_is_finite(emulated):
    K.check_randn_sizes("cpu")


def test_randn_moments_and_correlations(emulated):
    K.check_randn_moments("cpu")


def test_float4_entry_points_refuse_unaligned_pointers(emulated):
    K.check_alignment_refusals("cpu")

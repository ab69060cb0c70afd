"""The kernels between U-Net evaluations -- sampler, ODE, loss-head and optimizer launches -- on the MI355X against fp64: the
cases of the emulator suite (tests/test_update_cpu.py) and, per kernel, the "large" case whose grid-stride loop takes a
second, ragged pass past the block cap.  Cases, references, bounds and the reasons for them: _update_checks.py."""
import itertools

import pytest

import _update_checks as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
H_, W_ = 749, 467                     # 3 * 749 * 467 == K.LARGE
assert 3 * H_ * W_ == K.LARGE


@pytest.mark.parametrize("n", K.BATCHES)
def test_sumsq_per_sample(n):
    for per in K.PERS:
        K.check_sumsq(DEV, n, per)


@pytest.mark.parametrize("n", K.BATCHES)
def test_langevin_update(n):
    for per, (alpha_tab, step) in zip(K.PERS, itertools.cycle(K.LANGEVIN_MODES)):
        K.check_langevin(DEV, n, per, alpha_tab, step)
    for alpha_tab, step in K.LANGEVIN_MODES:
        K.check_langevin(DEV, n, 257, alpha_tab, step)


def test_langevin_update_large():
    K.check_langevin(DEV, 3, K.LARGE // 3, True, 3)


@pytest.mark.parametrize("with_z", [True, False])
def test_predictor_update(with_z):
    for numel, step in itertools.product(K.NUMELS, K.STEPS):
        K.check_predictor(DEV, numel, step, with_z)
    K.check_predictor(DEV, K.LARGE, 1, with_z)


@pytest.mark.parametrize("use_a,use_y,use_z", list(itertools.product([False, True], repeat=3)))
def test_sample_update_every_combination(use_a, use_y, use_z):
    for n, per in K.FEW_SHAPES:
        K.check_sample_update(DEV, n, per, use_a, use_y, use_z)


@pytest.mark.parametrize("n", K.BATCHES)
def test_sample_update_shapes(n):
    for per in K.PERS:
        K.check_sample_update(DEV, n, per, True, True, True)


def test_sample_update_large():
    K.check_sample_update(DEV, 3, K.LARGE // 3, True, True, True)


def test_project_update_elementwise():
    for (n, c, hw), step in itertools.product(K.PROJECT_SHAPES, K.STEPS):
        K.check_project(DEV, n, c, hw, step)
    K.check_project(DEV, 1, 1, K.LARGE, 1)


@pytest.mark.parametrize("own_mask", [False, True])
def test_project_update_colour_form(own_mask):
    for hw, step in itertools.product(K.COLOUR_HW, K.STEPS):
        K.check_project_colour(DEV, 3, hw, step, own_mask)


def test_project_update_colour_form_large():
    K.check_project_colour(DEV, 1, K.LARGE, 1, False)


@pytest.mark.parametrize("use_a", [False, True])
def test_perturb(use_a):
    for n, per in K.SHAPES:
        K.check_perturb(DEV, n, per, use_a)
    K.check_perturb(DEV, 3, K.LARGE // 3, use_a)


@pytest.mark.parametrize("use_dyn", [False, True])
def test_pf_drift(use_dyn):
    for numel in K.NUMELS:
        K.check_pf_drift(DEV, numel, use_dyn)
    K.check_pf_drift(DEV, K.LARGE, use_dyn)


@pytest.mark.parametrize("use_dyn,dst_off", [(False, 0), (False, 5), (True, 0), (True, 5)])
def test_hutch_div(use_dyn, dst_off):
    for n, per in K.SHAPES:
        K.check_hutch_div(DEV, n, per, use_dyn, dst_off)


@pytest.mark.parametrize("terms", sorted(K.RK_COEF))
def test_rk_combine_rows(terms):
    for n, n32 in itertools.product(K.NUMELS, K.N32_MODES):
        K.check_rk_combine(DEV, n, terms, None if n32 is None else min(n32, n - 1))


def test_rk_combine_rows_large():
    K.check_rk_combine(DEV, K.LARGE, 1, 100, rows=2)


@pytest.mark.parametrize("pair", [0, 1])
def test_rk_error_norm_rows(pair):
    for n in K.NUMELS:
        K.check_rk_error(DEV, n, pair)
    if pair:
        K.check_rk_error(DEV, 257, 1, zero=True)
        K.check_rk_error(DEV, 257, 1, h_abs=0.0)
    K.check_rk_error(DEV, (131072 if pair else 262144) + 261, pair)


def test_rk_error_norm_refusals_name_their_entry_point():
    K.check_rk_error_refusals(DEV)


@pytest.mark.parametrize("reduce_mean,lw", list(itertools.product([False, True], repeat=2)))
def test_dsm_loss(reduce_mean, lw):
    for (n, per), (gs, want) in itertools.product(K.DSM_SHAPES, K.DSM_MODES):
        K.check_dsm_loss(DEV, n, per, reduce_mean, lw, grad_scale=gs, want_grad=want)


def test_sumsq_flat():
    for numel in K.FLAT_NUMELS + (K.FLAT_LARGE,):
        K.check_sumsq_flat(DEV, numel)


@pytest.mark.parametrize("name", sorted(K.ADAM_CASES))
def test_adam_clip_ema_updates(name):
    for numel, wd, use_ema in itertools.product(K.ADAM_NUMELS, (0.0, 0.01), (True, False)):
        K.check_adam(DEV, numel, wd=wd, use_ema=use_ema, **K.ADAM_CASES[name])


def test_adam_clip_ema_updates_large():
    K.check_adam(DEV, K.ADAM_LARGE, wd=0.01, use_ema=True, **K.ADAM_CASES["clipped"])


def test_layout_to_nhwc():
    for mode, c_pad in itertools.product((0, 1, 2), (3, 4, 8)):
        K.check_to_nhwc(DEV, 3, 3, 5, 9, c_pad, mode)
    K.check_to_nhwc(DEV, 1, 3, H_, 3 * W_, 4, 1)                               # K.LARGE pixels


def test_layout_to_nchw():
    for mode, (alpha, acc) in itertools.product((0, 1, 2), K.NCHW_MODES):
        K.check_to_nchw(DEV, 3, 3, 5, 9, 8, mode, alpha, acc)
    K.check_to_nchw(DEV, 1, 3, H_, W_, 4, 2, 0.7, True)                        # K.LARGE elements


@pytest.mark.parametrize("act", [1, 3])
@pytest.mark.parametrize("use_bias", [False, True])
def test_fused_bias_act_forward_and_gradient_mode(act, use_bias):
    K.check_bias_act(DEV, (4, 6, 5, 7), act, use_bias)
    K.check_bias_act_empty(DEV)


def test_fused_bias_act_large():
    K.check_bias_act(DEV, (1, 3, H_, W_), 3, True)


@pytest.mark.parametrize("acc", [False, True])
def test_axpy(acc):
    for numel in K.NUMELS + (K.LARGE,):
        K.check_axpy(DEV, numel, acc)


def test_fill_from_table_and_step_inc():
    K.check_fill_and_step(DEV)
    K.check_step_sequence(DEV)


def test_randn_reproducible_and_seed_word():
    K.check_randn_reproducible(DEV)


def test_randn_every_size_is_finite():
    K.check_randn_sizes(DEV)


def test_randn_moments_and_correlations():
    K.check_randn_moments(DEV)


def test_randn_large_second_pass():
    K.check_randn_large(DEV)


def test_float4_entry_points_refuse_unaligned_pointers():
    K.check_alignment_refusals(DEV)

"""The resident 2-D engine (mtip2d_run and friends, the fused gfx950 step kernels of csrc/k_polar2d.hip; MTIP2D(..., resident=True))
on a real MI355X: the cases of tests/test_emul_resident2d.py through the HIP build, and the sizes the emulator cannot reach
(128 shells x M = 64, the worker at 32 x M = 16).  Run with `pytest -m gpu`."""
import pytest

import parity_cases as PC
import resident2d_cases as RC

pytestmark = pytest.mark.gpu


def test_trajectory_golden(golden_mtip2d):
    RC.check_trajectory_golden(golden_mtip2d)


@pytest.mark.parametrize('name', PC.MTIP2D_VARIANTS)
def test_variants_golden(golden_mtip2d, golden_mtip2d_variants, name):
    RC.check_variant_golden(golden_mtip2d, golden_mtip2d_variants, name)


@pytest.mark.parametrize('name', sorted(PC.SETTINGS_VARIANTS_2D))
def test_settings_vs_oracle(golden_mtip2d, name):
    RC.check_settings_vs_oracle(golden_mtip2d, None, name)


def test_unbuildable(golden_mtip2d):
    RC.check_unbuildable(golden_mtip2d)


def test_single_steps_golden(golden_mtip2d):
    RC.check_single_steps_golden(golden_mtip2d)


@pytest.mark.parametrize('name', sorted(RC.SCHEDULES))
def test_shadowed_schedule(golden_mtip2d, name):
    RC.check_shadowed_schedule_2d(golden_mtip2d, name)


@pytest.mark.parametrize('name', sorted(RC.SCHEDULES))
def test_shadowed_schedule_128xM64(golden_mtip2d, name):
    RC.check_shadowed_schedule_2d(golden_mtip2d, name, None, 128, 64, tol=RC.TOL_STEP_128)


def test_ft_stab_per_restart(golden_mtip2d):
    RC.check_ft_stab_per_restart(golden_mtip2d)


def test_ft_stab_disagreement(golden_mtip2d):
    RC.check_ft_stab_disagreement(golden_mtip2d)


@pytest.mark.parametrize('N,M', [(None, None), (128, 64)])
def test_split_invariance(golden_mtip2d, N, M):
    RC.check_split_invariance(golden_mtip2d, None, N, M)


@pytest.mark.parametrize('N,M', [(None, None), (32, 16)])
def test_worker_vs_oracle(golden_mtip2d, N, M):
    RC.check_worker_vs_oracle(golden_mtip2d, None, N, M)


def test_worker_default_unchanged(golden_mtip2d):
    RC.check_worker_default_unchanged(golden_mtip2d)


def test_wide_rows(golden_mtip2d):
    """8 shells x M = 64 and 16 shells x M = 64: rows of 129 values, the left-over column on the wave-per-output path"""
    RC.check_ft_stab_per_restart(golden_mtip2d, None, 8, 64)
    RC.check_wide_rows(golden_mtip2d, None, 16, 64)


# ---- the step kernels past one restart group and one row round, against the longdouble restatement (tests/resident2d_reference.py)
@pytest.mark.parametrize('N,M,B', sorted(RC.REFERENCE_SHAPES))
def test_step_vs_restatement(golden_mtip2d, N, M, B):
    RC.check_step_vs_restatement(golden_mtip2d, None, N, M, B)


def test_main_error_kinds(golden_mtip2d):
    RC.check_main_error_kinds(golden_mtip2d)


@pytest.mark.parametrize('name', sorted(RC.SCHEDULES))
def test_shadowed_schedule_nine_restarts(golden_mtip2d, name):
    RC.check_schedule_nine_restarts(golden_mtip2d, name)


def test_select_where_both_groups(golden_mtip2d):
    RC.check_select_where_both_groups(golden_mtip2d)


def test_lds_limit(golden_mtip2d):
    RC.check_lds_limit(golden_mtip2d)

"""CPU pre-flight of the resident 2-D engine (mtip2d_run and friends, the fused step kernels of csrc/k_polar2d.hip; MTIP2D(...,
resident=True)): the unchanged kernel sources on the CPU emulator, through the same cases as tests/test_gpu_resident2d.py at the
fixtures' size (12 shells x M = 6), plus what only the emulator can see (the launch log)."""
import os
import subprocess

import pytest

import resident2d_cases as RC
import parity_cases as PC

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


def test_trajectory_golden(emul_lib, golden_mtip2d):
    RC.check_trajectory_golden(golden_mtip2d, emul_lib)


@pytest.mark.parametrize('name', PC.MTIP2D_VARIANTS)
def test_variants_golden(emul_lib, golden_mtip2d, golden_mtip2d_variants, name):
    RC.check_variant_golden(golden_mtip2d, golden_mtip2d_variants, name, emul_lib)


@pytest.mark.parametrize('name', sorted(PC.SETTINGS_VARIANTS_2D))
def test_settings_vs_oracle(emul_lib, golden_mtip2d, name):
    RC.check_settings_vs_oracle(golden_mtip2d, emul_lib, name)


def test_unbuildable(emul_lib, golden_mtip2d):
    RC.check_unbuildable(golden_mtip2d, emul_lib)


def test_single_steps_golden(emul_lib, golden_mtip2d):
    RC.check_single_steps_golden(golden_mtip2d, emul_lib)


@pytest.mark.parametrize('name', sorted(RC.SCHEDULES))
def test_shadowed_schedule(emul_lib, golden_mtip2d, name):
    RC.check_shadowed_schedule_2d(golden_mtip2d, name, emul_lib)


def test_ft_stab_per_restart(emul_lib, golden_mtip2d):
    RC.check_ft_stab_per_restart(golden_mtip2d, emul_lib)


def test_wide_rows(emul_lib, golden_mtip2d):
    """8 shells x M = 64: rows of 129 values, the size at which the row transforms hand their left-over column to waves"""
    RC.check_ft_stab_per_restart(golden_mtip2d, emul_lib, 8, 64)
    RC.check_wide_rows(golden_mtip2d, emul_lib, 16, 64)


def test_ft_stab_disagreement(emul_lib, golden_mtip2d):
    RC.check_ft_stab_disagreement(golden_mtip2d, emul_lib)


def test_split_invariance(emul_lib, golden_mtip2d):
    RC.check_split_invariance(golden_mtip2d, emul_lib)


def test_worker_vs_oracle(emul_lib, golden_mtip2d):
    RC.check_worker_vs_oracle(golden_mtip2d, emul_lib)


def test_worker_default_unchanged(emul_lib, golden_mtip2d):
    RC.check_worker_default_unchanged(golden_mtip2d, emul_lib)


def test_launch_budget(emul_lib, golden_mtip2d):
    RC.check_launch_budget(golden_mtip2d, emul_lib)


# ---- the step kernels past one restart group and one row round (the same cases as tests/test_gpu_resident2d.py)
@pytest.mark.parametrize('N,M,B', sorted(RC.REFERENCE_SHAPES))
def test_step_vs_restatement(emul_lib, golden_mtip2d, N, M, B):
    RC.check_step_vs_restatement(golden_mtip2d, emul_lib, N, M, B)


def test_main_error_kinds(emul_lib, golden_mtip2d):
    RC.check_main_error_kinds(golden_mtip2d, emul_lib)


@pytest.mark.parametrize('name', sorted(RC.SCHEDULES))
def test_shadowed_schedule_nine_restarts(emul_lib, golden_mtip2d, name):
    RC.check_schedule_nine_restarts(golden_mtip2d, name, emul_lib)


def test_select_where_both_groups(emul_lib, golden_mtip2d):
    RC.check_select_where_both_groups(golden_mtip2d, emul_lib)


def test_lds_limit(emul_lib, golden_mtip2d):
    RC.check_lds_limit(golden_mtip2d, emul_lib)

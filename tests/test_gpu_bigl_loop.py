"""The phasing loop and the projection at band limits 64 <= L <= 128 on the MI355X (opt-in GPU.big_l_loop / MTIP_CFG_LOOP_BIG_L): the cases of
tests/bigl_loop_cases.py -- short schedules against the numpy oracle at the shapes that reach a block of shells across two restarts,
an odd L, the limit and the 512-point FFT; the projection with up to 201 and 129 rows; the real-arithmetic route inside a big-L
context; the tutorial's shape; the generic kernels (MTIP_SHT_TIER=0) as the second implementation; the group run; a non-FXS pair; the
limits."""
import os
import subprocess
import sys

import pytest

import bigl_loop_cases as BL

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(autouse=True)
def default_tiers(monkeypatch):
    monkeypatch.delenv('MTIP_SHT_TIER', raising=False)


@pytest.fixture(scope='module')
def loop_results():
    """case 1 with the default tiers, fused: checked once, its densities shared with the comparison against tier 0"""
    os.environ.pop('MTIP_SHT_TIER', None)
    return BL.check_loop_vs_oracle(BL.SHAPE_LOOP, BL.SCHEDULE, None, fused=True)


def test_loop_vs_oracle_L64_fused(loop_results):
    assert len(loop_results) == 2


def test_loop_vs_oracle_L64_reference_order():
    BL.check_loop_vs_oracle(BL.SHAPE_LOOP, BL.SCHEDULE, None, fused=False)


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'reference_order'])
def test_loop_vs_oracle_odd_L65(fused):
    BL.check_loop_vs_oracle(BL.SHAPE_ODD, BL.SCHEDULE, None, fused=fused)


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'reference_order'])
def test_loop_vs_oracle_L128(fused):
    BL.check_loop_vs_oracle(BL.SHAPE_LIMIT, BL.SCHEDULE_SHORT, None, fused=fused)


@pytest.mark.parametrize('shape', BL.PROJ_SHAPES, ids=str)
def test_projection_vs_oracle(shape):
    BL.check_projection(shape)


def test_projection_real_route():
    BL.check_projection_real()


def test_tutorial_shape():
    BL.check_tutorial_shape()


def test_tier0_second_implementation(loop_results, tmp_path):
    out = str(tmp_path / 'tier0.npz')
    code = 'import sys; sys.path[:0] = [%r, %r]; import bigl_loop_cases as BL; BL.run_tier0(%r)' % (HERE, os.path.dirname(HERE), out)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, MTIP_SHT_TIER='0'), capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and 'BIGL loop tier0 ok' in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    BL.check_tier0_agrees(loop_results, out)


def test_group_run_identical():
    BL.check_group_run_identical()


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'reference_order'])
def test_non_fxs_pair_vs_oracle(fused):
    BL.check_loop_vs_oracle(BL.SHAPE_LOOP, BL.SCHEDULE_SHORT, None, fused=fused, variant='non_fxs')


def test_flag_lifts_the_limit():
    BL.check_flag_lifts_the_limit()


def test_more_than_128_columns_refused():
    BL.check_columns_refused()


def test_per_restart_ft_stab_mask_refused():
    BL.check_ft_mask_refused()


def test_reserved_is_a_flag_word():
    BL.check_reserved_bits()


def test_default_unchanged():
    BL.check_default_unchanged()

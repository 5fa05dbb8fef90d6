"""CPU pre-flight of the phasing loop beyond L = 63 (opt-in GPU.big_l_loop / MTIP_CFG_LOOP_BIG_L): the unchanged kernel sources on the CPU
emulator through the cases of tests/bigl_loop_cases.py at shapes the fibers walk in under a minute, and what only the emulator can
see -- the launch log of a step (the modulus stage is k_sht_big_fft_inv, no separate modulus kernel), that the flag moves nothing below
L = 64, no access past a buffer's end, and that what is refused launches nothing."""
import os
import subprocess
import sys

import pytest

import bigl_loop_cases as BL

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


@pytest.fixture(autouse=True)
def default_tiers(monkeypatch):
    monkeypatch.delenv('MTIP_SHT_TIER', raising=False)


def _child(call, *args, **env):
    code = 'import sys; sys.path[:0] = [%r, %r]; import bigl_loop_cases as BL; BL.%s(*%r)' % (HERE, os.path.dirname(HERE), call, args)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, **env), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'reference_order'])
def test_loop_vs_oracle_L64(emul_lib, fused):
    BL.check_loop_vs_oracle(BL.EMUL_LOOP, BL.SCHEDULE_SHORT, emul_lib, fused=fused)


def test_step_vs_oracle_L128(emul_lib):
    BL.check_loop_vs_oracle(BL.EMUL_LIMIT, (1, False, 0), emul_lib, fused=True)


def test_no_access_past_buffer_ends(emul_lib):
    assert 'BIGL loop guarded ok' in _child('run_guarded', emul_lib, MTIP_EMUL_GUARD='1')


def test_step_kernels(emul_lib):
    BL.check_step_kernels(emul_lib)


def test_flag_moves_nothing_below_L64(emul_lib):
    BL.check_below_unchanged(emul_lib)


def test_flag_lifts_the_limit(emul_lib):
    BL.check_flag_lifts_the_limit(emul_lib)


def test_more_than_128_columns_refused(emul_lib):
    BL.check_columns_refused(emul_lib)


def test_per_restart_ft_stab_mask_refused(emul_lib):
    BL.check_ft_mask_refused(emul_lib)


def test_reserved_is_a_flag_word(emul_lib):
    BL.check_reserved_bits(emul_lib)


def test_default_unchanged(emul_lib):
    BL.check_default_unchanged(emul_lib)

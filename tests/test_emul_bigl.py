"""CPU pre-flight of the band limits 64 <= L <= 128 (csrc/k_sht_big.h, plan_sht, the loop's band limit): the unchanged kernel source on the
CPU emulator through the cases of tests/bigl_cases.py, and what only the emulator can see -- which kernels a plan launches (the new
ones beyond L = 63, the generic ones with MTIP_SHT_TIER=0, an odd n_theta or more than 128 theta pairs, none of the new ones below the limit), no access past a
buffer's end, and that the refused loop entry points launch nothing."""
import os
import subprocess
import sys

import pytest

import bigl_cases as BC

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


def _child(call, lib, **env):
    code = 'import sys; sys.path[:0] = [%r, %r]; import bigl_cases as BC; BC.%s(%r)' % (HERE, os.path.dirname(HERE), call, lib)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, **env), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


@pytest.mark.parametrize('shape', BC.EMUL_SHAPES, ids=str)
def test_operators_vs_oracle(emul_lib, monkeypatch, shape):
    monkeypatch.delenv('MTIP_SHT_TIER', raising=False)
    BC.check_operators(shape, emul_lib, BC.KERNELS_BIG)


def test_no_access_past_buffer_ends(emul_lib):
    assert 'BIGL guarded ok' in _child('run_guarded', emul_lib, MTIP_EMUL_GUARD='1')


def test_fallback_tier0(emul_lib):
    assert 'BIGL fallback ok' in _child('run_fallback', emul_lib, MTIP_SHT_TIER='0')


@pytest.mark.parametrize('shape', [BC.ODD_SHAPE, BC.TALL_SHAPE], ids=['odd_n_theta', 'n_theta_260'])
def test_unfit_n_theta_takes_generic_kernels(emul_lib, monkeypatch, shape):
    monkeypatch.delenv('MTIP_SHT_TIER', raising=False)
    BC.check_operators(shape, emul_lib, BC.KERNELS_GENERIC)


@pytest.mark.parametrize('shape', BC.BELOW, ids=str)
def test_nothing_moved_below_the_limit(emul_lib, monkeypatch, shape):
    monkeypatch.delenv('MTIP_SHT_TIER', raising=False)
    BC.check_operators(shape, emul_lib, BC.KERNELS_BELOW[shape])


def test_flow(emul_lib, monkeypatch):
    monkeypatch.delenv('MTIP_SHT_TIER', raising=False)
    BC.check_flow(BC.FLOW64, emul_lib)


def test_raises(emul_lib):
    BC.check_raises(emul_lib)

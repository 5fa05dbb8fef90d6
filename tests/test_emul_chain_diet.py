"""CPU emulator twin of tests/test_gpu_chain_diet.py: the cases of tests/chain_diet_cases.py on the kernel sources compiled for
the host, against the bits the parent commit's emulator build gave (tests/golden/chain_bits.npz, keys emul_*).  Also, here alone:
the L = 32 shape with every device buffer followed by an inaccessible page (the loads from d_PTw, the dump-entry stores of forward
phase 2), and the fallback for L = 32 on a grid the L = 32 instantiation is not compiled for."""
import os
import subprocess
import sys

import pytest

import chain_diet_cases as DC

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')


@pytest.fixture(scope='module')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.mark.parametrize('name', sorted(DC.CASES))
def test_transform_bits_as_the_parent(emul_lib, name):
    DC.check(DC.transform_results(name, emul_lib), 'emul')


def test_fused_step_bits_as_the_parent(emul_lib):
    DC.check(DC.steps_results(emul_lib), 'emul')


def test_no_access_past_buffer_ends(emul_lib):
    """in a child process (a stray access ends it)"""
    code = 'import sys; sys.path[:0] = [%r, %r]; import chain_diet_cases as DC; DC.run_guarded(%r)' % (HERE, os.path.dirname(HERE), emul_lib)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, MTIP_EMUL_GUARD='1'), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert 'CHAIN_DIET_GUARDED_OK' in r.stdout, r.stdout


def test_l32_on_another_grid_falls_back(emul_lib):
    DC.check_fallback(emul_lib)

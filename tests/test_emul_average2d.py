"""CPU pre-flight of the 2-D averaging (csrc/k_average2d.h, xframe_amd.fxs.average.average_reconstructions_2d): the unchanged kernel
sources on the CPU emulator through the cases of tests/average2d_cases.py, against the restatement of the reference's run_2d in
tests/average2d_reference.py; plus what only the emulator can see: the guard pages behind every device allocation and the launch log."""
import os
import subprocess
import sys

import pytest

import average2d_cases as AC

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


@pytest.mark.parametrize('n', AC.STACKS)
def test_transform_chunks(emul_lib, n):
    AC.check_transform_chunks(emul_lib, 12, 6, n)


@pytest.mark.parametrize('n', AC.STACKS)
@pytest.mark.parametrize('N,M', AC.SHAPES_CPU)
def test_grid_stats(emul_lib, N, M, n):
    AC.check_grid_stats(emul_lib, N, M, n)


@pytest.mark.parametrize('n', AC.STACKS)
@pytest.mark.parametrize('N,M', AC.SHAPES_CPU)
def test_phase_ramp(emul_lib, N, M, n):
    AC.check_phase_ramp(emul_lib, N, M, n)


@pytest.mark.parametrize('n', AC.STACKS)
@pytest.mark.parametrize('N,M', AC.SHAPES_CPU)
def test_inversion_metric(emul_lib, N, M, n):
    AC.check_inversion_metric(emul_lib, N, M, n)


@pytest.mark.parametrize('n', AC.STACKS)
@pytest.mark.parametrize('N,M', AC.SHAPES_CPU)
def test_combine(emul_lib, N, M, n):
    AC.check_combine(emul_lib, N, M, n)


@pytest.mark.parametrize('N,M', AC.SHAPES_CPU)
def test_curves(emul_lib, N, M):
    AC.check_curves(emul_lib, N, M)


@pytest.mark.parametrize('N,M', AC.SHAPES_CPU)
def test_fqcb(emul_lib, N, M):
    AC.check_fqcb(emul_lib, N, M)


@pytest.mark.parametrize('n,ref_pos', AC.FLOW_STACKS)
def test_flow(emul_lib, n, ref_pos):
    AC.check_flow(emul_lib, n, ref_pos, 'max')


@pytest.mark.parametrize('name', [k for k in AC.FLOW_OPTIONS if k != 'max'])
def test_flow_options(emul_lib, name):
    AC.check_flow(emul_lib, 5, 2, name)


def test_split_invariance(emul_lib):
    AC.check_split_invariance(emul_lib)


def test_raises(emul_lib):
    AC.check_raises(emul_lib)


def test_bit_limit():
    AC.check_bit_limit()


def test_no_access_past_buffer_ends(emul_lib):
    """in a child process (a stray access ends it): every new kernel, every device allocation of the emulator followed by an
    inaccessible page"""
    code = 'import sys; sys.path[:0] = [%r, %r]; import average2d_cases as AC; AC.run_guarded(%r)' % (HERE, os.path.dirname(HERE), emul_lib)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, MTIP_EMUL_GUARD='1'), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert 'AVG2D_GUARDED_DONE' in r.stdout


def test_launch_count(emul_lib):
    AC.check_launch_count(emul_lib)


def test_extract_2d(emul_lib):
    AC.check_extract_2d(emul_lib)


def test_extract_2d_masked_raises(emul_lib):
    AC.check_extract_2d_masked_raises(emul_lib)


def test_chain(emul_lib, golden_mtip2d):
    AC.check_chain(emul_lib, golden_mtip2d)


def test_fsc_3d(emul_lib):
    AC.check_fsc_3d(emul_lib)

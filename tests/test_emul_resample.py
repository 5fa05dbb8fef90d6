"""CPU pre-flight of the route detector frames -> polar patterns (mtip_resample_*, mtip_correlate_add_detector, csrc/k_resample.h;
fxs/correlate.py Resampler / Correlator.add_detector): the unchanged kernel source on the CPU emulator through the cases of
tests/test_gpu_resample.py, and what only the emulator can see (the launch log of the static mask, guarded buffer ends)."""
import os
import subprocess
import sys

import pytest

import resample_cases as RC

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


@pytest.fixture(scope='module')
def golden():
    return RC.load_golden()


def test_device_golden(emul_lib, golden):
    RC.check_device_golden(golden, emul_lib)


@pytest.mark.parametrize('order', RC.ORDERS)
@pytest.mark.parametrize('shape', RC.SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_shape_order(emul_lib, shape, order):
    RC.check_shape_order(emul_lib, shape, order)


@pytest.mark.parametrize('name', RC.SWITCH_NAMES)
def test_switches(emul_lib, name):
    for order in (2, 5):
        RC.check_switch(emul_lib, name, order)


def test_chunking(emul_lib):
    RC.check_chunking(emul_lib)


def test_batch_independence(emul_lib):
    RC.check_batch_independence(emul_lib)


def test_static_mask(emul_lib):
    RC.check_static_mask(emul_lib)


def test_host_and_device_input(emul_lib):
    RC.check_host_device(emul_lib)


def test_add_detector(emul_lib):
    RC.check_add_detector(emul_lib)


def test_raises(emul_lib):
    RC.check_raises(emul_lib)


def test_no_access_past_buffer_ends(emul_lib):
    """in a child process (a stray access ends it): the edge points -- corners, a hair inside and outside every edge, 4 x 5 frames
    whose taps go through the mirror more than once -- at every order, every device allocation of the emulator followed by an
    inaccessible page"""
    code = RC.GUARD_SCRIPT.format(tests=HERE, root=os.path.dirname(HERE), lib=emul_lib)
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, MTIP_EMUL_GUARD='1'), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert 'guarded run complete' in r.stdout

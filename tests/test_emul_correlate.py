"""CPU pre-flight of the route patterns -> C(q1, q2, Delta) (mtip_correlate_*, csrc/k_correlate.h; fxs/correlate.py): the unchanged
kernel source on the CPU emulator through the cases of tests/test_gpu_correlate.py at toy sizes, the numpy restatement and the host
tables against the reference's own outputs (G25), and what only the emulator can see (the launch log of the shared-mask set-up)."""
import os
import subprocess

import pytest

import correlate_cases as CO

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
    return CO.load_golden()


def test_restatement_golden(golden):
    CO.check_restatement_golden(golden)


def test_device_golden(emul_lib, golden):
    CO.check_device_golden(golden, emul_lib)


@pytest.mark.parametrize('name', list(CO.CASES) + ['grid_stride'])
def test_case(emul_lib, name):
    CO.check_case(emul_lib, name)


def test_sparse_masks(emul_lib):
    CO.check_sparse(emul_lib)


def test_shared_mask(emul_lib):
    CO.check_shared_mask(emul_lib)


def test_batch_independence(emul_lib):
    CO.check_batch_independence(emul_lib)


def test_partial_merge(emul_lib):
    CO.check_merge(emul_lib)


def test_finalize(emul_lib):
    CO.check_finalize(emul_lib)


def test_device_tensor(emul_lib):
    CO.check_device_tensor(emul_lib)


def test_end_to_end(emul_lib):
    CO.check_end_to_end(emul_lib)


def test_raises(emul_lib):
    CO.check_raises(emul_lib)

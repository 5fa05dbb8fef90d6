"""Every handle of the library gives back all of its device memory: tests/ownership_cases.py on the CPU emulator, whose runtime counts
the live device allocations.  In a child process, so that no engine of another test is collected between two readings."""
import os
import subprocess
import sys

import pytest

import ownership_cases as OC

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


def test_handles_release_their_device_memory(emul_lib):
    code = 'import sys; sys.path[:0] = [%r, %r]; import ownership_cases as OC; OC.run_all(%r)' % (HERE, os.path.dirname(HERE), emul_lib)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count('OWNERSHIP') == len(OC.CASES), r.stdout

"""CPU pre-flight of the reciprocal-metric kernels (csrc/k_metrics.hip): the unchanged kernel sources on the CPU emulator through
the cases of tests/metrics_cases.py, against the oracle's routines and a longdouble contraction of the device tables.  The shapes
are the smallest that leave the first tile of each size-dependent path (see SHAPES); 128 x L32 with 5 restarts, the size the timing
file quotes, runs on the MI355X only (tests/test_gpu_metrics.py): it reaches no path that these do not."""
import os
import subprocess

import pytest

import metrics_cases as MC

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, 'emul')
EMUL_LIB = os.path.join(EMUL_DIR, 'libmtip_emul.so')

SHAPES = [(10, 5, 2),      # the shape of fixture G19 on seeded data
          (24, 10, 3),     # two q' tiles of k_metric_fqc, the second half full
          (40, 32, 5),     # 3 q' tiles with a half-empty last one, 33 columns (lane 0's second column only), restart chunk 4 + 1
          (37, 40, 6),     # N % 8 = 5 (dead half-waves in the last pass), 41 columns, chunk 4 + 2, fold rows past 64
          (9, 63, 1),      # 64 columns (both columns of every lane), the 128 x 256 angular grid, one restart
          (130, 3, 2)]     # N^2 = 16 900 > 64 * 256: second grid-stride trip of II / ccd with a ragged end, 9 q' tiles


@pytest.fixture(scope='session')
def emul_lib():
    r = subprocess.run(['make', '-C', EMUL_DIR, '-j6'], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return EMUL_LIB


@pytest.mark.parametrize('N,L,B', SHAPES)
def test_metrics(emul_lib, N, L, B):
    MC.check_metrics(emul_lib, N, L, B)


def test_flag_subsets(emul_lib):
    MC.check_flag_subsets(emul_lib)


def test_rearm(emul_lib):
    MC.check_rearm(emul_lib)

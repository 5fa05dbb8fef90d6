"""The reciprocal-metric kernels on the MI355X (csrc/k_metrics.hip) through the cases of tests/metrics_cases.py: the shapes of
tests/test_emul_metrics.py, each the smallest that leaves the first tile of one size-dependent path, and 128 x L32 with 5 restarts,
the size profiles/r03_optional_metrics_cost.txt quotes times for (N^2 = 64 * 256 exactly, 33 columns, restart chunk 4 + 1) --
against the oracle's routines (a) and a longdouble contraction of the device tables (b).

Measured worst figures (MI355X; DESIGN section 1, G19, has the table): device against (b), and in brackets oracle (a) against (b)
  (N, L, B)       II_error, absolute      ccd_diff, relative      fqc_error, absolute per entry
  (10, 5, 2)      8.6e-17 (1.7e-16)       4.2e-17 (1.7e-16)       9.5e-17 (2.7e-16)
  (24, 10, 3)     2.9e-16 (2.9e-16)       2.7e-17 (2.7e-17)       1.7e-16 (1.7e-16)
  (40, 32, 5)     2.7e-16 (2.7e-16)       2.8e-16 (1.4e-16)       1.8e-16 (2.3e-16)
  (37, 40, 6)     1.5e-16 (2.1e-16)       2.2e-16 (2.9e-16)       1.8e-16 (2.1e-16)
  (9, 63, 1)      1.5e-16 (3.7e-16)       6.9e-16 (3.5e-16)       1.2e-16 (8.2e-17)
  (130, 3, 2)     2.3e-16 (2.3e-16)       3.6e-17 (1.2e-16)       3.4e-16 (1.9e-16)
  (128, 32, 5)    3.1e-16 (2.2e-16)       5.3e-16 (2.1e-16)       4.6e-16 (2.4e-16)
Against the oracle (a) the device is within 4.4e-16 (II, fqc) and 4.0e-16 relative (ccd) at every shape.  Every figure is more than a
factor 1000 inside its bound (1e-12; ccd against the oracle 1e-9): the device is as close to the longdouble values as the oracle is.
The 128 x L32 case spends its time on the host (the 143 MB table, five oracle evaluations, the longdouble contraction)."""
import pytest

import metrics_cases as MC

pytestmark = pytest.mark.gpu

SHAPES = [(10, 5, 2), (24, 10, 3), (40, 32, 5), (37, 40, 6), (9, 63, 1), (130, 3, 2), (128, 32, 5)]


@pytest.mark.parametrize('N,L,B', SHAPES)
def test_metrics(N, L, B):
    MC.check_metrics(None, N, L, B)


def test_flag_subsets():
    MC.check_flag_subsets(None)


def test_rearm():
    MC.check_rearm(None)

"""The alignment and averaging operators on the MI355X (csrc/k_align.hip, csrc/k_average.hip) at the sizes the README quotes
numbers for -- 128 x L32 with 8 restarts (Euler grid 66^3, grids of 1 048 576 points: the block count of k_av_* on its cap),
64 x L48, 3 x L63 on the 128 x 256 angular grid, and the 256 x L48 grid of config 5 (8.4 M points: several grid-stride trips per
thread) -- through the cases of tests/align_cases.py, against the longdouble references of tests/so3_reference.py.

Measured worst figures, as a fraction of the bound each is held to (MI355X; DESIGN section 5 has the table):
  correlation (max|C - ref| / max|C|)   1.4e-15 (128 x L32, B = 8)  1.5e-15 (shells [5, 100), B = 3)  1.6e-15 (64 x L48)  1.8e-15 (3 x L63)
      smallest reference gap between the two largest values: 1.7e-4 of max|C| (128 x L32 decaying; the condition asks > 1e-9)
  rotation, D from the host / built on the device        1.3e-14 / 1.5e-14 (128 x L32 flat)  2.8e-14 / 1.3e-14 (64 x L48 flat)  2.1e-14 / 2.0e-14 (3 x L63 flat)
      the rotated output evaluated at 20 points against f(R^-1 x): 1.4e-14 of max|f| (128 x L32)
  grid_stats sums (|got - ref| / sum|terms|)             1.5e-15 (128 x 64 x 128, n = 8)  2.1e-15 (256 x 128 x 256, n = 2 and n = 1); extrema, count exact
  phase ramp                                             3.8e-14 (128 x L32 grid, phases up to 127 rad)  5.3e-14 (256 x L48 grid, phases up to 255 rad)
  combine                                                1.7e-16 at every size
  PRTF mean (|got - ref| / mean|terms|), deviation       1.5e-16, 4e-16 relative (256 x L48 grid)
Every figure is at least a factor 18 inside its bound (1e-12; deviation 1e-10); the largest, the phase ramp's, is the rounding of a
phase of a few hundred radians (255 x 2^-53 = 2.8e-14 per rounding)."""
import pytest

import align_cases as AC

pytestmark = pytest.mark.gpu

SO3_SIZES = [(6, 1, 2, None, 'decay', 0, 0), (5, 4, 3, (1, 4), 'flat', 0, 0), (8, 10, 2, (7, 8), 'decay', 0, 0),
             (128, 32, 8, None, 'decay', 0, 0), (128, 32, 8, None, 'flat', 0, 0), (128, 32, 3, (5, 100), 'decay', 0, 0),
             (64, 48, 2, None, 'decay', 0, 0), (64, 48, 2, None, 'flat', 0, 0), (3, 63, 1, None, 'decay', 128, 256),
             (3, 63, 1, None, 'flat', 128, 256)]
GRIDS = [(6, 4, 1), (24, 10, 3), (128, 32, 8), (128, 32, 1), (256, 48, 2), (256, 48, 1)]


@pytest.mark.parametrize('N,L,B,shells,spectrum,n_theta,n_phi', SO3_SIZES)
def test_correlation(N, L, B, shells, spectrum, n_theta, n_phi):
    AC.check_correlation(None, N, L, B, shells, spectrum, n_theta, n_phi)


@pytest.mark.parametrize('N,L,B,shells,spectrum,n_theta,n_phi', SO3_SIZES)
def test_rotation(N, L, B, shells, spectrum, n_theta, n_phi):
    AC.check_rotation(None, N, L, B, spectrum, n_theta, n_phi, evaluate=(L == 32))


@pytest.mark.parametrize('N,L,n', GRIDS)
def test_grid_stats(N, L, n):
    AC.check_grid_stats(None, N, L, n)


def test_grid_stats_nan():
    AC.check_grid_stats_nan(None)


@pytest.mark.parametrize('N,L,n', GRIDS)
def test_phase_ramp(N, L, n):
    AC.check_phase_ramp(None, N, L, n)


@pytest.mark.parametrize('N,L,n', [(6, 4, 1), (6, 4, 2), (24, 10, 8), (128, 32, 8), (128, 32, 1), (256, 48, 2)])
def test_combine(N, L, n):
    AC.check_combine(None, N, L, n)


@pytest.mark.parametrize('N,L', [(6, 4), (24, 10), (128, 32), (256, 48)])
def test_prtf(N, L):
    AC.check_prtf(None, N, L)

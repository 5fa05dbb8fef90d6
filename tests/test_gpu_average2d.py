"""The 2-D averaging on the MI355X (csrc/k_average2d.h, xframe_amd.fxs.average.average_reconstructions_2d): the cases of
tests/average2d_cases.py on the HIP build, against the restatement of the reference's run_2d in tests/average2d_reference.py."""
import pytest

import average2d_cases as AC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('n', AC.STACKS)
def test_transform_chunks(n):
    AC.check_transform_chunks(None, 12, 6, n)


@pytest.mark.parametrize('n', AC.STACKS)
@pytest.mark.parametrize('N,M', AC.SHAPES_GPU)
def test_grid_stats(N, M, n):
    AC.check_grid_stats(None, N, M, n)


@pytest.mark.parametrize('n', AC.STACKS)
@pytest.mark.parametrize('N,M', AC.SHAPES_GPU)
def test_phase_ramp(N, M, n):
    AC.check_phase_ramp(None, N, M, n)


@pytest.mark.parametrize('n', AC.STACKS)
@pytest.mark.parametrize('N,M', AC.SHAPES_GPU)
def test_inversion_metric(N, M, n):
    AC.check_inversion_metric(None, N, M, n)


@pytest.mark.parametrize('n', AC.STACKS)
@pytest.mark.parametrize('N,M', AC.SHAPES_GPU)
def test_combine(N, M, n):
    AC.check_combine(None, N, M, n)


@pytest.mark.parametrize('N,M', AC.SHAPES_GPU)
def test_curves(N, M):
    AC.check_curves(None, N, M)


@pytest.mark.parametrize('N,M', AC.SHAPES_GPU)
def test_fqcb(N, M):
    AC.check_fqcb(None, N, M)


@pytest.mark.parametrize('n,ref_pos', AC.FLOW_STACKS)
def test_flow(n, ref_pos):
    AC.check_flow(None, n, ref_pos, 'max')


@pytest.mark.parametrize('name', [k for k in AC.FLOW_OPTIONS if k != 'max'])
def test_flow_options(name):
    AC.check_flow(None, 5, 2, name)


def test_split_invariance():
    AC.check_split_invariance(None)


def test_raises():
    AC.check_raises(None)


def test_extract_2d():
    AC.check_extract_2d(None)


def test_extract_2d_masked_raises():
    AC.check_extract_2d_masked_raises(None)


def test_chain(golden_mtip2d):
    AC.check_chain(None, golden_mtip2d)


def test_fsc_3d():
    AC.check_fsc_3d(None)

"""The restatement of the reference's 2-D averaging and 2-D extract rules (tests/average2d_reference.py) against outputs of the
reference's own functions (tests/golden/average2d.npz, written by tests/golden/make_golden_average2d.py): equal, or within a few ulp
where the result passes through a sum whose order is numpy's own or through an eigensolver."""
import os

import numpy as np
import pytest

import average2d_reference as AR
import average2d_cases as AC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'average2d.npz')
ULP = np.finfo(float).eps


@pytest.fixture(scope='module')
def g():
    return np.load(GOLDEN)


def test_prtf(g):
    for (m, s), args in (((g['prtf_mean'], g['prtf_std']), (g['a1'], g['a2'], np.sqrt(g['I1']), np.sqrt(g['I2']))),
                         ((g['prtf_single_mean'], g['prtf_single_std']), (g['a1'], g['a1'], np.sqrt(g['I1']), np.sqrt(g['I1'])))):
        mean, std = AR.prtf_numpy(*args)
        assert np.array_equal(mean, m) and np.array_equal(std, s)


def test_fsc_and_limit(g):
    assert np.array_equal(AR.fsc(g['a1'], g['a2']), g['fsc'])
    assert g['fsc'][3] == 1.0
    assert AR.fsc_bit_limit(0.5, np.zeros(tuple(g['grid_shape']))) == float(g['fsc_limit'])
    from xframe_amd.fxs.average import fsc_bit_limit
    assert fsc_bit_limit(0.5, tuple(g['grid_shape'])) == float(g['fsc_limit'])


def test_deg2_invariants(g):
    from oracle import polar2d as OP
    assert np.array_equal(OP.harmonic_forward(g['Id'].astype(complex)), g['cht_Id'])
    assert np.array_equal(AR.deg2_from_table(g['pr_mat'].T), g['b_target'])
    assert np.array_equal(AR.deg2_from_table(g['cht_Id'][:, :int(g['M']) + 1]), g['b_d'])
    assert g['b_d'].shape == (int(g['M']) + 1, int(g['N']), int(g['N']))


def test_fqcb(g):
    b_d, b_ftd, b_t = g['b_d'], g['b_ftd'], g['b_target']
    for name, args, kw in (('d', (b_d, b_t), {}), ('ftd', (b_ftd, b_t), {}), ('rec', (b_ftd, b_d), {}),
                           ('d_z', (b_d, b_t), {'include_zero_order': True}), ('ftd_z', (b_ftd, b_t), {'include_zero_order': True})):
        mean, std = AR.fqcb_2d(*args, skip_odd_orders=True, **kw)
        assert np.array_equal(mean, g['fqcb_' + name]) and np.array_equal(std, g['fqcb_' + name + '_std']), name
    mean, std = AR.fqcb_2d(b_d, b_t)
    assert np.array_equal(mean, g['fqcb_all_orders']) and np.array_equal(std, g['fqcb_all_orders_std'])
    assert g['fqcb_ftd'][int(g['N']) // 2] == 1.0                    # a vanishing row of |F|^2: denominator 0


def test_projection_vectors(g):
    """The restatement calls the reference's own eigensolver (scipy's eigh, driver 'ev'), but what LAPACK returns is fixed only up
    to its backward error -- the kernels of the BLAS underneath are chosen per CPU -- and an eigenvector only up to its phase.  So
    lambda v v^+ is compared, within that backward error: both decompositions are exact for a matrix within n eps |B| of B
    (LAPACK's bound for the symmetric QR iteration, with a modest factor taken as 1 per side), the eigenvalue moves by as much and
    the eigenvector by that over the gap to the second eigenvalue: |d(lambda v v^+)| <= 2 n eps |B| (1 + 2 |B| / gap) over both sides."""
    for i in range(3):
        v, ev = AR.projection_vector_2d(g['pv_B'][i], g['pv_lim'][i])
        ref = g[f'pv_{i}']
        assert v.shape == ref.shape
        if not ref.any():                                            # the zeroing branch: nothing to perturb
            assert not v.any() and ev == 0
            continue
        s_ = slice(*g['pv_lim'][i][0])
        blk = g['pv_B'][i][s_, s_]
        w = np.sort(np.linalg.eigvalsh((blk + blk.conj().T) / 2))[::-1]
        norm, gap, n = np.max(np.abs(w)), w[0] - w[1], len(w)
        bound = 2 * n * ULP * norm * (1 + 2 * norm / gap)
        diff = np.linalg.norm(v[:, None] * v[None, :].conj() - ref[:, None] * ref[None, :].conj(), 2)
        print(f'order {i}: |d(lambda v v^+)| = {diff:.2e}, bound {bound:.2e}; d lambda = {abs(ev - float(g[f"pv_eig_{i}"])):.2e}')
        assert diff <= bound, (i, diff, bound)
        assert abs(ev - float(g[f'pv_eig_{i}'])) <= 2 * n * ULP * norm
    assert not g['pv_2'].any() and float(g['pv_eig_2']) == 0 and not g['pv_1'][:3].any()


def test_center_shift_integrator(g):
    """on the reference's own grid angles (ft_grid_pairs builds them with linspace, one ulp from arange(n) / n * 2 pi at some points)
    the restatement of the centre, the shift operator and the integrator is the reference's arithmetic: equal"""
    fl = AR.Flow2D(g['rs'], g['qs'], 2 * int(g['M']) + 1, None, None, None, phis=g['phis'])
    assert np.array_equal(g['phis'], g['phis_reciprocal'])
    assert np.array_equal(fl.rs, AC.OP.radial_grids_2d(float(g['max_q']), int(g['N']), 2.0, 'midpoint')[0])
    assert np.array_equal(fl.find_center(g['dens']), g['center'])
    assert np.array_equal(fl.negative_shift(g['F'].copy(), g['center']), g['F_negative_shift'])
    assert AR.polar_integrate(g['dens'].real, fl.rs, fl.phis) == float(g['integral_real'])
    assert fl.integrate_reciprocal(np.abs(g['F'].imag)) == float(g['integral_reciprocal'])


def test_phase_reference_longdouble(g):
    """the longdouble yardstick of the phase-ramp kernel against the reference's double-precision shift operator.  One side is double:
    its phase k . c = q cos(phi) c_x + q sin(phi) c_y carries at most 4 roundings per term and one for the sum -- below
    5 eps (|q_x c_x| + |q_y c_y|) <= 5 sqrt(2) eps q |c| -- which reaches the factor exp(-i k . c) in full; cos, sin and the complex
    product add less than 4 eps.  Bound per element: (4 + 8 q_max |c|) eps |F|."""
    c = g['center']
    cart = [c[0] * np.cos(c[1]), c[0] * np.sin(c[1])]
    ld = AR.phase_ref(g['F'], cart, 1.0, g['qs'])
    phase = float(np.max(g['qs']) * c[0])
    err = np.max(np.abs(ld - g['F_shift'].astype(AR.CLD)) / np.abs(g['F']))
    print(f'phase_ref against the reference: {float(err) / ULP:.1f} ulp, bound {4 + 8 * phase:.0f} ulp (largest phase {phase:.1f})')
    assert err <= (4 + 8 * phase) * ULP

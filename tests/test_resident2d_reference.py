"""tests/resident2d_reference.py (the longdouble restatement of one resident 2-D step, the yardstick of resident2d_cases.py's
`check_step_vs_restatement`) against what already pins oracle/mtip2d.py: the oracle's own step from seeded states, and the
reference's own single steps of fixture G20.  Bound: 1e-12 (rel-L2 of F', rho'; relative for the scalars) -- the oracle works in
complex128 with numpy's FFT, its distance from a longdouble direct sum at 12 shells x 13 values is 1e-15 .. 1e-14.  No device."""
import numpy as np
import pytest

import parity_cases as PC
import resident2d_reference as RR
from helpers import rel_l2
from oracle import mtip as OM
from oracle import mtip2d as O2

TOL = 1e-12


@pytest.fixture(scope='module')
def oracle_g20(golden_mtip2d):
    data, o = PC.mtip2d_problem(golden_mtip2d)
    mo = O2.MTIP2D(OM.deep_update(o, RR.METRICS_ON), data)
    return mo, RR.tables_from_oracle(mo)


@pytest.mark.parametrize('method,ft_stab', [('HIO', True), ('HIO', False), ('ER', True), ('ER', False), ('HIO_non_FXS', True), ('ER_non_FXS', False)])
def test_restatement_vs_oracle_step(golden_mtip2d, oracle_g20, method, ft_stab):
    """seeded guesses with holes in the support, both reciprocal metrics on: every output of the step, and the inputs are not
    degenerate (errors > 0, every order's phase well conditioned)"""
    mo, t = oracle_g20
    rhos, sups = RR.seeded_inputs(golden_mtip2d['rho0'], 3, 41)
    fxs = not method.endswith('_non_FXS')
    for rho, sup in zip(rhos, sups):
        fixed = None if fxs else np.abs(mo.fp.ft(1.1 * rho))
        ref = RR.step(t, method, ft_stab, 0.45, rho, sup, fixed)
        got = RR.oracle_step(mo, method, ft_stab, 0.45, rho, sup, fixed)
        assert ref['err'] > 0 and rel_l2(np.asarray(ref['rho_new'], complex), rho) > 1e-3
        if fxs:
            assert ref['conditioning'].min() >= 1e-6 and ref['rl2'] > 0 and (ref['deg2'][t['deg2_norm'] != 0] > 0).all()
        d = RR.step_distance(got, ref, fxs)
        d['F_l2'], d['rho_l2'] = rel_l2(got['F_new'], ref['F_new']), rel_l2(got['rho_new'], ref['rho_new'])
        print(method, ft_stab, ' '.join(f'{k} {v:.2e}' for k, v in d.items()))
        assert max(d.values()) <= TOL, d


def test_restatement_vs_golden_steps(golden_mtip2d, oracle_g20):
    """the reference's own single steps (G20): HIO / ER, with and without ft_stab, initial support enforced and not"""
    g = golden_mtip2d
    mo, t = oracle_g20
    for enf in (1, 0):
        sup = g['step_support'] & mo.real_pr.initial_support if enf else g['step_support']
        for meth in ('HIO', 'ER', 'HIO_ft_stab', 'ER_ft_stab'):
            ref = RR.step(t, meth.replace('_ft_stab', ''), meth.endswith('ft_stab'), 0.45, g['step_rho_in'], sup)
            tag = f'step_{meth}_enf{enf}'
            d = (rel_l2(g[tag + '_F'], ref['F_new']), rel_l2(g[tag + '_rho'], ref['rho_new']), abs(float(g[tag + '_err']) / float(ref['err']) - 1))
            print(tag, 'F %.2e rho %.2e err %.2e' % d)
            assert max(d) <= TOL, (tag, d)


def test_main_error_kinds():
    """numpy's mean / min / max / prod, NaN included (a NaN anywhere gives NaN for every kind)"""
    LD = RR.LD
    deg2 = np.array([0.5, 0.25, 2.0], dtype=LD)
    assert RR.main_error('mean', ['real', 'l2_projection_diff'], LD(1), LD(3), None) == 2
    assert RR.main_error('min', ['deg2_invariant_l2_diff'], None, None, deg2) == 0.25
    assert RR.main_error('max', ['deg2_invariant_l2_diff'], None, None, deg2) == 2
    assert RR.main_error('prod', ['real', 'l2_projection_diff'], LD(2), LD(3), None) == 6
    for kind in RR.KINDS:
        assert np.isnan(RR.main_error(kind, ['real', 'l2_projection_diff'], LD(1), LD(np.nan), None))
        assert np.isnan(RR.main_error(kind, ['real', 'l2_projection_diff'], LD(np.nan), LD(1), None))

"""Cases of the 3-D loop's main error over any scalar metrics the loop records (mtip_set_main_error_ex; k_finish_step's item list:
generate_main_error_routine, fxs_IO_methods.py:746-765), shared by tests/test_emul_main_error.py (CPU emulator) and
tests/test_gpu_main_error.py (MI355X).

Yardstick: the numpy oracle's own loop (oracle.mtip.MTIP), whose main_error() is general.  It does not record II_error / ccd_diff
itself, so `oracle_run` appends oracle.metrics.*_routine of the coefficients that enter the projection to its error lists in every
FXS step (what parity_cases.check_invariant_metrics_vs_oracle evaluates after the fact): the oracle's loop then steers by the
combined main error -- best pair, enforce_initial_support, end-of-loop reselection.

Tolerances are the project's for these series: rtol 1e-6, atol 1e-12 on every metric and on main (parity_cases.py:1544-1549), densities
1e-8 rel-L2 and equal supports (that module's loop checks).

Problems: the 16 x L4 fixture with three restarts from different seeded guesses (k_finish_step is one block per restart: a wrong
(step, restart) index into a history row shows only when the restarts differ), and synthetic 12 x L6 invariants on the 20 x 32
angular grid with two restarts (the ragged trip of k_metric_rl2_shell).  Schedule: 3 HIO + SW + 2 ER with
best_density_not_in_first_n_iterations = 0, so the last density is the best one and the output depends on the selection."""
import functools
import os

import numpy as np
import pytest

import parity_cases as PC
from helpers import OracleTransforms, data_from_golden, golden_settings, rel_l2
from oracle import metrics as M
from oracle import mtip as OM
from oracle.fourier import FourierPair
from oracle.sht import SHT
from xframe_amd.fxs import _lib, hostsetup as hs, reconstruct as R, schedule, synthetic as S
from xframe_amd.fxs.engine import Engine, EngineGroup

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
WAVELENGTH = 1.23984
C_ORDER = 2
RTOL, ATOL, TOL_DENSITY = 1e-6, 1e-12, 1e-8
TYPES = ('mean', 'min', 'max', 'prod')
# main.metrics as (real, reciprocal); the reference reduces real + reciprocal in that order (fxs_IO_methods.py:753-757)
ITEM_SETS = {'real+II': (['l2_projection_diff'], ['II_error']),
             'real+ccd+rl2': (['l2_projection_diff'], ['ccd_diff', 'l2_projection_diff']),
             'II': ([], ['II_error']),
             'ranked+real': (['l2_projection_diff'], ['deg2_ranked_invariant_l2_diff'])}
ITEM_CODES = {'real+II': [0, 3], 'real+ccd+rl2': [0, 4, 2], 'II': [3], 'ranked+real': [0, 5]}
CALCULATE = ['II_error', 'ccd_diff', 'l2_projection_diff', 'deg2_invariant_l2_diff', 'deg2_ranked_invariant_l2_diff']
# (the degenerate problem's ccd reference has norm zero, which the metric's setup refuses, upstream too: fxs_IO_methods.py:669-670)
CALCULATE_DEGENERATE = ['II_error', 'l2_projection_diff', 'deg2_invariant_l2_diff']
SEEDS = {'golden': (3, 14, 29), 'synthetic': (3, 4)}
# the same problems inside a smaller initial support (250 in the settings: 512 / 1920 grid points; 125: 256 / 640; 75: 128 of the
# 16 x L4 grid): more of the density lies outside it, the real metric starts near 1 and crosses the reciprocal ones
# Inside 128 or 640 points the intensity coefficients that enter the projection are far from the data's and the polar factor of the
# reciprocal projection is badly conditioned: F' of these problems is compared at the project's bound for trajectories of problems
# other than the fixture (parity_cases.TOL_TRAJ = 1e-6; every real-space density, series, support and best error at the bounds above)
SUPPORT_RADIUS = {'golden@125': 125.0, 'golden@75': 75.0, 'synthetic@125': 125.0}
SEEDS.update({k: SEEDS[k.split('@')[0]] for k in SUPPORT_RADIUS})
# What min / max select in the oracle's runs, per (problem, item set, type), over all steps and restarts: VARIES, or the position in
# the list of the one item that is selected throughout.  The issue asks for a varying selection everywhere; these inputs cannot
# give it in the rows with a number -- over 60 seeded guesses of either problem deg2_ranked_invariant_l2_diff (0.17 .. 3.2) and, for
# the synthetic problem, II_error (0.07 .. 0.98) stay above the real metric (0.01 .. 0.45) in every step, and on the fixture the
# reciprocal l2_projection_diff does too.  Where the constant selection is the real metric (min, position 0) the main error EQUALS
# the real metric and the case alone does not tell whether the kernel reads its items.  Every such row therefore has a companion in
# EXTRA_CASES: the same problem, item set and type inside a smaller initial support, where the selection varies or is the other item.
VARIES = 'varies'
PICKS = {('golden', 'real+II', 'min'): VARIES, ('golden', 'real+II', 'max'): VARIES,
         ('golden', 'real+ccd+rl2', 'min'): 0, ('golden', 'real+ccd+rl2', 'max'): VARIES,
         ('golden', 'ranked+real', 'min'): 0, ('golden', 'ranked+real', 'max'): 1,
         ('synthetic', 'real+II', 'min'): 0, ('synthetic', 'real+II', 'max'): 1,
         ('synthetic', 'real+ccd+rl2', 'min'): VARIES, ('synthetic', 'real+ccd+rl2', 'max'): VARIES,
         ('synthetic', 'ranked+real', 'min'): 0, ('synthetic', 'ranked+real', 'max'): 1,
         ('golden@125', 'real+ccd+rl2', 'min'): VARIES, ('golden@125', 'real+ccd+rl2', 'max'): VARIES,
         ('golden@75', 'ranked+real', 'min'): VARIES, ('golden@75', 'ranked+real', 'max'): VARIES,
         ('synthetic@125', 'ranked+real', 'min'): VARIES, ('synthetic@125', 'ranked+real', 'max'): VARIES,
         ('synthetic@125', 'real+II', 'min'): 1, ('synthetic@125', 'real+II', 'max'): 0}
EXTRA_CASES = [k for k in PICKS if '@' in k[0]]
COMPANION = {('golden', 'real+ccd+rl2'): 'golden@125', ('golden', 'ranked+real'): 'golden@75', ('synthetic', 'ranked+real'): 'synthetic@125',
             ('synthetic', 'real+II'): 'synthetic@125'}
SCHEDULES = {}
SCHEDULES['main'] = (['HIO', 'SW', 'ER'], {'HIO': {'iterations': 3, 'ft_stab': True}, 'SW': 1, 'ER': {'iterations': 2, 'ft_stab': True}})
# *_non_FXS blocks record no reciprocal metric: after an FXS block the main error reads the last recorded values, in front of the
# first one a list is still empty and the reference's main error is -1 (its IndexError branch, fxs_IO_methods.py:762-764)
SCHEDULES['stale'] = (['HIO', 'HIO_non_FXS', 'ER_non_FXS', 'ER'],
                      {'HIO': {'iterations': 2, 'ft_stab': True}, 'HIO_non_FXS': {'iterations': 2, 'ft_stab': True},
                       'ER_non_FXS': {'iterations': 1, 'ft_stab': False}, 'ER': {'iterations': 1, 'ft_stab': True}})
SCHEDULES['empty'] = (['HIO_non_FXS', 'ER'], {'HIO_non_FXS': {'iterations': 2, 'ft_stab': False}, 'ER': {'iterations': 2, 'ft_stab': True}})
# at the settings' threshold 0.09 the new support of two of the three guesses lies inside the initial one and enforcing it changes
# nothing; at 0.02 more than 200 of its points lie outside for every guess
SW_THRESHOLD_FEEDBACK = 0.02


# ------------------------------------------------------------------------------------------------------------------- problems
@functools.lru_cache(maxsize=None)
def problem_data(name):
    """(invariants, N, L, grid overrides) -- shared by the tests of a session and never modified"""
    if name in SUPPORT_RADIUS:                              # the same problem inside a smaller initial support (settings())
        return problem_data(name.split('@')[0])
    if name == 'golden':
        g = np.load(os.path.join(GOLDEN, 'mtip_N16_L4.npz'))
        N, L = int(g['N']), int(g['L'])
        return data_from_golden(g, L), N, L, {}
    if name == 'degenerate':
        # V_l = 0 for l >= 1: the II reference sum_{l>=1} B_l vanishes and II_error is 0 / 0 (fxs_IO_methods.py:613-620)
        data, N, L, grid = problem_data('golden')
        data = dict(data)
        pms = np.empty(L + 1, dtype=object)
        for l in range(L + 1):
            pms[l] = np.array(data['data_projection_matrices'][l]) * (1.0 if l == 0 else 0.0)
        data['data_projection_matrices'] = pms
        return data, N, L, grid
    assert name == 'synthetic'
    N, L = 12, 6
    data, _ = S.make_invariants(OracleTransforms(FourierPair(SHT(L), N, S.data_cutoff(N), 2.0)), N, L)
    data['xray_wavelength'] = WAVELENGTH
    return data, N, L, {'n_theta': 20, 'n_phi': 32}


def settings(name, main_type='mean', item_set=None, sched='main', limit=None, n_used=None):
    """item_set None: the default main error (the real metric alone); limit: enforce_initial_support.if_error_bigger_than, together
    with the shrink-wrap threshold SW_THRESHOLD_FEEDBACK"""
    _, N, L, grid = problem_data(name)
    real_m, rec_m = (['l2_projection_diff'], []) if item_set is None else ITEM_SETS[item_set]
    opt = golden_settings(N, L, {'grid': grid, 'main_loop': {'error': {'methods': {
        'reciprocal': {'calculate': calculate_of(name, n_used), 'ccd_diff': {'C_order': C_ORDER}},
        'main': {'metrics': {'real': list(real_m), 'reciprocal': list(rec_m)}, 'type': main_type}}}}})
    if n_used is not None:
        opt['projections']['reciprocal']['used_order_ids'] = np.arange(n_used)
    if name in SUPPORT_RADIUS:
        opt['projections']['real']['projections']['support']['initial_support']['max_radius'] = SUPPORT_RADIUS[name]
    main = opt['main_loop']['sub_loops']['main']
    main['order'], main['methods'] = list(SCHEDULES[sched][0]), OM.deep_update(SCHEDULES[sched][1], {})
    main['iterations'] = 1
    main['best_density_not_in_first_n_iterations'] = 0
    opt['main_loop']['sub_loops']['order'] = ['main']
    if limit is not None:
        opt['projections']['real']['projections']['support']['enforce_initial_support'] = {'apply': True, 'if_error_bigger_than': float(limit)}
        opt['projections']['real']['shrink_wrap']['thresholds'] = [SW_THRESHOLD_FEEDBACK, SW_THRESHOLD_FEEDBACK]
    return opt


def calculate_of(name, n_used=None):
    """the reciprocal metrics the problem records: all five, less those that cannot be set up for it"""
    if name == 'degenerate':
        return list(CALCULATE_DEGENERATE)
    return [m for m in CALCULATE if n_used is None or m != 'II_error']        # (II_error raises upstream on a subset of the orders)


def n_steps_of(opt):
    main = opt['main_loop']['sub_loops']['main']
    return sum(main['methods'][k]['iterations'] for k in main['order'] if not k.startswith('SW'))


def fxs_steps_of(opt):
    """bool per step: an FXS step (one that records the reciprocal metrics)"""
    main = opt['main_loop']['sub_loops']['main']
    return np.array([('_non_FXS' not in k) for k in main['order'] if not k.startswith('SW') for _ in range(main['methods'][k]['iterations'])])


# --------------------------------------------------------------------------------------------------------------- the yardstick
def _oracle(opt, data):
    """oracle.mtip.MTIP that also records II_error / ccd_diff in every FXS step, so that its main_error() finds them"""
    calc = list(opt['main_loop']['error']['methods']['reciprocal']['calculate'])
    extra = [n for n in calc if n in ('II_error', 'ccd_diff')]
    oopt = OM.deep_update(opt, {})
    oopt['main_loop']['error']['methods']['reciprocal']['calculate'] = [n for n in calc if n not in extra]
    om = OM.MTIP(oopt, data)
    rm = om.rp.radial_mask
    inv = rm[:, :, None] * rm[:, None, :]
    ref = np.array([p @ p.conj().T for p in om.rp.projection_matrices])
    routines = {}
    if 'II_error' in extra:
        routines['II_error'] = M.II_error_routine(om.rp.radial_points, ref, om.rp.used_orders, inv)
    if 'ccd_diff' in extra:
        routines['ccd_diff'] = M.ccd_diff_routine(om.rp.radial_points, ref, om.rp.used_orders, float(om.rp.number_of_particles[0]), inv,
                                                  C_ORDER, WAVELENGTH)
    own_errors, own_state = om._reciprocal_errors, om.create_initial_state

    def reciprocal_errors(F, F_new, Ilm):
        own_errors(F, F_new, Ilm)
        for n in extra:
            om.errors['reciprocal'][n].append(float(np.real(routines[n]([np.array(a) for a in Ilm]))))

    def create_initial_state(rho0):
        state = own_state(rho0)
        for n in extra:
            om.errors['reciprocal'][n] = []
        return state
    om._reciprocal_errors, om.create_initial_state = reciprocal_errors, create_initial_state
    return om


@functools.lru_cache(maxsize=None)
def guess(name, seed):
    data = problem_data(name)[0]
    return _oracle(settings(name), data).density_guess(np.random.default_rng(seed))


@functools.lru_cache(maxsize=None)
def oracle_run(name, main_type='mean', item_set=None, seed=3, sched='main', limit=None, n_used=None):
    """the oracle's loop steered by that main error: (result dict, enforce decisions, density after every step); computed once per
    session, shared, never modified"""
    data = problem_data(name)[0]
    om = _oracle(settings(name, main_type, item_set, sched, limit, n_used), data)
    after, enforced, own = [], [], om.run_sub_loop

    def run_sub_loop(*args):
        state, iteration = own(*args)
        enforced[:] = [np.asarray(e).reshape(-1) for e in state['enforce_initial_support_list']]
        return state, iteration
    om.run_sub_loop = run_sub_loop
    res = om.phasing_loop(rho0=guess(name, seed), step_hook=lambda key, step, pair, main: after.append(np.array(pair[1])))
    return res, enforced, after


def _items_of(ref, item_set, n):
    """(n_steps, n_items) the listed metrics' recorded values of an oracle run in list order (FXS-only schedules)"""
    ed = ref['error_dict']
    real_m, rec_m = ITEM_SETS[item_set]
    return np.stack([np.asarray(ed['real'][m], float) for m in real_m] + [np.asarray(ed['reciprocal'][m], float) for m in rec_m], axis=1)[:n]


def check_inputs_discriminate(name, main_type, item_set, seeds):
    """conditions on the inputs, from the oracle's runs alone, asserted before anything is compared.  mean / prod, and a single item:
    the combined main error differs from the real metric in every step (a kernel that ignores the items fails).  min / max over
    several items: the selection is what PICKS records -- it varies over the steps and restarts, or it is the one recorded item; the
    main error differs from the real metric in every step that selects another item than the real metric, and there is such a
    step unless PICKS records the real metric itself, in which case a companion case with another selection must exist."""
    real_pos = ITEM_CODES[item_set].index(0) if 0 in ITEM_CODES[item_set] else -1
    picks, differing = [], []
    for seed in seeds:
        ref = oracle_run(name, main_type, item_set, seed)[0]
        main, real = np.asarray(ref['error_dict']['main']), np.asarray(ref['error_dict']['real']['l2_projection_diff'])
        assert main.shape == real.shape and np.isfinite(main).all()
        items = _items_of(ref, item_set, len(main))
        fn = {'mean': np.mean, 'min': np.min, 'max': np.max, 'prod': np.prod}[main_type]
        assert np.allclose(main, fn(items, axis=1), rtol=1e-15, atol=0)
        differs = np.abs(main - real) > 10 * RTOL * np.abs(real)            # (far outside the comparison's tolerance)
        if main_type in ('min', 'max') and items.shape[1] > 1:
            pick = (np.argmin if main_type == 'min' else np.argmax)(items, axis=1)
            picks += list(pick)
            differing += list(differs[pick != real_pos])
        else:
            assert differs.all(), (main, real)
    if picks:
        expect = PICKS[(name, item_set, main_type)]
        if expect == VARIES:
            assert len(set(picks)) > 1, (name, item_set, main_type, picks)
        else:
            assert set(picks) == {expect}, (name, item_set, main_type, picks)
        if expect == real_pos:                                              # main == real throughout: the companion case discriminates
            other = PICKS[(COMPANION[(name, item_set)] if '@' not in name else name.split('@')[0], item_set, main_type)]
            assert not differing and other != real_pos, (name, item_set, main_type)
        else:
            assert len(differing) > 0 and all(differing), (name, item_set, main_type, differing)
    return picks


# ------------------------------------------------------------------------------------------------- case 1: the trajectories
def _compare_restart(tag, r, ref, fxs=None, calculate=CALCULATE, tol_reciprocal=None):
    ed, od = r['error_dict'], ref['error_dict']
    n = len(od['main'])
    fxs = np.ones(n, bool) if fxs is None else fxs
    print(f"{tag}: main {np.asarray(ed['main'])} oracle {np.asarray(od['main'])}")
    assert len(ed['main']) == n
    assert np.allclose(ed['main'], od['main'], rtol=RTOL, atol=ATOL, equal_nan=True), (tag, ed['main'], od['main'])
    assert np.allclose(ed['real']['l2_projection_diff'], od['real']['l2_projection_diff'], rtol=RTOL, atol=ATOL), tag
    for m in calculate:
        got, want = np.asarray(ed['reciprocal'][m], float)[fxs], np.asarray(od['reciprocal'][m], float)
        print(f'{tag}: {m} max deviation {np.nanmax(np.abs(got - want)) if got.shape == want.shape else None}')
        assert got.shape == want.shape, (tag, m, got.shape, want.shape)
        assert np.allclose(got, want, rtol=RTOL, atol=ATOL, equal_nan=True), (tag, m, got, want)
    dens = {k: rel_l2(r[k], ref[k]) for k in ('real_density', 'last_real_density', 'reciprocal_density', 'last_reciprocal_density')}
    print(f'{tag}: densities {dens}')
    for k, d in dens.items():
        assert d < (tol_reciprocal if tol_reciprocal is not None and k.endswith('reciprocal_density') else TOL_DENSITY), (tag, k, d)
    assert (r['support_mask'] != ref['support_mask']).sum() == 0 and (r['last_support_mask'] != ref['last_support_mask']).sum() == 0, tag
    assert np.isclose(r['final_error'], ref['final_error'], rtol=RTOL, atol=ATOL, equal_nan=True), (tag, r['final_error'], ref['final_error'])


def run_product(name, main_type, item_set, seeds, lib_path=None, fused=True, sched='main', limit=None, n_used=None, keep=None):
    """the product's loop (reconstruct.MTIP) from the oracle's guesses; `keep` receives the engine's launch log of the loop"""
    data = problem_data(name)[0]
    opt = settings(name, main_type, item_set, sched, limit, n_used)
    R.MTIP.preinit(opt, data)
    m = R.MTIP(n_restarts=len(seeds), initial_densities=[guess(name, s) for s in seeds], lib_path=lib_path, fused=fused)
    m.generate_phasing_loop()
    try:
        PC.launched_kernels(m.engine, ('k_',))
        res = m.phasing_loop()
        if keep is not None:
            keep['launched'] = PC.launched_kernels(m.engine, ('k_',))
            keep['items'] = list(m.engine.main_items)
    finally:
        m.engine.close()
    return res


def check_trajectory(name, main_type, item_set, lib_path=None, fused=True):
    seeds = SEEDS[name]
    check_inputs_discriminate(name, main_type, item_set, seeds)
    keep = {}
    res = run_product(name, main_type, item_set, seeds, lib_path, fused, keep=keep)
    assert keep['items'] == ITEM_CODES[item_set], keep['items']
    for b, seed in enumerate(seeds):
        _compare_restart(f'{name} {main_type} {item_set} fused={fused} restart {b}', res[b], oracle_run(name, main_type, item_set, seed)[0],
                         tol_reciprocal=PC.TOL_TRAJ if name in SUPPORT_RADIUS else None)
    assert rel_l2(res[0]['last_real_density'], res[1]['last_real_density']) > 1e-3          # the restarts are different runs


class _GroupState:
    """schedule.walk's protocol over the engines of an EngineGroup (direct form): the restarts of all engines side by side"""

    def __init__(self, group):
        self.g, self.es = group, group.engines

    def check_method(self, key):
        pass

    def begin_sub_loop(self):
        for e in self.es:
            e.begin_sub_loop()

    def shrinkwrap(self, sigma, threshold, limit):
        return np.concatenate([e.shrinkwrap(sigma, threshold, limit) for e in self.es])

    def before_sw_center(self, limit):
        return None

    def refresh_reciprocal_density(self):
        for e in self.es:
            e.refresh_reciprocal_density()

    def run(self, key, ft_stab, betas):
        self.g.run(key, ft_stab, betas)

    def main_errors(self, first, n):
        return np.concatenate([e.fetch_main_errors(first, n) for e in self.es], axis=1)

    def select_best(self, where):
        i = 0
        for e in self.es:
            e.select_best(where[i:i + e.B])
            i += e.B


def check_group_trajectory(name='golden', main_type='max', item_set='real+ccd+rl2', lib_path=None, sizes=(2, 1)):
    """the same loop through mtip_run_group_async: two engines (2 + 1 restarts), every restart against its own oracle run"""
    seeds = SEEDS[name]
    assert sum(sizes) == len(seeds)
    check_inputs_discriminate(name, main_type, item_set, seeds)
    data = problem_data(name)[0]
    opt = settings(name, main_type, item_set)
    engines = [Engine(opt, data, n_batch=b, lib_path=lib_path) for b in sizes]
    try:
        i = 0
        for e in engines:
            for b in range(e.B):
                e.set_density(b, guess(name, seeds[i]))
                i += 1
            e.init_state()
        grp = EngineGroup(engines)
        _, n = schedule.walk(opt, _GroupState(grp), schedule.ShrinkWrapRamps(opt, engines[0].default_sigma), len(seeds))
        assert grp.calls['group'] == 2 and n == n_steps_of(opt)
        i = 0
        for e in engines:
            main, inv, rl2 = e.fetch_main_errors(0, n), e.fetch_invariant_metrics(0, n), e.fetch_reciprocal_l2(0, n)
            best = e.best_error()[0]
            for b in range(e.B):
                ref = oracle_run(name, main_type, item_set, seeds[i])[0]
                od = ref['error_dict']
                tag = f'group engine of {e.B}, restart {b}'
                print(f"{tag}: main {main[:, b]} oracle {np.asarray(od['main'])}")
                assert np.allclose(main[:, b], od['main'], rtol=RTOL, atol=ATOL), tag
                assert np.allclose(inv['ccd_diff'][:, b], od['reciprocal']['ccd_diff'], rtol=RTOL, atol=ATOL), tag
                assert np.allclose(inv['II_error'][:, b], od['reciprocal']['II_error'], rtol=RTOL, atol=ATOL), tag
                assert np.allclose(rl2[:, b], od['reciprocal']['l2_projection_diff'], rtol=RTOL, atol=ATOL), tag
                assert np.isclose(best[b], ref['final_error'], rtol=RTOL, atol=ATOL), tag
                for key, got in (('last_real_density', e.density(b)), ('real_density', e.density(b, best=True)),
                                 ('last_reciprocal_density', e.reciprocal_density(b))):
                    assert rel_l2(got, ref[key]) < TOL_DENSITY, (tag, key, rel_l2(got, ref[key]))
                assert (e.support(b) != ref['last_support_mask']).sum() == 0 and (e.support(b, best=True) != ref['support_mask']).sum() == 0
                i += 1
    finally:
        for e in engines:
            e.close()


# -------------------------------------------------------------------------------------------- case 2: the main error feeds back
def check_feedback(name='golden', main_type='mean', item_set='real+II', lib_path=None, fused=True):
    """enforce_initial_support.if_error_bigger_than between the real-only and the combined main error at the SW step: the oracle's
    two runs (default main, combined main) differ in the enforce decision and in the density after SW; the product matches the
    combined one, enforce decisions included"""
    seeds = SEEDS[name]
    n_before_sw = SCHEDULES['main'][1]['HIO']['iterations']
    # the limit from the oracle's runs with the limit out of reach (the steps in front of SW do not depend on it)
    lo, hi = [], []
    for seed in seeds:
        ed = oracle_run(name, main_type, item_set, seed, limit=1e30)[0]['error_dict']
        a, b = float(ed['real']['l2_projection_diff'][n_before_sw - 1]), float(ed['main'][n_before_sw - 1])
        lo.append(min(a, b))
        hi.append(max(a, b))
    assert max(lo) < min(hi), (lo, hi)                        # one limit separates the two for every restart
    limit = float(np.sqrt(max(lo) * min(hi)))
    for seed in seeds:
        (rd, ed_, ad), (rc, ec_, ac) = oracle_run(name, 'mean', None, seed, limit=limit), oracle_run(name, main_type, item_set, seed, limit=limit)
        assert len(ed_) == 1 and len(ec_) == 1 and bool(ed_[0][0]) != bool(ec_[0][0]), (ed_, ec_)
        assert rel_l2(ad[n_before_sw - 1], ac[n_before_sw - 1]) < 1e-12 and rel_l2(ad[n_before_sw], ac[n_before_sw]) > 1e-6
    data = problem_data(name)[0]
    opt = settings(name, main_type, item_set, limit=limit)
    R.MTIP.preinit(opt, data)
    m = R.MTIP(n_restarts=len(seeds), initial_densities=[guess(name, s) for s in seeds], lib_path=lib_path, fused=fused)
    m.generate_phasing_loop()
    enforced = []
    own = m.engine.shrinkwrap
    m.engine.shrinkwrap = lambda *a: enforced.append(own(*a)) or enforced[-1]
    try:
        res = m.phasing_loop()
    finally:
        m.engine.close()
    assert len(enforced) == 1
    for b, seed in enumerate(seeds):
        ref, eis, _ = oracle_run(name, main_type, item_set, seed, limit=limit)
        assert bool(enforced[0][b]) == bool(eis[0][0]), (b, enforced, eis)
        _compare_restart(f'feedback restart {b}', res[b], ref)


# ----------------------------------------------------------------------------------------------------- case 3: NaN is data
def check_nan_main(lib_path=None, fused=True, name='degenerate', item_set='real+II'):
    """II_error = 0 / 0 in every step: the main error is NaN for all four types on both sides and the best pair never changes (it
    stays the initial one: `best_error > nan` is False, reconstruct.py:934)"""
    seeds = SEEDS['golden'][:2]
    for main_type in TYPES:
        refs = [oracle_run(name, main_type, item_set, s)[0] for s in seeds]
        for ref in refs:                                        # first, on the CPU: the oracle gives NaN there
            assert np.isnan(np.asarray(ref['error_dict']['reciprocal']['II_error'])).all() and np.isnan(ref['error_dict']['main']).all()
            assert np.isfinite(np.asarray(ref['error_dict']['real']['l2_projection_diff'])).all()
            assert ref['final_error'] == np.inf and rel_l2(ref['real_density'], ref['initial_density']) < 1e-12
        res = run_product(name, main_type, item_set, seeds, lib_path, fused)
        for b, ref in enumerate(refs):
            r = res[b]
            assert np.isnan(r['error_dict']['main']).all() and len(r['error_dict']['main']) == len(ref['error_dict']['main']), (main_type, r['error_dict']['main'])
            assert np.isnan(r['error_dict']['reciprocal']['II_error']).all()
            assert np.allclose(r['error_dict']['real']['l2_projection_diff'], ref['error_dict']['real']['l2_projection_diff'], rtol=RTOL, atol=ATOL)
            assert r['final_error'] == np.inf
            for k in ('real_density', 'last_real_density', 'reciprocal_density', 'last_reciprocal_density'):
                assert rel_l2(r[k], ref[k]) < TOL_DENSITY, (main_type, b, k, rel_l2(r[k], ref[k]))
            assert rel_l2(r['real_density'], r['initial_density']) < 1e-12
            assert (r['support_mask'] != ref['support_mask']).sum() == 0 and (r['last_support_mask'] != ref['last_support_mask']).sum() == 0


# ------------------------------------------------------------------------------------------- case 4: stale and empty lists
def check_stale_and_empty(lib_path=None, fused=True, name='golden', main_type='mean', item_set='real+ccd+rl2'):
    """a *_non_FXS block after an FXS block (the reciprocal items keep the values of the last FXS step) and a schedule that starts
    with one (a list is still empty: the oracle's main error is -1 there, which becomes the best error): whatever the oracle gives"""
    seeds = SEEDS[name][:2]
    for sched in ('stale', 'empty'):
        opt = settings(name, main_type, item_set, sched)
        fxs = fxs_steps_of(opt)
        refs = [oracle_run(name, main_type, item_set, s, sched)[0] for s in seeds]
        for ref in refs:
            main, real = np.asarray(ref['error_dict']['main']), np.asarray(ref['error_dict']['real']['l2_projection_diff'])
            assert len(main) == len(fxs) and (main != real).all()
            if not fxs[0]:
                assert (main[~fxs] == -1).all() and ref['final_error'] == -1
            else:
                k = int(np.argmin(fxs))                           # first non-FXS step: the reciprocal items of step k - 1
                want = np.mean([real[k]] + [ref['error_dict']['reciprocal'][m][k - 1] for m in ITEM_SETS[item_set][1]])
                assert np.isclose(main[k], want, rtol=1e-14), (main[k], want)
        res = run_product(name, main_type, item_set, seeds, lib_path, fused, sched)
        for b, ref in enumerate(refs):
            _compare_restart(f'{sched} schedule, restart {b}', res[b], ref, fxs)


# --------------------------------------------------------------------------------------------- case 5: the C entry's refusals
def _armed_engine(lib_path, calculate, n_batch=2, name='golden'):
    data = problem_data(name)[0]
    opt = settings(name)
    opt['main_loop']['error']['methods']['reciprocal']['calculate'] = list(calculate)
    e = Engine(opt, data, n_batch=n_batch, lib_path=lib_path)
    for b in range(n_batch):
        e.set_density(b, guess(name, SEEDS[name][b]))
    e.init_state()
    return e


def _set_ex(e, main_type, items, column=0):
    it = np.ascontiguousarray(items, dtype=np.int32)
    rc = e.lib.mtip_set_main_error_ex(e.ctx, main_type, len(it), _lib.ptr(it), column)
    return rc, e.lib.mtip_last_error(e.ctx).decode()


def check_refusals(lib_path=None):
    EINVAL, ESTATE = -1, -5
    e = _armed_engine(lib_path, ['deg2_invariant_l2_diff'])
    other = _armed_engine(lib_path, CALCULATE, n_batch=1)
    try:
        for items, word in (([6], 'items 0'), ([0, -1], 'items 0'), ([0] * 9, 'at most 8'), ([1, 0], 'anything else'), ([0, 1], 'anything else'),
                            ([1, 1], 'anything else'), ([5], 'deg2_ranked_column')):
            rc, msg = _set_ex(e, 0, items, column=e.L + 1)
            assert rc == EINVAL and word in msg, (items, rc, msg)
        rc, msg = _set_ex(e, 4, [0])
        assert rc == EINVAL and 'type' in msg, (rc, msg)
        # a refused list leaves the one before it in place; an item whose metric is off fails the run before any launch
        beta = np.full(1, 0.5)
        for items, word in (([0, 3], 'II_error'), ([4], 'ccd_diff'), ([0, 2], 'reciprocal l2_projection_diff')):
            rc, msg = _set_ex(e, 0, items)
            assert rc == 0, (items, msg)
            PC.launched_kernels(e, ('k_',))
            rc = e.lib.mtip_run_async(e.ctx, 1, 1, 1, _lib.ptr(beta))
            msg = e.lib.mtip_last_error(e.ctx).decode()
            assert rc == ESTATE and word in msg, (items, rc, msg)
            launched = PC.launched_kernels(e, ('k_',))
            assert launched is None or launched == (), launched
            assert e.best_error()[1] == 0
            # in a group run nothing is launched for any member, whichever of them is the one that cannot run
            for pair in ((other, e), (e, other)):
                arr = (_lib.C.c_void_p * 2)(*[x.ctx for x in pair])
                rc = e.lib.mtip_run_group_async(arr, 2, 1, 1, 1, _lib.ptr(beta))
                assert rc == ESTATE and word in e.lib.mtip_last_error(e.ctx).decode(), rc
                launched = PC.launched_kernels(e, ('k_',))
                assert launched is None or launched == (), launched
                assert e.best_error()[1] == 0 and other.best_error()[1] == 0
        # the fourth metric: deg2_ranked_invariant_l2_diff on an engine whose deg2 metric is off
        bare = _armed_engine(lib_path, [], n_batch=1)
        try:
            rc, msg = _set_ex(bare, 0, [0, 5], column=2)
            assert rc == 0, msg
            PC.launched_kernels(bare, ('k_',))
            rc = bare.lib.mtip_run_async(bare.ctx, 0, 1, 1, _lib.ptr(beta))
            msg = bare.lib.mtip_last_error(bare.ctx).decode()
            assert rc == ESTATE and 'deg2_ranked_invariant_l2_diff' in msg, (rc, msg)
            launched = PC.launched_kernels(bare, ('k_',))
            assert (launched is None or launched == ()) and bare.best_error()[1] == 0, launched
        finally:
            bare.close()
    finally:
        e.close()
        other.close()


def check_metric_switched_on_late(lib_path=None):
    """a metric that is switched on after FXS steps of the same reconstruction has no value yet: a *_non_FXS step that follows gives
    -1 (not the zeros of the new history), and an FXS step records it"""
    e = _armed_engine(lib_path, ['deg2_invariant_l2_diff'], n_batch=2)
    try:
        e.run('ER', True, [0.5], fetch=False)
        wr, wt, _ = hs.error_weights(e.rs, e.n_theta, e.shape, False)
        keep = (_lib.as_f64(wr), _lib.as_f64(wt))
        e._ck(e.lib.mtip_set_reciprocal_l2_metric(e.ctx, _lib.ptr(keep[0]), _lib.ptr(keep[1])))
        e.reciprocal_l2 = True
        rc, msg = _set_ex(e, 1, [0, 2])
        assert rc == 0, msg
        e.run('ER_non_FXS', False, [0.5], fetch=False)
        e.run('ER', True, [0.5], fetch=False)
        e.run('ER_non_FXS', False, [0.5], fetch=False)
        main, real, rl2 = e.fetch_main_errors(0, 4), e.fetch_errors(0, 4)[0], e.fetch_reciprocal_l2(0, 4)
        print('metric switched on late: main', main.T, 'real', real.T, 'reciprocal l2', rl2.T)
        assert (main[1] == -1).all() and (real[1] > 0).all()
        assert np.array_equal(main[2], np.minimum(real[2], rl2[2])) and (rl2[2] > 0).all()
        assert np.array_equal(main[3], np.minimum(real[3], rl2[2]))                     # the value of the last FXS step
    finally:
        e.close()


def check_old_entry_bits(lib_path=None, n_hio=2, n_er=2):
    """mtip_set_main_error(ctx, 0, t) and (ctx, 1, t) followed by the same short run give bit-identical histories to the _ex forms
    [0] and [1]"""
    for use_deg2 in (0, 1):
        for main_type in (0, 2):
            out = []
            for form in ('old', 'ex'):
                e = _armed_engine(lib_path, ['deg2_invariant_l2_diff'])
                if form == 'old':
                    e._ck(e.lib.mtip_set_main_error(e.ctx, use_deg2, main_type))
                else:
                    rc, msg = _set_ex(e, main_type, [use_deg2])
                    assert rc == 0, msg
                e.run('HIO', True, np.full(n_hio, 0.45), fetch=False)
                enforced = e.shrinkwrap(e.default_sigma, 0.09, 6e-3)
                e.run('ER', True, np.full(n_er, 0.5), fetch=False)
                n = n_hio + n_er
                out.append((e.fetch_main_errors(0, n),) + e.fetch_errors(0, n) + (enforced, e.best_error()[0], e.density(0), e.density(1, best=True)))
                e.close()
            for a, b in zip(*out):
                assert np.array_equal(a, b) and np.isfinite(a).all(), (use_deg2, main_type)
            assert (out[0][0] > 0).all()
            if use_deg2:
                assert not np.array_equal(out[0][0], out[0][1])                        # the main error is not the real metric there


# ------------------------------------------------------------------------------------------------ the Python layer's refusals
def check_engine_refusals(lib_path=None, name='golden'):
    data = problem_data(name)[0]

    def engine(real_m, rec_m, calculate=CALCULATE):
        opt = settings(name)
        em = opt['main_loop']['error']['methods']
        em['reciprocal']['calculate'] = list(calculate)
        em['main'] = {'metrics': {'real': real_m, 'reciprocal': rec_m}, 'type': 'mean'}
        Engine(opt, data, lib_path=lib_path).close()
    with pytest.raises(NotImplementedError, match='reference itself raises'):
        engine(['l2_projection_diff'], ['deg2_invariant_l2_diff'])
    with pytest.raises(NotImplementedError, match='reference itself raises'):
        engine([], ['II_error', 'deg2_invariant_l2_diff'])
    with pytest.raises(NotImplementedError, match='fqc_error'):
        engine(['l2_projection_diff'], ['fqc_error'], CALCULATE + ['fqc_error'])
    with pytest.raises(KeyError, match='II_error'):
        engine(['l2_projection_diff'], ['II_error'], ['ccd_diff'])
    with pytest.raises(KeyError, match='deg2_invariant_l2_diff'):
        engine([], ['deg2_invariant_l2_diff'], ['ccd_diff'])
    engine([], ['deg2_invariant_l2_diff'])                                           # (today's two forms still build)
    engine(['l2_projection_diff'], [])


# ------------------------------------------------------------------------------- case 6: ccd_diff on a subset of the orders
def check_ccd_subset_operator(lib_path=None):
    """ccd_diff with used_order_ids = arange(L) of L + 1 at operator level against the reference's own routine (fixture G32,
    tests/golden/make_metrics_subset.py; rtol 1e-9 as G19).  The fixture also records that upstream's II_error and fqc_error raise on
    such a subset: the tables refuse them"""
    import metrics_cases as MTC
    g = np.load(os.path.join(GOLDEN, 'metrics_subset.npz'))
    N, L = int(g['G32_N']), int(g['G32_L'])
    assert bool(g['G32_ccd_runs']) and not bool(g['G32_II_runs']) and not bool(g['G32_fqc_runs'])
    assert 'IndexError' in str(g['G32_II_raises']) and 'IndexError' in str(g['G32_fqc_raises'])
    ref = g['G32_ref']
    assert ref.shape == (L, N, N)
    w, v = np.linalg.eigh(ref)
    pms = [v[l] * np.sqrt(np.clip(w[l], 0, None))[None, :] for l in range(L)] + [np.zeros((N, N), complex)]
    args = (g['G32_qs'], pms, g['G32_radial_mask'], float(g['G32_wavelength']), int(g['G32_C_order']))
    for name in ('II_error', 'fqc_error'):
        with pytest.raises(NotImplementedError, match='upstream raises'):
            hs.invariant_metric_tables([name, 'ccd_diff'], *args, used_ids=range(L))
    t = hs.invariant_metric_tables(['ccd_diff'], *args, used_ids=range(L))
    assert not t['ccd_weights'][L].any() and t['zero_mask'][L].all()
    e = MTC.metrics_engine(N, L, 2, lib_path)
    try:
        MTC.arm_metrics(e, t, 2)
        Ilm = np.stack([np.concatenate([g[f'G32_{pre}{l}'] for l in range(L + 1)], axis=1) for pre in ('I', 'J')])
        got = e.invariant_metrics_of(Ilm)['ccd_diff']
        want = np.array([g['G32_ccd_I'].real, g['G32_ccd_J'].real])
        print('ccd_diff on a subset:', got, 'reference', want)
        assert want.min() > 1e-3 and np.allclose(got, want, rtol=1e-9, atol=0), (got, want)
        # the unused order takes no part: with all orders used and the same (zero) reference for order L the value differs
        full = hs.invariant_metric_tables(['ccd_diff'], *args)
        MTC.arm_metrics(e, full, 2)
        assert not np.allclose(e.invariant_metrics_of(Ilm)['ccd_diff'], want, rtol=1e-6)
    finally:
        e.close()


def check_ccd_subset_loop(lib_path=None, fused=True, name='golden', main_type='mean', item_set='real+ccd+rl2'):
    """the same along the loop, steered by a main error that lists ccd_diff, as case 1; II_error and fqc_error with a subset still
    raise when the engine is set up"""
    data, N, L, _ = problem_data(name)
    seeds = SEEDS[name]
    check_inputs_discriminate(name, main_type, item_set, seeds)
    calc = calculate_of(name, L)
    res = run_product(name, main_type, item_set, seeds, lib_path, fused, n_used=L)
    for b, seed in enumerate(seeds):
        ref = oracle_run(name, main_type, item_set, seed, n_used=L)[0]
        full = oracle_run(name, main_type, item_set, seed)[0]
        assert not np.allclose(ref['error_dict']['reciprocal']['ccd_diff'], full['error_dict']['reciprocal']['ccd_diff'], rtol=1e-3)
        _compare_restart(f'ccd_diff on orders 0 .. {L - 1}, fused={fused}, restart {b}', res[b], ref, calculate=calc)
    for metric in ('II_error', 'fqc_error'):
        opt = settings(name, n_used=L)
        opt['main_loop']['error']['methods']['reciprocal']['calculate'] = ['ccd_diff', metric]
        with pytest.raises(NotImplementedError, match=metric + '.*subset of the orders'):
            Engine(opt, data, lib_path=lib_path)

"""Cases of the resident 2-D engine (mtip2d_run and friends, csrc/k_polar2d.hip; `MTIP2D(..., resident=True)`), shared by the CPU
emulator suite (tests/test_emul_resident2d.py, lib_path = the emulation build) and the MI355X suite (tests/test_gpu_resident2d.py,
lib_path = None).  The yardsticks are the ones the operator-level 2-D loop is held to: the reference's own 2-D runs (fixtures G20,
G22), oracle/mtip2d.py, and the operator-level calls themselves (`Engine2D.step`, `.shrinkwrap`), which this engine leaves as they
are; section 8 adds a longdouble restatement of one step (tests/resident2d_reference.py) at the shapes where the geometry of the fused
kernels changes."""
import numpy as np

import parity_cases as PC
from helpers import rel_l2
from oracle import mtip as OM
from xframe_amd.fxs import reconstruct as R
from xframe_amd.fxs._lib import MtipError
from xframe_amd.fxs.reconstruct2d import MTIP2D

TOL_STEP = 1e-9                  # the project's single-step bound (rel-L2 of F', rho'; relative for the error values)
TOL_STEP_128 = TOL_STEP          # at 128 shells x M = 64: holds as it is (figures in check_shadowed_schedule_2d)


def launch_log(e):
    """all kernel names the CPU emulator launched since the previous call (None on the GPU build); the log is reset"""
    return PC.launched_kernels(e, prefixes=('k',))


# ---------------------------------------------------------------------------------------------------------------- 1. reference runs
def check_trajectory_golden(g, lib_path=None):
    data, o = PC.mtip2d_problem(g)
    m = MTIP2D(o, data, n_restarts=2, initial_densities=[g['rho0'], g['rho0']], lib_path=lib_path, resident=True)
    res = m.phasing_loop()
    m.close()
    for r in res:
        PC._compare_mtip2d_trajectory(r, g, 1e-8, 1e-8)


def check_variant_golden(g, gv, name, lib_path=None):
    data, o, ref = PC.mtip2d_variant_problem(g, gv, name)
    m = MTIP2D(o, data, n_restarts=2, initial_densities=[g['rho0'], g['rho0']], lib_path=lib_path, resident=True)
    res = m.phasing_loop()
    m.close()
    for r in res:
        PC._compare_mtip2d_variant(r, ref, 1e-8, 1e-8)


def check_settings_vs_oracle(g, lib_path, name):
    """PC.check_mtip2d_settings_vs_oracle with the resident loop: same settings, same tolerances"""
    from oracle import mtip2d as O2
    data, o = PC.mtip2d_problem(g)
    main = o['main_loop']['sub_loops']['main']
    main['methods']['HIO']['iterations'] = 3
    main['methods']['ER']['iterations'] = 2
    main['iterations'] = 2
    o = OM.deep_update(o, PC.SETTINGS_VARIANTS_2D[name])
    rho0 = np.asarray(g['rho0'])
    ref = O2.MTIP2D(o, data).phasing_loop(rho0=rho0)
    m = MTIP2D(o, data, n_restarts=2, initial_densities=[rho0, 1.5 * rho0], lib_path=lib_path, resident=True)
    r = m.phasing_loop()[0]
    m.close()
    assert len(r['error_dict']['main']) == len(ref['error_dict']['main'])
    assert np.allclose(r['error_dict']['main'], ref['error_dict']['main'], rtol=1e-8), name
    for k in ('real_density', 'last_real_density', 'reciprocal_density', 'last_reciprocal_density', 'fxs_unknowns', 'last_deg2_invariant'):
        assert rel_l2(r[k], ref[k]) < 1e-8, (name, k)
    assert (r['support_mask'] != ref['support_mask']).sum() == 0 and (r['last_support_mask'] != ref['last_support_mask']).sum() == 0
    assert np.isclose(r['final_error'], ref['final_error'], rtol=1e-8)


def check_unbuildable(g, lib_path=None):
    """what raises NotImplementedError / IndexError in the operator-level 2-D loop raises the same on the resident one"""
    import pytest
    data, o = PC.mtip2d_problem(g)
    cases = [
        ({'density_guess': {'type': 'low_resolution_autocorrelation'}}, NotImplementedError),
        ({'main_loop': {'sub_loops': {'main': {'order': ['HIO', 'RAAR'], 'methods': {'RAAR': 1}}}}}, NotImplementedError),
        ({'main_loop': {'error': {'methods': {'reciprocal': {'calculate': ['l2_projection_diff']}}},
                        'sub_loops': {'main': {'order': ['HIO', 'HIO_non_FXS'], 'methods': {'HIO_non_FXS': 1}}}}}, NotImplementedError),
        ({'main_loop': {'sub_loops': {'main': {'order': ['SW_center', 'HIO'], 'methods': {'SW_center': 1}}}}}, IndexError),
    ]
    for upd, exc in cases:
        for resident in (False, True):
            m = MTIP2D(OM.deep_update(o, upd), data, n_restarts=1, lib_path=lib_path, resident=resident)
            with pytest.raises(exc):
                m.phasing_loop()
            m.close()
    for resident in (False, True):
        with pytest.raises(NotImplementedError):
            MTIP2D(OM.deep_update(o, {'main_loop': {'error': {'methods': {'reciprocal': {'calculate': ['fqc_error']}}}}}), data, n_restarts=1,
                   lib_path=lib_path, resident=resident)


# ---------------------------------------------------------------------------------------------------------------- 2. single steps
def _engine_from(m, rhos):
    e = m.engine
    for b, r in enumerate(rhos):
        e.set_density(b, r)
    e.set_initial_support(m.initial_support)
    e.set_reciprocal_metrics()
    e.set_main_error('mean', ['real'])
    e.init_state()
    return e


def check_single_steps_golden(g, lib_path=None):
    """one resident step of HIO / ER, with and without ft_stab, initial support enforced and not, from the fixture's step input against
    the reference's own steps (G20): F', rho' rel-L2 <= 1e-9, error rtol 1e-9; the shrink-wrap mask equal"""
    data, o = PC.mtip2d_problem(g)
    m = MTIP2D(o, data, n_restarts=2, initial_densities=[g['rho0'], g['rho0']], lib_path=lib_path, resident=True)
    e = _engine_from(m, [g['rho0'], g['rho0']])
    assert rel_l2(e.density()[1], g['step_rho_in']) < 1e-12 and rel_l2(e.reciprocal_density()[0], g['step_F0']) < 1e-12
    worst = 0.0
    for enf in (1, 0):
        sup = g['step_support'] & m.initial_support if enf else g['step_support']
        for meth in ('HIO', 'ER', 'HIO_ft_stab', 'ER_ft_stab'):
            e.init_state()
            for b in range(2):
                e.set_support(b, sup)
            err = e.run(meth.replace('_ft_stab', ''), meth.endswith('ft_stab'), [0.45])
            tag = f'step_{meth}_enf{enf}'
            Fn, rn = e.reciprocal_density(), e.density()
            for b in range(2):
                dF, dr, de = rel_l2(Fn[b], g[tag + '_F']), rel_l2(rn[b], g[tag + '_rho']), abs(err[0, b] / float(g[tag + '_err']) - 1)
                worst = max(worst, dF, dr, de)
                print(f'{tag} restart {b}: F {dF:.2e} rho {dr:.2e} err {de:.2e}')
                assert dF <= TOL_STEP and dr <= TOL_STEP and de <= TOL_STEP, tag
    e.init_state()
    e.shrinkwrap_state(20.0, 0.09, np.inf)
    assert (e.support()[1] != g['step_SW_mask']).sum() == 0
    m.close()
    return worst


# ---------------------------------------------------------------------------------------------------------------- 3. shadowed schedules
SCHEDULE_A = {'main_loop': {
    'error': {'methods': {'reciprocal': {'calculate': ['deg2_invariant_l2_diff', 'l2_projection_diff'], 'deg2_invariant_l2_diff': {'order': 2}}}},
    'sub_loops': {'order': ['main', 'refinement'],
                  'main': {'order': ['HIO', 'SW', 'ER', 'SW_center'], 'iterations': 2, 'best_density_not_in_first_n_iterations': 0,
                           'methods': {'HIO': {'iterations': 4, 'ft_stab': True}, 'SW': 1, 'ER': {'iterations': 3, 'ft_stab': False}, 'SW_center': 1}},
                  'refinement': {'order': ['SW', 'ER'], 'iterations': 2, 'best_density_not_in_first_n_iterations': np.inf,
                                 'methods': {'SW': 1, 'ER': {'iterations': 3, 'ft_stab': True}}}}}}
SCHEDULE_B = {'main_loop': {
    'sub_loops': {'order': ['main'],
                  'main': {'order': ['HIO', 'HIO_non_FXS', 'SW', 'ER_non_FXS', 'ER'], 'iterations': 2,
                           'methods': {'HIO': {'iterations': 3, 'ft_stab': True}, 'HIO_non_FXS': {'iterations': 2, 'ft_stab': True}, 'SW': 1,
                                       'ER_non_FXS': {'iterations': 2, 'ft_stab': False}, 'ER': {'iterations': 2, 'ft_stab': True}}}}}}
SCHEDULES = {'fxs_sw_center_reselect_metrics': SCHEDULE_A, 'non_fxs': SCHEDULE_B}


class _Shadow2D:
    """Wraps the resident calls of one Engine2D.  Every step of a `run` goes out on its own; before it the device's state (density,
    support, the pair before the most recent step) is fetched, after it the new pair, the error values and the reciprocal metrics
    are compared with ONE operator-level step (`Engine2D.step`, the parent commit's code, same context) from that state; every
    shrink-wrap is compared with `Engine2D.shrinkwrap` of the fetched density and the enforce decision with the last main error."""

    def __init__(self, m, tol):
        self.m, self.e, self.tol = m, m.engine, tol
        self.worst = {'F': 0.0, 'rho': 0.0, 'err': 0.0, 'main': 0.0, 'deg2': 0.0, 'l2': 0.0}
        self.n_steps = self.n_sw = self.n_select = self.flips = 0
        self.stale_F = None
        self.fixed = None
        e = self.e
        self._run, self._sw, self._begin, self._select = e.run, e.shrinkwrap_state, e.begin_sub_loop, e.select_best
        e.run, e.shrinkwrap_state, e.begin_sub_loop, e.select_best = self.run, self.shrinkwrap_state, self.begin_sub_loop, self.select_best

    def begin_sub_loop(self):
        self._begin()
        self.stale_F, self.fixed = self.e.reciprocal_density(), None

    def select_best(self, where=None):
        e = self.e
        before = (e.reciprocal_density(), e.density(), e.support())
        best = (e.reciprocal_density(True), e.density(True), e.support(True))
        self._select(where)
        sel = np.ones(e.B, bool) if where is None else np.asarray(where, bool)
        for a, b, c in zip(before, best, (e.reciprocal_density(), e.density(), e.support())):
            assert np.array_equal(np.where(sel.reshape(-1, 1, 1), b, a), c)
        self.n_select += 1

    def shrinkwrap_state(self, sigma, threshold, limit):
        e, m = self.e, self.m
        rho = e.density()
        enforced = self._sw(sigma, threshold, limit)
        last = e.fetch_main_errors(e.n_steps - 1, 1)[0] if e.n_steps else None
        expect_enf = last > limit if last is not None else np.zeros(e.B, bool)
        assert np.array_equal(enforced, expect_enf)
        new = e.shrinkwrap(rho, sigma, threshold)
        expect = np.where(expect_enf[:, None, None], new & m.initial_support, new)
        self.flips += int((e.support() != expect).sum())
        self.n_sw += 1
        return enforced

    def run(self, method, ft_stab, betas, fetch=True):
        e, m = self.e, self.m
        fxs = not method.endswith('_non_FXS')
        if fxs:
            self.fixed = None
        elif self.fixed is None:
            self.fixed = np.abs(self.stale_F)
        if len(np.atleast_1d(betas)) == 0:
            return self._run(method, ft_stab, betas, fetch)
        want = bool(m.reciprocal_metrics)
        for beta in np.atleast_1d(betas):
            rho, sup, F_before = e.density(), e.support(), e.reciprocal_density()
            self._run(method, ft_stab, [beta], fetch=False)
            ref = m._step(method, ft_stab, float(beta), rho, sup, self.fixed, want)
            s = e.n_steps - 1
            err, main = e.fetch_errors(s, 1)[0], e.fetch_main_errors(s, 1)[0]
            recip = m._reciprocal_errors(ref[4], ref[0], ref[5]) if want else {}
            got = e.fetch_reciprocal_metrics(s, 1) if want else {}
            d = {'F': max(rel_l2(a, b) for a, b in zip(e.reciprocal_density(), ref[0])),
                 'rho': max(rel_l2(a, b) for a, b in zip(e.density(), ref[1])),
                 'err': float(np.max(np.abs(err / ref[2] - 1))),
                 'main': float(np.max(np.abs(main / m._main_error(ref[2], recip) - 1)))}
            if 'deg2_invariant_l2_diff' in recip:
                d['deg2'] = float(np.max(np.abs(got['deg2_invariant_l2_diff'][0] / recip['deg2_invariant_l2_diff'] - 1)))
            if 'l2_projection_diff' in recip:
                d['l2'] = float(np.max(np.abs(got['l2_projection_diff'][0] / recip['l2_projection_diff'] - 1)))
            if fxs:                                                   # (informative: the phase of an order whose scalar product is rounding noise is arbitrary)
                d_unk = rel_l2(e.unknowns(), ref[3])
                print(f'step {s}: unknowns {d_unk:.2e}')
            print(f'step {s} {method} ft_stab={ft_stab}: ' + ' '.join(f'{k} {v:.2e}' for k, v in d.items()))
            for k, v in d.items():
                self.worst[k] = max(self.worst[k], v)
                assert v <= self.tol, (s, method, k, v)
            self.stale_F = F_before
            self.n_steps += 1
        return None


def check_shadowed_schedule_2d(g, name, lib_path=None, N=None, M=None, tol=TOL_STEP, n_restarts=2):
    """the resident loop along a whole schedule, every step and every shrink-wrap shadowed by the operator-level call from the state
    the device holds (one-step shadows: chaos does not enter); support masks must be EQUAL (no flip is excused: the shrink-wrap of
    the resident state runs the operator path's launches on the same values).

    The direction of the shadow: the RESIDENT loop runs, and each of its steps is re-done by one operator-level step from the state
    the device held before it (as check_shadowed_schedule does for 3-D with the oracle), so both paths see identical inputs in
    every step.  Bound: TOL_STEP = 1e-9, the project's single-step bound, relative also for the error values -- at the fixture's
    size and at 128 shells x M = 64 (TOL_STEP_128 = TOL_STEP: it did not have to be derived from the oracle distance).  Measured on
    the MI355X at 128 x M64, seeds 31 / 32: one operator-level step against one oracle/mtip2d.py step F' 2.2e-15 .. 2.7e-15,
    rho' 6.5e-15 .. 8.6e-15 (HIO with / without ft_stab, ER); the resident step against the operator-level step, worst over all
    steps of both schedules: F' 3.4e-16, rho' 1.6e-15, real / main error 2.3e-14, deg2 metric 4.0e-15, reciprocal l2 1.2e-15; no
    support point differs.  At 12 x M6 (emulator and MI355X): F' <= 1.1e-16, rho' 7.1e-16, errors 4.7e-15."""
    data, o = PC.mtip2d_scaled_problem(g, N, M)
    o = OM.deep_update(o, SCHEDULES[name])
    eis = o['projections']['real']['projections']['support']['enforce_initial_support']
    eis['apply'], eis['if_error_bigger_than'] = True, 0.05
    rng = np.random.default_rng(5)
    if N is None:
        rho0 = np.asarray(g['rho0'])
        rhos = [rho0 * (1.0 + (0.5 + b) * rng.random(rho0.shape)) for b in range(n_restarts)]
        m = MTIP2D(o, data, n_restarts=n_restarts, initial_densities=rhos, lib_path=lib_path, resident=True)
    else:
        m = MTIP2D(o, data, n_restarts=n_restarts, seeds=[31 + b for b in range(n_restarts)], lib_path=lib_path, resident=True)
    sh = _Shadow2D(m, tol)
    res = m.phasing_loop()
    m.close()
    n_expected = sum(lo['iterations'] * sum(v['iterations'] if isinstance(v, dict) else 0 for k, v in lo['methods'].items() if k in lo['order'])
                     for lo in (o['main_loop']['sub_loops'][n_] for n_ in o['main_loop']['sub_loops']['order']))
    assert sh.n_steps == n_expected == len(res[0]['error_dict']['main']) and sh.n_sw > 0
    assert sh.flips == 0
    if name == 'fxs_sw_center_reselect_metrics':
        assert sh.n_select > 0
    print('worst', sh.worst)
    return sh


# ---------------------------------------------------------------------------------------------------------------- 4. per-restart ft_stab
def check_ft_stab_per_restart(g, lib_path=None, N=None, M=None):
    """three restarts with ft_stab flags (1, 0, 1) in ONE run equal three single-restart runs bit for bit (N, M given: a scaled
    problem with seeded guesses -- M = 64 gives rows of 129 values, one more than a round of the 1024-thread workgroups takes, so the
    left-over column goes through the wave-per-output path of the row transforms)"""
    data, o = PC.mtip2d_scaled_problem(g, N, M)
    rng = np.random.default_rng(3)
    if N is None:
        rho0 = np.asarray(g['rho0'])
    else:
        m0 = MTIP2D(o, data, n_restarts=1, seeds=[4], lib_path=lib_path)
        rho0 = m0._initial_density(0)
        m0.close()
    rhos = [rho0 * (1.0 + b * rng.random(rho0.shape)) for b in range(3)]
    flags = np.array([True, False, True])
    betas = [0.45, 0.44, 0.43]
    m = MTIP2D(o, data, n_restarts=3, lib_path=lib_path, resident=True)
    e = _engine_from(m, rhos)
    e.run('HIO', flags, betas, fetch=False)
    err = e.run('ER', flags, betas[:2], fetch=False)
    assert err is None
    batch = (e.fetch_errors(0, 5), e.density(), e.reciprocal_density(), e.unknowns())
    m.close()
    for b in range(3):
        m1 = MTIP2D(o, data, n_restarts=1, lib_path=lib_path, resident=True)
        e1 = _engine_from(m1, [rhos[b]])
        e1.run('HIO', bool(flags[b]), betas, fetch=False)
        e1.run('ER', bool(flags[b]), betas[:2], fetch=False)
        single = (e1.fetch_errors(0, 5), e1.density(), e1.reciprocal_density(), e1.unknowns())
        m1.close()
        assert np.array_equal(batch[0][:, b], single[0][:, 0])
        for x, y in zip(batch[1:], single[1:]):
            assert np.array_equal(x[b], y[0])
    # and the flags matter
    assert not np.array_equal(batch[1][0], batch[1][1])


def check_wide_rows(g, lib_path, N, M):
    """one resident step of HIO_non_FXS, HIO and ER against the operator-level step from the same state on a scaled problem with
    rows of 2 M + 1 = 129 values (M = 64): F', rho' <= 1e-9, error values 1e-9"""
    data, o = PC.mtip2d_scaled_problem(g, N, M)
    m = MTIP2D(o, data, n_restarts=2, seeds=[11, 12], lib_path=lib_path, resident=True)
    e = _engine_from(m, [m._initial_density(b) for b in range(2)])
    rho, sup, F0 = e.density(), e.support(), e.reciprocal_density()
    for method, ft in (('HIO_non_FXS', True), ('HIO', True), ('ER', False)):
        e.init_state()
        err = e.run(method, ft, [0.5])
        ref = e.step(method, ft, 0.5, rho, sup, fixed_intensity=np.abs(F0))
        d = (max(rel_l2(a, b) for a, b in zip(e.reciprocal_density(), ref[0])), max(rel_l2(a, b) for a, b in zip(e.density(), ref[1])),
             float(np.max(np.abs(err[0] / ref[2] - 1))))
        print(f'{N} x M{M} {method}: F {d[0]:.2e} rho {d[1]:.2e} err {d[2]:.2e}')
        assert max(d) <= TOL_STEP, (method, d)
    m.close()


def check_ft_stab_disagreement(g, lib_path=None):
    """PC.check_mtip2d_ft_stab_disagreement's construction on the resident loop: two restarts that disagree on the ft_stab link, each
    against the oracle's own run of it at 1e-8; the disagreement reaches the engine as a per-restart mask in one run"""
    from oracle import mtip2d as O2
    data, o = PC.mtip2d_problem(g)
    o = OM.deep_update(o, {'main_loop': {'sub_loops': {'main': {'iterations': 3, 'order': ['HIO', 'SW', 'ER'], 'methods': {
        'HIO': {'iterations': 3, 'ft_stab': 'link_to_enforce_initial_support', 'link_to_enforce_initial_support': {'delay': 1}},
        'SW': 1, 'ER': {'iterations': 2, 'ft_stab': 'link_to_enforce_initial_support', 'link_to_enforce_initial_support': {'delay': 1}}}}}}})
    rho_a = np.asarray(g['rho0'])
    rho_b = rho_a * (1.0 + 2.0 * np.random.default_rng(9).random(rho_a.shape)) + 0.3 * np.abs(rho_a).max() * np.random.default_rng(10).random(rho_a.shape)
    refs = [O2.MTIP2D(o, data).phasing_loop(rho0=r) for r in (rho_a, rho_b)]
    e3 = [r['error_dict']['main'][2] for r in refs]
    assert max(e3) > 1.3 * min(e3)
    eis = o['projections']['real']['projections']['support']['enforce_initial_support']
    eis['apply'], eis['if_error_bigger_than'] = True, float(np.sqrt(e3[0] * e3[1]))
    refs = [O2.MTIP2D(o, data).phasing_loop(rho0=r) for r in (rho_a, rho_b)]
    m = MTIP2D(o, data, n_restarts=2, initial_densities=[rho_a, rho_b], lib_path=lib_path, resident=True)
    seen = []
    orig = m.engine.run

    def spy(method, ft_stab, betas, fetch=True):
        seen.append(ft_stab)
        return orig(method, ft_stab, betas, fetch)
    m.engine.run = spy
    res = m.phasing_loop()
    m.close()
    assert any(isinstance(f, np.ndarray) for f in seen)
    for r, ref in zip(res, refs):
        assert np.allclose(r['error_dict']['main'], ref['error_dict']['main'], rtol=1e-8)
        for k in ('real_density', 'last_real_density', 'reciprocal_density', 'last_reciprocal_density', 'fxs_unknowns'):
            assert rel_l2(r[k], ref[k]) < 1e-8, k
        assert (r['last_support_mask'] != ref['last_support_mask']).sum() == 0


# ---------------------------------------------------------------------------------------------------------------- 5. splits, determinism
def check_split_invariance(g, lib_path=None, N=None, M=None):
    """run of n steps == n runs of one step == the same without fetching and a later fetch_errors: bit-identical histories and final
    state; a repeated run from the same state is bit-identical"""
    data, o = PC.mtip2d_scaled_problem(g, N, M)
    o = OM.deep_update(o, {'main_loop': {'error': {'methods': {'reciprocal': {'calculate': ['deg2_invariant_l2_diff', 'l2_projection_diff'],
                                                                                'deg2_invariant_l2_diff': {'order': 2}}}}}})
    kw = dict(initial_densities=[g['rho0'], 1.3 * np.asarray(g['rho0'])]) if N is None else dict(seeds=[5, 6])
    m = MTIP2D(o, data, n_restarts=2, lib_path=lib_path, resident=True, **kw)
    rhos = [m._initial_density(b) for b in range(2)]
    betas = np.array([0.5, 0.49, 0.48, 0.47])
    flags = np.array([True, False])

    def state(e):
        n = e.n_steps
        rec = e.fetch_reciprocal_metrics(0, n)
        return (e.fetch_errors(0, n), e.fetch_main_errors(0, n), rec['deg2_invariant_l2_diff'], rec['l2_projection_diff'], e.density(),
                e.reciprocal_density(), e.density(True), e.support(True), e.unknowns(), e.best_error()[0])

    def prepare():
        e = m.engine
        for b in range(2):
            e.set_density(b, rhos[b])
        e.set_initial_support(m.initial_support)
        ref = m._deg2_ref.copy()
        ref[m.rsetup.used_orders[0]] = m._deg2_ref[m.rsetup.used_orders[0]] / m.rsetup.number_of_particles
        from xframe_amd.fxs.reconstruct2d import polar_integrator_weights
        w = polar_integrator_weights(e.rs, e.phis)
        w[m.N - 2] = 0
        e.set_reciprocal_metrics(ref, m._deg2_norm, w)
        e.set_main_error('mean', ['real', 'l2_projection_diff'])
        e.init_state()
        return e

    e = prepare()
    got = e.run('HIO', flags, betas)
    e.shrinkwrap_state(m.default_sigma, 0.06, np.inf)
    got2 = e.run('ER', True, betas[:3])
    a = state(e)
    assert np.array_equal(got, a[0][:4]) and np.array_equal(got2, a[0][4:])
    e = prepare()                                                      # the same again: deterministic
    e.run('HIO', flags, betas, fetch=False)
    e.shrinkwrap_state(m.default_sigma, 0.06, np.inf)
    e.run('ER', True, betas[:3], fetch=False)
    b_ = state(e)
    e = prepare()                                                      # one step per run
    for beta in betas:
        e.run('HIO', flags, [beta], fetch=bool(beta > 0.485))
    e.shrinkwrap_state(m.default_sigma, 0.06, np.inf)
    for beta in betas[:3]:
        e.run('ER', True, [beta], fetch=False)
    c = state(e)
    m.close()
    for x, y, z in zip(a, b_, c):
        assert np.array_equal(x, y) and np.array_equal(x, z)
    assert np.isfinite(a[0]).all() and np.isfinite(a[2]).all()


# ---------------------------------------------------------------------------------------------------------------- 6. worker
def check_worker_vs_oracle(g, lib_path=None, N=None, M=None, n_restarts=3):
    """PC.check_mtip2d_worker_vs_oracle with `GPU.resident_2d: True`: seeded guesses, every restart against the oracle's loop (1e-7)"""
    from oracle import mtip2d as O2
    data, o = PC.mtip2d_scaled_problem(g, N, M)
    o = OM.deep_update(o, {'multi_process': {'use': True, 'n_parallel_reconstructions': n_restarts},
                           'GPU': {'use': True, 'n_gpu_workers': 1, 'resident_2d': True}})
    seeds = [77 + i for i in range(n_restarts)]
    w = R.ProjectWorker(o, data, seeds=seeds, lib_path=lib_path)
    res, _ = w.run()
    assert all(m.loop2d.resident for m in w.mtip_instances)
    assert len(res) == n_restarts and set(w.results['reconstruction_results']) == {str(i) for i in range(n_restarts)}
    for b in range(n_restarts):
        ref = O2.MTIP2D(o, data).phasing_loop(rng=np.random.default_rng(seeds[b]))
        assert rel_l2(res[b]['initial_density'], ref['initial_density']) < 1e-12
        assert np.allclose(res[b]['error_dict']['main'], ref['error_dict']['main'], rtol=1e-7)
        for k in ('real_density', 'last_real_density', 'reciprocal_density', 'last_reciprocal_density', 'last_deg2_invariant', 'fxs_unknowns'):
            assert rel_l2(res[b][k], ref[k]) < 1e-7, k
        assert (res[b]['support_mask'] != ref['support_mask']).sum() == 0 and (res[b]['last_support_mask'] != ref['last_support_mask']).sum() == 0
    for m in w.mtip_instances:
        m.engine.close()


def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def check_worker_default_unchanged(g, lib_path=None, n_restarts=3):
    """with the key absent the worker takes the operator-level loop: bit-identical to a direct MTIP2D(resident=False) run; and the
    resident result dicts have the same keys, shapes and dtypes"""
    data, o = PC.mtip2d_problem(g)
    o = OM.deep_update(o, {'multi_process': {'use': True, 'n_parallel_reconstructions': n_restarts}, 'GPU': {'use': True, 'n_gpu_workers': 1}})
    assert 'resident_2d' not in o['GPU']
    seeds = [77 + i for i in range(n_restarts)]
    w = R.ProjectWorker(o, data, seeds=seeds, lib_path=lib_path)
    res, _ = w.run()
    assert not any(m.loop2d.resident for m in w.mtip_instances)
    for m in w.mtip_instances:
        m.engine.close()
    direct = MTIP2D(o, data, n_restarts=n_restarts, seeds=seeds, lib_path=lib_path)
    ref = direct.phasing_loop()
    direct.close()
    resident = MTIP2D(o, data, n_restarts=n_restarts, seeds=seeds, lib_path=lib_path, resident=True)
    rres = resident.phasing_loop()
    resident.close()
    for b in range(n_restarts):
        assert set(res[b]) == set(ref[b]) == set(rres[b])
        for k in ref[b]:
            assert _same(res[b][k], ref[b][k]), k

        def shapes(x):
            if isinstance(x, dict):
                return {k: shapes(v) for k, v in x.items()}
            return (type(x).__name__,) if not isinstance(x, np.ndarray) else (x.shape, x.dtype)
        assert shapes(ref[b]) == shapes(rres[b])


# ---------------------------------------------------------------------------------------------------------------- 7. launch budget
def check_launch_budget(g, lib_path):
    """emulator launch log: 5 steps of HIO with ft_stab, of ER, of HIO without ft_stab log at most 30 k2d_* launches and nothing else
    (no metric enabled); a *_non_FXS run launches no projection; wrong-state calls return an error and launch nothing"""
    data, o = PC.mtip2d_problem(g)
    m = MTIP2D(o, data, n_restarts=3, lib_path=lib_path, resident=True)
    e = _engine_from(m, [g['rho0']] * 3)
    betas = [0.5] * 5
    for method, ft in (('HIO', True), ('ER', True), ('HIO', False), ('HIO', np.array([True, False, True]))):
        launch_log(e)
        e.run(method, ft, betas, fetch=False)
        log = launch_log(e)
        assert all(k.startswith('k2d_') for k in log) and 5 <= len(log) <= 30, log
        assert sum(k == 'k2d_rs_mid' for k in log) == 5
    launch_log(e)
    e.run('HIO_non_FXS', True, betas, fetch=False)
    e.run('ER_non_FXS', False, betas, fetch=False)
    log = launch_log(e)
    assert len(log) <= 51 and all(k.startswith('k2d_') for k in log), log
    assert not any(k in ('k2d_rs_head', 'k2d_rs_mid', 'k2d_rs_deg2', 'k2d_project') for k in log), log      # no harmonic part, no projection
    assert sum(k == 'k2d_rs_mid_nonfxs' for k in log) == 10
    unk = e.unknowns()
    e.run('ER_non_FXS', False, betas[:1], fetch=False)
    assert np.array_equal(unk, e.unknowns())
    m.close()
    # wrong state
    from xframe_amd.fxs.polar2d import Engine2D
    e = Engine2D(int(g['N']), int(g['M']), float(g['max_q']), n_batch=2, lib_path=lib_path)
    launch_log(e)
    for call in (lambda: e.run('HIO', True, betas), lambda: e.init_state(), lambda: e.shrinkwrap_state(1.0, 0.1, np.inf), lambda: e.begin_sub_loop(),
                 lambda: e.select_best(), lambda: e.density()):
        try:
            call()
            raise AssertionError('no error')
        except MtipError as ex:
            assert 'error -5' in str(ex), ex
    e.set_error_weights(np.ones(e.shape))
    for b in range(2):
        e.set_density(b, g['rho0'])
    e.set_initial_support(m.initial_support)
    launch_log(e)
    e.init_state()                                       # no projection yet: the non-FXS methods can run, an FXS method cannot
    launch_log(e)
    try:
        e.run('HIO', True, betas)
        raise AssertionError('no error')
    except MtipError as ex:
        assert 'error -5' in str(ex) and 'mtip2d_set_projection' in str(ex), ex
    assert launch_log(e) == ()
    e.close()


# ---------------------------------------------------------------------------------------------------------------- 8. the step kernels' geometry
# One resident step against the longdouble restatement (tests/resident2d_reference.py) at the shapes where the geometry of the k2d_rs_*
# kernels changes: (shells N, max order M, restarts) -> what the shape reaches.  Rows have 2 M + 1 values.
REFERENCE_SHAPES = {
    (5, 6, 9): 'second restart group with one restart; Hankel slices of 2, 2, 1, 0 shells; finish wave 0 takes restarts 0, 4, 8',
    (13, 6, 17): 'three groups, a full middle one; last Hankel slice of one shell',
    (6, 64, 3): '129 values: one left-over column on the wave-per-output path',
    (6, 65, 2): '131 values: the first row length back on the two-round path',
    (6, 86, 9): '173 values: the largest row the LDS limit admits, two groups',
    (7, 1, 2): '3 values, 2 coefficient outputs: the wave path with no full round',
}
# Distance of oracle/mtip2d.py's step (complex128, numpy FFT, pairwise sums) from the restatement, measured on the CPU with
# `oracle_distance` below from the very states of these cases, worst restart and method; per quantity the largest deviation of a row
# relative to the restart's largest value (F', rho'), relative for the scalars:
#            shape          F'       rho'     unknowns  real err  l2       deg2      main
ORACLE_DISTANCE = {
    (5, 6, 9):     (1.5e-15, 9.6e-16, 1.4e-14, 6.6e-16, 4.2e-16, 1.1e-14, 6.6e-16),
    (13, 6, 17):   (1.1e-15, 1.0e-15, 8.8e-15, 2.6e-15, 6.1e-16, 3.9e-14, 2.6e-15),
    (6, 64, 3):    (7.8e-15, 1.9e-15, 3.1e-14, 2.3e-16, 7.5e-16, 2.6e-14, 2.3e-16),
    (6, 65, 2):    (5.9e-15, 2.3e-15, 2.8e-14, 4.8e-16, 4.5e-16, 1.4e-14, 4.8e-16),
    (6, 86, 9):    (4.3e-14, 3.9e-15, 4.4e-14, 8.4e-16, 8.9e-16, 4.6e-14, 8.4e-16),
    (7, 1, 2):     (4.8e-16, 4.8e-16, 1.1e-16, 2.1e-15, 3.4e-16, 1.1e-15, 2.1e-15),
}                                                                     # largest: 4.6e-14 -> BOUND_STEP = 2.3e-12
# The bound of the comparison is 50 x the largest of these figures: a sequential sum of n terms (the device, up to 173 per row) against
# numpy's pairwise one loses up to n / log2(n) ~ 23 times more, with a factor 2 on top.  It never comes from what the resident engine
# gives, and it has to stay below the project's single-step bound.  (For comparison only, the resident engine against the
# restatement on the MI355X, same quantities: (5, 6, 9) 1.0e-13 (deg2), (13, 6, 17) 3.1e-14 (unknowns), (6, 64, 3) 3.9e-14 (deg2),
# (6, 65, 2) 9.1e-14 (deg2), (6, 86, 9) 1.6e-13 (deg2; F' 1.4e-13), (7, 1, 2) 1.0e-15; every column in profiles/resident2d_coverage.txt.)
BOUND_STEP = 50 * max([max(v) for v in ORACLE_DISTANCE.values()] or [0.0])
assert BOUND_STEP <= TOL_STEP
STEP_RUNS = (('HIO', 'mask'), ('ER', False), ('HIO_non_FXS', True), ('ER_non_FXS', False))
QUANTITIES = ('F', 'rho', 'unknowns', 'err', 'l2', 'deg2', 'main')
_SEEDS = {(5, 6, 9): 101, (13, 6, 17): 102, (6, 64, 3): 103, (6, 65, 2): 104, (6, 86, 9): 105, (7, 1, 2): 106}


class _RecordedTables:
    """wraps the engine's setters while an MTIP2D is built: what the host hands to the context is what the restatement gets"""
    NAMES = ('set_projection', 'set_so_freedom', 'set_real_constraints', 'set_error_weights')

    def __enter__(self):
        from xframe_amd.fxs import polar2d as P2D
        self.P2D, self.rec = P2D, {}
        self.saved = {k: getattr(P2D.Engine2D, k) for k in self.NAMES}
        self.saved_w = P2D.assemble_weights_2d

        def wrap(name):
            def call(eng, *a):
                self.rec[name] = a
                return self.saved[name](eng, *a)
            return call

        def weights(*a):
            self.rec['weights'] = self.saved_w(*a)
            return self.rec['weights']
        for k in self.NAMES:
            setattr(P2D.Engine2D, k, wrap(k))
        P2D.assemble_weights_2d = weights
        return self

    def __exit__(self, *exc):
        for k in self.NAMES:
            setattr(self.P2D.Engine2D, k, self.saved[k])
        self.P2D.assemble_weights_2d = self.saved_w

    def tables(self, e, deg2_ref=None, deg2_norms=None, l2_weights=None):
        import resident2d_reference as RR
        r = self.rec
        vectors, used, rmask, n_particles = r['set_projection'] if 'set_projection' in r else (np.zeros((0, e.N)), {}, np.zeros((0, e.N)), 1.0)
        ids = np.array(list(used.values()), dtype=int)
        return RR.make_tables(e.N, e.M, r['weights'][0], r['weights'][1], np.zeros(e.n_phi, bool), vectors, np.asarray(rmask, bool)[ids], ids, e.qs,
                              n_particles, r['set_so_freedom'][0] if 'set_so_freedom' in r else None, r['set_real_constraints'], r['set_error_weights'][0],
                              deg2_ref, deg2_norms, l2_weights)


class _StepProblem:
    """one of REFERENCE_SHAPES: the scaled problem with the orders 0 .. min(M, 6) used (the orders beyond carry no signal at these
    shell counts: their scalar products are rounding noise whose phase is arbitrary on either side), both reciprocal metrics on, a
    seeded guess and a random support with holes per restart"""

    def __init__(self, g, lib_path, N, M, B, restarts=None, nan_in=None):
        import resident2d_reference as RR
        self.RR, self.shape, self.lib_path = RR, (N, M, B), lib_path
        data, o = PC.mtip2d_scaled_problem(g, N, M)
        o = OM.deep_update(o, RR.METRICS_ON)
        o['projections']['reciprocal']['used_order_ids'] = np.arange(min(M, 6) + 1)
        self.data, self.o = data, o
        self.pick = list(range(B)) if restarts is None else list(restarts)         # (a single-restart twin of restart b: restarts=[b])
        with _RecordedTables() as rec:
            self.m = m = MTIP2D(o, data, n_restarts=len(self.pick), seeds=[4] * len(self.pick), lib_path=lib_path, resident=True)
        self.e = e = m.engine
        rhos, sups = RR.seeded_inputs(m._initial_density(0), B, _SEEDS[(N, M, B)])
        if nan_in is not None:
            rhos[nan_in][N // 2, M] = np.nan
        self.rhos, self.sups = [rhos[b] for b in self.pick], [sups[b] for b in self.pick]
        self.mask = np.array([b % 3 != 1 for b in self.pick])
        ref = m._deg2_ref.copy()                                                  # as MTIP2D._loop_resident hands them over
        ref[m.rsetup.used_orders[0]] = m._deg2_ref[m.rsetup.used_orders[0]] / m.rsetup.number_of_particles
        from xframe_amd.fxs.reconstruct2d import polar_integrator_weights
        w_l2 = polar_integrator_weights(e.rs, e.phis)
        w_l2[N - 2, :] = 0.0
        self.metrics = (ref, m._deg2_norm, w_l2)
        self.t = rec.tables(e, *self.metrics)
        for b, r in enumerate(self.rhos):
            e.set_density(b, r)
        e.set_initial_support(m.initial_support)
        self.prepare(True)
        self.rho_in, self.F0 = e.density(), e.reciprocal_density()

    def prepare(self, fxs, kind='mean', items=('real',)):
        e = self.e
        e.set_reciprocal_metrics(*(self.metrics if fxs else ()))
        e.set_main_error(kind, list(items))
        e.init_state()
        for b, s in enumerate(self.sups):
            e.set_support(b, s)

    def run(self, method, ft, beta=0.45, kind='mean', items=('real',)):
        """one step from the prepared state -> per restart the dict layout of resident2d_reference.step"""
        e, fxs = self.e, not method.endswith('_non_FXS')
        self.prepare(fxs, kind, items)
        err = e.run(method, self.mask if isinstance(ft, str) else ft, [beta])
        F, rho, main = e.reciprocal_density(), e.density(), e.fetch_main_errors(0, 1)[0]
        unk = e.unknowns() if fxs else None
        rec = e.fetch_reciprocal_metrics(0, 1) if fxs else {}
        # the first step after init_state improves on the best error inf (unless its main error is NaN): its pair and support are kept
        kept = ~np.isnan(main)
        for latest, best in ((F, e.reciprocal_density(True)), (rho, e.density(True)), (np.array(self.sups), e.support(True))):
            assert np.array_equal(latest[kept], best[kept]), (self.shape, method)
        assert np.array_equal(e.best_error()[0][kept], main[kept])
        return [dict(F_new=F[b], rho_new=rho[b], err=err[0, b], main=main[b], unknowns=unk[b] if fxs else None,
                     rl2=rec['l2_projection_diff'][0, b] if fxs else None, deg2=rec['deg2_invariant_l2_diff'][0, b] if fxs else None)
                for b in range(len(self.pick))]

    def reference(self, method, ft, b, beta=0.45):
        """the restatement's step of restart b (position in `pick`) from the state the device holds; conditions on the inputs asserted"""
        RR, fxs = self.RR, not method.endswith('_non_FXS')
        flag = bool(self.mask[b]) if isinstance(ft, str) else ft
        ref = RR.step(self.t, method, flag, beta, self.rho_in[b], self.sups[b], None if fxs else RR.modulus(self.F0[b]))
        assert ref['err'] > 0 and rel_l2(np.asarray(ref['rho_new'], complex), self.rho_in[b]) > 1e-3, (self.shape, method, b)
        if fxs:
            assert ref['conditioning'].min() >= 1e-6, (self.shape, method, b, ref['conditioning'])
            assert ref['rl2'] > 0 and (ref['deg2'][self.t['deg2_norm'] != 0] > 0).all() and (ref['deg2'][self.t['deg2_norm'] == 0] == -1).all()
        ref['main'] = RR.main_error('mean', ['real'], ref['err'], ref['rl2'], ref['deg2'])
        return ref

    def close(self):
        self.m.close()


def _distance(RR, got, ref, fxs):
    d = RR.step_distance(got, ref, fxs)
    if 'main' in got:
        d['main'] = RR.deviation(got['main'], ref['main'])
    return d


def check_step_vs_restatement(g, lib_path, N, M, B):
    """one step of HIO (ft_stab per restart, b % 3 != 1: the mask alternates inside and across the groups), ER, HIO_non_FXS and
    ER_non_FXS from one state against the restatement: every shell row of every restart, every scalar, bound BOUND_STEP; then the
    restarts 0, 7, 8 and B - 1 of the batch against single-restart runs of the resident engine, bit for bit"""
    import resident2d_reference as RR
    p = _StepProblem(g, lib_path, N, M, B)
    assert np.isfinite(p.rho_in).all()
    worst = dict.fromkeys(QUANTITIES, 0.0)
    batch = {}
    for method, ft in STEP_RUNS:
        fxs = not method.endswith('_non_FXS')
        refs = [p.reference(method, ft, b) for b in range(B)]       # (conditions first: nothing is compared on a degenerate input)
        if fxs:
            print(f'{N} x M{M} x {B} {method}: smallest conditioning %.2e' % min(r['conditioning'].min() for r in refs))
        batch[method] = got = p.run(method, ft)
        for b in range(B):
            d = _distance(RR, got[b], refs[b], fxs)
            print(f'{N} x M{M} x {B} {method} restart {b}: ' + ' '.join(f'{k} {v:.2e}' for k, v in d.items()))
            for k, v in d.items():
                worst[k] = max(worst[k], v)
        assert max(worst.values()) <= BOUND_STEP, (method, worst, BOUND_STEP)
    p.close()
    print(f'{N} x M{M} x {B} worst ' + ' '.join(f'{k} {v:.2e}' for k, v in worst.items()), 'bound %.2e' % BOUND_STEP)
    for b in sorted({0, 7, 8, B - 1} & set(range(B))):
        p1 = _StepProblem(g, lib_path, N, M, B, restarts=[b])
        assert np.array_equal(p1.rho_in[0], p.rho_in[b])
        for method, ft in STEP_RUNS:
            one = p1.run(method, ft)[0]
            for k, v in one.items():
                assert v is None or np.array_equal(v, batch[method][b][k]), (N, M, B, method, b, k)
        p1.close()
    return worst


def oracle_distance(g, lib_path, N, M, B):
    """how ORACLE_DISTANCE was measured: oracle/mtip2d.py's step from the states of check_step_vs_restatement against the restatement
    with the oracle's own tables (the state comes from the engine: any build will do, the figures are the oracle's)"""
    import resident2d_reference as RR
    from oracle import mtip2d as O2
    p = _StepProblem(g, lib_path, N, M, B)
    mo = O2.MTIP2D(p.o, p.data)
    t = RR.tables_from_oracle(mo)
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for method, ft in STEP_RUNS:
        fxs = not method.endswith('_non_FXS')
        for b in range(B):
            flag = bool(p.mask[b]) if isinstance(ft, str) else ft
            fixed = None if fxs else RR.modulus(p.F0[b])
            ref = RR.step(t, method, flag, 0.45, p.rho_in[b], p.sups[b], fixed)
            got = RR.oracle_step(mo, method, flag, 0.45, p.rho_in[b], p.sups[b], None if fxs else np.asarray(fixed, float))
            got['main'], ref['main'] = got['err'], ref['err']
            for k, v in _distance(RR, got, ref, fxs).items():
                worst[k] = max(worst[k], v)
    p.close()
    return worst


def check_main_error_kinds(g, lib_path=None, N=5, M=6, B=9):
    """mean / min / max / prod over ['real'], ['real', 'l2_projection_diff'] and ['deg2_invariant_l2_diff'] in k2d_rs_finish against the
    restatement (numpy's functions on its values), nine restarts: a wave of the finish kernel takes more than one.  Then NaN as
    data: one NaN in the guess of restart 4 -- its error, main error and best error are what numpy's functions give (NaN; the best
    error stays inf, nothing is kept as better), the other eight restarts are bit-equal to the run without it; and a NaN in the deg2
    reference of one order behind finite ones -- min and max over the orders are NaN as numpy's are"""
    import resident2d_reference as RR
    p = _StepProblem(g, lib_path, N, M, B)
    refs = [p.reference('HIO', 'mask', b) for b in range(B)]
    item_sets = (['real'], ['real', 'l2_projection_diff'], ['deg2_invariant_l2_diff'])
    clean = {}
    for kind in ('mean', 'min', 'max', 'prod'):
        for items in item_sets:
            got = p.run('HIO', 'mask', kind=kind, items=items)
            best = p.e.best_error()[0]
            for b in range(B):
                want = RR.main_error(kind, items, refs[b]['err'], refs[b]['rl2'], refs[b]['deg2'])
                d = RR.deviation(got[b]['main'], want)
                print(f'{kind} {items} restart {b}: {d:.2e}')
                assert d <= BOUND_STEP and best[b] == got[b]['main'], (kind, items, b, d)
            clean[kind, tuple(items)] = got
    # the kinds differ on these values (a swap of two of them would show)
    for b in range(B):
        vals = {k: clean[k, ('deg2_invariant_l2_diff',)][b]['main'] for k in ('mean', 'min', 'max', 'prod')}
        assert len(set(vals.values())) == 4 and vals['min'] < vals['mean'] < vals['max'], vals
    p.close()
    q = _StepProblem(g, lib_path, N, M, B, nan_in=4)
    assert np.isnan(q.rho_in[4]).all() and np.isfinite(np.delete(q.rho_in, 4, axis=0)).all()
    for kind in ('mean', 'min', 'max', 'prod'):
        for items in item_sets:
            got = q.run('HIO', 'mask', kind=kind, items=items)
            best, best_rho = q.e.best_error()[0], q.e.density(True)
            want = RR.main_error(kind, items, got[4]['err'], got[4]['rl2'], got[4]['deg2'])         # numpy's function on the device's values
            assert np.isnan(got[4]['err']) and np.isnan(want) and np.isnan(got[4]['main']), (kind, items, got[4])
            assert best[4] == np.inf and np.array_equal(best_rho[4], q.rho_in[4], equal_nan=True)          # not "better": nothing was kept
            for b in range(B):
                if b != 4:
                    for k, v in got[b].items():
                        assert np.array_equal(v, clean[kind, tuple(items)][b][k]), (kind, items, b, k)
                    assert best[b] == got[b]['main']
    # a NaN behind finite values: order 2 of the deg2 reference (orders 0 .. 6 used, the odd ones have no norm: -1)
    ref, norms, w_l2 = q.metrics
    bad = ref.copy()
    bad[2, 1, 1] = np.nan
    q.metrics = (bad, norms, w_l2)
    for kind in ('mean', 'min', 'max', 'prod'):
        got = q.run('HIO', 'mask', kind=kind, items=['deg2_invariant_l2_diff'])
        for b in range(B):
            d2 = got[b]['deg2']
            assert np.isnan(d2[2]) and (b == 4 or (np.isfinite(d2[0]) and d2[1] == -1.0)), (b, d2)
            assert np.isnan(RR.KINDS[kind](d2)) and np.isnan(got[b]['main']), (kind, b, d2, got[b]['main'])
    q.close()


def check_schedule_nine_restarts(g, name, lib_path=None):
    """check_shadowed_schedule_2d with nine restarts (two groups, the second with one restart): its own bound, supports equal"""
    sh = check_shadowed_schedule_2d(g, name, lib_path, n_restarts=9)
    assert sh.e.B == 9 and sh.flips == 0
    return sh


def check_select_where_both_groups(g, lib_path=None, N=5, M=6, B=9):
    """select_best with a `where` mask that picks restarts of both groups (1, 7, 8 of nine), at a moment when every restart's best
    pair is NOT its latest one: the picked restarts take their best pair and support, the others keep theirs, bit for bit"""
    p = _StepProblem(g, lib_path, N, M, B)
    e = p.e
    p.prepare(True)
    e.run('ER', False, [0.5, 0.5], fetch=False)
    rng = np.random.default_rng(77)
    for b in range(B):
        e.set_support(b, rng.random(e.shape) > 0.7)                 # far fewer points allowed: the next step's error is larger
    e.run('HIO', p.mask, [0.5], fetch=False)
    main = e.fetch_main_errors(0, 3)
    assert (main[2] > main[:2].min(axis=0)).all(), main
    where = np.array([b in (1, 7, 8) for b in range(B)])
    before = (e.reciprocal_density(), e.density(), e.support())
    best = (e.reciprocal_density(True), e.density(True), e.support(True))
    assert all(not np.array_equal(before[1][b], best[1][b]) for b in range(B))
    assert np.array_equal(e.best_error()[0], main.min(axis=0))
    e.select_best(where)
    for a, b_, c in zip(before, best, (e.reciprocal_density(), e.density(), e.support())):
        assert np.array_equal(np.where(where[:, None, None], b_, a), c)
    err = e.run('ER', False, [0.5])                                  # and the loop goes on from the selected state (coefficients refreshed)
    assert np.isfinite(err).all()
    p.close()


def check_lds_limit(g, lib_path=None):
    """rows of 175 values (M = 87) need more LDS than the fused step kernels may take: the resident calls refuse with error -1 and launch
    nothing, the operator-level step of the same context still works; 173 values (M = 86) are accepted"""
    import resident2d_reference as RR
    rng = np.random.default_rng(8)

    def build(M):
        data, o = PC.mtip2d_scaled_problem(g, 4, M)
        o['projections']['reciprocal']['used_order_ids'] = np.arange(7)
        with _RecordedTables() as rec:
            m = MTIP2D(o, data, n_restarts=1, seeds=[4], lib_path=lib_path, resident=True)
        top = np.abs(m._initial_density(0)).max()
        rho = top * (rng.random(m.shape) - 0.3) + 0.01j * top * rng.standard_normal(m.shape)
        return m, m.engine, rec, rho, rng.random(m.shape) > 0.3
    m, e, rec, rho, sup = build(87)
    assert e.n_phi == 175
    launch_log(e)
    for call in (lambda: e.set_density(0, rho), lambda: e.set_initial_support(sup), lambda: e.set_support(0, sup)):
        try:
            call()
            raise AssertionError('no error')
        except MtipError as ex:
            assert 'error -1' in str(ex) and 'LDS' in str(ex), ex
    try:
        e.init_state()
        raise AssertionError('no error')
    except MtipError as ex:
        assert 'error -5' in str(ex), ex
    assert launch_log(e) in (None, ())
    t = rec.tables(e)
    for method in ('HIO', 'ER_non_FXS'):                                 # the operator-level step of this context is not concerned
        fxs = method == 'HIO'
        fixed = None if fxs else np.asarray(RR.modulus(1.5 * e.fourier_transform(rho)[0]), float)
        got = e.step(method, True, 0.5, rho, sup, fixed_intensity=fixed)
        ref = RR.step(t, method, True, 0.5, rho, sup, fixed)
        assert ref['err'] > 0 and (not fxs or ref['conditioning'].min() >= 1e-6)
        d = RR.step_distance(dict(F_new=got[0][0], rho_new=got[1][0], err=got[2][0], unknowns=got[3][0] if fxs else None), ref, fxs)
        print('4 x M87 operator-level', method, d)
        assert max(d.values()) <= BOUND_STEP, (method, d)
    m.close()
    m, e, rec, rho, sup = build(86)
    assert e.n_phi == 173
    e.set_density(0, rho)
    e.set_initial_support(sup)
    e.init_state()
    assert np.isfinite(e.run('HIO', True, [0.5])).all() and np.isfinite(e.density()).all()
    m.close()

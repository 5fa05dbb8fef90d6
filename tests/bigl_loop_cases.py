"""Cases of the phasing loop and the projection at band limits 64 <= L <= 128 (opt-in: GPU.big_l_loop / MTIP_CFG_LOOP_BIG_L; k_sht_big_fft_inv's
modulus epilogue with the slot-indirect output, the routes of plan_projection for orders with up to 257 rows), shared by
tests/test_emul_bigl_loop.py (CPU emulator) and tests/test_gpu_bigl_loop.py (MI355X).

Yardstick: the numpy oracle (oracle.mtip.MTIP; om.rp.approximate_unknowns / mtip_projection) with the project's tolerances -- projection
TOL_SHT = 1e-10 rel-L2 (parity_cases.check_projection_vs_oracle), densities of a short schedule 1e-9 rel-L2, supports equal, error series
rtol 1e-8 (parity_cases.check_split_shell_steps_vs_oracle).

The problems: synthetic invariants (xframe_amd.fxs.synthetic) made with the oracle's transforms on the angular grid of the case.  With the
250 A particle radius of the BASELINE configs a grid of 2 .. 6 shells has one shell inside the initial support, the real error metric
(evaluated inside it) is exactly zero in every step and a comparison of error series would compare zeros (with two shells the
synthetic particle even misses every grid point): here the particle, the support and the guess reach out to between two shells,
max(2, Nq / 2) of them inside, and every compared series is asserted to be non-zero.  With two to five shells the density of such
a problem is still positive everywhere inside the support (0.17 .. 0.47 after the first step in the oracle's runs), no constraint is
violated there and the metric stays zero: those problems also get an upper value bound that cuts through that range.  Below four
shells the cubic regridding of the invariants has too few nodes: those problems take the data grid itself (grid.max_q = the data's
cut-off) and linear regridding, which is then the identity.

problem() and check_loop_vs_oracle() also serve the default context below L = 64 (big_l = False: tests/sht_plan_cases.py, and the
problems of parity_cases.check_split_shell_steps_vs_oracle and chain_latency_cases.check_fused_steps_ft_stab)."""
import functools
import os

import numpy as np
import pytest

import bigl_cases as BC
import parity_cases as PC
from helpers import OracleTransforms, golden_settings, rel_l2
from oracle import mtip as OM
from oracle.fourier import FourierPair
from oracle.sht import SHT
from xframe_amd.fxs import _lib, hostsetup as hs, reconstruct as R, synthetic as S
from xframe_amd.fxs.engine import Engine, EngineGroup

# (Nq, L, n_theta, n_phi, n_batch): each the smallest shape that reaches one way to go wrong
SHAPE_LOOP = (6, 64, 66, 256, 2)        # Q = 12: a full block of 8 shells that straddles the two restarts and a tail of 4; 129 rows, 6 columns
SHAPE_ODD = (5, 65, 0, 0, 1)            # odd L on the default 128 x 256 grid
SHAPE_LIMIT = (3, 128, 130, 512, 1)     # the 512-point FFT (one row per pass), the limit, 257-row orders with 3 columns, a tail-only block
PROJ_SHAPES = ((80, 64, 66, 256, 2),    # columns up to 80 (beyond the 71 that fit LDS), 129 rows at l = 64
               (12, 100, 0, 0, 1))      # 201 rows with few columns: fits LDS, not the row slots of the LDS Jacobi
REAL_SHAPE = (48, 64, 66, 256, 2)       # used_order_ids = arange(20): the real-arithmetic route inside a big-L context
TUTORIAL_SHAPE = (128, 64, 0, 0, 2)     # reconstruct/tutorial.yaml: 128 shells, max_order 64 on its default grid, used_order_ids arange(64)
EMUL_LOOP = (2, 64, 66, 256, 1)
EMUL_LIMIT = (2, 128, 130, 512, 1)
BELOW = (4, 32, 0, 0, 2)
COLUMNS_SHAPE = (130, 64, 66, 256, 1)   # order 64 active with min(129, 130) = 129 columns: refused

VALUE_HI = 0.3                          # upper value bound of the problems with fewer than six shells (see the module docstring)
SCHEDULE = (2, True, 2)                 # HIO steps, shrink wrap, ER steps: 4 steps, the output slot wraps past the three history slots
SCHEDULE_SHORT = (1, False, 1)
TOL_DENSITY, RTOL_ERR = 1e-9, 1e-8
# the parent commit's messages, verbatim
MSG_LOOP = ('phasing loop: the phasing loop and the projection are built for max_order <= 63; this context has L = 64 and runs the '
            'transforms only (DESIGN section 6)')
MSG_CREATE = ('mtip_create: invalid cfg: need Nq>=2, 0<=L<=128 (the transforms; the phasing loop and the projection: L<=63), n_batch>=1, '
              'n_phi a power of two in [4,512] and > 2L, n_theta > L')
MSG_ENGINE = ('max_order = 64 with invariants: the phasing loop and the projection are built for max_order <= 63; beyond it (up to 128) '
              'an engine without data runs the transforms only (DESIGN section 6)')
MSG_FT_MASK = 'a per-restart ft_stab mask needs the fused one-pass step (cfg.fused, tiled Hankel kernel, real update in the SHT epilogue)'


# ------------------------------------------------------------------------------------------------------------------- problems
@functools.lru_cache(maxsize=None)
def problem(N, L, nt, nphi, n_used=None, *, big_l=True):
    """(invariants, settings) of one geometry, with GPU.big_l_loop unless big_l is False (the default context, for L <= 63:
    tests/sht_plan_cases.py); shared by the tests of a session and never modified"""
    fpd = FourierPair(SHT(L, nt, nphi), N, S.data_cutoff(N), 2.0)
    q_d = S.midpoint_points(S.data_cutoff(N), N)
    small = N < 4
    max_q = float(S.data_cutoff(N)) if small else False
    rs, _ = hs.radial_grids(max_q if small else float(np.max(q_d)), N, 2.0, 'midpoint')
    n_in = max(2, N // 2)
    radius = float((rs[n_in - 1] + rs[n_in]) / 2) if n_in < N else float(rs[-1] * 1.25)
    # synthetic.make_invariants with the particle scaled to that radius (its 250 A balls lie inside the first of two or three shells)
    tr = OracleTransforms(fpd)
    F = tr.ft(S.ball_density(tr.rs, tr.thetas, tr.phis, particle_radius=radius))
    data = S.invariants_from_intensity_coefficients(tr.forward_l(F * F.conj()), q_d, L, tr)
    opt = golden_settings(N, L, {
        'grid': {'n_theta': nt, 'n_phi': nphi, 'max_q': max_q}, 'particle_radius': radius, 'density_guess': {'radius': radius},
        'projections': {'reciprocal': {'regrid': {'interpolation': 'linear' if small else 'cubic'},
                                       'used_order_ids': np.arange(L + 1 if n_used is None else n_used)},
                        'real': {'projections': {'support': {'initial_support': {'max_radius': radius}},
                                                 'value_threshold': {'threshold': [0, VALUE_HI if N < 6 else False]}}}},
        'GPU': {'big_l_loop': bool(big_l)}})
    return data, opt


def with_schedule(opt, schedule, order=None, methods=None):
    n_hio, sw, n_er = schedule
    opt = OM.deep_update(opt, {})
    main = opt['main_loop']['sub_loops']['main']
    main['methods']['HIO']['iterations'] = n_hio
    main['methods']['ER']['iterations'] = n_er
    main['order'] = ['HIO', 'SW', 'ER'] if sw else ['HIO', 'ER']
    if methods is not None:
        main['methods'], main['order'] = methods, order
    main['iterations'] = 1
    return opt


@functools.lru_cache(maxsize=None)
def oracle_loop(shape4, schedule, seed, variant=None, big_l=True):
    """the oracle's phasing loop from its own seeded guess: computed once per session, shared, never modified"""
    data, opt = problem(*shape4, big_l=big_l)
    opt = with_schedule(opt, schedule, *(NON_FXS if variant == 'non_fxs' else ()))
    om = OM.MTIP(opt, data)
    rho0 = om.density_guess(np.random.default_rng(seed))
    return rho0, om.phasing_loop(rho0=rho0)


NON_FXS = (['HIO', 'HIO_non_FXS', 'ER_non_FXS', 'ER'],
           {'HIO': {'iterations': 1, 'ft_stab': True}, 'HIO_non_FXS': {'iterations': 1, 'ft_stab': True},
            'ER_non_FXS': {'iterations': 1, 'ft_stab': False}, 'ER': {'iterations': 1, 'ft_stab': True}})


def _n_steps(opt):
    main = opt['main_loop']['sub_loops']['main']
    return sum(main['methods'][k]['iterations'] for k in main['order'] if k != 'SW')


# --------------------------------------------------------------------------------------------- cases 1, 2, 3, 7, 9: the loop
def check_loop_vs_oracle(shape, schedule=SCHEDULE, lib_path=None, fused=True, seeds=(3, 4), variant=None, tag='', big_l=True,
                         before_run=None, after_run=None, figures=None):
    """a short schedule from seeded guesses (a different one per restart), every restart against its own oracle run: the real error
    series the engine records (mtip_fetch_errors) against the oracle's at rtol 1e-8, the four densities at 1e-9 rel-L2, equal
    supports; the compared series and the distance the density travelled are non-zero.  big_l = False: the default context (for
    L <= 63).  before_run / after_run are called with the engine in front of and behind the loop; the dict `figures` receives the
    largest deviations seen ('density', 'errors') before they are judged.  Returns the result dicts."""
    N, L, nt, nphi, B = shape
    data, opt = problem(N, L, nt, nphi, big_l=big_l)
    opt = with_schedule(opt, schedule, *(NON_FXS if variant == 'non_fxs' else ()))
    refs = [oracle_loop((N, L, nt, nphi), schedule, seeds[b], variant, big_l) for b in range(B)]
    R.MTIP.preinit(opt, data)
    m = R.MTIP(n_restarts=B, initial_densities=[r[0] for r in refs], lib_path=lib_path, fused=fused)
    m.generate_phasing_loop()
    assert m.engine.big_l_loop == big_l and m.engine.L == L
    if before_run is not None:
        before_run(m.engine)
    res = m.phasing_loop()
    n = _n_steps(opt)
    err = m.engine.fetch_errors(0, n)[0]
    if after_run is not None:
        after_run(m.engine)
    m.engine.close()
    for b in range(B):
        rho0, ref = refs[b]
        want = np.asarray(ref['error_dict']['real']['l2_projection_diff'])
        moved = rel_l2(res[b]['last_real_density'], rho0)
        dens = {k: rel_l2(res[b][k], ref[k]) for k in ('real_density', 'last_real_density', 'reciprocal_density', 'last_reciprocal_density')}
        if figures is not None:
            figures['density'] = max(figures.get('density', 0.0), max(dens.values()))
            figures['errors'] = max(figures.get('errors', 0.0), float((np.abs(err[:, b] - want)[want > 0] / want[want > 0]).max()))
        print(f'{tag}{shape} fused={fused} restart {b}: errors {err[:, b]} oracle {want} max rel dev {np.abs(err[:, b] - want).max() / want.max():.2e}; '
              f'densities {dens}; moved {moved:.3f}; support differs at {(res[b]["last_support_mask"] != ref["last_support_mask"]).sum()}')
        assert want.shape == (n,) and (want > 0).any() and np.isfinite(want).all(), want       # not zeros against zeros
        assert moved > 1e-3, moved
        assert np.allclose(err[:, b], want, rtol=RTOL_ERR, atol=0), (err[:, b], want)
        assert np.allclose(res[b]['error_dict']['main'], ref['error_dict']['main'], rtol=RTOL_ERR, atol=0)
        for k, d in dens.items():
            assert d < TOL_DENSITY, (k, d)
        assert (res[b]['last_support_mask'] != ref['last_support_mask']).sum() == 0
        assert (res[b]['support_mask'] != ref['support_mask']).sum() == 0
    if B > 1:
        assert rel_l2(res[0]['last_real_density'], res[1]['last_real_density']) > 1e-3          # the restarts are different runs
    return res


def run_tier0(out_path, lib_path=None):
    """case 7, child process with MTIP_SHT_TIER=0: the generic kernels (k_fft_inv<EPI_MODULUS> with slots) as the second implementation
    of case 1, same bounds against the oracle; the final densities go to out_path for the comparison with the default run"""
    assert os.environ.get('MTIP_SHT_TIER') == '0'
    res = check_loop_vs_oracle(SHAPE_LOOP, SCHEDULE, lib_path, fused=True, tag='tier 0 ')
    np.savez(out_path, **{f'rho{b}': r['last_real_density'] for b, r in enumerate(res)})
    print('BIGL loop tier0 ok')


def check_tier0_agrees(res_default, out_path):
    z = np.load(out_path)
    for b, r in enumerate(res_default):
        d = rel_l2(r['last_real_density'], z[f'rho{b}'])
        print(f'default tiers against tier 0, restart {b}: {d:.2e}')
        assert d < TOL_DENSITY, d


def run_guarded(lib_path):
    """child process with MTIP_EMUL_GUARD=1: every device allocation of the emulator ends at an inaccessible page"""
    check_loop_vs_oracle(EMUL_LOOP, SCHEDULE_SHORT, lib_path, fused=True, tag='guarded ')
    print('BIGL loop guarded ok')


# --------------------------------------------------------------------------------------------------- cases 4, 5: the projection
def check_projection(shape, lib_path=None, seed=1):
    """parity_cases.check_projection_vs_oracle on the case's grid with the flag: random coefficients, cold and warm call"""
    N, L, nt, nphi, B = shape
    data, opt = problem(N, L, nt, nphi)
    e = Engine(opt, data, n_batch=B, lib_path=lib_path)
    om = OM.MTIP(opt, data)
    Ilm = PC.cplx(np.random.default_rng(seed), (B, N, e.nlm))
    PC.launched_kernels(e, ('k_',))
    for rep in range(2):
        proj = e.project_coefficients(Ilm)
        for b in range(B):
            Il = [Ilm[b][:, l * l:(l + 1) ** 2] for l in range(L + 1)]
            ref = np.concatenate(om.rp.mtip_projection(Il, om.rp.approximate_unknowns(Il)), axis=1)
            d = rel_l2(proj[b], ref)
            print(f'projection {shape} call {rep} restart {b}: {d:.2e}')
            assert d < PC.TOL_SHT, (rep, b, d)
    launched = PC.launched_kernels(e, ('k_',))
    e.close()
    return launched


def check_projection_real(shape=REAL_SHAPE, n_used=20, lib_path=None, seed=1):
    """real V_l and the coefficients of a real intensity (parity_cases.check_projection_real_vs_oracle) in a context beyond L = 63
    whose solved orders stop at 18: k_rproj runs (its slots are reported, on the emulator it is in the launch log)"""
    N, L, nt, nphi, B = shape
    data, opt = problem(N, L, nt, nphi, n_used)
    assert all(np.all(np.asarray(p).imag == 0) for p in data['data_projection_matrices'])
    sht = SHT(L, nt, nphi)
    e = Engine(opt, data, n_batch=B, lib_path=lib_path)
    om = OM.MTIP(opt, data)
    rng = np.random.default_rng(seed)
    PC.launched_kernels(e, ('k_',))
    for rep in range(2):
        grid = rng.uniform(0.0, 1.0, (B, N, sht.n_theta, sht.n_phi)) * rng.uniform(0.5, 2.0, (B, N, 1, 1))
        Ilm = np.stack([np.concatenate(sht.forward_l(g.astype(complex)), axis=1) for g in grid])
        proj = e.project_coefficients(Ilm, real_intensity=True)
        assert e.projection_slots() > 0, 'the real-arithmetic projection was expected to run'
        for b in range(B):
            Il = [Ilm[b][:, l * l:(l + 1) ** 2] for l in range(L + 1)]
            ref = np.concatenate(om.rp.mtip_projection(Il, om.rp.approximate_unknowns(Il)), axis=1)
            d = rel_l2(proj[b], ref)
            worst = max(rel_l2(proj[b][:, l * l:(l + 1) ** 2], ref[:, l * l:(l + 1) ** 2]) for l in range(n_used))
            print(f'real projection {shape} call {rep} restart {b}: {d:.2e}, worst used order {worst:.2e}')
            assert d < PC.TOL_SHT and worst < PC.TOL_SHT, (rep, b, d, worst)
            assert np.array_equal(proj[b][:, n_used * n_used:], Ilm[b][:, n_used * n_used:])      # unused orders pass through
    launched = PC.launched_kernels(e, ('k_',))
    assert launched is None or ('k_rproj' in launched and 'k_polar_jacobi' not in launched), launched
    e.close()


# -------------------------------------------------------------------------------------------------------- case 6: the tutorial
def check_tutorial_shape(lib_path=None, shape=TUTORIAL_SHAPE, n_more=10):
    """reconstruct/tutorial.yaml's grid and orders (used_order_ids arange(64), the odd ones zero) plus GPU.big_l_loop through MTIP(...): one
    HIO and one ER step against the oracle, then n_more steps as properties -- finite, the ER error does not increase, the two restarts
    (equal guesses) stay bit-identical"""
    N, L, nt, nphi, B = shape
    data, opt = problem(N, L, nt, nphi, 64)
    assert opt['projections']['reciprocal']['odd_orders_to_0'] and len(opt['projections']['reciprocal']['used_order_ids']) == 64
    opt = with_schedule(opt, SCHEDULE_SHORT)
    rho0, ref = oracle_loop((N, L, nt, nphi, 64), SCHEDULE_SHORT, 3)
    R.MTIP.preinit(opt, data)
    m = R.MTIP(n_restarts=B, initial_densities=[rho0] * B, lib_path=lib_path)
    m.generate_phasing_loop()
    res = m.phasing_loop()
    e = m.engine
    err = e.fetch_errors(0, 2)[0]
    want = np.asarray(ref['error_dict']['real']['l2_projection_diff'])
    dens = {k: rel_l2(res[0][k], ref[k]) for k in ('last_real_density', 'last_reciprocal_density')}
    print(f'tutorial shape: errors {err[:, 0]} oracle {want}; densities {dens}; moved {rel_l2(res[0]["last_real_density"], rho0):.3f}')
    assert (want > 0).all() and np.allclose(err[:, 0], want, rtol=RTOL_ERR, atol=0), (err[:, 0], want)
    assert all(d < TOL_DENSITY for d in dens.values()), dens
    assert rel_l2(res[0]['last_real_density'], rho0) > 1e-3
    n_hio = n_more // 2
    eh, _ = e.run('HIO', True, np.full(n_hio, 0.45))
    ee, _ = e.run('ER', True, np.full(n_more - n_hio, 0.5))
    errs = np.concatenate([err, eh, ee])
    print('tutorial shape, ER errors:', ee[:, 0])
    assert np.isfinite(errs).all() and (errs > 0).all()
    assert (np.diff(ee[:, 0]) <= 1e-12 * ee[:-1, 0]).all(), ee[:, 0]
    assert np.array_equal(errs[:, 0], errs[:, 1])
    assert np.array_equal(e.density(0), e.density(1)) and np.isfinite(e.density(0)).all()
    assert np.array_equal(e.reciprocal_density(0), e.reciprocal_density(1))
    e.close()


# ----------------------------------------------------------------------------------------------------------- case 8: the group
def check_group_run_identical(shape=SHAPE_LOOP, lib_path=None, sizes=(2, 1), n_hio=2, n_er=2):
    """mtip_run_group_async with two L = 64 contexts is bit-identical to independent runs (parity_cases.check_group_run_identical_synthetic)"""
    N, L, nt, nphi, _ = shape
    data, opt = problem(N, L, nt, nphi)
    radius = opt['particle_radius']
    out = {}
    for mode in ('group', 'single'):
        engines = [Engine(opt, data, n_batch=b, lib_path=lib_path) for b in sizes]
        i = 0
        for e in engines:
            for b in range(e.B):
                e.set_density(b, hs.bump_density(e.rs, e.shape, radius, 0.3, 2, np.random.default_rng(1000 + i),
                                                 e.rsetup.integrated_intensity, e.int_wr, e.int_wt))
                i += 1
            e.init_state()
        grp = EngineGroup(engines)
        for kind, betas in (('HIO', np.full(n_hio, 0.45)), ('SW', None), ('ER', np.full(n_er, 0.5))):
            if kind == 'SW':
                for e in engines:
                    e.shrinkwrap(e.default_sigma, 0.09, 1e9)
            elif mode == 'group':
                grp.run(kind, True, betas)
            else:
                for e in engines:
                    e.run(kind, True, betas, fetch=False)
        if mode == 'group':
            assert grp.calls['group'] == 2
        out[mode] = [(e.fetch_errors(0, n_hio + n_er)[0], [e.density(b) for b in range(e.B)]) for e in engines]
        for e in engines:
            e.close()
    for (ea, da), (eb, db) in zip(out['group'], out['single']):
        print('group run, errors:', ea.T.tolist())
        assert np.array_equal(ea, eb), (ea, eb)
        assert np.isfinite(ea).all() and (ea >= 0).all() and (ea > 0).any(axis=0).all(), ea
        for x, y in zip(da, db):
            assert np.array_equal(x, y) and np.isfinite(x).all()


# ---------------------------------------------------------------------------------------------------------- case 10: the limits
def _transforms_engine(shape, lib_path, big_l_loop):
    N, L, nt, nphi, B = shape
    return Engine({'grid': {'n_radial_points': N, 'max_order': L, 'n_theta': nt, 'n_phi': nphi}}, None, n_batch=B, lib_path=lib_path,
                  max_q=1.0, big_l_loop=big_l_loop)


def _loop_calls(e):
    lib, ctx = e.lib, e.ctx
    keep = {'err': np.full(4, np.nan), 'deg2': np.full(4 * (e.L + 1), np.nan), 'beta': np.full(1, 0.5),
            'out': np.full((e.B, e.N, e.nlm), np.nan, complex), 'Ilm': _lib.as_c128(np.ones((e.B, e.N, e.nlm))),
            'V': _lib.as_c128(np.ones((e.N, 1))), 'mask': _lib.as_u8(np.ones(e.N))}
    calls = (('phasing loop', lambda: lib.mtip_run(ctx, 0, 0, 1, _lib.ptr(keep['beta']), _lib.ptr(keep['err']), _lib.ptr(keep['deg2']))),
             ('mtip_op_project_coefficients', lambda: lib.mtip_op_project_coefficients(ctx, _lib.ptr(keep['Ilm']), _lib.ptr(keep['out']))),
             ('mtip_op_project_real_intensity', lambda: lib.mtip_op_project_real_intensity(ctx, _lib.ptr(keep['Ilm']), _lib.ptr(keep['out']))),
             ('mtip_set_projection_matrix', lambda: lib.mtip_set_projection_matrix(ctx, 0, _lib.ptr(keep['V']), 1, _lib.ptr(keep['mask']), 1)))
    return calls, keep


def check_flag_lifts_the_limit(lib_path=None):
    """with the flag the four calls of bigl_cases.check_raises succeed or fail for their own reasons only, and nothing is launched by
    those that fail"""
    e = _transforms_engine((2, 64, 66, 256, 1), lib_path, True)
    calls, keep = _loop_calls(e)
    PC.launched_kernels(e, ('k_',))
    own = {'phasing loop': 'mtip_set_initial_support has not been called',
           'mtip_op_project_coefficients': 'mtip_set_projection_matrix missing for some order',
           'mtip_op_project_real_intensity': 'mtip_set_projection_matrix missing for some order', 'mtip_set_projection_matrix': None}
    for name, call in calls:
        rc = call()
        msg = e.lib.mtip_last_error(e.ctx).decode()
        if own[name] is None:
            assert rc == 0, (name, rc, msg)
        else:
            assert rc == -5 and msg == own[name], (name, rc, msg)
        assert 'max_order <= 63' not in msg or rc == 0
    assert np.isnan(keep['err']).all() and np.isnan(keep['out']).all()
    launched = PC.launched_kernels(e, ('k_',))
    assert launched is None or launched == (), launched
    e.close()
    try:
        Engine({'grid': {'n_radial_points': 2, 'max_order': 64}}, {'data_radial_points': np.arange(1.0, 3.0)}, lib_path=lib_path,
               big_l_loop=True)
        raised = None
    except Exception as ex:                                  # (an invariants dict without matrices: whatever it raises is its own)
        raised = ex
    assert not isinstance(raised, NotImplementedError) and 'max_order <= 63' not in str(raised), raised


def check_columns_refused(lib_path=None, shape=COLUMNS_SHAPE):
    """an active order with more than 128 columns (Nq = 130, order 64: min(129, 130) = 129): the projection operators and the loop
    return MTIP_ESTATE with the limit in the message, the NaN-prefilled outputs stay, nothing is launched"""
    e = _transforms_engine(shape, lib_path, True)
    N, L, lib, ctx = e.N, e.L, e.lib, e.ctx
    rng = np.random.default_rng(0)
    mask = _lib.as_u8(np.ones(N))
    for l in range(L + 1):
        if l == L:
            V = _lib.as_c128(rng.normal(size=(N, min(2 * l + 1, N))))
            e._ck(lib.mtip_set_projection_matrix(ctx, l, _lib.ptr(V), V.shape[1], _lib.ptr(mask), 1))
        else:
            e._ck(lib.mtip_set_projection_matrix(ctx, l, None, 1, None, 0))
    e._ck(lib.mtip_set_initial_support(ctx, _lib.ptr(_lib.as_u8(np.ones(e.shape)))))
    e._ck(lib.mtip_set_error_weights(ctx, _lib.ptr(np.ones(N)), _lib.ptr(np.ones(e.n_theta)), 0))
    calls, keep = _loop_calls(e)                              # (the check comes before the one for mtip_init_state)
    PC.launched_kernels(e, ('k_',))
    for name, call in calls[:3]:
        rc = call()
        msg = lib.mtip_last_error(ctx).decode()
        assert rc == -5 and name in msg and 'l = 64' in msg and '129 columns' in msg and 'at most 128 columns' in msg, (name, rc, msg)
    enforced = np.zeros(1, np.uint8)
    rc = lib.mtip_shrinkwrap(ctx, 1.0, 0.1, 1.0, _lib.ptr(enforced))
    assert rc == -5 and 'at most 128 columns' in lib.mtip_last_error(ctx).decode()
    assert np.isnan(keep['err']).all() and np.isnan(keep['deg2']).all() and np.isnan(keep['out']).all()
    launched = PC.launched_kernels(e, ('k_',))
    assert launched is None or launched == (), launched
    e.close()


def check_ft_mask_refused(lib_path=None, shape=EMUL_LOOP):
    """a per-restart ft_stab mask beyond L = 63 (no real update in the SHT epilogue there) is refused as everywhere else, before any launch"""
    N, L, nt, nphi, _ = shape
    data, opt = problem(N, L, nt, nphi)
    e = Engine(opt, data, n_batch=2, lib_path=lib_path)
    for b in range(2):
        e.set_density(b, np.ones(e.shape, complex))
    e.init_state()
    e.set_ft_stab_mask([True, False])
    PC.launched_kernels(e, ('k_',))
    beta = np.full(1, 0.5)
    rc = e.lib.mtip_run_async(e.ctx, 1, 1, 1, _lib.ptr(beta))
    msg = e.lib.mtip_last_error(e.ctx).decode()
    assert rc == -5 and msg == MSG_FT_MASK, (rc, msg)
    launched = PC.launched_kernels(e, ('k_',))
    assert launched is None or launched == (), launched
    e.close()


def check_reserved_bits(lib_path=None):
    """mtip_cfg.reserved is a flag word: any bit but MTIP_CFG_LOOP_BIG_L fails mtip_create, naming the field"""
    import ctypes as C
    lib = _lib.load(lib_path)
    assert _lib.MTIP_CFG_LOOP_BIG_L == 1
    for word in (2, 3, 1 << 30, -2):
        cfg = _lib.MtipCfg(2, 4, 8, 16, 1, 0, 1, word)
        ctx = lib.mtip_create(C.byref(cfg), 0)
        msg = lib.mtip_last_error(None).decode()
        assert not ctx and 'invalid cfg' in msg and 'reserved' in msg, (word, msg)
    for word in (0, 1):
        cfg = _lib.MtipCfg(2, 4, 8, 16, 1, 0, 1, word)
        ctx = lib.mtip_create(C.byref(cfg), 0)
        assert ctx, lib.mtip_last_error(None).decode()
        got = _lib.MtipCfg()
        assert lib.mtip_get_cfg(ctx, C.byref(got)) == 0 and got.reserved == word
        lib.mtip_destroy(ctx)


def check_default_unchanged(lib_path=None):
    """without the flag nothing changed: bigl_cases.check_raises as it stands, and the parent commit's messages verbatim"""
    BC.check_raises(lib_path)
    e = _transforms_engine((2, 64, 66, 256, 1), lib_path, None)
    assert not e.big_l_loop
    calls, _ = _loop_calls(e)
    assert calls[0][1]() == -5 and e.lib.mtip_last_error(e.ctx).decode() == MSG_LOOP
    for name, call in calls[1:]:
        assert call() == -5 and e.lib.mtip_last_error(e.ctx).decode() == MSG_LOOP.replace('phasing loop:', name + ':', 1)
    e.close()
    with pytest.raises(_lib.MtipError) as ei:
        Engine({'grid': {'n_radial_points': 2, 'max_order': 129}}, None, lib_path=lib_path, max_q=1.0)
    assert str(ei.value) == MSG_CREATE
    for kw in ({}, {'big_l_loop': False}):
        with pytest.raises(NotImplementedError) as ei:
            Engine({'grid': {'n_radial_points': 2, 'max_order': 64}}, {'data_radial_points': np.arange(1.0, 3.0)}, lib_path=lib_path, **kw)
        assert str(ei.value) == MSG_ENGINE
    from xframe_amd.fxs import settings as ST
    assert ST.resolve(None)['GPU']['big_l_loop'] is False


# ------------------------------------------------------------------------------------------- emulator only: the launch log
def check_step_kernels(lib_path, shape=EMUL_LOOP):
    """the FXS step beyond L = 63, from the launch log: the modulus stage is k_sht_big_fft_inv (F' written once, straight into the
    forward transform of F'), no separate modulus kernel, no generic FFT / Legendre kernel"""
    N, L, nt, nphi, B = shape
    data, opt = problem(N, L, nt, nphi)
    for fused in (True, False):
        e = Engine(opt, data, n_batch=B, lib_path=lib_path, fused=fused)
        e.set_density(0, np.ones(e.shape, complex))
        e.init_state()
        PC.launched_kernels(e, ('k_',))
        e.run('ER', True, [0.5], fetch=False)
        e.synchronize()
        log = PC.launched_kernels(e, ('k_',))
        e.close()
        assert log is not None
        big_f, big_i = ('k_sht_big_fft_fwd', 'k_sht_big_leg_fwd'), ('k_sht_big_leg_inv', 'k_sht_big_fft_inv')
        i = log.index('k_polar_jacobi')
        after = log[i + 1:]
        assert after[0] == 'k_proj_mfma' and after[1:5] == big_i + big_f, log            # apply, I' -> F' (modulus epilogue), SHT(F')
        assert 'k_modulus' not in log and not any(k in BC._GEN_F + BC._GEN_I for k in log), log
        assert log[:2] == big_f and log.count('k_real_update') == 1 and log[-1] == 'k_finish_step', log
        assert ('k_coeff_diff' in log) == fused, log


def check_below_unchanged(lib_path, shape=BELOW):
    """below L = 64 the flag has no effect: the transforms launch what bigl_cases.KERNELS_BELOW records for the commit before the
    big-L kernels, a step launches the same kernels with the flag as without, none of them a big-L kernel"""
    N, L, nt, nphi, B = shape
    data, opt = problem(N, L, nt, nphi)
    logs = {}
    for flag in (True, False):
        e = Engine(opt, data, n_batch=B, lib_path=lib_path, big_l_loop=flag)
        rng = np.random.default_rng(0)
        g, co = PC.cplx(rng, (B,) + e.shape), PC.cplx(rng, (B, N, e.nlm))
        seen = []
        PC.launched_kernels(e)
        e.sht_forward(g)
        seen.append(PC.launched_kernels(e))
        e.sht_inverse(co)
        seen.append(PC.launched_kernels(e))
        e.sht_inverse_forward(co, 0)
        seen.append(PC.launched_kernels(e))
        assert tuple(seen) == BC.KERNELS_BELOW[shape], seen
        for b in range(B):
            e.set_density(b, np.ones(e.shape, complex))
        e.init_state()
        PC.launched_kernels(e, ('k_',))
        e.run('HIO', True, [0.5, 0.5], fetch=False)
        e.shrinkwrap(e.default_sigma, 0.09, 1e9)
        e.run('ER', True, [0.5], fetch=False)
        e.synchronize()
        logs[flag] = PC.launched_kernels(e, ('k_',))
        e.close()
    assert logs[True] == logs[False] and len(logs[True]) > 6
    assert not any(k.startswith('k_sht_big') for k in logs[True]), logs[True]

"""Cases of the band limits 64 <= L <= 128 (csrc/k_sht_big.h, plan_sht, the loop's band limit in mtip_api.hip, Engine, simulate_ccd), shared by
tests/test_emul_bigl.py (CPU emulator) and tests/test_gpu_bigl.py (MI355X).

Yardsticks: the oracle (oracle.sht.SHT, oracle.fourier.FourierPair) through parity_cases.check_transforms with the project's tolerances
TOL_SHT = 1e-10 / TOL_OP = 1e-12 rel-L2 -- the oracle alone round-trips O(1) coefficients to 2e-11 .. 3e-11 max-abs on the default grids
at L = 64 .. 128 and its P_mm table agrees with the kernels' recurrence to 7e-15, the smallest |P_mm| (2.6e-260 at L = 128 on 256 x 512)
is a normal double -- and, for the flow, the same flow composed from the oracle and the numpy restatements of simulate_cases."""
import numpy as np
import pytest

import ccextract_cases as CC
import parity_cases as PC
import simulate_cases as SC
from helpers import rel_l2
from oracle.fourier import FourierPair
from oracle.sht import SHT
from xframe_amd.fxs import _lib, extract as X, io as IO, settings as ST, simulate_ccd as SIM
from xframe_amd.fxs.engine import Engine

# (N, L, n_theta, n_phi, n_batch): each the smallest shape that reaches one way for the kernels to go wrong
SHAPES = ((3, 64, 66, 256, 2),          # first L beyond the old limit; n_theta / 2 = 33 odd; two restarts
          (2, 85, 0, 0, 1),             # last L on the 128 x 256 grid; odd L: the parity classes of l - m are unequal
          (2, 86, 0, 0, 1),             # first L with the 512-point FFT
          (3, 97, 100, 512, 1),         # L + 1 - m and n_theta / 2 = 50 off every tile multiple
          (3, 128, 0, 0, 1),            # the limit on its default 256 x 512 grid
          (2, 128, 130, 512, 2))        # the limit with 65 theta pairs
SHAPE_WIDE = (130, 64, 66, 256, 1)      # GPU only: second Hankel row block at a large L, more than one column tile in the Legendre products
EMUL_SHAPES = ((2, 64, 66, 256, 1), (2, 128, 130, 512, 1))
FALLBACK_SHAPE = (3, 64, 66, 256, 2)    # with MTIP_SHT_TIER=0
ODD_SHAPE = (2, 64, 67, 256, 1)         # odd n_theta: no north/south pairs, the plan gives it the generic kernels
TALL_SHAPE = (2, 64, 260, 256, 1)       # 130 theta pairs: more than the synthesis holds (128), the plan gives it the generic kernels
BELOW = ((3, 63, 0, 0, 1), (4, 32, 0, 0, 2))

_BIG_F, _BIG_I = ('k_sht_big_fft_fwd', 'k_sht_big_leg_fwd'), ('k_sht_big_leg_inv', 'k_sht_big_fft_inv')
_GEN_F, _GEN_I = ('k_fft_fwd', 'k_leg_fwd'), ('k_leg_inv', 'k_fft_inv')
KERNELS_BIG = (_BIG_F, _BIG_I, _BIG_I + _BIG_F)
KERNELS_GENERIC = (_GEN_F, _GEN_I, _GEN_I + _GEN_F)
# what the commit before these kernels launches below the limit (its own launch log on the emulator): 128 x 256 grid at L = 63 (the
# spectra of a shell do not fit the wide kernel's LDS: the Stockham tier), 64 x 128 at L = 32
KERNELS_BELOW = {(3, 63, 0, 0, 1): (('k_sht_fwd_fused',), ('k_sht_inv_fused',), ('k_sht_inv_fused', 'k_sht_fwd_fused')),
                 (4, 32, 0, 0, 2): (('k_sht_fwd_pair',), ('k_sht_inv_wide',), ('k_sht_chain',))}

FLOW64 = {'grid': {'max_q': False, 'oversampling': 4, 'max_order': 64, 'n_theta': 66, 'n_phi': 256, 'n_radial_points': 6},
          'shapes': SC.FLOW['shapes'], 'cross_correlation': {'method': 'back_substitution'}}
FLOW128 = {**FLOW64, 'grid': {**FLOW64['grid'], 'max_order': 128, 'n_theta': 130, 'n_phi': 512, 'n_radial_points': 4}}
LIMIT = r'max_order <= 63'


def check_operators(shape, lib_path=None, expect_kernels=None):
    """case 1 (and 2): every transform operator against the oracle at one geometry"""
    N, L, nt, nphi, B = shape
    PC.check_transforms(N, L, lib_path, n_theta=nt, n_phi=nphi, n_batch=B, expect_kernels=expect_kernels)


def run_guarded(lib_path):
    """child process with MTIP_EMUL_GUARD=1: every device allocation of the emulator ends at an inaccessible page"""
    check_operators(EMUL_SHAPES[0], lib_path, KERNELS_BIG)
    print('BIGL guarded ok')


def run_fallback(lib_path=None):
    """child process with MTIP_SHT_TIER=0: the generic kernels as the independent second implementation"""
    check_operators(FALLBACK_SHAPE, lib_path, KERNELS_GENERIC)
    print('BIGL fallback ok')


def oracle_flow(settings):
    """the flow of simulate_ccd composed from the oracle: FT -> |.|^2 -> SHT -> I_l I_l^+ -> back substitution (numpy restatement)"""
    opt = ST.resolve_simulate_ccd(settings)
    max_q, n, _ = SIM.simulation_grid(opt)
    g = opt['grid']
    L = int(g['max_order'])
    sht = SHT(L, g['n_theta'], g['n_phi'])
    fp = FourierPair(sht, n, max_q, float(ST.reciprocity_coefficient(opt['fourier_transform'])), 'midpoint')
    density = SIM.shape_density(fp.grid.real_grid(), opt['shapes'])
    F = fp.ft(density.astype(complex))
    Ilm = sht.forward_d(F * F.conj())
    bl = np.stack([Ilm[:, l * l:(l + 1) ** 2] @ Ilm[:, l * l:(l + 1) ** 2].conj().T for l in range(L + 1)])
    return {'density': density, 'qs': fp.qs, 'bl': bl, 'cc': SC.r_back_substitution(bl, fp.qs),
            'average_intensity': np.sqrt(np.diag(bl[0]).real / (4 * np.pi))}


def check_flow(settings, lib_path=None, through_extract=True):
    """case 4: simulate_ccd beyond L = 63 against oracle_flow (B_l, cc, average_intensity <= 1e-10 rel-L2, the keys of
    simulate_cases.check_flow); then its cc_data through io.load_ccd and extract_from_cross_correlation: the even orders of B_l come
    back within 1e-10 (the numpy restatements alone: 1.3e-15 at 6 x L64, so the bound catches a wrong order or sign and rounding
    cannot trip it).  through_extract False (max_order 128): extract's kernel takes at most 64 orders, L = 128 has 65 even ones."""
    res = SIM.simulate_ccd(settings, lib_path=lib_path)
    ref = oracle_flow(settings)
    cc_data = res.cc_data
    L = int(settings['grid']['max_order'])
    assert set(cc_data) == {'radial_points', 'angular_points', 'xray_wavelength', 'cross_correlation', 'average_intensity',
                            'deg_2_invariant', 'number_of_particles'}
    assert np.array_equal(res.density, ref['density']) and 0 < np.count_nonzero(res.density) < res.density.size
    assert np.array_equal(cc_data['angular_points'], np.arange(2 * L) * np.pi / L)
    bl, cc = cc_data['deg_2_invariant']['I1I1'], cc_data['cross_correlation']['I1I1']
    for name, got, want, tol in (('B_l', bl, ref['bl'], SC.TOL_FT), ('cc', cc, ref['cc'], SC.TOL_FT),
                                 ('average_intensity', cc_data['average_intensity'], ref['average_intensity'], SC.TOL_FT),
                                 ('radial_points', cc_data['radial_points'], ref['qs'], 1e-15)):
        d = rel_l2(got, want)
        print(f'flow L{L} {name}: {d:.2e}')
        assert np.shape(got) == np.shape(want) and d <= tol, (name, d)
    if not through_extract:
        return
    e = CC.small_engine(lib_path)
    ccd = IO.load_ccd(cc_data, 'direct')
    data = X.extract_from_cross_correlation(e, ccd, CC.flow_settings(L, CC.MASK_CASES['none'], modify_cc={}, enforce_psd=False))
    e.close()
    back = np.asarray(data['b_coeff']['I1I1'])
    assert back.shape == bl.shape, (back.shape, bl.shape)
    d = rel_l2(back[::2], bl[::2])
    print(f'flow L{L} round trip through extract, even orders: {d:.2e}')
    assert d <= 1e-10, d


def check_raises(lib_path=None):
    """case 5: the limits.  On a transforms-only L = 64 context the loop's entry points return the state error with the limit in the
    message, leave their NaN-prefilled outputs alone and launch nothing"""
    grid = {'n_radial_points': 2, 'max_order': 129}
    with pytest.raises(_lib.MtipError, match=r'mtip_create: invalid cfg.*0<=L<=128'):
        Engine({'grid': grid}, None, lib_path=lib_path, max_q=1.0)
    with pytest.raises(NotImplementedError, match=LIMIT + r'.*DESIGN section 6'):
        Engine({'grid': {**grid, 'max_order': 64}}, {'data_radial_points': np.arange(1.0, 3.0)}, lib_path=lib_path)
    e = Engine({'grid': {'n_radial_points': 2, 'max_order': 64, 'n_theta': 66, 'n_phi': 256}}, None, lib_path=lib_path, max_q=1.0)
    lib, ctx = e.lib, e.ctx
    PC.launched_kernels(e, ('k_',))
    err, deg2 = np.full(4, np.nan), np.full(4 * 65, np.nan)
    beta = np.full(1, 0.5)
    out = np.full((1, 2, e.nlm), np.nan, complex)
    Ilm = _lib.as_c128(np.ones((1, 2, e.nlm)))
    V = _lib.as_c128(np.ones((2, 1)))
    mask = _lib.as_u8(np.ones(2))
    calls = (('phasing loop', lambda: lib.mtip_run(ctx, 0, 0, 1, _lib.ptr(beta), _lib.ptr(err), _lib.ptr(deg2))),
             ('mtip_op_project_coefficients', lambda: lib.mtip_op_project_coefficients(ctx, _lib.ptr(Ilm), _lib.ptr(out))),
             ('mtip_op_project_real_intensity', lambda: lib.mtip_op_project_real_intensity(ctx, _lib.ptr(Ilm), _lib.ptr(out))),
             ('mtip_set_projection_matrix', lambda: lib.mtip_set_projection_matrix(ctx, 0, _lib.ptr(V), 1, _lib.ptr(mask), 1)))
    for name, call in calls:
        rc = call()
        msg = lib.mtip_last_error(ctx).decode()
        assert rc == -5 and name in msg and 'max_order <= 63' in msg and 'L = 64' in msg, (name, rc, msg)
    assert np.isnan(err).all() and np.isnan(deg2).all() and np.isnan(out).all()
    launched = PC.launched_kernels(e, ('k_',))
    assert launched is None or launched == (), launched
    e.close()

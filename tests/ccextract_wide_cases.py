"""Cases of cross-correlation -> B_l beyond 64 extracted orders (mtip_op_cc_to_deg2_wide, k_cc_deg2<HM> in csrc/k_extract.hip,
Engine.cc_to_deg2(wide=True), fxs/extract.py), shared by tests/test_emul_ccextract_wide.py (CPU emulator) and
tests/test_gpu_ccextract_wide.py (MI355X).

Yardsticks: the numpy restatement of tests/ccextract_cases.py (held to the reference's own outputs, G24, by a CPU test) with its
two bounds -- whole array TOL_OP = 1e-12, per order ORDER_MARGIN x (rfft route against direct-sum route of the restatement), floor
1e-12, the input rejected above ORDER_CAP = 1e-5 -- and tests/ccmask_cases.py's restatement of prepare + back-substitution for the
masked case.  Inputs: ccextract_cases.synthetic_cc, seed 24, noise 1e-4, default decay; the reference side alone gives per-order
bounds <= 4e-11 at every shape of SHAPES."""
import functools

import numpy as np
import pytest

import ccextract_cases as CC
import ccmask_cases as CM
import parity_cases as PC
from helpers import rel_l2
from xframe_amd.fxs import _lib, extract as X, io as IO

SEED = 24
# (n_q, max_order, n_delta, assume_zero_odd_orders): each the smallest shape that reaches one way for the slots to go wrong
SHAPES = ((17, 128, 256, True),         # 65 orders, HM = 2, one harmonic in slot 1; half fold, nfold = 65: a full chunk + a tail of 1; a
                                        # second workgroup with a tail of one pair
          (17, 128, 256, False),        # 129 orders, HM = 3, slot 2 holds one harmonic; m = 128 is the Nyquist term of n = 256
          (33, 127, 300, False),        # 128 orders: two exactly full slots; three workgroups in x
          (17, 64, 131, False),         # the first count beyond the narrow entry at stride 1; odd n_delta, no fold
          (5, 128, 2100, False),        # twiddle table beyond 1024 entries: read from global memory; n_q below one pair block
          (5, 128, 2100, True))
EMUL_SHAPES = (SHAPES[0], SHAPES[3], SHAPES[5])
SAME_KERNEL_SHAPES = ((17, 126, 256, True), (18, 20, 50, False))      # 64 and 21 orders: both entries launch the HM = 1 kernel
MODIFY_ALL = {'subtract_average_intensity': True, 'pi_periodicity': True, 'q1q2_symmetric': True}
DIM2_SHAPE = (5, 128, 257)
TOL_DIM2 = 1e-12
FLOW_SHAPE = (12, 128, 256)             # shells, max_order, angles of the synthetic flows
# relative deviation of the HIO step's error metric, data through extract against data built from the original B_l: the numpy
# restatement through the same flow gives LOOP_RESTATEMENT (see check_into_loop); the bound is ORDER_MARGIN x that, floor 1e-9
LOOP_RESTATEMENT = 3.765e-8
LOOP_BOUND = max(CC.ORDER_MARGIN * LOOP_RESTATEMENT, 1e-9)


@functools.lru_cache(maxsize=None)
def reference(nq, L, n_delta, zero_odd):
    """(qs, phis, cc, avg, restatement, its two-route deviation, per-order bound) of one shape: computed once, shared, never modified"""
    stride = 2 if zero_odd else 1
    qs, phis, cc, avg, _ = CC.synthetic_cc(nq, L, n_delta, SEED, stride, noise=1e-4)
    ref, dev, bound = CC.order_bounds(cc, qs, phis, L, zero_odd, avg)
    for a in (qs, phis, cc, avg, ref, dev, bound):
        a.setflags(write=False)
    return qs, phis, cc, avg, ref, dev, bound


def _compare(tag, b, ref, dev, bound, L, stride):
    whole = rel_l2(b, ref)
    per = np.array([rel_l2(b[l], ref[l]) for l in range(L + 1)])
    sel = np.arange(0, L + 1, stride)
    print(f'{tag}: whole {whole:.2e}; reference-side deviation max {dev[sel].max():.2e} at l = {sel[dev[sel].argmax()]}; device max '
          f'{per[sel].max():.2e} at l = {sel[per[sel].argmax()]}; worst ratio to bound {(per[sel] / bound[sel]).max():.2e}; '
          f'max bound {bound[sel].max():.2e}')
    assert b.shape == ref.shape and b.dtype == np.complex128
    assert whole <= CC.TOL_OP, whole
    assert (per[sel] <= bound[sel]).all(), (per[sel], bound[sel])
    if stride == 2:
        assert not np.any(b[1::2])


def check_operator(lib_path, nq, L, n_delta, zero_odd):
    """Engine.cc_to_deg2(wide=True) against the restatement: whole array <= 1e-12, every extracted order within its bound"""
    stride = 2 if zero_odd else 1
    qs, phis, cc, avg, ref, dev, bound = reference(nq, L, n_delta, zero_odd)
    e = CC.small_engine(lib_path)
    b = e.cc_to_deg2(cc, L, stride, 3, legendre=X.legendre_table(qs, CC.WAVELENGTH, L, stride), wide=True)
    e.close()
    _compare(f'wide operator {nq} x L{L} x {n_delta} stride {stride} ({L // stride + 1} orders)', b, ref, dev, bound, L, stride)


def check_dim2(lib_path):
    """dimensions = 2, 129 harmonics at stride 1, odd n_delta: B_m = C_m against the restatement.  The input is white (every harmonic
    has the size n^-1/2 of the samples), so a harmonic of any slot that is wrong shows in the whole-array figure, and each harmonic
    is held to the same 1e-12 on its own: 257 products of O(1) samples and O(1) twiddles round to at most 257 eps = 6e-14 of the
    samples, 1e-12 of a harmonic of size 1 / 16"""
    nq, L, nd = DIM2_SHAPE
    rng = np.random.default_rng(SEED)
    cc = rng.standard_normal((nq, nq, nd))
    qs, phis = CC.radial_points(nq), np.arange(nd) * 2 * np.pi / nd
    ref, _ = CC.r_cc_to_deg2(cc, 2, qs, phis, L, False, {}, None)
    e = CC.small_engine(lib_path)
    b = e.cc_to_deg2(cc, L, 1, 2, wide=True)
    e.close()
    per = np.array([rel_l2(b[m], ref[m]) for m in range(L + 1)])
    print(f'wide dim 2 {nq} x {L + 1} harmonics x {nd}: whole {rel_l2(b, ref):.2e}, worst harmonic {per.max():.2e} at m = {per.argmax()}')
    assert b.shape == (L + 1, nq, nq) and rel_l2(b, ref) <= TOL_DIM2 and (per <= TOL_DIM2).all(), per


def check_modify_flags(lib_path, shape=SHAPES[0]):
    """the three modify_cc switches together at 65 orders, against r_modify + the restatement (the bounds from the modified data)"""
    nq, L, nd, zero_odd = shape
    stride = 2 if zero_odd else 1
    qs, phis, cc, avg, _, _, _ = reference(*shape)
    mod_cc = CC.r_modify(cc, phis, avg, MODIFY_ALL)
    ref, dev, bound = CC.order_bounds(mod_cc, qs, phis, L, zero_odd, avg)
    e = CC.small_engine(lib_path)
    b, qq = X.cross_correlation_to_deg2_invariant(e, cc.copy(), 3, **CC.metadata(qs, phis, L, zero_odd, MODIFY_ALL, avg))
    e.close()
    assert qq.all() and qq.shape == (nq, nq)
    _compare(f'wide operator, modify_cc all, {nq} x L{L} x {nd}', b, ref, dev, bound, L, stride)


def check_same_kernel(lib_path):
    """up to 64 extracted orders the wide entry launches the kernel of the narrow one: equal bits, and (emulator) the same launch log"""
    e = CC.small_engine(lib_path)
    for nq, L, nd, zero_odd in SAME_KERNEL_SHAPES:
        stride = 2 if zero_odd else 1
        qs, phis, cc, avg, _ = CC.synthetic_cc(nq, L, nd, SEED, stride, noise=1e-4)
        leg = X.legendre_table(qs, CC.WAVELENGTH, L, stride)
        out, logs = [], []
        for wide in (False, True):
            PC.launched_kernels(e, ('k_',))
            out.append(e.cc_to_deg2(cc, L, stride, 3, legendre=leg, wide=wide))
            logs.append(PC.launched_kernels(e, ('k_',)))
        assert np.array_equal(out[0], out[1]) and np.any(out[0][L - L % stride]), (nq, L, nd)
        assert all(log is None or log == ('k_cc_deg2',) for log in logs), logs
        ref, _ = CC.r_cc_to_deg2(cc, 3, qs, phis, L, zero_odd, {}, avg)
        assert rel_l2(out[1], ref) <= CC.TOL_OP
    e.close()


def check_limits(lib_path):
    """beyond max_order 128 the wide entry returns an error code with the entry, its limits and the values in the message and leaves
    the NaN-prefilled output alone; at the limit a NaN-prefilled output comes back finite, the odd orders exactly zero; one launch"""
    e = CC.small_engine(lib_path)
    nq = 5
    out = np.full((130, nq, nq), np.nan, complex)
    small = _lib.as_f64(np.zeros((nq, nq, 260)))
    leg = _lib.as_f64(np.zeros((nq, 130 * 131 // 2)))
    for args, words in (((nq, 260, 129, 1, 3, 0), ('max_order', '129', '128')), ((nq, 260, 129, 2, 2, 0), ('max_order', '129')),
                        ((nq, 200, 128, 1, 3, 0), ('n_delta', '200')), ((5000, 260, 128, 1, 3, 0), ('n_q', '5000')),
                        ((nq, 5000, 128, 2, 3, 0), ('n_delta', '5000'))):
        rc = e.lib.mtip_op_cc_to_deg2_wide(e.ctx, *args, _lib.ptr(small), None, None, _lib.ptr(leg), _lib.ptr(out))
        msg = e.lib.mtip_last_error(e.ctx).decode()
        assert rc != 0 and 'cc_to_deg2_wide' in msg and all(w in msg for w in words), (args, rc, msg)
        assert np.isnan(out).all()
    L, nd = 128, 256
    qs, phis, cc, avg, _ = CC.synthetic_cc(nq, L, nd, SEED, 2, noise=1e-4)
    legc, ccc = _lib.as_f64(X.legendre_table(qs, CC.WAVELENGTH, L, 2)), _lib.as_f64(cc)
    out = np.full((L + 1, nq, nq), np.nan, complex)
    PC.launched_kernels(e, ('k_',))
    rc = e.lib.mtip_op_cc_to_deg2_wide(e.ctx, nq, nd, L, 2, 3, 0, _lib.ptr(ccc), None, None, _lib.ptr(legc), _lib.ptr(out))
    log = PC.launched_kernels(e, ('k_',))
    assert rc == 0, e.lib.mtip_last_error(e.ctx).decode()
    assert np.isfinite(out).all() and not np.any(out[1::2]) and np.any(out[0]) and np.any(out[128])
    assert log is None or log == ('k_cc_deg2',), log
    ref, _ = CC.r_cc_to_deg2(cc, 3, qs, phis, L, True, {}, avg)
    assert rel_l2(out, ref) <= CC.TOL_OP
    # the narrow entry keeps its refusal (ccextract_cases.check_raises pins its message)
    with pytest.raises(_lib.MtipError, match='at most 64 extracted orders'):
        e.cc_to_deg2(cc, L, 2, 3, legendre=legc)
    e.close()


def check_masked_back_substitution(lib_path, nq=9, L=128, nd=256):
    """65 orders through masked_cross_correlation_to_deg2_invariant with a direct mask that removes interior samples: against
    ccmask_cases' restatement of the interpolation followed by the restatement of the back-substitution, at that module's tolerance"""
    qs, phis, cc, avg, _ = CC.synthetic_cc(nq, L, nd, SEED, 2, noise=1e-4)
    mask = CM.direct_mask(nq, nd)
    assert 0 < np.count_nonzero(~mask.all(-1)) and mask[0, 0, 0] and mask[0, 0, -1]
    meta = CM.metadata(qs, phis, L, True, {}, avg, {'type': 'direct', 'direct': {'mask': mask.copy()}}, 'back_substitution')
    e = CC.small_engine(lib_path)
    b, qq = X.masked_cross_correlation_to_deg2_invariant(e, cc.copy(), 3, **meta)
    e.close()
    cc2, _ = CM.r_modify_masked(cc, mask, phis, avg, {'interpolate_masked': True})
    ref, _ = CC.r_cc_to_deg2(cc2, 3, qs, phis, L, True, {}, avg)
    err = rel_l2(b, ref)
    print(f'masked back substitution at 65 orders vs restatement: {err:.2e}')
    assert b.shape == ref.shape and err <= CM.TOL_OP and qq.all() and not np.any(b[1::2]) and np.any(b[128])


def _ccd(qs, phis, cc, avg):
    return IO.load_ccd({'cross_correlation': {'I1I1': cc.copy()}, 'radial_points': qs, 'angular_points': phis, 'average_intensity': avg,
                        'xray_wavelength': CC.WAVELENGTH})


def check_lstsq_refused(lib_path, nq=5, L=128, nd=256):
    """bl_extraction_method lstsq at 65 orders: the flow surfaces the refusal of mtip_op_cc_lstsq_deg2 and nothing else"""
    qs, phis, cc, avg, _ = CC.synthetic_cc(nq, L, nd, SEED, 2)
    s = CC.flow_settings(L, CC.MASK_CASES['none'], modify_cc={}, enforce_psd=False)
    s['cross_correlation']['datasets']['I1I1']['bl_extraction_method'] = 'lstsq'
    e = CC.small_engine(lib_path)
    with pytest.raises(_lib.MtipError, match='cc_lstsq_deg2.*at most 64 extracted orders'):
        X.extract_from_cross_correlation(e, _ccd(qs, phis, cc, avg), s)
    e.close()


def check_flow_simulated(lib_path=None):
    """simulate_ccd at 4 x L128 through io.load_ccd and extract_from_cross_correlation: bigl_cases.check_flow with the extract half
    switched on (its 1e-10 whole-array bound is dominated by B_0: it proves the wiring, the per-order cases prove the arithmetic)"""
    import bigl_cases as BC
    BC.check_flow(BC.FLOW128, lib_path, through_extract=True)


@functools.lru_cache(maxsize=None)
def flow_inputs():
    nq, L, nd = FLOW_SHAPE
    qs = CC.radial_points(nq)
    bl = CC.synthetic_bl(nq, L, SEED, stride=2)
    cc = CC.cc_from_bl(bl, qs, nd, 2)
    phis = np.arange(nd) * 2 * np.pi / nd
    avg = np.sqrt(np.abs(np.diagonal(bl[0]))) / np.sqrt(4 * np.pi)
    for a in (qs, bl, cc, phis, avg):
        a.setflags(write=False)
    return qs, phis, cc, avg, bl


def flow_synthetic(e):
    """(data dict of extract_from_cross_correlation, projection matrices of the original B_l) of the 12 x L128 synthetic flow"""
    qs, phis, cc, avg, bl = flow_inputs()
    L = FLOW_SHAPE[1]
    data = X.extract_from_cross_correlation(e, _ccd(qs, phis, cc, avg), CC.flow_settings(L, CC.MASK_CASES['none'], modify_cc={},
                                                                                         enforce_psd=False))
    ref_pm, _ = X.deg2_invariant_to_projection_matrices(e, bl.astype(complex))
    return data, ref_pm


def check_flow_synthetic(lib_path=None):
    """synthetic B_l (12 shells, max_order 128, even orders) -> C with 256 angles -> load_ccd -> extract_from_cross_correlation:
    V_l V_l^+ against deg2_invariant_to_projection_matrices on the original B_l <= TOL_FLOW |B|, shapes (12, min(2l+1, 12)), the keys
    `reconstruct` reads; the same with dimensions 2 at 129 harmonics"""
    nq, L, nd = FLOW_SHAPE
    bl = flow_inputs()[4]
    e = CC.small_engine(lib_path)
    data, ref_pm = flow_synthetic(e)
    for k in CC.RECONSTRUCT_KEYS:
        assert k in data, k
    assert data['max_order'] == L and data['dimensions'] == 3 and len(data['data_projection_matrices']) == L + 1
    worst = 0.0
    for l in range(L + 1):
        a, b = data['data_projection_matrices'][l], ref_pm[l]
        assert a.shape == b.shape == (nq, min(2 * l + 1, nq)), (l, a.shape, b.shape)
        worst = max(worst, np.linalg.norm(a @ a.conj().T - b @ b.conj().T) / np.linalg.norm(bl))
    print(f'synthetic flow {nq} x L{L} x {nd}: V V^+ worst {worst:.2e}')
    assert worst <= CC.TOL_FLOW, worst
    # (V_l of the highest orders are zero in both: |B_l| falls below numpy.isclose's 1e-8, fxs_invariant_tools.py:1123-1130)
    assert np.any(data['b_coeff']['I1I1'][128]) and not np.any(data['b_coeff']['I1I1'][127])
    # dimensions 2: 129 plain Fourier harmonics B_n (real, positive semi-definite), n_delta = 258
    nd2 = 258
    qs = CC.radial_points(nq)
    bn = CC.synthetic_bl(nq, L, SEED + 2, stride=1)
    ccn = np.zeros((nq, nq, nd2 // 2 + 1), complex)
    ccn[..., :L + 1] = np.moveaxis(bn, 0, -1)
    cc2 = np.fft.irfft(ccn * nd2, nd2, axis=-1)
    avg = np.sqrt(np.abs(np.diagonal(bn[0])))
    s = CC.flow_settings(L, CC.MASK_CASES['none'], modify_cc={}, enforce_psd=False, dimensions=2)
    s['cross_correlation']['datasets']['I1I1']['assume_zero_odd_orders'] = False
    data2 = X.extract_from_cross_correlation(e, _ccd(qs, np.arange(nd2) * 2 * np.pi / nd2, cc2, avg), s)
    ref2, _ = X.deg2_invariant_to_projection_matrices_2d(e, bn.astype(complex))
    e.close()
    pms = data2['data_projection_matrices']
    assert data2['max_order'] == L and data2['dimensions'] == 2 and isinstance(pms, np.ndarray) and pms.shape == (L + 1, nq)
    worst = max(np.linalg.norm(np.outer(pms[n], pms[n].conj()) - np.outer(ref2[n], ref2[n].conj())) for n in range(L + 1)) / np.linalg.norm(bn)
    back = rel_l2(data2['b_coeff']['I1I1'], bn)
    print(f'synthetic flow, dimensions 2, {nq} x {L + 1} harmonics x {nd2}: v v^+ worst {worst:.2e}, B_n {back:.2e}')
    assert worst <= CC.TOL_FLOW and back <= CC.TOL_FLOW, (worst, back)
    assert np.any(data2['b_coeff']['I1I1'][128]) and np.any(data2['b_coeff']['I1I1'][127])


def loop_settings():
    from helpers import golden_settings
    nq, L, _ = FLOW_SHAPE
    opt = golden_settings(nq, L, {'grid': {'n_theta': 130, 'n_phi': 512}, 'GPU': {'big_l_loop': True}})
    main = opt['main_loop']['sub_loops']['main']
    main['methods'] = {'HIO': dict(main['methods']['HIO'], iterations=1)}
    main['order'] = ['HIO']
    main['iterations'] = 1
    return opt


def direct_data(data, ref_pm):
    """the dict of the flow with the projection matrices of the original B_l in place of the extracted ones"""
    direct = dict(data)
    direct['data_projection_matrices'] = np.empty(len(ref_pm), dtype=object)
    for l, m in enumerate(ref_pm):
        direct['data_projection_matrices'][l] = m
    low = np.empty(len(data['data_low_resolution_intensity_coefficients']), dtype=object)
    for l in range(len(low)):
        low[l] = ref_pm[l]
    direct['data_low_resolution_intensity_coefficients'] = low
    return direct


def check_into_loop(lib_path=None):
    """the dict of the synthetic flow through MTIP.preinit into MTIP(n_restarts=1, big_l_loop=True) on the 12 x L128 grid (130 x 512
    angles): one HIO step from a stored guess, its error metric against the same step on the dict built from the original B_l.

    What the deviation measures is how well double precision recovers B_l from C, not the device: the numpy restatement
    (ccextract_cases.r_cc_to_deg2, rfft route) pushed through the same flow on the CPU -- its B_l through
    deg2_invariant_to_projection_matrices, one HIO step of the oracle -- deviates by LOOP_RESTATEMENT = 3.765e-8 (error metric
    0.21951583 on the direct data; the restatement fed with direct-sum harmonics: 6.9e-8; the kernel's B_l from the CPU emulator
    through the same oracle step: 1.3e-7); the bound is ORDER_MARGIN = 10 x that (a third summation order: the kernel's), floor
    1e-9: 3.8e-7.  The restatement's deviation is below 1e-6, so the input keeps ccextract_cases.synthetic_bl's default decay."""
    from oracle import mtip as OM
    from xframe_amd.fxs import reconstruct as R
    e = CC.small_engine(lib_path)
    data1, ref_pm = flow_synthetic(e)
    e.close()
    direct = direct_data(data1, ref_pm)
    opt = loop_settings()
    rho0 = OM.MTIP(opt, direct).density_guess(np.random.default_rng(3))
    errs = []
    for data in (direct, data1):
        R.MTIP.preinit(opt, data)
        m = R.MTIP(n_restarts=1, initial_densities=[rho0], lib_path=lib_path, big_l_loop=True)
        m.generate_phasing_loop()
        assert m.engine.big_l_loop and m.engine.L == FLOW_SHAPE[1]
        errs.append(np.asarray(m.phasing_loop()[0]['error_dict']['main'], dtype=float))
        m.engine.close()
    dev = np.abs(errs[1] / errs[0] - 1).max()
    print(f'into the loop: error metric {errs[0]} vs {errs[1]}, relative deviation {dev:.2e} (bound {LOOP_BOUND:.1e})')
    assert len(errs[0]) == len(errs[1]) == 1 and np.isfinite(errs[0]).all() and (errs[0] > 0).all()
    assert dev <= LOOP_BOUND, dev


# (l, m) and q of the table entries held to mpmath: the corners and the middle of the triangle beyond the orders G24 reaches
LEGENDRE_LM = ((128, 128), (128, 0), (128, 64), (127, 127), (127, 1), (65, 64), (64, 64), (100, 37))
LEGENDRE_QS = (0.01, 0.3, 0.9)


def check_legendre_table():
    """extract.legendre_table up to order 128 against mpmath at 60 digits: sqrt((2l+1)/(4 pi) (l-m)!/(l+m)!) P_l^m(x) (Ferrers
    function, Condon-Shortley phase: gsl_sf_legendre_sphPlm), relative error <= 1e-13 (measured 7.7e-15)"""
    import mpmath as mp
    mp.mp.dps = 60
    qs = np.array(LEGENDRE_QS)
    tab = X.legendre_table(qs, CC.WAVELENGTH, 128, 1)
    assert tab.shape == (3, 129 * 130 // 2)
    worst = 0.0
    for iq, q in enumerate(qs):
        x = mp.mpf(float(np.cos(np.arccos(q * CC.WAVELENGTH / (4 * np.pi)))))
        for l, m in LEGENDRE_LM:
            want = mp.sqrt(mp.mpf(2 * l + 1) / (4 * mp.pi) * mp.factorial(l - m) / mp.factorial(l + m)) * mp.legenp(l, m, x, type=2)
            got = tab[iq, l * (l + 1) // 2 + m]
            err = abs(float((mp.mpf(float(got)) - want) / want))
            worst = max(worst, err)
            assert err <= 1e-13, (q, l, m, got, float(want), err)
    print(f'legendre_table vs mpmath: worst relative error {worst:.2e}')

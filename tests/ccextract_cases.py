"""Cases of the route cross-correlation -> B_l -> V_l (csrc/k_extract.hip, Engine.cc_to_deg2, fxs/extract.py), shared by
tests/test_emul_ccextract.py (CPU emulator, toy sizes) and tests/test_gpu_ccextract.py (MI355X).

Two yardsticks:
  * G24 (tests/golden/cc_extract.npz): outputs of the reference's own functions at 16 shells x L = 8 x 64 angles;
  * for sizes the fixture cannot hold, the numpy restatement of the route below (each function cites its reference lines); a CPU test
    holds it to G24.
Every input has max(q) lambda / 4 pi <= 0.1: the triangular system of the back-substitution is only well conditioned for small-angle
geometry."""
import os

import numpy as np

import parity_cases as PC
from helpers import rel_l2
from xframe_amd.fxs import _lib, extract as X, hostsetup as hs, io as IO
from xframe_amd.fxs.engine import Engine

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'cc_extract.npz')
WAVELENGTH = 1.23984
TOL_OP = 1e-12                    # whole-array operator tolerance (parity_cases.TOL_SHT's decade; the CPU floor is 1e-14 here)
TOL_FLOW = 1e-10                  # what G15 holds `extract` to: eigenvectors are compared through V V^+
ORDER_MARGIN, ORDER_FLOOR, ORDER_CAP = 10.0, 1e-12, 1e-5

# name -> (cc key, dim, assume_zero_odd_orders, modify_cc)
VARIANTS = {
    's2': ('cc', 3, True, {}),
    's1': ('cc', 3, False, {}),
    'sub': ('cc', 3, True, {'subtract_average_intensity': True}),
    'pi': ('cc', 3, True, {'pi_periodicity': True}),
    'sym': ('cc', 3, True, {'q1q2_symmetric': True}),
    'all': ('cc', 3, True, {'subtract_average_intensity': True, 'pi_periodicity': True, 'q1q2_symmetric': True}),
    'all_s1': ('cc', 3, False, {'subtract_average_intensity': True, 'pi_periodicity': True, 'q1q2_symmetric': True}),
    'odd_n': ('cc_odd', 3, True, {'subtract_average_intensity': True, 'q1q2_symmetric': True}),
    'odd_n_s1': ('cc_odd', 3, False, {}),
    'dim2': ('cc', 2, True, {}),
    'dim2_s1': ('cc', 2, False, {'subtract_average_intensity': True}),
}
MASK_CASES = {
    'none': {'min': {'type': 'none'}, 'max': {'type': 'none'}},
    'line1': {'min': {'type': 'line', 'line': [[0, 0.02], [8, 0.3]]}, 'max': {'type': 'none'}},
    'line2': {'min': {'type': 'line', 'line': ([[0, 0.02], [8, 0.3]], [[0, 0.04], [8, 0.2]])},
              'max': {'type': 'line', 'line': ([[0, 0.7], [8, 0.9]], [[0, 0.75], [8, 0.85]])}},
}
FLOW_MODIFY = {'subtract_average_intensity': True, 'pi_periodicity': False, 'q1q2_symmetric': False}


def small_engine(lib_path=None):
    """an engine whose own grid does not matter: the extract operators take their sizes as arguments"""
    return Engine({'grid': {'n_radial_points': 8, 'max_order': 2}}, None, n_batch=1, lib_path=lib_path, max_q=1.0)


def radial_points(nq, q_max=0.9):
    return (np.arange(nq) + 0.5) * (q_max / nq)


def metadata(qs, phis, max_order, zero_odd, modify_cc, avg, mode='back_substitution'):
    """what the worker hands to cross_correlation_to_deg2_invariant (extract.py:134)"""
    thetas = np.arccos(qs * WAVELENGTH / (4 * np.pi))
    return {'data_grid': {'qs': qs, 'thetas': thetas, 'phis': phis.copy()}, 'orders': np.arange(max_order + 1), 'mode': mode,
            'assume_zero_odd_orders': zero_odd, 'modify_cc': dict(modify_cc), 'cc_mask': {'type': 'none'}, 'xray_wavelength': WAVELENGTH,
            'average_intensity': avg}


# ---- numpy restatement of the route ---------------------------------------------------------------------------------------------------
def legendre_products(qs, l, stride):
    """ccd_associated_legendre_matrices_single_l(thetas, l, l)[..., ::stride] (fxs_invariant_tools.py:60-74, 630): (q, q', m)"""
    x = np.cos(np.arccos(qs * WAVELENGTH / (4 * np.pi)))                         # 602, 65
    p = hs.sph_plm(l, np.arange(l + 1)[None, :], x[:, None])
    return (p[None, :, :] * p[:, None, :] / (2 * l + 1))[..., ::stride]


def r_modify(cc, phis, avg, modify_cc):
    """modify_cross_correlation (fxs_invariant_tools.py:235-289), unmasked data, the three switches in its order"""
    cc = np.array(cc, dtype=float)
    if modify_cc.get('subtract_average_intensity', False):                       # 245-247
        cc -= avg[:, None, None] * avg[None, :, None]
    if modify_cc.get('pi_periodicity', False):                                   # 264-269
        assert cc.shape[-1] % 2 == 0
        bad = (phis < np.pi / 2) | (phis >= 3 * np.pi / 2)
        cc[..., bad] = 0
        cc += np.roll(cc, len(phis) // 2, axis=-1)
    if modify_cc.get('q1q2_symmetric', False):                                   # 271-279 (masked_mean of two unmasked arrays)
        sw = cc.copy()
        sw[..., 1:] = cc[..., 1:][..., ::-1]
        cc = (np.swapaxes(sw, 0, 1) + cc) / 2
    return cc


def r_harmonics(cc, n_orders, route='rfft'):
    """circularHarmonicTransform_real_forward (mathLibrary.py:484-490): rfft / n; route 'direct': the same sums as a plain table
    contraction (another summation order: the yardstick of the per-order bound)"""
    n = cc.shape[-1]
    if route == 'rfft':
        return np.fft.rfft(cc, axis=-1)[..., :n_orders] / n
    k = (np.arange(n_orders)[:, None] * np.arange(n)[None, :]) % n
    cos, sin = np.cos(2 * np.pi * k / n).T.copy(), np.sin(2 * np.pi * k / n).T.copy()
    flat = cc.reshape(-1, n)
    out = np.empty((flat.shape[0], n_orders), dtype=complex)
    for i in range(0, flat.shape[0], 16384):                                     # (in pieces: the table product of a 2 GB array)
        out[i:i + 16384] = (flat[i:i + 16384] @ cos - 1j * (flat[i:i + 16384] @ sin)) / n
    return out.reshape(cc.shape[:-1] + (n_orders,))


def r_back_substitution(ccn, qs, max_order, stride):
    """the loop of fxs_invariant_tools.py:622-632 on the harmonics m = 0, stride, .. of all pairs; returns (Nq, Nq, n_m)"""
    ccn = np.array(ccn[..., :max_order + 1:stride], dtype=complex)
    bl = np.zeros(ccn.shape, dtype=complex)
    for l in range(0, max_order + 1, stride)[::-1]:
        col = legendre_products(qs, l, stride)
        bl[..., l // stride] = ccn[..., -1] / col[..., -1]
        ccn = ccn[..., :-1] - bl[..., l // stride, None] * col[..., :-1]
    return bl


def r_cc_to_deg2(cc, dim, qs, phis, max_order, zero_odd, modify_cc, avg, route='rfft'):
    """cross_correlation_to_deg2_invariant (fxs_invariant_tools.py:374-422) for unmasked data and mode back_substitution:
    (b_coeff (max_order + 1, Nq, Nq), qq_mask)"""
    cc = r_modify(cc, phis, avg, modify_cc)
    stride = 2 if zero_odd else 1
    sel = np.arange(0, max_order + 1, stride)
    ccn = r_harmonics(cc, max_order + 1, route)
    b = np.zeros(cc.shape[:2] + (max_order + 1,), dtype=complex)
    if dim == 2:
        b[..., sel] = ccn[..., sel]                                              # 813-839: B_m = C_m
    else:
        b[..., sel] = r_back_substitution(ccn, qs, int(sel.max()), stride)
    return np.moveaxis(b, -1, 0), np.ones(cc.shape[:2], dtype=bool)


# ---- synthetic data ---------------------------------------------------------------------------------------------------------------------
def synthetic_bl(nq, max_order, seed, decay=0.3, stride=2):
    """seeded positive semi-definite B_l (rank min(2l+1, nq)) with a spectrum that falls as exp(-decay l), as measured data does"""
    rng = np.random.default_rng(seed)
    qs = radial_points(nq)
    b = np.zeros((max_order + 1, nq, nq))
    env = np.exp(-qs / qs.max())
    for l in range(0, max_order + 1, stride):
        a = rng.normal(size=(nq, min(2 * l + 1, nq))) * env[:, None]
        b[l] = a @ a.T * np.exp(-decay * l) / a.shape[1]
    return b


def cc_from_bl(bl, qs, n_delta, stride=2):
    """C(q1, q2, Delta) = irfft(n C_m), C_m = sum_l B_l c_l^m (the relation the back-substitution inverts, fxs_invariant_tools.py:582)"""
    max_order = len(bl) - 1
    ccn = np.zeros(bl.shape[1:] + (n_delta // 2 + 1,), dtype=complex)
    for l in range(0, max_order + 1, stride):
        if np.any(bl[l]):
            col = legendre_products(qs, l, 1)
            ccn[..., :l + 1] += bl[l][..., None] * col
    return np.fft.irfft(ccn * n_delta, n_delta, axis=-1)


def synthetic_cc(nq, max_order, n_delta, seed, stride=2, noise=0.0, decay=0.3):
    qs = radial_points(nq)
    bl = synthetic_bl(nq, max_order, seed, decay, stride)
    cc = cc_from_bl(bl, qs, n_delta, stride)
    rng = np.random.default_rng(seed + 1)
    if noise:
        cc = cc + noise * np.abs(cc).max() * rng.normal(size=cc.shape)
    avg = np.sqrt(np.abs(np.diagonal(bl[0]))) * (1 + 0.1 * rng.random(nq)) / np.sqrt(4 * np.pi)
    return qs, np.arange(n_delta) * 2 * np.pi / n_delta, cc, avg, bl


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def load_golden():
    return np.load(GOLDEN)


def check_restatement_golden(g):
    """the numpy restatement against the reference's own functions (G24): 0.0 .. 1e-15 whole-array"""
    L = int(g['G24_L'])
    worst = 0.0
    for name, (key, dim, zero_odd, mod) in VARIANTS.items():
        cc = g['G24_' + key]
        phis = np.arange(cc.shape[-1]) * 2 * np.pi / cc.shape[-1]
        b, m = r_cc_to_deg2(cc, dim, g['G24_qs'], phis, L, zero_odd, mod, g['G24_avg'])
        d = rel_l2(b, g[f'G24_{name}_b'])
        worst = max(worst, d)
        print(f'restatement vs G24 {name}: {d:.2e}')
        assert d <= 1e-15, (name, d)
        assert np.array_equal(m, g[f'G24_{name}_qq_mask'])
    return worst


def check_operator_golden(g, lib_path=None):
    """case 1: every variant of G24 through cross_correlation_to_deg2_invariant on the device; b_coeff whole-array rel-L2 <= 1e-12,
    qq_mask equal, the assumed-zero odd orders exactly zero"""
    e = small_engine(lib_path)
    L = int(g['G24_L'])
    for name, (key, dim, zero_odd, mod) in VARIANTS.items():
        cc = g['G24_' + key]
        phis = np.arange(cc.shape[-1]) * 2 * np.pi / cc.shape[-1]
        b, m = X.cross_correlation_to_deg2_invariant(e, cc.copy(), dim, **metadata(g['G24_qs'], phis, L, zero_odd, mod, g['G24_avg']))
        ref = g[f'G24_{name}_b']
        d = rel_l2(b, ref)
        print(f'operator vs G24 {name}: {d:.2e}')
        assert b.shape == ref.shape and b.dtype == np.complex128
        assert d <= TOL_OP, (name, d)
        assert np.array_equal(m, g[f'G24_{name}_qq_mask']) and m.dtype == bool
        if zero_odd:
            assert not np.any(b[1::2])
    e.close()


def order_bounds(cc, qs, phis, L, zero_odd, avg):
    """per-order bound from the reference side alone: the restatement fed with rfft harmonics against the restatement fed with
    direct-sum harmonics, times ORDER_MARGIN (a third summation order: the kernel's), floor ORDER_FLOOR; above ORDER_CAP the input is
    too ill-conditioned to test anything"""
    a, _ = r_cc_to_deg2(cc, 3, qs, phis, L, zero_odd, {}, avg, 'rfft')
    b, _ = r_cc_to_deg2(cc, 3, qs, phis, L, zero_odd, {}, avg, 'direct')
    dev = np.array([rel_l2(b[l], a[l]) for l in range(L + 1)])
    bound = np.maximum(ORDER_MARGIN * dev, ORDER_FLOOR)
    assert bound.max() <= ORDER_CAP, 'input too ill-conditioned: per-order bound %.2e at l = %d' % (bound.max(), int(bound.argmax()))
    return a, dev, bound


def check_operator_restatement(lib_path, nq, L, n_delta, zero_odd=True, seed=24, on_device_tensor=False):
    """case 2: the operator against the restatement at sizes the fixture cannot hold; whole array <= 1e-12, per order the bound of
    order_bounds"""
    stride = 2 if zero_odd else 1
    qs, phis, cc, avg, _ = synthetic_cc(nq, L, n_delta, seed, stride, noise=1e-4)
    ref, dev, bound = order_bounds(cc, qs, phis, L, zero_odd, avg)
    e = small_engine(lib_path)
    leg = X.legendre_table(qs, WAVELENGTH, L, stride)
    if on_device_tensor:
        import torch
        b = e.cc_to_deg2(torch.from_numpy(cc).to(f'cuda:{e.device_index}'), L, stride, 3, legendre=leg).cpu().numpy()
    else:
        b = e.cc_to_deg2(cc, L, stride, 3, legendre=leg)
    e.close()
    whole = rel_l2(b, ref)
    per = np.array([rel_l2(b[l], ref[l]) for l in range(L + 1)])
    sel = np.arange(0, L + 1, stride)
    print(f'operator vs restatement {nq} x L{L} x {n_delta} stride {stride}: whole {whole:.2e}; reference-side deviation max '
          f'{dev[sel].max():.2e} at l = {sel[dev[sel].argmax()]}; device max {per[sel].max():.2e} at l = {sel[per[sel].argmax()]}; '
          f'worst ratio to bound {(per[sel] / bound[sel]).max():.2e}')
    assert whole <= TOL_OP, whole
    assert (per[sel] <= bound[sel]).all(), (per[sel], bound[sel])
    if zero_odd:
        assert not np.any(b[1::2])
    return whole, dev, per


def flow_settings(max_order, bl_q_limits, modify_cc=None, enforce_psd=True, **top):
    s = {'dimensions': 3, 'max_order': max_order, 'bl_eig_sort_mode': 'eigenvalues', 'extraction_mode': 'cross_correlation',
         'optimize_projection_matrices': {'use': False}, 'low_resolution_intensity_approximation': {'max_order': 4},
         'cross_correlation': {'datasets_to_process': ['I1I1'], 'datasets': {'I1I1': {
             'bl_extraction_method': 'back_substitution', 'assume_zero_odd_orders': True, 'cc_mask': {'type': 'none'},
             'modify_cc': dict(FLOW_MODIFY if modify_cc is None else modify_cc), 'bl_enforce_psd': enforce_psd,
             'bl_q_limits': bl_q_limits, 'masked_values_to_zero': False}}}}
    s.update(top)
    return s


def golden_ccd(g):
    cc = g['G24_cc']
    phis = np.arange(cc.shape[-1]) * 2 * np.pi / cc.shape[-1]
    return IO.load_ccd({'cross_correlation': {'I1I1': cc.copy()}, 'radial_points': g['G24_qs'], 'angular_points': phis,
                        'average_intensity': g['G24_avg'], 'xray_wavelength': WAVELENGTH})


RECONSTRUCT_KEYS = ('dimensions', 'xray_wavelength', 'average_intensity', 'data_radial_points', 'data_angular_points', 'max_order',
                    'data_projection_matrices', 'data_projection_matrices_q_id_limits', 'data_low_resolution_intensity_coefficients')


def check_flow_golden(g, lib_path=None):
    """case 3: masks and q_id_limits of every MASK_CASES entry against InvariantExtractor.calc_deg_2_invariant_masks (equal);
    extract_from_cross_correlation on G24's data against the reference's chain (constraints, B_0 replacement, projection matrices
    through V V^+, error estimate) <= 1e-10; the keys `reconstruct` reads"""
    L, nq = int(g['G24_L']), len(g['G24_qs'])
    for name, lim in MASK_CASES.items():
        mask, ids = X.calc_deg_2_invariant_masks({'bl_q_limits': lim}, (L + 1, nq, nq), np.ones((nq, nq), bool), g['G24_qs'], L)
        assert np.array_equal(mask, g[f'G24_mask_{name}']), name
        assert np.array_equal(ids, g[f'G24_qid_{name}']), name
    e = small_engine(lib_path)
    for name in ('none', 'line1'):
        data = X.extract_from_cross_correlation(e, golden_ccd(g), flow_settings(L, MASK_CASES[name]))
        for k in RECONSTRUCT_KEYS:
            assert k in data, k
        assert np.array_equal(data['deg_2_invariant_masks']['I1I1'], g[f'G24_mask_{name}'])
        assert np.array_equal(data['deg_2_invariant_q_id_limits']['I1I1'], g[f'G24_qid_{name}'])
        assert np.array_equal(data['data_projection_matrices_q_id_limits']['I1I1'], g[f'G24_qid_{name}'][:, 0])
        d = rel_l2(data['deg_2_invariant']['I1I1'], g[f'G24_flow_{name}_b'])
        print(f'flow {name}: constrained B_l {d:.2e}')
        assert d <= TOL_FLOW, (name, d)
        pms = data['data_projection_matrices']
        assert len(pms) == L + 1 and len(data['data_low_resolution_intensity_coefficients']) == 5
        for l in range(L + 1):
            ref = g[f'G24_flow_{name}_pm{l}']
            assert pms[l].shape == ref.shape, (l, pms[l].shape, ref.shape)
            vv, rr = pms[l] @ pms[l].conj().T, ref @ ref.conj().T
            scale = max(np.linalg.norm(g[f'G24_flow_{name}_b'][l]), 1e-300)
            assert np.linalg.norm(vv - rr) <= TOL_FLOW * scale, (name, l, np.linalg.norm(vv - rr) / scale)
        assert np.isclose(data['integrated_intensity'], float(g['G24_integrated_intensity']), rtol=1e-13)
        assert data['max_order'] == L and data['dimensions'] == 3
    e.close()


def check_end_to_end(lib_path, N, L, n_delta=None):
    """case 4: B_l of the benchmark's synthetic density -> synthetic C -> extract_from_cross_correlation -> V_l V_l^+ against
    deg2_invariant_to_projection_matrices on the original B_l (<= 1e-10); then MTIP.preinit takes the dict and a run of one HIO step
    from a stored initial density gives the error metric of the run on the direct data to a relative 1e-7.

    What that last figure measures is the data, not the device.  The benchmark's B_l fall steeply (|B_32| / |B_0| = 9e-11 at
    128 x L32), so any double-precision route recovers the high orders from C only to 1e-7 .. 2e-6 of themselves, and the error metric
    sees it.  Measured on an MI355X at 128 x L32, relative deviation of the HIO step's metric from the run on the direct data:
        n_delta = 136 (4 L + 8):  device 1.4e-7,  the reference's rfft route (numpy restatement) through the same flow 1.2e-7,
                                  a direct-sum DFT in numpy 1.5e-7   -- the reference's own route misses the bound there;
        n_delta = 1024:           device 5.2e-8,  rfft route 5.0e-8,  direct-sum DFT in numpy 1.2e-7.
    (More angles average the rounding of C itself.)  n_delta is therefore the tutorial's 1024 on the GPU, where the reference's own
    route is below the bound; the emulator's 32 x L8 gives 2e-9 at 4 L + 8 angles.  B_l rounded differently at
    1e-15 (another eigensolver call on the same matrices) moves the metric by 2e-10."""
    from helpers import golden_settings
    from oracle import mtip as OM
    from xframe_amd.fxs import reconstruct as R, synthetic as S
    n_delta = n_delta or 4 * L + 8
    data0, _ = PC.synthetic_problem(1, lib_path, N, L)
    te = small_engine(lib_path)
    bl = np.array([np.asarray(p) @ np.asarray(p).conj().T for p in data0['data_projection_matrices']]).real
    bl[1::2] = 0                                                                  # (an intensity has no odd orders: rounding residue)
    qs = np.asarray(data0['data_radial_points'], dtype=float)
    assert qs.max() * WAVELENGTH / (4 * np.pi) <= 0.1
    cc = cc_from_bl(bl, qs, n_delta, 2)
    phis = np.arange(n_delta) * 2 * np.pi / n_delta
    ccd = IO.load_ccd({'cross_correlation': {'I1I1': cc}, 'radial_points': qs, 'angular_points': phis,
                       'average_intensity': np.asarray(data0['average_intensity'], dtype=float), 'xray_wavelength': WAVELENGTH})
    data1 = X.extract_from_cross_correlation(te, ccd, flow_settings(L, MASK_CASES['none'], modify_cc={}, enforce_psd=False))
    ref_pm, _ = X.deg2_invariant_to_projection_matrices(te, bl.astype(complex))
    te.close()
    worst = 0.0
    for l in range(L + 1):
        a, b = data1['data_projection_matrices'][l], ref_pm[l]
        assert a.shape == b.shape
        worst = max(worst, np.linalg.norm(a @ a.conj().T - b @ b.conj().T) / np.linalg.norm(bl))
    print(f'end to end {N} x L{L} x {n_delta}: V V^+ worst {worst:.2e}')
    assert worst <= TOL_FLOW, worst
    # the reconstruct worker takes the dict
    opt = golden_settings(N, L)
    main = opt['main_loop']['sub_loops']['main']
    main['methods'] = {'HIO': dict(main['methods']['HIO'], iterations=1)}
    main['order'] = ['HIO']
    main['iterations'] = 1
    direct = dict(data0)
    direct['data_projection_matrices'] = np.empty(L + 1, dtype=object)
    for l in range(L + 1):
        direct['data_projection_matrices'][l] = ref_pm[l]
    rho0 = OM.MTIP(opt, direct).density_guess(np.random.default_rng(3))
    errs = []
    for data in (direct, data1):
        R.MTIP.preinit(opt, data)
        m = R.MTIP(n_restarts=1, initial_densities=[rho0], lib_path=lib_path)
        m.generate_phasing_loop()
        errs.append(np.asarray(m.phasing_loop()[0]['error_dict']['main'], dtype=float))
        m.engine.close()
    dev = np.abs(errs[1] / errs[0] - 1).max()
    print(f'end to end: error metric {errs[0]} vs {errs[1]}, relative deviation {dev:.2e}')
    assert len(errs[0]) == len(errs[1]) == 1 and dev <= 1e-7, dev


def check_raises(g, lib_path=None):
    """case 5: everything the reference offers and this route does not build raises NotImplementedError; sizes beyond the kernel's
    limits come back as an error code with a message"""
    import pytest
    e = small_engine(lib_path)
    L, qs, avg = int(g['G24_L']), g['G24_qs'], g['G24_avg']
    cc = g['G24_cc']
    phis = np.arange(cc.shape[-1]) * 2 * np.pi / cc.shape[-1]

    def meta(**kw):
        m = metadata(qs, phis, L, True, {}, avg)
        m.update(kw)
        return m
    for mode in ('lstsq', 'legendre', 'back_substitution_psd', 'back_substitution_qqsym', 'back_substitution_memory_hungry'):
        with pytest.raises(NotImplementedError, match=mode):
            X.cross_correlation_to_deg2_invariant(e, cc, 3, **meta(mode=mode))
    with pytest.raises(NotImplementedError, match='is unknown. Known modes are'):
        X.cross_correlation_to_deg2_invariant(e, cc, 3, **meta(mode='legendre_approx'))
    for t in ('pixel_arc', 'pixel_custom', 'custom'):
        with pytest.raises(NotImplementedError, match='cc_mask'):
            X.cross_correlation_to_deg2_invariant(e, cc, 3, **meta(cc_mask={'type': t}))
    for key, val in (('interpolate_masked', True), ('apply_binned_mean', True), ('low_pass_order_in_q', 3), ('enforce_max_order', True),
                     ('enforce_zero_odd_harmonics', True)):
        with pytest.raises(NotImplementedError, match=key):
            X.cross_correlation_to_deg2_invariant(e, cc, 3, **meta(modify_cc={key: val}))
    with pytest.raises(ValueError):                                               # n_delta < 2 max_order
        X.cross_correlation_to_deg2_invariant(e, cc[..., :14].copy(), 3, **metadata(qs, phis[:14], L, True, {}, avg))
    ccd = golden_ccd(g)
    ccd['cross_correlation']['I2I2'] = cc
    s = flow_settings(L, MASK_CASES['none'])
    s['cross_correlation']['datasets']['I2I2'] = s['cross_correlation']['datasets']['I1I1']
    s['cross_correlation']['datasets_to_process'] = ['I1I1', 'I2I2']
    with pytest.raises(NotImplementedError, match='I2I2'):
        X.extract_from_cross_correlation(e, ccd, s)
    with pytest.raises(NotImplementedError, match='optimize_projection_matrices'):
        X.extract_from_cross_correlation(e, golden_ccd(g), flow_settings(L, MASK_CASES['none'], optimize_projection_matrices={'use': True}))
    # the kernel's limits: an error code and a message, never values
    out = np.full((3, 2, 2), np.nan, complex)
    small = _lib.as_f64(np.zeros((2, 2, 8)))
    leg = _lib.as_f64(np.zeros((2, 3)))
    for args, word in (((2, 8, 2, 3, 3, 0), 'stride'), ((2, 8, 6, 2, 3, 0), 'n_delta'), ((5000, 8, 2, 2, 3, 0), 'n_q'),
                       ((2, 5000, 2, 2, 3, 0), 'n_delta'), ((2, 8, 2, 2, 3, 8), 'flag'), ((2, 7, 2, 2, 3, 2), 'pi_periodicity')):
        rc = e.lib.mtip_op_cc_to_deg2(e.ctx, *args, _lib.ptr(small), _lib.ptr(small), _lib.ptr(small.view(np.uint8)), _lib.ptr(leg),
                                      _lib.ptr(out))
        msg = e.lib.mtip_last_error(e.ctx).decode()
        assert rc != 0 and 'cc_to_deg2' in msg and word in msg, (args, rc, msg)
        assert np.isnan(out).all()
    with pytest.raises(_lib.MtipError, match='extracted orders'):                 # 65 orders at stride 1
        e.cc_to_deg2(np.zeros((2, 2, 130)), 64, 1, 2)
    e.close()


def check_overwrite_and_launches(lib_path):
    """case 6 (emulator): an output pre-filled with NaN comes back fully overwritten, odd orders as zeros; one call launches the one
    kernel, whatever Nq and n_delta are"""
    e = small_engine(lib_path)
    logs = []
    for nq, L, nd in ((5, 3, 9), (18, 4, 20), (33, 6, 50)):
        qs, phis, cc, avg, _ = synthetic_cc(nq, L, nd, 3)
        leg = X.legendre_table(qs, WAVELENGTH, L, 2)
        out = np.full((L + 1, nq, nq), np.nan, complex)
        ccc, legc = _lib.as_f64(cc), _lib.as_f64(leg)
        PC.launched_kernels(e, ('k_',))
        rc = e.lib.mtip_op_cc_to_deg2(e.ctx, nq, nd, L, 2, 3, 0, _lib.ptr(ccc), None, None, _lib.ptr(legc), _lib.ptr(out))
        logs.append(PC.launched_kernels(e, ('k_',)))
        assert rc == 0, e.lib.mtip_last_error(e.ctx).decode()
        assert np.isfinite(out).all() and not np.any(out[1::2]) and np.any(out[0])
        ref, _ = r_cc_to_deg2(cc, 3, qs, phis, L, True, {}, avg)
        assert rel_l2(out, ref) <= TOL_OP
    assert all(log == ('k_cc_deg2',) for log in logs), logs
    e.close()


def check_load_ccd():
    """io.load_ccd on seeded trees: the direct layout and the legacy one (thinned radial axis, default wavelength, pi_in_q)"""
    rng = np.random.default_rng(11)
    qs, phis = radial_points(6), np.arange(10) * 2 * np.pi / 10
    cc, avg = rng.random((6, 6, 10)), rng.random(6)
    d = IO.load_ccd({'cross_correlation': {'I1I1': cc}, 'radial_points': qs, 'angular_points': phis, 'average_intensity': avg,
                     'xray_wavelength': 1.5})
    assert set(d) >= {'cross_correlation', 'average_intensity', 'radial_points', 'angular_points', 'xray_wavelength', 'data_grid',
                      'dimensions'}
    assert d['dimensions'] == 3 and np.array_equal(d['cross_correlation']['I1I1'], cc) and np.array_equal(d['average_intensity'], avg)
    assert np.array_equal(d['data_grid']['thetas'], np.arccos(qs * 1.5 / (4 * np.pi)))
    assert d['data_grid']['qs'] is not None and np.array_equal(d['data_grid']['phis'], phis)
    q2 = radial_points(12)
    legacy = {'ccf_q1q2_2p': rng.random((6, 12, 10)) + 0j, 'q1': qs, 'q2': q2, 'phi': phis, 'iaverage': rng.random(12),
              'ccf_q1q2_4p': rng.random((6, 6, 10)) + 0j, 'pi_in_q': False}
    d = IO.load_ccd(legacy, 'legacy', dimensions=2)
    assert d['cross_correlation']['I1I1'].shape == (6, 6, 10) and np.array_equal(d['cross_correlation']['I1I1'], legacy['ccf_q1q2_2p'].real[:, ::2])
    assert 'I2I2' in d['cross_correlation'] and 'I2I1' not in d['cross_correlation']
    assert np.array_equal(d['radial_points'], q2) and np.array_equal(d['average_intensity'], legacy['iaverage'][::2])
    assert d['xray_wavelength'] == 1.23984 and d['dimensions'] == 2 and d['pi_in_q'] is False
    assert np.array_equal(d['thetas'], np.arccos(q2 * 1.23984 / 2))
    import pytest
    with pytest.raises(AssertionError):
        IO.load_ccd({}, 'other')

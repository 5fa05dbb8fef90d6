"""Cases of the back-substitution modes beside `back_substitution` (csrc/k_extract_psd.h: mtip_op_nearest_psd, mtip_op_cm_backsub;
Engine.nearest_psd / cm_backsub; extract.masked_cross_correlation_to_deg2_invariant with bl_extraction_method
back_substitution_memory_hungry, back_substitution_qqsym, back_substitution_psd), shared by tests/test_ccmodes_reference.py (CPU: the
restatement against G31), tests/test_emul_ccmodes.py (the unchanged kernel source on the CPU emulator) and tests/test_gpu_ccmodes.py.

Two yardsticks:
  * G31 (tests/golden/cc_backsub_modes.npz, written by tests/golden/make_golden_ccmodes.py): outputs of the reference's own three mode
    functions through cross_correlation_to_deg2_invariant, of nearest_positive_semidefinite_matrix, and of the extract chain behind them;
  * beyond the fixture the numpy restatement tests/ccmodes_reference.py (held to G31 by a CPU test), with the per-order bound of
    ccextract_cases.order_bounds: ten times the restatement's own deviation between rfft and direct-sum harmonics, floor 1e-12."""
import os

import numpy as np

import ccextract_cases as CC
import ccmask_cases as MC
import ccmodes_reference as R
import parity_cases as PC
from helpers import rel_l2
from xframe_amd.fxs import _lib, extract as X

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'cc_backsub_modes.npz')
WAVELENGTH = CC.WAVELENGTH
TOL_OP, TOL_FLOW = CC.TOL_OP, CC.TOL_FLOW
TOL_RESTATEMENT = 1e-13
MODES = R.MODES
ALL_SWITCHES = {'subtract_average_intensity': True, 'pi_periodicity': True, 'q1q2_symmetric': True}
# name -> (max_order, assume_zero_odd_orders, masked, modify_cc) of the operator outputs of G31
VARIANTS = {'s2': (8, True, False, {}), 's1': (8, False, False, {}), 'odd9': (9, True, False, {}), 'masked': (8, True, True, {}),
            'masked_all': (8, True, True, ALL_SWITCHES)}
G31_SHAPE = (6, 9, 32)                 # n_q, the highest max_order of a variant, n_delta
# label -> (n_q, max_order, n_delta, order stride); the emulator takes the first three
SHAPES = {'5xL8': (5, 8, 32, 2), '17xL9': (17, 9, 40, 2), '33xL12': (33, 12, 50, 1), '130xL6': (130, 6, 24, 2)}
PSD_SIZES = (1, 2, 5, 17, 64, 65, 129)  # one and two LDS tiles of k_sym_eig's range, a tail, past the 128-column solver
PSD_KINDS = ('hermitian', 'symmetric', 'psd', 'zero', 'general', 'pairs')


def load_golden():
    return np.load(GOLDEN)


def modes_cc(nq, L, nd, seed, stride, noise=1e-3):
    """ccextract_cases.synthetic_cc with noise, plus a noise term of the same size that is antisymmetric in Delta: the harmonics
    get an imaginary part, C_m(q1, q2) is neither Hermitian nor definite"""
    qs, phis, cc, avg, _ = CC.synthetic_cc(nq, L, nd, seed, stride, noise=noise)
    r = np.random.default_rng(seed + 7).normal(size=cc.shape)
    anti = (r - r[..., (-np.arange(nd)) % nd]) / 2
    return qs, phis, cc + noise * np.abs(cc).max() * anti, avg


def pair_mask(nq, nd, pairs=((1, 2), (4, 0))):
    """a 'direct' mask that removes interior samples of two pairs (samples 0 and n - 1 stay: memory_hungry interpolates)"""
    m = np.ones((nq, nq, nd), dtype=bool)
    m[pairs[0]][nd // 4:nd // 4 + 3] = False
    m[pairs[1]][nd // 2] = False
    return m


def golden_inputs():
    nq, L, nd = G31_SHAPE
    return modes_cc(nq, L, nd, 3131, 1, noise=0.02)


def psd_matrix(kind, n, seed=0):
    rng = np.random.default_rng(1000 * n + seed)
    a = rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))
    if kind == 'hermitian':
        return (a + a.conj().T) / 2
    if kind == 'symmetric':
        return ((a.real + a.real.T) / 2).astype(complex)
    if kind == 'psd':                                                             # rank about n / 2: a null space to count
        h = a[:, :max(n // 2, 1)]
        return h @ h.conj().T
    if kind == 'zero':
        return np.zeros((n, n), complex)
    if kind == 'general':
        return a
    # exact +x / -x eigenvalue pairs, [[0, 1], [1, 0]] (x) D: the matrices mtip_op_hermitian_eig repeats through the host
    d = np.diag(np.arange(1, n // 2 + 1, dtype=float))
    out = np.zeros((n, n), complex)
    out[:2 * (n // 2), :2 * (n // 2)] = np.kron(np.array([[0, 1], [1, 0]]), d)
    return out


# ---- restatement against the reference's own outputs (CPU) ---------------------------------------------------------------------------
def variant_call(name, mode):
    """(cc, qs, phis, max_order, zero_odd, modify_cc, avg, cc_mask or None) of an operator variant of G31 (the same for every mode)"""
    qs, phis, cc, avg = golden_inputs()
    L, zero_odd, masked, mod = VARIANTS[name]
    return cc, qs, phis, L, zero_odd, mod, avg, (pair_mask(len(qs), len(phis)) if masked else None)


def check_restatement_golden(g):
    """case 2: tests/ccmodes_reference.py against the reference's own functions: whole-array relative L2 <= 1e-13, masks equal"""
    worst = 0.0
    for mode in MODES:
        for name in VARIANTS:
            cc, qs, phis, L, zero_odd, mod, avg, mask = variant_call(name, mode)
            b, qq, _ = R.cc_to_deg2(mode, cc, qs, phis, L, zero_odd, mod, avg, mask)
            ref = g[f'G31_{mode}_{name}_b']
            d = rel_l2(b, ref)
            worst = max(worst, d)
            print(f'restatement vs G31 {mode} {name}: {d:.2e}')
            assert b.shape == ref.shape and np.array_equal(qq, g[f'G31_{mode}_{name}_qq_mask']), (mode, name)
            assert d <= TOL_RESTATEMENT, (mode, name, d)
    stack = g['G31_psd_in']
    d = rel_l2(R.nearest_psd(stack), g['G31_psd_out'])
    print(f'restatement vs G31 nearest_psd: {d:.2e}')
    assert d <= TOL_RESTATEMENT, d
    # the shifted eigh the device takes is the same projection
    d = rel_l2(R.nearest_psd(stack, R.shifted_eigh), g['G31_psd_out'])
    print(f'shifted-eigh restatement vs G31 nearest_psd: {d:.2e}')
    assert d <= TOL_RESTATEMENT, d
    return worst


# ---- mtip_op_nearest_psd ------------------------------------------------------------------------------------------------------------------
def check_nearest_psd(lib_path, n):
    """case 3: every kind of matrix at size n against numpy: |out - ref|_F <= 1e-12 |A|_F, out Hermitian to 1e-15 |A|_F, smallest
    eigenvalue of out >= -1e-13 |A|_F, n_clipped = numpy's count wherever numpy's eigenvalue is farther than 1e-10 |A|_F from zero;
    a stack of 7 gives the bits of 7 single calls"""
    e = CC.small_engine(lib_path)
    for kind in PSD_KINDS:
        A = psd_matrix(kind, n)
        out, clipped = e.nearest_psd(A)
        ref = R.nearest_psd(A)
        scale = np.linalg.norm(A)
        err = np.linalg.norm(out - ref)
        herm = np.abs(out - out.conj().T).max()
        low = np.linalg.eigvalsh((out + out.conj().T) / 2).min() if scale else 0.0
        neg, band = R.clip_counts(A)
        print(f'nearest_psd n = {n} {kind}: error {err / max(scale, 1e-300):.2e} |A|_F, Hermitian to {herm / max(scale, 1e-300):.1e}, '
              f'smallest eigenvalue {low / max(scale, 1e-300):.1e}, clipped {int(clipped[0])} (numpy {neg}, {band} in the guard band)')
        assert out.shape == (n, n) and out.dtype == np.complex128 and clipped.shape == (1,) and clipped.dtype == np.int32
        assert np.isfinite(out).all()
        assert err <= TOL_OP * scale, (n, kind, err, scale)
        assert herm <= 1e-15 * scale, (n, kind, herm, scale)
        assert low >= -1e-13 * scale, (n, kind, low, scale)
        # eigenvalues inside the band may fall on either side of zero
        w = np.linalg.eigvalsh((A + A.conj().T) / 2)
        sure = int((w < -R.CLIP_GUARD * scale).sum())
        assert sure <= int(clipped[0]) <= sure + band, (n, kind, int(clipped[0]), sure, band)
        if kind == 'psd':
            assert err <= TOL_OP * scale and int(clipped[0]) <= band
        if kind == 'zero':
            assert not np.any(out) and clipped[0] == 0
    stack = np.array([psd_matrix(PSD_KINDS[k % len(PSD_KINDS)], n, seed=k) for k in range(7)])
    out, clipped = e.nearest_psd(stack)
    for k in range(7):
        o1, c1 = e.nearest_psd(stack[k])
        assert np.array_equal(out[k], o1) and clipped[k] == c1[0], (n, k)
    e.close()


# ---- mtip_op_cm_backsub and the public function ---------------------------------------------------------------------------------------------
_CASE_CACHE = {}


def case_reference(label):
    """inputs and restatement outputs of one shape, computed once: per mode the rfft-route result, the per-order deviation of the
    direct-sum route and the bound (the scheme of ccextract_cases.order_bounds); for psd the steps' clip counts"""
    if label in _CASE_CACHE:
        return _CASE_CACHE[label]
    nq, L, nd, stride = SHAPES[label]
    qs, phis, cc, avg = modes_cc(nq, L, nd, 31, stride)
    zero_odd = stride == 2
    ref = {'inputs': (qs, phis, cc, avg, L, zero_odd)}
    for mode in MODES + ('qqsym_masked', 'psd_masked'):
        m = {'qqsym_masked': MODES[1], 'psd_masked': MODES[2]}.get(mode, mode)
        mask = pair_mask(nq, nd) if mode.endswith('_masked') else None
        a, qq, steps = R.cc_to_deg2(m, cc, qs, phis, L, zero_odd, {}, avg, mask, 'rfft')
        b, _, _ = R.cc_to_deg2(m, cc, qs, phis, L, zero_odd, {}, avg, mask, 'direct')
        dev = np.array([rel_l2(b[l], a[l]) if np.any(a[l]) else 0.0 for l in range(L + 1)])
        bound = np.maximum(CC.ORDER_MARGIN * dev, CC.ORDER_FLOOR)
        assert bound.max() <= CC.ORDER_CAP, ('input too ill-conditioned', label, mode, bound.max())
        ref[mode] = (a, qq, steps, dev, bound)
    for v in ref.values():
        for x in v:
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
    _CASE_CACHE[label] = ref
    return ref


def assert_not_vacuous(label):
    """from the restatement alone: at least one step of the psd elimination clips an eigenvalue below -1e-6 |A_l|, and the psd
    result differs from the plain back-substitution by more than 1e-4"""
    ref = case_reference(label)
    qs, phis, cc, avg, L, zero_odd = ref['inputs']
    psd, _, steps, _, _ = ref[MODES[2]]
    plain, _ = CC.r_cc_to_deg2(cc, 3, qs, phis, L, zero_odd, {}, avg)
    most_negative = min(s[2] for s in steps)
    d = rel_l2(psd, plain)
    print(f'{label}: most negative eigenvalue of a step {most_negative:.2e} |A_l|; psd vs back_substitution {d:.2e}; clipped per step '
          f'{[s[0] for s in steps]}')
    assert most_negative < -1e-6, (label, most_negative)
    assert d > 1e-4, (label, d)


def compare_orders(label, what, b, a, bound, L):
    whole = rel_l2(b, a)
    per = np.array([rel_l2(b[l], a[l]) if np.any(a[l]) else float(np.abs(b[l]).max()) for l in range(L + 1)])
    print(f'{label} {what}: whole {whole:.2e}; per order worst ratio to bound {(per / bound).max():.2e} at l = {int((per / bound).argmax())}')
    assert b.shape == a.shape and np.isfinite(b).all()
    assert whole <= TOL_OP, (label, what, whole)
    assert (per <= bound).all(), (label, what, per, bound)


def check_modes_restatement(lib_path, label):
    """case 4: Engine.cm_backsub (psd with info, plain, plain with the Hermitian mean, a masked pair) and the public function in the
    three modes against the restatement: whole array <= 1e-12, per order <= max(10 d_l, 1e-12); memory_hungry bit-equal to
    back_substitution on the device"""
    assert_not_vacuous(label)
    ref = case_reference(label)
    qs, phis, cc, avg, L, zero_odd = ref['inputs']
    nq, nd = cc.shape[0], cc.shape[-1]
    stride = 2 if zero_odd else 1
    l_max = (L // stride) * stride
    e = CC.small_engine(lib_path)
    # the operator on harmonics from the dimensions = 2 entry
    cm = e.cc_to_deg2(cc, l_max, order_stride=1, dimensions=2)
    leg1, legs = X.legendre_table(qs, WAVELENGTH, l_max, 1), X.legendre_table(qs, WAVELENGTH, l_max, stride)
    pad = lambda b: np.concatenate([b, np.zeros((L + 1 - b.shape[0],) + b.shape[1:], complex)]) if b.shape[0] < L + 1 else b
    # (psd with a masked pair and its clip counts here, unmasked through the public function below; qqsym the other way round)
    for what, mode, kw in (('psd masked', 'psd_masked', {'qq_mask': pair_mask(nq, nd).all(-1)}), ('qqsym', MODES[1], {})):
        a, _, steps, _, bound = ref[mode]
        psd = what.startswith('psd')
        b, info = e.cm_backsub(cm, leg1 if psd else legs, order_stride=stride, mode='psd' if psd else 'plain', hermitian_mean=not psd, **kw)
        compare_orders(label, 'cm_backsub ' + what, pad(b), a, bound, L)
        if zero_odd:
            assert not np.any(b[1::2])
        if psd:
            assert info.dtype == np.int32 and info.shape == (l_max + 1,)
            for l, (neg, band, _) in enumerate(steps):
                # the restatement's count; eigenvalues within 1e-10 |A_l| of zero may fall on either side
                assert abs(int(info[l]) - neg) <= band, (label, what, l, int(info[l]), neg, band)
        else:
            assert info is None
    # plain without the mean: the elimination of back_substitution on the same harmonics
    b, _ = e.cm_backsub(cm, legs, order_stride=stride, mode='plain')
    a, _, _, _, bound = ref[MODES[0]]
    compare_orders(label, 'cm_backsub plain', pad(b), a, bound, L)
    # the public function
    for mode in MODES:
        a, qq_ref, _, _, bound = ref[mode]
        meta = MC.metadata(qs, phis, L, zero_odd, {}, avg, {'type': 'none'}, mode)
        b, qm = X.masked_cross_correlation_to_deg2_invariant(e, cc.copy(), 3, **meta)
        compare_orders(label, mode, b, a, bound, L)
        assert b.dtype == np.complex128 and qm.dtype == bool and np.array_equal(qm, qq_ref)
        if zero_odd:
            assert not np.any(b[1::2])
    plain, _ = X.masked_cross_correlation_to_deg2_invariant(e, cc.copy(), 3, **MC.metadata(qs, phis, L, zero_odd, {}, avg, {'type': 'none'},
                                                                                           'back_substitution'))
    hungry, _ = X.masked_cross_correlation_to_deg2_invariant(e, cc.copy(), 3, **MC.metadata(qs, phis, L, zero_odd, {}, avg, {'type': 'none'},
                                                                                            MODES[0]))
    assert np.array_equal(plain, hungry)
    # masked data through the public function: qq_mask from the mask, masked pairs zero (qqsym) / entering as zeros (psd)
    mset = {'type': 'direct', 'direct': {'mask': pair_mask(nq, nd)}}
    for mode, key in ((MODES[1], 'qqsym_masked'), (MODES[2], 'psd_masked')):
        a, qq_ref, _, _, bound = ref[key]
        b, qm = X.masked_cross_correlation_to_deg2_invariant(e, cc.copy(), 3, **MC.metadata(qs, phis, L, zero_odd, {}, avg, mset, mode))
        compare_orders(label, mode + ' masked', b, a, bound, L)
        assert np.array_equal(qm, qq_ref) and not qm.all()
    e.close()


def check_operator_golden(g, lib_path=None):
    """the public function in the three modes on every variant of G31 (odd orders assumed zero and not, an odd max_order, a direct
    mask, the mask with every modify_cc switch): b_coeff within TOL_OP of the reference's own, qq_mask equal"""
    e = CC.small_engine(lib_path)
    for mode in MODES:
        for name in VARIANTS:
            cc, qs, phis, L, zero_odd, mod, avg, mask = variant_call(name, mode)
            mset = {'type': 'none'} if mask is None else {'type': 'direct', 'direct': {'mask': mask}}
            b, qq = X.masked_cross_correlation_to_deg2_invariant(e, cc.copy(), 3, **MC.metadata(qs, phis, L, zero_odd, mod, avg, mset, mode))
            ref = g[f'G31_{mode}_{name}_b']
            d = rel_l2(b, ref)
            print(f'{mode} vs G31 {name}: {d:.2e}')
            assert b.shape == ref.shape and np.array_equal(qq, g[f'G31_{mode}_{name}_qq_mask']), (mode, name)
            assert d <= TOL_OP, (mode, name, d)
    out, _ = e.nearest_psd(g['G31_psd_in'])
    d = rel_l2(out, g['G31_psd_out'])
    print(f'nearest_psd vs G31: {d:.2e}')
    assert d <= TOL_OP, d
    e.close()


# ---- flows and refusals -------------------------------------------------------------------------------------------------------------------
def flow_settings(L, mode):
    s = CC.flow_settings(L, CC.MASK_CASES['none'], enforce_psd=False)
    s['cross_correlation']['datasets']['I1I1']['bl_extraction_method'] = mode
    return s


def flow_ccd():
    from xframe_amd.fxs import io as IO
    qs, phis, cc, avg = golden_inputs()
    return IO.load_ccd({'cross_correlation': {'I1I1': cc.copy()}, 'radial_points': qs, 'angular_points': phis, 'average_intensity': avg,
                        'xray_wavelength': WAVELENGTH})


def check_flow_golden(g, lib_path=None):
    """case 5: extract_from_cross_correlation with bl_extraction_method = each mode (bl_q_limits none, subtract_average_intensity)
    against the reference's chain: b_coeff <= 1e-12, V_l through V V^+ <= 1e-10"""
    e = CC.small_engine(lib_path)
    L = 8
    for mode in MODES:
        assert X._wants_masked_route(flow_settings(L, mode)['cross_correlation']['datasets']['I1I1'])
        data = X.extract_from_cross_correlation(e, flow_ccd(), flow_settings(L, mode))
        ref_b = g[f'G31_flow_{mode}_b']
        d = rel_l2(data['b_coeff']['I1I1'], ref_b)
        print(f'flow {mode}: b_coeff {d:.2e}')
        assert d <= TOL_OP, (mode, d)
        assert np.array_equal(data['deg_2_invariant_masks']['I1I1'], g[f'G31_flow_{mode}_mask'])
        pms = data['data_projection_matrices']
        assert len(pms) == L + 1
        for l in range(L + 1):
            ref = g[f'G31_flow_{mode}_pm{l}']
            assert pms[l].shape == ref.shape, (mode, l, pms[l].shape, ref.shape)
            vv, rr = pms[l] @ pms[l].conj().T, ref @ ref.conj().T
            scale = max(np.linalg.norm(ref_b[l]), 1e-300)
            assert np.linalg.norm(vv - rr) <= TOL_FLOW * scale, (mode, l, np.linalg.norm(vv - rr) / scale)
    e.close()


def check_refusals(lib_path=None):
    """case 5: legendre still raises through the masked route, dim = 2 still raises, a conditioning stage with masked data is refused
    by name for qqsym and psd; n_q = 1025 with psd, n_q = 4097 with plain, max_order = 129 and n = 1025 of nearest_psd return the error
    code with the limit named and leave NaN-filled outputs untouched"""
    import pytest
    qs, phis, cc, avg = golden_inputs()
    nq, nd = cc.shape[0], cc.shape[-1]
    e = CC.small_engine(lib_path)
    with pytest.raises(NotImplementedError, match='legendre'):
        X.masked_cross_correlation_to_deg2_invariant(e, cc.copy(), 3, **MC.metadata(qs, phis, 8, True, {}, avg, {'type': 'none'}, 'legendre'))
    for mode in MODES:
        with pytest.raises(NotImplementedError, match='dimensions = 2'):
            X.masked_cross_correlation_to_deg2_invariant(e, cc.copy(), 2, **MC.metadata(qs, phis, 8, True, {}, avg, {'type': 'none'}, mode))
    mset = {'type': 'direct', 'direct': {'mask': pair_mask(nq, nd)}}
    for mode in MODES[1:]:
        with pytest.raises(NotImplementedError, match='enforce_max_order'):
            X.masked_cross_correlation_to_deg2_invariant(e, cc.copy(), 3, **MC.metadata(qs, phis, 8, True, {'enforce_max_order': True}, avg,
                                                                                        mset, mode))
    small = np.zeros((3, 2, 2), complex)
    leg = _lib.as_f64(np.ones((2, 6)))
    out, info = np.full((3, 2, 2), np.nan, complex), np.full(200, -7, np.int32)
    for (nqq, L, stride, mode), words in (((1025, 2, 1, 1), ('1024', '1025')), ((4097, 2, 1, 0), ('4096', '4097')), ((2, 129, 1, 1), ('128', '129')),
                                          ((2, 129, 2, 0), ('128', '129'))):
        rc = e.lib.mtip_op_cm_backsub(e.ctx, nqq, L, stride, mode, 0, _lib.ptr(small), _lib.ptr(leg), None, _lib.ptr(out), _lib.ptr(info))
        msg = e.lib.mtip_last_error(e.ctx).decode()
        assert rc == -1 and 'cm_backsub' in msg and all(w in msg for w in words), (nqq, L, rc, msg)
        assert np.isnan(out).all() and (info == -7).all()
    for args in ((2, 2, 3, 1, 0), (2, 2, 1, 2, 0), (2, 2, 1, 0, 2), (2, 2, 1, 1, 1)):    # stride 3, mode 2, unknown flag, the mean with psd
        rc = e.lib.mtip_op_cm_backsub(e.ctx, *args, _lib.ptr(small), _lib.ptr(leg), None, _lib.ptr(out), _lib.ptr(info))
        assert rc == -1 and 'cm_backsub' in e.lib.mtip_last_error(e.ctx).decode(), args
        assert np.isnan(out).all() and (info == -7).all()
    clip = np.full(3, -7, np.int32)
    for n in (1025, 0):
        rc = e.lib.mtip_op_nearest_psd(e.ctx, n, 1, _lib.ptr(small), _lib.ptr(out), _lib.ptr(clip))
        msg = e.lib.mtip_last_error(e.ctx).decode()
        assert rc == -1 and 'nearest_psd' in msg and '1024' in msg and str(n) in msg, (n, rc, msg)
        assert np.isnan(out).all() and (clip == -7).all()
    e.close()


def check_launches(lib_path):
    """case 6 (emulator): one psd call is the fixed launch list -- the batched projection of the C_m, the first input, then per order
    one k_herm_eig and one k_psd_step -- whatever the data: with harmonics whose matrices carry exact +x / -x eigenvalue pairs (what
    mtip_op_hermitian_eig answers with a second k_herm_eig launch after a round trip through host memory) the list is the same: no
    repeat, and nothing between the first and the last step depends on a value read on the host"""
    e = CC.small_engine(lib_path)
    nq, L = 6, 4
    qs = CC.radial_points(nq)
    leg = X.legendre_table(qs, WAVELENGTH, L, 1)
    expected = ('k_psd_prep', 'k_herm_eig', 'k_psd_rebuild', 'k_psd_prep') + ('k_herm_eig', 'k_psd_step') * (L + 1)
    rng = np.random.default_rng(6)
    noise = rng.normal(size=(L + 1, nq, nq)) + 1j * rng.normal(size=(L + 1, nq, nq))
    pairs = np.array([psd_matrix('pairs', nq) for _ in range(L + 1)])
    for cm in (noise, pairs):
        PC.launched_kernels(e, ('k_',))
        b, info = e.cm_backsub(cm, leg, order_stride=1, mode='psd')
        log = PC.launched_kernels(e, ('k_',))
        assert log == expected, log
        assert np.isfinite(b).all()
    PC.launched_kernels(e, ('k_',))
    _, clipped = e.nearest_psd(pairs)
    assert (clipped == nq // 2).all()                                             # the -x half of the pairs
    assert PC.launched_kernels(e, ('k_',)) == ('k_psd_prep', 'k_herm_eig', 'k_psd_rebuild')
    e.close()

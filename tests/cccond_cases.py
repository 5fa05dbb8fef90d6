"""Cases of the conditioning stages of `extract` (csrc/k_extract_cond.h: Engine.cc_lowpass_q / cc_harmonic_filter / cc_binned_mean,
extract.modify_masked_cross_correlation) and of the truncated minimum-norm least squares (k_cc_lstsq<NT, true>,
Engine.cc_lstsq_deg2_minnorm), shared by tests/test_emul_cccond.py (the unchanged kernel source on the CPU emulator) and
tests/test_gpu_cccond.py.

Yardsticks:
  * G30 (tests/golden/cc_condition.npz, written by tests/golden/make_golden_cccond.py): outputs of the reference's own
    modify_cross_correlation, binned_mean and cross_correlation_to_deg2_invariant on seeded data of 6 shells, 64 and 70 angles,
    max_order 8;
  * scipy.signal.sosfilt, numpy.fft.rfft / irfft and a longdouble masked mean called directly, for the shapes beyond the fixture;
  * for the rank-deficient pairs numpy.linalg.lstsq (rank, solution) and a longdouble minimum-norm solution x = A^T (A A^T)^-1 c
    (through a longdouble QR of A^T, refined) or, for the rank-1 pairs on the Ewald limit, the closed form a mean(c) / |a|^2.
Tolerances: ccextract_cases.TOL_OP (1e-12 of the largest reference value) for the operators; for the minimum-norm solutions the rule
of ccmask_cases.check_lstsq_refined with its constants: LSQ_MARGIN x LAPACK's own deviation from the longdouble yardstick in the
same case, floor LSQ_FLOOR, the yardstick a hundred times finer than the bound."""
import os

import numpy as np

import ccextract_cases as CC
import ccmask_cases as MC
from helpers import rel_l2
from xframe_amd.fxs import _lib, extract as X

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'cc_condition.npz')
WAVELENGTH = CC.WAVELENGTH
TOL_OP, TOL_FLOW = CC.TOL_OP, CC.TOL_FLOW
LSQ_MARGIN, LSQ_FLOOR = MC.LSQ_MARGIN, MC.LSQ_FLOOR
EPS = np.finfo(float).eps

# ---- the data of G30 -------------------------------------------------------------------------------------------------------------------
G_NQ, G_L, G_NDS, G_SEED, G_CUTOFF = 6, 8, (64, 70), 30, 1.0
# name -> modify_cc of the modify_cross_correlation cases of G30, all on cond_mask
MODIFY_VARIANTS = {
    'lowpass': {'low_pass_order_in_q': G_CUTOFF},
    'maxorder': {'enforce_max_order': True},
    'zeroodd': {'enforce_zero_odd_harmonics': True},
    'binned': {'apply_binned_mean': True},
    'all': {'subtract_average_intensity': True, 'low_pass_order_in_q': G_CUTOFF, 'enforce_max_order': True,
            'enforce_zero_odd_harmonics': True, 'pi_periodicity': True, 'q1q2_symmetric': True, 'apply_binned_mean': True,
            'interpolate_masked': True},
}
BL_MODIFY = {'apply_binned_mean': True, 'interpolate_masked': True}
BL_MODES = ('lstsq', 'back_substitution')
CUSTOM_MASK = {'type': 'pixel_custom', 'pixel_custom': {'n_masked_pixels_phi': 0.02, 'n_masked_pixels_q': 0.4, 'mask_at_pi': False}}
FLOW_ND = 70
STARVED_PAIR, STARVED_SAMPLES = (1, 4), (11, 12, 33, 52)            # the bins 3, 8 and 12 of sixteen keep a sample: five even orders
# name -> (bl_extraction_method, modify_cc beside ccextract_cases.FLOW_MODIFY, whether the mask starves STARVED_PAIR)
# The least-squares flow runs without interpolate_masked: the interpolation returns an all-true mask (fxs_invariant_tools.py:287), behind
# which no pair can be short of samples.
FLOWS = {'binned_lstsq_starved': ('lstsq', {'apply_binned_mean': True}, True),
         'binned_backsub': ('back_substitution', {'apply_binned_mean': True, 'interpolate_masked': True}, False)}


def cond_mask(nq, nd, seed=G_SEED):
    """ccmask_cases.direct_mask (interior holes, the rows (3, 5) and (5, 3) fully masked, samples 0 and nd - 1 valid elsewhere) with the
    pair (0, 1) fully valid and a run of nine interior samples of (2, 2) masked: a whole bin of the binned mean without a sample"""
    m = MC.direct_mask(nq, nd, seed)
    m[0, 1] = True
    m[2, 2, nd // 4:nd // 4 + 9] = False
    return m


def golden_inputs(nd):
    qs, phis, cc, avg, _ = CC.synthetic_cc(G_NQ, G_L, nd, G_SEED, 2, noise=0.02)
    return cc, qs, avg, phis, cond_mask(G_NQ, nd)


def starved_mask(base):
    m = np.array(base, dtype=bool)
    m[STARVED_PAIR] = False
    m[STARVED_PAIR][list(STARVED_SAMPLES)] = True
    return m


def flow_settings(flow, mask):
    method, extra, _ = FLOWS[flow]
    s = CC.flow_settings(G_L, CC.MASK_CASES['none'], modify_cc={**CC.FLOW_MODIFY, **extra})
    d = s['cross_correlation']['datasets']['I1I1']
    d['cc_mask'] = {'type': 'direct', 'direct': {'mask': mask.copy()}}
    d['bl_extraction_method'] = method
    return s


def flow_ccd(nd=FLOW_ND):
    from xframe_amd.fxs import io as IO
    cc, qs, avg, phis, _ = golden_inputs(nd)
    return IO.load_ccd({'cross_correlation': {'I1I1': cc.copy()}, 'radial_points': qs, 'angular_points': phis, 'average_intensity': avg,
                        'xray_wavelength': WAVELENGTH})


def load_golden():
    return np.load(GOLDEN)


def close(v, ref, what):
    """the operator tolerance: every element within TOL_OP of the largest reference value"""
    v, ref = np.asarray(v), np.asarray(ref)
    assert v.shape == ref.shape, (what, v.shape, ref.shape)
    scale = max(float(np.abs(ref).max()), 1e-300)
    err = float(np.abs(v - ref).max()) / scale
    print(f'{what}: worst element {err:.2e} of the largest reference value')
    assert err <= TOL_OP, (what, err)
    return err


# ---- the three operators against scipy / numpy / longdouble ---------------------------------------------------------------------------
def sos_sections(nq):
    """the order-1 section the reference asks for (fxs_invariant_tools.py:250) and a genuine biquad: all six coefficients non-zero"""
    from scipy.signal import butter
    first = butter(1, 0.2 * nq, 'lp', fs=nq, output='sos')
    second = butter(2, 0.15 * nq, 'lp', fs=nq, output='sos')
    assert first.shape == second.shape == (1, 6) and first[0, 2] == 0 and first[0, 5] == 0 and np.all(second != 0)
    return {'order1': first, 'biquad': second}


def check_lowpass(lib_path, nq, nd, section, subtract):
    """scipy.signal.sosfilt along axis 0, then axis 1, called directly; the average intensity subtracted first where `subtract`"""
    from scipy.signal import sosfilt
    rng = np.random.default_rng(nq * 1000 + nd)
    cc = rng.normal(size=(nq, nq, nd)) + 5.0
    avg = 1 + rng.random(nq)
    sos = sos_sections(nq)[section]
    x = cc - avg[:, None, None] * avg[None, :, None] if subtract else cc
    ref = sosfilt(sos, sosfilt(sos, x, axis=0), axis=1)
    e = CC.small_engine(lib_path)
    out = e.cc_lowpass_q(cc.copy(), sos, average_intensity=avg if subtract else None)
    e.close()
    return close(out, ref, f'low pass {nq} x {nd} {section}{" - I I" if subtract else ""}')


def r_harmonic_filter(cc, max_order, zero_odd):
    """fxs_invariant_tools.py:253-263 with mathLibrary.py:484-496: numpy's rfft / n, zeros, irfft(. n, n)"""
    n = cc.shape[-1]
    c = np.fft.rfft(cc) / n
    if max_order is not None:
        c[..., max_order + 1:] = 0
    if zero_odd:
        c[..., 1::2] = 0
    return np.fft.irfft(c * n, n)


HARMONIC_SHAPES = {   # label -> (nq, n_delta, max_order of the cut): even, odd, 4 x 15, 2 x 37, the default of `correlate` at 129 kept harmonics
    '64': (3, 64, 8), '65_odd': (3, 65, 8), '60': (3, 60, 8), '74': (3, 74, 8), '1536': (3, 1536, 128),
}


def check_harmonic(lib_path, label):
    """each flag alone, both together, a cut at or above n / 2 (nothing zeroed) and the subtraction, against numpy"""
    nq, nd, mo = HARMONIC_SHAPES[label]
    rng = np.random.default_rng(nd)
    cc = rng.normal(size=(nq, nq, nd)) + 5.0
    avg = 1 + rng.random(nq)
    e = CC.small_engine(lib_path)
    worst = 0.0
    for what, max_order, zero_odd in (('cut', mo, False), ('odd', None, True), ('both', mo, True), ('none', nd // 2, False),
                                      ('beyond', nd, False)):
        out = e.cc_harmonic_filter(cc.copy(), max_order=max_order, zero_odd=zero_odd)
        worst = max(worst, close(out, r_harmonic_filter(cc, max_order, zero_odd), f'harmonic filter {label} {what}'))
    out = e.cc_harmonic_filter(cc.copy(), max_order=mo, zero_odd=True, average_intensity=avg)
    close(out, r_harmonic_filter(cc - avg[:, None, None] * avg[None, :, None], mo, True), f'harmonic filter {label} both - I I')
    e.close()
    return worst


def r_binned_mean_longdouble(cc, mask, phis, max_order):
    """the masked mean of every bin in longdouble; the bin of a sample from the reference's expression (312-314)"""
    step = np.pi / max_order
    ids = (phis + step / 2) // step
    ids[ids == 2 * max_order] = 0
    ids = ids.astype(int)
    out = np.zeros(cc.shape[:2] + (2 * max_order,), np.longdouble)
    cnt = np.zeros(out.shape, int)
    x = np.where(mask, cc, 0.0).astype(np.longdouble)
    for d, b in enumerate(ids):
        out[..., b] += x[..., d]
        cnt[..., b] += mask[..., d]
    nz = cnt != 0
    out[nz] /= cnt[nz]
    return np.asarray(out, dtype=float), nz


BINNED_SHAPES = {'64': (4, 64, 8), '70_uneven': (4, 70, 8), '1536': (3, 1536, 69)}      # label -> (nq, n_delta, max_order)


def check_binned(lib_path, label):
    """uneven bins and a roll, against the longdouble masked mean: a bin with every sample masked, a pair with none valid, an
    all-valid pair; new angles arange(n_bins) 2 pi / n_bins"""
    nq, nd, mo = BINNED_SHAPES[label]
    rng = np.random.default_rng(nd + mo)
    phis = np.arange(nd) * 2 * np.pi / nd
    cc = rng.normal(size=(nq, nq, nd)) + 5.0
    avg = 1 + rng.random(nq)
    mask = rng.random((nq, nq, nd)) > 0.3
    mask[0, 1] = True
    mask[1, 2] = False
    bin_start, n_roll, new_phis = X.binned_mean_tables(phis, mo)
    mask[2, 0, :bin_start[3] - n_roll] = False                                    # the bins 0 .. 2 of this pair lose every sample:
    mask[2, 0, nd - n_roll:] = False                                              # bin 0 begins with the last n_roll angles
    assert len(bin_start) == 2 * mo + 1 and np.array_equal(new_phis, np.arange(2 * mo) * 2 * np.pi / (2 * mo))
    if label != '64':
        assert n_roll > 0 and len(set(np.diff(bin_start))) > 1, 'this shape is here for its roll and its uneven bins'
    e = CC.small_engine(lib_path)
    out, m = e.cc_binned_mean(cc.copy(), mask.copy(), bin_start, n_roll)
    ref, rm = r_binned_mean_longdouble(cc, mask, phis, mo)
    assert m.dtype == bool and np.array_equal(m, rm) and not m[1, 2].any() and m[0, 1].all() and not m[2, 0, :3].any() and m[2, 0, 3:].all()
    assert not np.any(out[~m])                                                    # 329: what the masked sum leaves there
    err = close(out, ref, f'binned mean {label}')
    out, m = e.cc_binned_mean(cc.copy(), mask.copy(), bin_start, n_roll, average_intensity=avg)
    ref, _ = r_binned_mean_longdouble(cc - avg[:, None, None] * avg[None, :, None], mask, phis, mo)
    close(out, ref, f'binned mean {label} - I I')
    e.close()
    return err


# ---- against the reference's own outputs (G30) ---------------------------------------------------------------------------------------------
def check_modify_golden(g, lib_path=None):
    """modify_cross_correlation of the reference: each new key alone, and all stages together, at 64 and 70 angles: masks and new
    angles equal, values within TOL_OP; binned_mean called alone"""
    e = CC.small_engine(lib_path)
    for nd in G_NDS:
        cc, qs, avg, phis, mask = golden_inputs(nd)
        for name, mod in MODIFY_VARIANTS.items():
            v, m, p = X.modify_masked_cross_correlation(e, cc.copy(), mask.copy(), phis.copy(), G_L, average_intensity=avg, **mod)
            assert np.array_equal(np.asarray(m, dtype=bool), g[f'G30_{nd}_{name}_mask']), (nd, name)
            assert np.array_equal(p, g[f'G30_{nd}_{name}_phis']), (nd, name)
            close(v, g[f'G30_{nd}_{name}_cc'], f'modify vs G30 {nd} {name}')
        bin_start, n_roll, new_phis = X.binned_mean_tables(phis, G_L)
        v, m = e.cc_binned_mean(cc.copy(), mask.copy(), bin_start, n_roll)
        assert np.array_equal(m, g[f'G30_{nd}_binned_mean_mask']) and not m.all() and np.array_equal(new_phis, g[f'G30_{nd}_binned_mean_phis'])
        assert not np.any(v[~m])
        close(v, g[f'G30_{nd}_binned_mean_cc'], f'binned_mean vs G30 {nd}')
    e.close()


def bl_metadata(nd, mode):
    cc, qs, avg, phis, mask = golden_inputs(nd)
    return cc, MC.metadata(qs, phis, G_L, True, dict(BL_MODIFY), avg, {'type': 'direct', 'direct': {'mask': mask}}, mode)


def check_bl_golden(g, lib_path=None):
    """cross_correlation_to_deg2_invariant of the reference with binned mean + interpolation in the modes lstsq and back_substitution:
    B_l within TOL_OP, qq_mask equal, data_grid['phis'] the new angles (395)"""
    e = CC.small_engine(lib_path)
    for nd in G_NDS:
        for mode in BL_MODES:
            cc, meta = bl_metadata(nd, mode)
            b, qq = X.masked_cross_correlation_to_deg2_invariant(e, cc.copy(), 3, **meta)
            ref = g[f'G30_{nd}_bl_{mode}']
            err = rel_l2(b, ref)
            print(f'B_l vs G30 {nd} {mode}: {err:.2e}')
            assert b.shape == ref.shape and err <= TOL_OP, (nd, mode, err)
            assert np.array_equal(qq, g[f'G30_{nd}_bl_{mode}_qq']) and not np.any(b[1::2])
            assert np.array_equal(meta['data_grid']['phis'], np.arange(2 * G_L) * 2 * np.pi / (2 * G_L))
    e.close()


def check_flow_golden(g, lib_path=None):
    """extract_from_cross_correlation with apply_binned_mean on a pixel_custom mask against the reference's chain (the tolerances of
    ccmask_cases.check_flow_golden): lstsq with the opt-in on a mask that leaves one pair three bins for five orders, and
    back_substitution with interpolate_masked.  Without the opt-in the starved pair raises the pinned text."""
    import pytest
    e = CC.small_engine(lib_path)
    for flow, (method, _, starved) in FLOWS.items():
        mask = g[f'G30_flow_{flow}_cc_mask']
        s = flow_settings(flow, mask)
        assert X._wants_masked_route(s['cross_correlation']['datasets']['I1I1'])
        if starved:
            with pytest.raises(NotImplementedError, match=r'1 of 36 pairs are rank deficient.*\(q1, q2\) = \(1, 4\) with 3 valid samples'):
                X.extract_from_cross_correlation(e, flow_ccd(), s)
            s['GPU'] = {'lstsq_minimum_norm': True}
        data = X.extract_from_cross_correlation(e, flow_ccd(), s)
        assert np.array_equal(data['deg_2_invariant_masks']['I1I1'], g[f'G30_flow_{flow}_mask']), flow
        assert np.array_equal(data['deg_2_invariant_q_id_limits']['I1I1'], g[f'G30_flow_{flow}_qid']), flow
        ref_b = g[f'G30_flow_{flow}_b']
        d = rel_l2(data['deg_2_invariant']['I1I1'], ref_b)
        print(f'flow {flow}: constrained B_l {d:.2e}')
        assert d <= TOL_FLOW, (flow, d)
        pms = data['data_projection_matrices']
        assert len(pms) == G_L + 1
        for l in range(G_L + 1):
            ref = g[f'G30_flow_{flow}_pm{l}']
            assert pms[l].shape == ref.shape, (flow, l, pms[l].shape, ref.shape)
            vv, rr = pms[l] @ pms[l].conj().T, ref @ ref.conj().T
            scale = max(np.linalg.norm(ref_b[l]), 1e-300)
            assert np.linalg.norm(vv - rr) <= TOL_FLOW * scale, (flow, l, np.linalg.norm(vv - rr) / scale)
    e.close()


# ---- truncated minimum-norm least squares --------------------------------------------------------------------------------------------------
def ewald_limit_q():
    """a radial point with q lambda / (4 pi) = 1 exactly as numpy rounds it: theta = arccos(1) = 0, x(Delta) = cos theta_2 for every
    Delta, so every row of F is the same and its rank is exactly 1"""
    q = 4 * np.pi / WAVELENGTH
    for _ in range(8):
        r = q * WAVELENGTH / (4 * np.pi)
        if r == 1.0:
            return q
        q = np.nextafter(q, 0.0 if r > 1.0 else np.inf)
    raise AssertionError('no double q with q lambda / (4 pi) == 1')


def _pick(nd, count, seed):
    m = np.zeros(nd, dtype=bool)
    m[np.sort(np.random.default_rng(seed).permutation(nd)[:count])] = True
    return m


def minnorm_case(label):
    """label -> (qs, phis, cc, orders, mask, {deficient pair: expected n_valid})"""
    if label == '4of9_1of9':                                                       # the refusal case of ccmask_cases.check_lstsq_random_masks
        nq, L, nd, stride = 5, 8, 70, 1
        mask = MC.random_pair_masks(nq, nd)
        mask[1, 4] = False
        mask[1, 4, [3, 30, 31, 50]] = True
        mask[0, 2] = False
        mask[0, 2, 17] = True
        short = {(1, 4): 4, (0, 2): 1}
    elif label == '63of64':                                                        # the widest register instantiation
        nq, L, nd, stride = 2, 63, 256, 1
        mask = np.ones((nq, nq, nd), dtype=bool)
        mask[0, 1] = False
        mask[0, 1, 0:126:2] = True                                                 # 63 angles <= pi: Delta and 2 pi - Delta share their row of F
        mask[1, 1] = False
        short = {(0, 1): 63}
    elif label == '10of17':
        nq, L, nd, stride = 3, 32, 200, 2
        mask = MC.periodic_mask(nq, nd, 1 / 25)
        mask[2, 0] = _pick(nd, 10, 10)
        mask[1, 1] = False
        short = {(2, 0): 10}
    elif label == 'ewald_limit':
        nq, L, nd, stride = 4, 8, 70, 1
        # numpy's second singular value of a matrix of identical rows is rounding residue about a hundred times below its cut,
        # whatever the row count; the pairs kept here clear the factor 100 of check_gap (184 x, 184 x, 198 x), the pairs (0, 3),
        # (1, 3) and their mirrors (94 x, 109 x) get no sample
        mask = MC.random_pair_masks(5, nd)[:nq, :nq]
        mask[:2, 3] = mask[3, :2] = False
        mask[2, 3] = mask[3, 2] = mask[3, 3] = True
        short = {}
    else:
        raise KeyError(label)
    qs, phis, cc, _, _ = CC.synthetic_cc(nq, L, nd, 27, stride, noise=1e-3)
    if label == 'ewald_limit':
        qs = qs.copy()
        qs[-1] = ewald_limit_q()
        short = {(i, j): int(mask[i, j].sum()) for i in range(nq) for j in range(nq) if (i == nq - 1 or j == nq - 1) and mask[i, j].any()}
    return qs, phis, cc, np.arange(0, L + 1, stride), mask, short


MINNORM_CASES = ('4of9_1of9', '63of64', '10of17', 'ewald_limit')


def check_gap(A, what):
    """the condition on the inputs: no singular value of F[valid], as numpy computes it, within a factor 100 of numpy's cut
    eps max(M, N) sigma_max.  Near the cut LAPACK's own rank is an accident of rounding and no parity is defined."""
    sv = np.linalg.svd(A, compute_uv=False)
    cut = EPS * max(A.shape) * sv[0]
    near = (sv > cut / 100) & (sv < cut * 100)
    gap = min([s / cut for s in sv if s > cut] + [cut / s for s in sv if 0 < s <= cut] + [np.inf])
    assert not near.any(), (what, sv / cut)
    return int((sv > cut).sum()), gap


def minnorm_longdouble(A, c):
    """x = A^T (A A^T)^-1 c for A of full row rank, in longdouble: A^T = Q R by Gram-Schmidt with reorthogonalisation, R^T z = c,
    x = Q z, then rounds of refinement on the residual c - A x.  Returns (x, relative size of the last correction)."""
    At = A.T.astype(np.longdouble)
    n, m = At.shape
    Q = np.zeros((n, m), np.longdouble)
    R = np.zeros((m, m), np.longdouble)
    for k in range(m):
        v = At[:, k].copy()
        for _ in range(2):
            h = Q[:, :k].T @ v
            v = v - Q[:, :k] @ h
            R[:k, k] += h
        R[k, k] = np.sqrt(v @ v)
        Q[:, k] = v / R[k, k]

    def solve(rhs):                                                                # R^T z = rhs, forward substitution
        z = np.zeros(m, np.longdouble)
        for k in range(m):
            z[k] = (rhs[k] - R[:k, k] @ z[:k]) / R[k, k]
        return Q @ z
    cl, Al = c.astype(np.longdouble), A.astype(np.longdouble)
    x = solve(cl)
    last = np.inf
    for _ in range(3):
        dx = solve(cl - Al @ x)
        x = x + dx
        last = float(np.sqrt(dx @ dx) / np.sqrt(x @ x))
    return x, last


def check_minnorm(lib_path, label):
    """numpy's rank for every pair; the bits of mtip_op_cc_lstsq_deg2 for every pair that kernel solves at full rank; zeros and rank 0
    for a pair without a sample; the deficient pairs against numpy.linalg.lstsq within the bound LAPACK's own deviation from the
    longdouble yardstick sets.  Returns (worst LAPACK deviation, worst device deviation, smallest gap to the cut)."""
    qs, phis, cc, orders, mask, short = minnorm_case(label)
    nq, n = len(qs), len(orders)
    thetas = np.arccos(qs * WAVELENGTH / (4 * np.pi))
    assert np.isfinite(thetas).all()
    e = CC.small_engine(lib_path)
    b, nv, rc, rank = e.cc_lstsq_deg2_minnorm(cc, mask, orders, thetas, phis)
    b0, nv0, rc0 = e.cc_lstsq_deg2(cc, mask, orders, thetas, phis)
    e.close()
    assert b.shape == (int(orders.max()) + 1, nq, nq) and rank.dtype == np.int32 and rank.shape == (nq, nq)
    assert np.array_equal(nv, mask.sum(-1)) and np.array_equal(nv, nv0) and np.array_equal(rc, rc0)
    deficient = (nv > 0) & ((nv < n) | (rc < 1e-12))
    assert {tuple(p) for p in np.argwhere(deficient)} == set(short), (np.argwhere(deficient), short)
    assert np.array_equal(b[:, ~deficient], b0[:, ~deficient]), 'a pair outside the list changed its bits'
    worst_np = worst_dev = worst_last = 0.0
    gap = np.inf
    devs = []
    for i in range(nq):
        for j in range(nq):
            m = mask[i, j]
            if not m.any():
                assert rank[i, j] == 0 and not np.any(b[:, i, j])
                continue
            A = MC.legendre_matrix(qs, phis, orders, i, j)[m]
            if not deficient[i, j]:
                assert rank[i, j] == n
                continue
            assert nv[i, j] == short[(i, j)]
            r_np, g_ij = check_gap(A, (label, i, j))
            gap = min(gap, g_ij)
            x_np, _, r_lapack, _ = np.linalg.lstsq(A, cc[i, j, m], rcond=None)
            assert r_np == r_lapack and rank[i, j] == r_lapack, (label, i, j, int(rank[i, j]), int(r_lapack))
            if r_lapack == A.shape[0]:                                             # full row rank
                ref, last = minnorm_longdouble(A, cc[i, j, m])
            else:                                                                  # identical rows: rank 1
                assert r_lapack == 1 and np.array_equal(A, np.broadcast_to(A[0], A.shape))
                a = A[0].astype(np.longdouble)
                ref, last = a * (cc[i, j, m].astype(np.longdouble).mean() / (a @ a)), 0.0
            scale = float(np.sqrt(ref @ ref))
            worst_last = max(worst_last, last)
            worst_np = max(worst_np, float(np.linalg.norm(np.asarray(x_np - ref, dtype=float))) / scale)
            dev = float(np.linalg.norm(np.asarray(b[orders, i, j].real - ref, dtype=float))) / scale
            devs.append(((i, j), dev))
            worst_dev = max(worst_dev, dev)
            assert not np.any(b[:, i, j].imag) and not np.any(np.delete(b[:, i, j], orders))
    bound = max(LSQ_MARGIN * worst_np, LSQ_FLOOR)
    print(f'minimum norm {label}: {len(short)} deficient pairs of {nq * nq}; LAPACK {worst_np:.2e}, device {worst_dev:.2e}, bound {bound:.2e}; '
          f'last correction of the yardstick {worst_last:.1e}; smallest gap to the cut {gap:.0f} x')
    assert short and worst_last <= bound / 100, ('the yardstick has not converged', label, worst_last, bound)
    assert worst_dev <= bound, (label, devs, bound)
    return worst_np, worst_dev, gap


def check_minnorm_public(lib_path):
    """through extract.masked_cross_correlation_to_deg2_invariant: the default still raises the pinned text; the opt-in returns
    numpy's solution for the starved pair and the bits of the default for a mask without one"""
    import pytest
    nq, L, nd = 5, 8, 70
    qs, phis, cc, avg, _ = CC.synthetic_cc(nq, L, nd, 27, 1, noise=1e-3)
    mask = MC.random_pair_masks(nq, nd)
    short = mask.copy()
    short[1, 4] = False
    short[1, 4, [3, 30, 31, 50]] = True
    e = CC.small_engine(lib_path)
    meta = MC.metadata(qs, phis, L, False, {}, avg, {'type': 'direct', 'direct': {'mask': short}}, 'lstsq')
    with pytest.raises(NotImplementedError, match=r'1 of 25 pairs are rank deficient.*\(q1, q2\) = \(1, 4\) with 4 valid samples'):
        X.masked_cross_correlation_to_deg2_invariant(e, cc, 3, **meta)
    with pytest.raises(NotImplementedError, match=r'1 of 25 pairs are rank deficient.*\(q1, q2\) = \(1, 4\) with 4 valid samples'):
        X.masked_cross_correlation_to_deg2_invariant(e, cc, 3, rank_deficient='raise', **meta)
    with pytest.raises(ValueError, match='rank_deficient'):
        X.masked_cross_correlation_to_deg2_invariant(e, cc, 3, rank_deficient='pinv', **meta)
    b, qq = X.masked_cross_correlation_to_deg2_invariant(e, cc, 3, rank_deficient='minimum_norm', **meta)
    A = MC.legendre_matrix(qs, phis, np.arange(L + 1), 1, 4)[short[1, 4]]
    check_gap(A, 'public')
    x = np.linalg.lstsq(A, cc[1, 4, short[1, 4]], rcond=None)[0]
    assert qq[1, 4] and not qq[2, 3] and np.linalg.norm(b[:, 1, 4].real - x) <= 1e-12 * np.linalg.norm(x)
    meta = MC.metadata(qs, phis, L, False, {}, avg, {'type': 'direct', 'direct': {'mask': mask}}, 'lstsq')
    b0, _ = X.masked_cross_correlation_to_deg2_invariant(e, cc, 3, **meta)
    b1, _ = X.masked_cross_correlation_to_deg2_invariant(e, cc, 3, rank_deficient='minimum_norm', **meta)
    assert np.array_equal(b0, b1)
    e.close()


# ---- composition, limits and refusals ----------------------------------------------------------------------------------------------------
class CountingEngine:
    """an engine that counts the calls of its cc_* methods"""

    def __init__(self, engine):
        self._engine, self.calls = engine, []

    def __getattr__(self, name):
        attr = getattr(self._engine, name)
        if name.startswith('cc_') and callable(attr):
            def counted(*a, **k):
                self.calls.append(name)
                return attr(*a, **k)
            return counted
        return attr


def check_composition(lib_path=None):
    """the stages run in the reference's order and the subtraction goes to the first of them; with none of the new keys the route is
    the ONE cc_prepare_masked call it was, with the same bits"""
    cc, qs, avg, phis, mask = golden_inputs(64)
    e = CountingEngine(CC.small_engine(lib_path))
    old = {'subtract_average_intensity': True, 'pi_periodicity': True, 'q1q2_symmetric': True, 'interpolate_masked': True}
    v, m, p = X.modify_masked_cross_correlation(e, cc.copy(), mask.copy(), phis, G_L, average_intensity=avg, **old)
    assert e.calls == ['cc_prepare_masked'] and np.array_equal(p, phis)
    ref, rm = MC.r_modify_masked(cc, mask, phis, avg, old)
    assert np.array_equal(m, rm) and rel_l2(v, ref) <= 1e-15
    v2, m2, _ = MC.prepare(e._engine, cc.copy(), mask.copy(), phis, avg, old)
    assert np.array_equal(v, v2) and np.array_equal(m, m2)
    e.calls.clear()
    X.modify_masked_cross_correlation(e, cc.copy(), mask.copy(), phis, G_L, average_intensity=avg, **MODIFY_VARIANTS['all'])
    assert e.calls == ['cc_lowpass_q', 'cc_harmonic_filter', 'cc_prepare_masked', 'cc_binned_mean', 'cc_prepare_masked'], e.calls
    e.calls.clear()
    v, m, p = X.modify_masked_cross_correlation(e, cc.copy(), mask.copy(), phis, G_L, average_intensity=avg, subtract_average_intensity=True,
                                                apply_binned_mean=True)
    assert e.calls == ['cc_binned_mean'] and len(p) == 2 * G_L
    ref, _ = r_binned_mean_longdouble(cc - avg[:, None, None] * avg[None, :, None], mask, phis, G_L)
    close(v, ref, 'subtraction folded into the binned mean')
    # low_pass_order_in_q: a bool of either value means no filter upstream (248)
    e.calls.clear()
    X.modify_masked_cross_correlation(e, cc.copy(), mask.copy(), phis, G_L, low_pass_order_in_q=True)
    assert e.calls == ['cc_prepare_masked']
    for key in ('low_pass_order_in_q', 'enforce_max_order', 'enforce_zero_odd_harmonics', 'apply_binned_mean'):
        assert X._wants_masked_route({'modify_cc': {key: 1.0 if key.startswith('low') else True}}), key
    assert not X._wants_masked_route({'modify_cc': {'apply_binned_mean': False, 'low_pass_order_in_q': False}})
    e._engine.close()


def check_limits(lib_path=None):
    """n_q or n_delta of 5000 come back as an error code with a message that names the operator and the size, and NaN-filled outputs
    stay NaN; so do a section with a0 != 1, no filter asked for, and bin offsets that do not rise to n_delta"""
    e = CC.small_engine(lib_path)
    small, smask = _lib.as_f64(np.zeros((2, 2, 8))), np.ones((2, 2, 8), np.uint8)
    tab = _lib.as_f64(np.linspace(0.5, 0.6, 8))
    sos = _lib.as_f64(np.array([0.5, 0.5, 0.0, 1.0, -0.1, 0.0]))
    start = np.array([0, 4, 8], dtype=np.int32)
    out, mout = np.full((2, 2, 8), np.nan), np.full((2, 2, 8), 9, np.uint8)
    lib, p = e.lib, _lib.ptr

    def refused(r, op, word):
        msg = lib.mtip_last_error(e.ctx).decode()
        assert r != 0 and op in msg and word in msg, (op, word, r, msg)
        assert np.isnan(out).all() and (mout == 9).all()
    for nq, nd, word in ((2, 5000, 'n_delta'), (5000, 8, 'n_q')):
        refused(lib.mtip_op_cc_lowpass_q(e.ctx, nq, nd, p(sos), p(small), None, p(out)), 'cc_lowpass_q', word)
        refused(lib.mtip_op_cc_harmonic_filter(e.ctx, nq, nd, 2, 1, p(small), None, p(out)), 'cc_harmonic_filter', word)
        refused(lib.mtip_op_cc_binned_mean(e.ctx, nq, nd, 2, p(start), 0, p(small), p(smask), None, p(out), p(mout)), 'cc_binned_mean', word)
    refused(lib.mtip_op_cc_lowpass_q(e.ctx, 2, 8, p(_lib.as_f64(np.array([0.5, 0.5, 0.0, 2.0, -0.1, 0.0]))), p(small), None, p(out)),
            'cc_lowpass_q', 'a0 = 1')
    refused(lib.mtip_op_cc_harmonic_filter(e.ctx, 2, 8, -1, 0, p(small), None, p(out)), 'cc_harmonic_filter', 'zero_odd')
    for bad in ([0, 4, 7], [0, 4, 4], [1, 4, 8]):
        refused(lib.mtip_op_cc_binned_mean(e.ctx, 2, 8, 2, p(np.array(bad, dtype=np.int32)), 0, p(small), p(smask), None, p(out), p(mout)),
                'cc_binned_mean', 'bin_start')
    refused(lib.mtip_op_cc_binned_mean(e.ctx, 2, 8, 2, p(start), 8, p(small), p(smask), None, p(out), p(mout)), 'cc_binned_mean', 'n_roll')
    # the minimum-norm entry keeps the limits of mtip_op_cc_lstsq_deg2
    bout = np.full((70, 2, 2), np.nan, complex)
    nv, rc, rank = np.full((2, 2), -7, np.int32), np.full((2, 2), np.nan), np.full((2, 2), -7, np.int32)
    orders = np.arange(70, dtype=np.int32)
    for (nq, nd, n), word in (((2, 8, 65), 'orders'), ((2, 5000, 3), 'n_delta'), ((5000, 8, 3), 'n_q')):
        r = lib.mtip_op_cc_lstsq_deg2_minnorm(e.ctx, nq, nd, n, p(orders), p(small), p(smask), p(tab), p(tab), p(bout), p(nv), p(rc), p(rank))
        msg = lib.mtip_last_error(e.ctx).decode()
        assert r != 0 and 'cc_lstsq_deg2_minnorm' in msg and word in msg, (nq, nd, n, r, msg)
        assert np.isnan(bout).all() and np.isnan(rc).all() and (nv == -7).all() and (rank == -7).all()
    # the prepare operator still refuses flag bit 16: the new stages have entry points of their own
    status = np.full(2, -7, np.int32)
    r = lib.mtip_op_cc_prepare_masked(e.ctx, 2, 8, 16, p(small), p(smask), p(tab), p(smask.ravel()), p(tab), p(out), p(mout), p(status))
    assert r != 0 and 'flag' in lib.mtip_last_error(e.ctx).decode()
    e.close()


def check_refusals(lib_path=None):
    """before any launch: a cutoff outside (0, n_q / 2) raises ValueError as scipy does; a grid that leaves a bin without a sample
    raises ValueError; the unmasked operator keeps refusing the four keys"""
    import pytest
    from scipy.signal import butter
    cc, qs, avg, phis, mask = golden_inputs(64)
    e = CountingEngine(CC.small_engine(lib_path))
    for value in (0.0, -1.0, G_NQ / 2, 10.0, np.nan):
        if np.isfinite(value):
            with pytest.raises(ValueError):                                       # scipy itself
                butter(1, value, 'lp', fs=G_NQ, output='sos')
        with pytest.raises(ValueError, match='low_pass_order_in_q'):
            X.modify_masked_cross_correlation(e, cc.copy(), mask.copy(), phis, G_L, low_pass_order_in_q=value)
    gappy = np.delete(phis, np.arange(20, 28))                                      # no angle left in bin 6
    with pytest.raises(ValueError, match='apply_binned_mean'):
        X.binned_mean_tables(gappy, G_L)
    with pytest.raises(ValueError, match='apply_binned_mean'):
        X.modify_masked_cross_correlation(e, np.delete(cc, np.arange(20, 28), axis=-1), np.delete(mask, np.arange(20, 28), axis=-1), gappy,
                                          G_L, apply_binned_mean=True)
    with pytest.raises(ValueError, match='apply_binned_mean'):
        X.binned_mean_tables(phis[:12], G_L)                                        # fewer angles than bins
    assert e.calls == [], e.calls
    for key, value in (('low_pass_order_in_q', 1.0), ('enforce_max_order', True), ('enforce_zero_odd_harmonics', True),
                       ('apply_binned_mean', True)):
        with pytest.raises(NotImplementedError, match=key):
            X.cross_correlation_to_deg2_invariant(e, cc.copy(), 3, **CC.metadata(qs, phis, G_L, True, {key: value}, avg))
    e._engine.close()

"""Cases of `extract` on MASKED cross-correlation data (csrc/k_extract_lsq.h, Engine.cc_prepare_masked / cc_lstsq_deg2,
extract.cross_correlation_mask / masked_cross_correlation_to_deg2_invariant), shared by tests/test_ccmask_reference.py (CPU: restatement
and host masks against G27), tests/test_emul_ccmask.py (the unchanged kernel source on the CPU emulator) and tests/test_gpu_ccmask.py.

Two yardsticks:
  * G27 (tests/golden/cc_masked.npz, written by tests/golden/make_golden_ccmask.py): outputs of the reference's own
    cross_correlation_mask, modify_cross_correlation, interpolate, bl_3d_least_squares_worker and
    ccd_to_deg2_invariant_3d_back_substitution on the data of G24 (16 shells, L = 8, 64 angles);
  * for sizes the fixture cannot hold, the numpy / scipy restatement below (held to G27 by a CPU test) and, for the least squares, a
    longdouble-refined solution: the device gets 10 x LAPACK's own worst error against it (floor 1e-13)."""
import os

import numpy as np

import ccextract_cases as CC
from helpers import rel_l2
from xframe_amd.fxs import _lib, extract as X

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'cc_masked.npz')
WAVELENGTH = CC.WAVELENGTH
TOL_OP, TOL_FLOW = CC.TOL_OP, CC.TOL_FLOW
LSQ_MARGIN, LSQ_FLOOR = 10.0, 1e-13

# name -> cc_mask settings of the generators (the 'direct' array is made by direct_mask below and stored in G27)
MASK_SETTINGS = {
    'none': {'type': 'none'},
    'custom': {'type': 'pixel_custom', 'pixel_custom': {'n_masked_pixels_phi': 0.05, 'n_masked_pixels_q': 0.1, 'mask_at_pi': False}},
    'custom_pi': {'type': 'pixel_custom', 'pixel_custom': {'n_masked_pixels_phi': 0.05, 'n_masked_pixels_q': 0.1, 'mask_at_pi': True}},
    'flat': {'type': 'pixel_flat', 'pixel_flat': {'pixel_size': 70.0, 'mask_at_pi': False}},
    'flat_pi': {'type': 'pixel_flat', 'pixel_flat': {'pixel_size': 70.0, 'mask_at_pi': True}},
    'flat_wide': {'type': 'pixel_flat', 'pixel_flat': {'pixel_size': 300.0, 'mask_at_pi': False}},
    'arc': {'type': 'pixel_arc', 'pixel_arc': {'pixel_size': 70.0, 'mask_at_pi': False}},
    'arc_pi': {'type': 'pixel_arc', 'pixel_arc': {'pixel_size': 70.0, 'mask_at_pi': True}},
}
LSQ_MASKS = ('flat', 'none')                          # masks of the least-squares cases of G27
# name -> modify_cc switches of the prepare cases of G27, all on the 'direct' mask
PREPARE_VARIANTS = {
    'sub': {'subtract_average_intensity': True},
    'pi': {'pi_periodicity': True},
    'sym': {'q1q2_symmetric': True},
    'interp': {'interpolate_masked': True},
    'all': {'subtract_average_intensity': True, 'pi_periodicity': True, 'q1q2_symmetric': True, 'interpolate_masked': True},
}
# name -> (mask name, bl_extraction_method) of the flows of G27 (modify_cc = CC.FLOW_MODIFY, bl_q_limits none, bl_enforce_psd)
FLOWS = {'flat_lstsq': ('flat', 'lstsq'), 'flat_wide_lstsq': ('flat_wide', 'lstsq'), 'direct_backsub': ('direct', 'back_substitution')}


def direct_mask(nq, nd, seed=27):
    """interior holes: a band around pi in the pairs near the diagonal, scattered single samples everywhere, the rows (3, 5) and
    (5, 3) fully masked; samples 0 and nd - 1 stay valid in every other row"""
    rng = np.random.default_rng(seed)
    m = np.ones((nq, nq, nd), dtype=bool)
    near = np.abs(np.arange(nq)[:, None] - np.arange(nq)[None, :]) <= 2
    band = np.zeros(nd, dtype=bool)
    band[nd // 2 - 3:nd // 2 + 4] = True
    m[near[:, :, None] & band[None, None, :]] = False
    m[rng.random(m.shape) < 0.03] = False
    m[..., 0] = m[..., -1] = True
    m[3, 5] = m[5, 3] = False
    return m


def grid_of(qs, phis):
    return {'qs': qs, 'thetas': np.arccos(qs * WAVELENGTH / (4 * np.pi)), 'phis': phis.copy()}


def metadata(qs, phis, max_order, zero_odd, modify_cc, avg, cc_mask, mode):
    m = CC.metadata(qs, phis, max_order, zero_odd, modify_cc, avg, mode=mode)
    m['cc_mask'] = cc_mask
    return m


def mask_settings(name, g=None):
    return {'type': 'direct', 'direct': {'mask': g['G27_mask_direct'].copy()}} if name == 'direct' else MASK_SETTINGS[name]


def golden_inputs():
    g24 = CC.load_golden()
    cc = g24['G24_cc']
    phis = np.arange(cc.shape[-1]) * 2 * np.pi / cc.shape[-1]
    return cc, g24['G24_qs'], g24['G24_avg'], phis, int(g24['G24_L'])


def load_golden():
    return np.load(GOLDEN)


# ---- numpy / scipy restatement ----------------------------------------------------------------------------------------------------------
def r_modify_masked(cc, mask, phis, avg, modify_cc):
    """modify_cross_correlation with a mask (fxs_invariant_tools.py:235-289; masked_mean mathLibrary.py:1346-1351; interpolate 335-351)"""
    cc, mask = np.array(cc, dtype=float), np.array(mask, dtype=bool)
    if modify_cc.get('subtract_average_intensity', False):
        cc -= avg[:, None, None] * avg[None, :, None]
    if modify_cc.get('pi_periodicity', False):
        bad = (phis < np.pi / 2) | (phis >= 3 * np.pi / 2)
        cc[..., bad] = 0
        cc += np.roll(cc, len(phis) // 2, axis=-1)
        mask = mask | np.roll(mask, len(phis) // 2, axis=-1)
    if modify_cc.get('q1q2_symmetric', False):
        sw, msw = cc.copy(), mask.copy()
        sw[..., 1:] = cc[..., 1:][..., ::-1]
        msw[..., 1:] = mask[..., 1:][..., ::-1]
        data, masks = [np.swapaxes(sw, 0, 1), cc], [np.swapaxes(msw, 0, 1), mask]
        counts = np.sum(masks, axis=0)
        total = np.sum(data, where=masks, axis=0)
        nz = counts != 0
        total[nz] = total[nz] / counts[nz]
        cc, mask = total, counts.astype(bool)
    if modify_cc.get('interpolate_masked', False):
        cc, mask = r_interpolate(cc, mask, phis), np.ones_like(mask)
    return cc, mask


def r_interpolate(cc, mask, phis):
    from scipy.interpolate import interp1d
    out = np.array(cc, dtype=float).reshape(-1, len(phis))
    for d, m in zip(out, mask.reshape(-1, len(phis))):
        if m.any():
            d[~m] = interp1d(phis[m], d[m])(phis[~m])
    return out.reshape(cc.shape)


def legendre_matrix(qs, phis, orders, q1, q2):
    """ccd_legendre_matrices (76-97) of one pair: (n_delta, n_orders)"""
    from scipy.special import eval_legendre
    th = np.arccos(qs * WAVELENGTH / (4 * np.pi))
    x = np.cos(th[q1]) * np.cos(th[q2]) + np.sin(th[q1]) * np.sin(th[q2]) * np.cos(phis)
    return (1 / (4 * np.pi) * eval_legendre(np.asarray(orders)[:, None], x[None, :])).T


def r_lstsq(cc, mask, qs, phis, orders):
    """bl_3d_least_squares_worker (485-517) over all pairs: (Nq, Nq, n_orders) real, zeros where a pair has no valid sample"""
    nq = len(qs)
    out = np.zeros((nq, nq, len(orders)))
    for i in range(nq):
        for j in range(nq):
            m = mask[i, j]
            if m.any():
                out[i, j] = np.linalg.lstsq(legendre_matrix(qs, phis, orders, i, j)[m], cc[i, j, m], rcond=None)[0]
    return out


def refined_lstsq(A, b, passes=4):
    """the yardstick of the cases beyond the fixture: numpy's least-squares solution, then `passes` rounds of residual refinement in
    longdouble.  The refinement is the one that converges for a least-squares problem (Bjorck's, on the augmented system
    r + A x = b, A^T r = 0): BOTH residuals f = b - r - A x and g = -A^T r are taken in longdouble and the corrections come from a
    double-precision QR of A,  z = R^-T g,  dx = R^-1 (Q^T f - z),  dr = f - A dx.
    Refining x alone (x += lstsq(A, b - A x)) does NOT converge when the residual is not zero: the correction is A^+ r with r almost
    orthogonal to range(A), and its error eps cond^2 |r| is the very term being measured.  Measured at 8 x L63 x 256 against a
    Householder solution computed entirely in longdouble (worst pair, full rows / 1/64 masked): that variant stays at LAPACK's own
    solution, 1.3e-12 / 6.4e-12 from the truth, and so reports LAPACK's error as 2.7e-14 / 9.7e-14; this one is within 1.5e-15 and
    reports LAPACK's error as 1.3e-12 / 6.3e-12.  Returns (x longdouble, relative size of the last correction)."""
    Q, R = np.linalg.qr(A)
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    x = np.linalg.lstsq(A, b, rcond=None)[0].astype(np.longdouble)
    r = bl - Al @ x
    last = np.inf
    for _ in range(passes):
        f = np.asarray(bl - r - Al @ x, dtype=float)
        g = np.asarray(-(Al.T @ r), dtype=float)
        z = np.linalg.solve(R.T, g)
        dx = np.linalg.solve(R, Q.T @ f - z)
        r = r + (f - A @ dx)
        x = x + dx
        last = float(np.linalg.norm(dx) / np.linalg.norm(np.asarray(x, dtype=float)))
    return x, last


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def check_masks_golden(g):
    """case 1: the four generators (and 'none') against the reference's, exact equality, mask_at_pi on and off; an unknown type asserts
    with the reference's text"""
    import pytest
    _, qs, _, phis, _ = golden_inputs()
    for name, setting in MASK_SETTINGS.items():
        m = X.cross_correlation_mask(grid_of(qs, phis), {'cc_mask': setting, 'xray_wavelength': WAVELENGTH})
        ref = g['G27_mask_' + name]
        assert m.dtype == bool and m.shape == ref.shape, name
        assert np.array_equal(m, ref), (name, int((m != ref).sum()))
        print(f'mask {name}: {int((~m).sum())} of {m.size} samples masked, equal')
    d = g['G27_mask_direct']
    assert X.cross_correlation_mask(grid_of(qs, phis), {'cc_mask': {'type': 'direct', 'direct': {'mask': d}}}) is d or \
        np.array_equal(X.cross_correlation_mask(grid_of(qs, phis), {'cc_mask': {'type': 'direct', 'direct': {'mask': d}}}), d)
    with pytest.raises(AssertionError, match='Given Cross-Correlation mask type "custom" not known. Known types are'):
        X.cross_correlation_mask(grid_of(qs, phis), {'cc_mask': {'type': 'custom'}})


def check_restatement_golden(g):
    """the numpy / scipy restatement of this file against the reference's own outputs"""
    cc, qs, avg, phis, L = golden_inputs()
    d = g['G27_mask_direct']
    for name, mod in PREPARE_VARIANTS.items():
        v, m = r_modify_masked(cc, d, phis, avg, mod)
        assert np.array_equal(m, g[f'G27_prep_{name}_mask']), name
        e = rel_l2(v, g[f'G27_prep_{name}_cc'])
        print(f'restatement prepare {name}: {e:.2e}')
        assert e <= 1e-15, (name, e)
    for mname in LSQ_MASKS:
        for oname, orders in (('even', np.arange(0, L + 1, 2)), ('all', np.arange(L + 1))):
            e = rel_l2(r_lstsq(cc, g['G27_mask_' + mname], qs, phis, orders), g[f'G27_lstsq_{mname}_{oname}'])
            print(f'restatement lstsq {mname} {oname}: {e:.2e}')
            assert e <= 1e-13, (mname, oname, e)


def prepare(e, cc, mask, phis, avg, mod):
    kw = {}
    if mod.get('subtract_average_intensity', False):
        kw['average_intensity'] = avg
    if mod.get('pi_periodicity', False):
        kw['bad_angles'] = (phis < np.pi / 2) | (phis >= 3 * np.pi / 2)
    if mod.get('interpolate_masked', False):
        kw['interpolate_phis'] = phis
    return e.cc_prepare_masked(cc, mask, q1q2_symmetric=bool(mod.get('q1q2_symmetric', False)), **kw)


def check_prepare_golden(g, lib_path=None):
    """case 2: the prepare kernel against modify_cross_correlation of the reference: every switch alone, then all together, on the
    direct mask: masks equal, values within TOL_OP, no row reported as impossible to interpolate"""
    cc, qs, avg, phis, _ = golden_inputs()
    e = CC.small_engine(lib_path)
    d = g['G27_mask_direct']
    for name, mod in PREPARE_VARIANTS.items():
        v, m, status = prepare(e, cc.copy(), d.copy(), phis, avg, mod)
        ref = g[f'G27_prep_{name}_cc']
        err = rel_l2(v, ref)
        print(f'prepare vs G27 {name}: {err:.2e}, worst sample {np.abs(v - ref).max() / np.abs(ref).max():.2e}')
        assert m.dtype == bool and np.array_equal(m, g[f'G27_prep_{name}_mask']), name
        assert status[0] == 0, (name, status)
        assert err <= TOL_OP and np.abs(v - ref).max() <= TOL_OP * np.abs(ref).max(), (name, err)
    # with an all-true mask the kernel is today's unmasked arithmetic
    v, m, _ = prepare(e, cc.copy(), np.ones_like(d), phis, avg, PREPARE_VARIANTS['all'])
    ref = CC.r_modify(cc, phis, avg, PREPARE_VARIANTS['all'])
    assert m.all() and rel_l2(v, ref) <= 1e-15
    e.close()


def check_interpolation_scipy(lib_path=None):
    """case 2, interpolation: a seeded 5 x 5 x 200 array with random holes (ends valid), one fully masked row and one fully valid
    row, against scipy.interpolate.interp1d directly; then what scipy raises ValueError for must be reported and raised, never
    extrapolated: Delta = 0 masked, the last angle masked, a row with a single valid sample"""
    import pytest
    rng = np.random.default_rng(5)
    nq, nd = 5, 200
    phis = np.arange(nd) * 2 * np.pi / nd
    cc = rng.normal(size=(nq, nq, nd))
    mask = rng.random((nq, nq, nd)) > 0.3
    mask[0, 1, 60:140] = False                                                    # a hole longer than a 64-sample word
    mask[..., 0] = mask[..., -1] = True
    mask[2, 2] = False
    mask[4, 0] = True
    e = CC.small_engine(lib_path)
    v, m, status = e.cc_prepare_masked(cc, mask, interpolate_phis=phis)
    ref = r_interpolate(cc, mask, phis)
    err = np.abs(v - ref).max()
    print(f'interpolation vs scipy: max abs deviation {err:.2e} on {int((~mask).sum())} masked samples')
    assert status == (0, np.iinfo(np.int32).max) and m.all()
    assert err <= TOL_OP * np.abs(ref).max()
    assert np.array_equal(v[mask], cc[mask]) and np.array_equal(v[2, 2], cc[2, 2])
    qs = CC.radial_points(nq)
    for what, bad_mask, first in (('first', 0, (1, 2)), ('last', nd - 1, (3, 0)), ('single', None, (4, 4))):
        mk = mask.copy()
        if bad_mask is None:
            mk[first] = False
            mk[first][77] = True
        else:
            mk[first][bad_mask] = False
        with pytest.raises(ValueError):                                           # scipy itself
            r_interpolate(cc, mk, phis)
        _, _, status = e.cc_prepare_masked(cc, mk, interpolate_phis=phis)
        assert status == (1, first[0] * nq + first[1]), (what, status)
        meta = metadata(qs, phis, 4, True, {'interpolate_masked': True}, np.ones(nq), {'type': 'direct', 'direct': {'mask': mk}}, 'lstsq')
        with pytest.raises(ValueError, match=r'\(q1, q2\) = \(%d, %d\)' % first):
            X.masked_cross_correlation_to_deg2_invariant(e, cc, 3, **meta)
    e.close()


def check_lstsq_golden(g, lib_path=None):
    """case 3: the least-squares kernel against bl_3d_least_squares_worker of the reference, even orders and all orders, on a
    pixel_flat mask that leaves pairs without any sample, and on the all-true mask: whole array within TOL_OP (the condition numbers
    are 5 .. 10 here); zeros and qq_mask False exactly where a pair has no sample"""
    cc, qs, avg, phis, L = golden_inputs()
    e = CC.small_engine(lib_path)
    for mname in LSQ_MASKS:
        mask = g['G27_mask_' + mname]
        for oname, zero_odd in (('even', True), ('all', False)):
            meta = metadata(qs, phis, L, zero_odd, {}, avg, MASK_SETTINGS[mname], 'lstsq')
            b, qq = X.masked_cross_correlation_to_deg2_invariant(e, cc.copy(), 3, **meta)
            orders = np.arange(0, L + 1, 2 if zero_odd else 1)
            ref = np.zeros((L + 1,) + cc.shape[:2], complex)
            ref[orders] = np.moveaxis(g[f'G27_lstsq_{mname}_{oname}'], -1, 0)
            err = rel_l2(b, ref)
            print(f'lstsq vs G27 {mname} {oname}: {err:.2e}; pairs without a sample: {int((~qq).sum())}')
            assert b.shape == ref.shape and b.dtype == np.complex128 and qq.dtype == bool
            assert err <= TOL_OP, (mname, oname, err)
            assert np.array_equal(qq, mask.any(-1))
            assert not np.any(b[:, ~qq]) and not np.any(b.imag)
            if zero_odd:
                assert not np.any(b[1::2])
    e.close()


def periodic_mask(nq, nd, fraction):
    """`fraction` of the angles masked in every pair, half around Delta = 0 and half around pi"""
    m = np.ones((nq, nq, nd), dtype=bool)
    w = int(round(nd * fraction / 4))
    if w:
        m[..., :w] = m[..., nd - w:] = False
        m[..., nd // 2 - w:nd // 2 + w] = False
    return m


def check_lstsq_refined(lib_path, nq, L, zero_odd, nd, mask, label, seed=27):
    """cases 4 and 5: the kernel against the longdouble-refined solution, per pair relative error; bound = LSQ_MARGIN x the worst
    relative error of numpy's own solution against the same yardstick in this case (a blocked reduction in another order may differ
    by a small multiple), floor LSQ_FLOOR.  Returns (worst LAPACK error, worst device error, worst condition number)."""
    stride = 2 if zero_odd else 1
    orders = np.arange(0, L + 1, stride)
    qs, phis, cc, _, _ = CC.synthetic_cc(nq, L, nd, seed, stride, noise=1e-3)
    e = CC.small_engine(lib_path)
    b, nv, rc = e.cc_lstsq_deg2(cc, mask, orders, np.arccos(qs * WAVELENGTH / (4 * np.pi)), phis)
    e.close()
    assert b.shape == (int(orders.max()) + 1, nq, nq) and nv.dtype == np.int32 and np.array_equal(nv, mask.sum(-1))
    worst_np = worst_dev = worst_cond = worst_last = 0.0
    for i in range(nq):
        for j in range(nq):
            m = mask[i, j]
            if not m.any():
                assert not np.any(b[:, i, j]) and rc[i, j] == 0
                continue
            A = legendre_matrix(qs, phis, orders, i, j)[m]
            ref, last = refined_lstsq(A, cc[i, j, m])
            worst_last = max(worst_last, last)
            scale = float(np.linalg.norm(np.asarray(ref, dtype=float)))
            x_np = np.linalg.lstsq(A, cc[i, j, m], rcond=None)[0]
            worst_np = max(worst_np, float(np.linalg.norm(np.asarray(x_np - ref, dtype=float))) / scale)
            worst_dev = max(worst_dev, float(np.linalg.norm(np.asarray(b[orders, i, j].real - ref, dtype=float))) / scale)
            sv = np.linalg.svd(A, compute_uv=False)
            worst_cond = max(worst_cond, sv[0] / sv[-1])
            assert 0 < rc[i, j] <= 1
    bound = max(LSQ_MARGIN * worst_np, LSQ_FLOOR)
    print(f'lstsq vs refined {label}: {nq} x {len(orders)} orders x {nd}: cond <= {worst_cond:.1e}; LAPACK {worst_np:.2e}, '
          f'device {worst_dev:.2e}, bound {bound:.2e}; last correction of the yardstick {worst_last:.1e}')
    # the yardstick has to be a hundred times finer than the bound it serves.  Its last correction stalls at the rounding of the
    # longdouble residuals times the conditioning (eps 1.1e-19 x cond: 1e-15 at cond 8e3, where the bound is 1e-11), so the
    # requirement is relative to the bound of the case -- at the floor of the bound it is 1e-15.
    assert worst_last <= bound / 100, ('the yardstick has not converged', label, worst_last, bound)
    assert worst_dev <= bound, (label, worst_dev, bound)
    if zero_odd:
        assert not np.any(b[1::2])
    return worst_np, worst_dev, worst_cond


REFINED_SHAPES = {                                    # label -> (nq, L, zero_odd, n_delta, masked fraction)
    '16xL8_even': (16, 8, True, 64, 1 / 16), '16xL8_all': (16, 8, False, 64, 1 / 16),
    '12xL32_even': (12, 32, True, 200, 1 / 25), '12xL32_all': (12, 32, False, 200, 1 / 25),
    '8xL63_full': (8, 63, False, 256, 0.0), '8xL63_masked': (8, 63, False, 256, 1 / 64),
}


def check_lstsq_shape(lib_path, label):
    nq, L, zero_odd, nd, fraction = REFINED_SHAPES[label]
    return check_lstsq_refined(lib_path, nq, L, zero_odd, nd, periodic_mask(nq, nd, fraction), label)


def random_pair_masks(nq=5, nd=70, seed=9):
    """per-pair random masks with 20 .. 70 valid samples (both sides of one 64-row block), one pair without any sample"""
    rng = np.random.default_rng(seed)
    m = np.zeros((nq, nq, nd), dtype=bool)
    counts = rng.integers(20, nd + 1, size=(nq, nq))
    counts[0, 0], counts[0, 1], counts[1, 0], counts[4, 4] = nd, 64, 63, 65
    for i in range(nq):
        for j in range(nq):
            m[i, j, rng.permutation(nd)[:counts[i, j]]] = True
    m[2, 3] = False
    return m


def check_lstsq_random_masks(lib_path):
    """case 5, last row: compaction that differs per pair, and through the public function: zeros and qq_mask False for the pair
    without a sample; a pair with fewer valid samples than orders raises NotImplementedError"""
    import pytest
    nq, L, nd = 5, 8, 70
    mask = random_pair_masks(nq, nd)
    out = check_lstsq_refined(lib_path, nq, L, False, nd, mask, '5xL8_random')
    qs, phis, cc, avg, _ = CC.synthetic_cc(nq, L, nd, 27, 1, noise=1e-3)
    e = CC.small_engine(lib_path)
    meta = metadata(qs, phis, L, False, {}, avg, {'type': 'direct', 'direct': {'mask': mask}}, 'lstsq')
    b, qq = X.masked_cross_correlation_to_deg2_invariant(e, cc, 3, **meta)
    assert not qq[2, 3] and qq.sum() == nq * nq - 1 and not np.any(b[:, 2, 3]) and np.all(np.any(b[:, qq] != 0, axis=0))
    short = mask.copy()
    short[1, 4] = False
    short[1, 4, [3, 30, 31, 50]] = True                                           # 4 samples, 9 orders
    meta = metadata(qs, phis, L, False, {}, avg, {'type': 'direct', 'direct': {'mask': short}}, 'lstsq')
    with pytest.raises(NotImplementedError, match=r'1 of 25 pairs are rank deficient.*\(q1, q2\) = \(1, 4\) with 4 valid samples'):
        X.masked_cross_correlation_to_deg2_invariant(e, cc, 3, **meta)
    with pytest.raises(NotImplementedError, match='dimensions = 2'):
        X.masked_cross_correlation_to_deg2_invariant(e, cc, 2, **meta)
    e.close()
    return out


def check_limits(lib_path=None):
    """case 6: 65 orders, n_delta = 5000 and n_q = 5000 come back as an error code with a message from both operators, and a
    NaN-filled output stays NaN"""
    e = CC.small_engine(lib_path)
    small, smask = _lib.as_f64(np.zeros((2, 2, 8))), np.ones((2, 2, 8), np.uint8)
    tab = _lib.as_f64(np.linspace(0.0, 0.1, 8))
    out = np.full((70, 2, 2), np.nan, complex)
    nv, rc = np.full((2, 2), -7, np.int32), np.full((2, 2), np.nan)
    orders = np.arange(70, dtype=np.int32)
    for (nq, nd, n), word in (((2, 8, 65), 'orders'), ((2, 5000, 3), 'n_delta'), ((5000, 8, 3), 'n_q')):
        r = e.lib.mtip_op_cc_lstsq_deg2(e.ctx, nq, nd, n, _lib.ptr(orders), _lib.ptr(small), _lib.ptr(smask), _lib.ptr(tab), _lib.ptr(tab),
                                        _lib.ptr(out), _lib.ptr(nv), _lib.ptr(rc))
        msg = e.lib.mtip_last_error(e.ctx).decode()
        assert r != 0 and 'cc_lstsq_deg2' in msg and word in msg, (nq, nd, n, r, msg)
        assert np.isnan(out).all() and np.isnan(rc).all() and (nv == -7).all()
    bad_orders = np.array([0, 2, 2], dtype=np.int32)
    r = e.lib.mtip_op_cc_lstsq_deg2(e.ctx, 2, 8, 3, _lib.ptr(bad_orders), _lib.ptr(small), _lib.ptr(smask), _lib.ptr(tab), _lib.ptr(tab),
                                    _lib.ptr(out), _lib.ptr(nv), _lib.ptr(rc))
    assert r != 0 and 'increasing' in e.lib.mtip_last_error(e.ctx).decode() and np.isnan(out).all()
    vout, mout, status = np.full((2, 2, 8), np.nan), np.full((2, 2, 8), 9, np.uint8), np.full(2, -7, np.int32)
    for (nq, nd, flags), word in (((2, 5000, 0), 'n_delta'), ((5000, 8, 0), 'n_q'), ((2, 8, 16), 'flag'), ((2, 7, 2), 'pi_periodicity')):
        r = e.lib.mtip_op_cc_prepare_masked(e.ctx, nq, nd, flags, _lib.ptr(small), _lib.ptr(smask), _lib.ptr(tab), _lib.ptr(smask.ravel()),
                                            _lib.ptr(tab), _lib.ptr(vout), _lib.ptr(mout), _lib.ptr(status))
        msg = e.lib.mtip_last_error(e.ctx).decode()
        assert r != 0 and 'cc_prepare_masked' in msg and word in msg, (nq, nd, flags, r, msg)
        assert np.isnan(vout).all() and (mout == 9).all() and (status == -7).all()
    with __import__('pytest').raises(_lib.MtipError, match='64 extracted orders'):
        e.cc_lstsq_deg2(np.zeros((2, 2, 140)), np.ones((2, 2, 140), bool), np.arange(65), tab[:2], np.zeros(140))
    e.close()


def flow_settings(g, L, flow):
    mname, method = FLOWS[flow]
    s = CC.flow_settings(L, CC.MASK_CASES['none'])
    d = s['cross_correlation']['datasets']['I1I1']
    d['cc_mask'] = mask_settings(mname, g)
    d['bl_extraction_method'] = method
    return s


def check_flow_golden(g, lib_path=None):
    """case 7: extract_from_cross_correlation on the data of G24 with pixel_flat + lstsq (a mask that leaves pairs without a sample,
    and a wider one that leaves every pair solvable) and with a direct interior mask + back_substitution: deg_2_invariant, the masks
    and q_id_limits against the reference's chain, V_l through V V^+ at TOL_FLOW; with cc_mask none + back_substitution the flow is
    bit-equal to cross_correlation_to_deg2_invariant called directly (the unmasked path is the one taken)"""
    cc, qs, avg, phis, L = golden_inputs()
    g24 = CC.load_golden()
    e = CC.small_engine(lib_path)
    for flow in FLOWS:
        data = X.extract_from_cross_correlation(e, CC.golden_ccd(g24), flow_settings(g, L, flow))
        assert np.array_equal(data['deg_2_invariant_masks']['I1I1'], g[f'G27_flow_{flow}_mask']), flow
        assert np.array_equal(data['deg_2_invariant_q_id_limits']['I1I1'], g[f'G27_flow_{flow}_qid']), flow
        ref_b = g[f'G27_flow_{flow}_b']
        d = rel_l2(data['deg_2_invariant']['I1I1'], ref_b)
        print(f'flow {flow}: constrained B_l {d:.2e}; q_id_limits {g[f"G27_flow_{flow}_qid"][0].tolist()}')
        assert d <= TOL_FLOW, (flow, d)
        pms = data['data_projection_matrices']
        assert len(pms) == L + 1
        for l in range(L + 1):
            ref = g[f'G27_flow_{flow}_pm{l}']
            assert pms[l].shape == ref.shape, (flow, l, pms[l].shape, ref.shape)
            vv, rr = pms[l] @ pms[l].conj().T, ref @ ref.conj().T
            scale = max(np.linalg.norm(ref_b[l]), 1e-300)
            assert np.linalg.norm(vv - rr) <= TOL_FLOW * scale, (flow, l, np.linalg.norm(vv - rr) / scale)
    s = CC.flow_settings(L, CC.MASK_CASES['none'], enforce_psd=False, modify_cc={})
    data = X.extract_from_cross_correlation(e, CC.golden_ccd(g24), s)
    direct, qq = X.cross_correlation_to_deg2_invariant(e, cc.copy(), 3, **CC.metadata(qs, phis, L, True, {}, avg))
    assert np.array_equal(data['deg_2_invariant']['I1I1'], direct) and qq.all()
    e.close()


def check_back_substitution_golden(g, lib_path=None):
    """back_substitution on masked data against ccd_to_deg2_invariant_3d_back_substitution of the reference (interpolation first,
    605-608): B_l within TOL_OP, qq_mask all true (609 after 287)"""
    cc, qs, avg, phis, L = golden_inputs()
    e = CC.small_engine(lib_path)
    meta = metadata(qs, phis, L, True, {}, avg, mask_settings('direct', g), 'back_substitution')
    b, qq = X.masked_cross_correlation_to_deg2_invariant(e, cc.copy(), 3, **meta)
    ref = np.zeros_like(b)
    ref[::2] = np.moveaxis(g['G27_backsub_direct_b'], -1, 0)
    err = rel_l2(b, ref)
    print(f'back substitution on the direct mask vs G27: {err:.2e}')
    assert err <= TOL_OP and np.array_equal(qq, g['G27_backsub_direct_qq_mask']) and qq.all()
    e.close()


def check_end_to_end_correlator(lib_path=None, n_q=16, L=4, n_phi=64, P=8):
    """case 8: a small seeded stack of patterns -> Correlator.result() -> io.load_ccd -> extract_from_cross_correlation with
    pixel_custom + lstsq -> V_l, without an exception; shapes and qq_mask (every pair keeps samples under this mask)"""
    import correlate_cases as RC
    from xframe_amd.fxs import io as IO
    qs, _, images = RC.synthetic_patterns(n_q, L, n_phi, P, 2027)
    settings = RC.make_settings(n_q, n_phi, q_step=0.03125, q_min=0.015625, wavelength=WAVELENGTH)
    e = CC.small_engine(lib_path)
    c = RC.run(e, settings, images, np.ones((n_q, n_phi), np.int64), shared_mask=True)
    res = c.result()
    c.close()
    s = CC.flow_settings(L, CC.MASK_CASES['none'], enforce_psd=False, modify_cc={'q1q2_symmetric': True})
    d = s['cross_correlation']['datasets']['I1I1']
    d['cc_mask'] = MASK_SETTINGS['custom_pi']
    d['bl_extraction_method'] = 'lstsq'
    ccd = IO.load_ccd(res, 'direct')
    data = X.extract_from_cross_correlation(e, ccd, s)
    meta = metadata(qs, np.asarray(ccd['angular_points']), L, True, {'q1q2_symmetric': True}, np.asarray(ccd['average_intensity']),
                    MASK_SETTINGS['custom_pi'], 'lstsq')
    meta['data_grid'] = ccd['data_grid']
    _, qq = X.masked_cross_correlation_to_deg2_invariant(e, np.asarray(ccd['cross_correlation']['I1I1']).copy(), 3, **meta)
    e.close()
    b = data['deg_2_invariant']['I1I1']
    assert res['num_images_good'] == P
    assert b.shape == (L + 1, n_q, n_q) and np.isfinite(b).all() and not np.any(b[1::2]) and np.any(b[0]) and np.any(b[L])
    assert qq.shape == (n_q, n_q) and qq.dtype == bool and qq.all()
    assert data['deg_2_invariant_masks']['I1I1'].shape == (L + 1, n_q, n_q) and data['deg_2_invariant_masks']['I1I1'].all()
    pms = data['data_projection_matrices']
    assert len(pms) == L + 1 and all(pms[l].shape == (n_q, min(n_q, 2 * l + 1)) for l in range(L + 1))
    assert all(np.isfinite(np.asarray(p)).all() for p in pms)

"""Numerics of the upstream `extract` step: B_l -> eigenpairs -> projection matrices V_l, and the
positive-semidefinite projection of B_l.  Host mirror of

    xframe/projects/fxs/projectLibrary/fxs_invariant_tools.py:1079-1207   deg2_invariant_to_projection_matrices(_3d),
                                                                           deg2_invariant_eigenvalues
    xframe/library/mathLibrary.py:872-892                                  nearest_positive_semidefinite_matrix
    xframe/projects/fxs/extract.py:418-430                                 apply_invariant_constraints (bl_enforce_psd)

with the eigen-decompositions on the device (``Engine.hermitian_eig``: real symmetric matrices up to 128 x 128 in the LDS-
resident solver k_sym_eig, anything else in the general Hermitian kernel); sorting, cuts and clipping are the reference's rules.
All orders of a B_l stack go to the device in one batch (the reference spreads them over worker processes, 1106)."""
import numpy as np


def _batched_eigh(engine, mats):
    """eigenvalues ASCENDING (K, n) and eigenvectors (K, n, n) in columns, like numpy.linalg.eigh, from the device solver"""
    if engine is None or not hasattr(engine, 'hermitian_eig'):
        raise TypeError('the extract rules need an eigensolver object with `hermitian_eig` (an Engine: the device solvers); there is no '
                        'CPU fallback in the product')
    vals, vecs = engine.hermitian_eig(np.asarray(mats))          # descending
    vecs = vecs[:, :, ::-1]
    if not np.iscomplexobj(np.asarray(mats)):
        vecs = vecs.real
    return vals[:, ::-1].copy(), np.ascontiguousarray(vecs)


def deg2_invariant_eigenvalues(engine, b_matrices, sort_mode=0):
    """fxs_invariant_tools.py:1114-1141 for a stack (K, n, n): returns (eigenvalues (K, n), eigenvectors (K, n, n)) sorted in
    descending order of the eigenvalue (sort_mode 0) or of median_q |sqrt|lambda| v(q)| sign(lambda) (sort_mode 1); a matrix that
    is zero to numpy.isclose gets zero eigenpairs (1123-1130)."""
    b = np.asarray(b_matrices)
    b = (b + np.conj(np.swapaxes(b, -1, -2))) / 2                                  # 1122
    K, n = b.shape[0], b.shape[1]
    if n == 0:
        return np.zeros((K, 0)), np.zeros((K, 0, 0))
    zero = np.array([np.isclose(m, 0).all() for m in b])
    w = np.zeros((K, n))
    v = np.zeros((K, n, n), dtype=b.dtype)
    if (~zero).any():
        w[~zero], v[~zero] = _batched_eigh(engine, b[~zero])
    signs = np.sign(w)
    if sort_mode == 0:
        metric = w
    else:
        metric = np.median(np.abs(np.sqrt(np.abs(w[:, None, :])) * v), axis=1) * signs
    ids = np.argsort(metric, axis=1)[:, ::-1]
    return np.take_along_axis(w, ids, axis=1).real, np.take_along_axis(v, ids[:, None, :], axis=2)


def deg2_invariant_to_projection_matrices(engine, b_coeff, q_id_limits=False, sort_mode=0):
    """fxs_invariant_tools.py:1079-1112 (dim 3) with 1171-1207 per order: V_l = the first min(block, 2l+1) eigenvectors of the
    block q_id_limits[l, 0] of B_l times sqrt(eigenvalue), negative eigenvalues zeroed, embedded in Nq rows.  Returns
    (tuple of V_l (complex, like 1207), tuple of eigenvalues)."""
    b_coeff = np.asarray(b_coeff)
    n_orders, nq = b_coeff.shape[0], b_coeff.shape[-1]
    if isinstance(q_id_limits, bool):                                              # 1092-1094
        lim = np.zeros((n_orders, 2, 2), dtype=int)
        lim[..., 1] = nq
    else:
        lim = np.array(q_id_limits)
    if not (lim[:, 0, :] == lim[:, 1, :]).all():                                   # 1095-1099
        lim[:, 1] = lim[:, 0]
    # orders with the same block go to the device together
    pairs = [None] * n_orders
    blocks = {}
    for o in range(n_orders):
        blocks.setdefault((int(lim[o, 0, 0]), int(lim[o, 0, 1])), []).append(o)
    for (lo, hi), orders in blocks.items():
        sub = b_coeff[orders][:, lo:hi, lo:hi]
        w, v = deg2_invariant_eigenvalues(engine, sub, sort_mode)
        for i, o in enumerate(orders):
            pairs[o] = (w[i], v[i], lo, hi)
    pms, evs = [], []
    for o in range(n_orders):
        w, v, lo, hi = pairs[o]
        n_full = min(nq, 2 * o + 1)
        full_v = np.zeros((nq, n_full), dtype=v.dtype)
        full_w = np.zeros(n_full)
        if len(w) != 0:
            n = min(len(v), 2 * o + 1)
            vv, ww = v[:, :n].copy(), w[:n].copy()
            neg = ww < 0
            ww[neg] = 0
            vv[:, neg] = 0
            full_v[lo:hi, :n] = vv
            full_w[:n] = ww
        pms.append((full_v * np.sqrt(full_w)[None, :]).astype(complex))
        evs.append(full_w)
    return tuple(pms), tuple(evs)


def deg2_invariant_to_projection_matrices_2d(engine, b_coeff, q_id_limits=False, sort_mode=0):
    """fxs_invariant_tools.py:1079-1104 (dim 2) with 1143-1169 per order: v_n = the first eigenvector of the block q_id_limits[n, 0]
    of B_n times sqrt(its eigenvalue), embedded in Nq rows; an eigenvalue that is not >= 0 gives a zero vector and the eigenvalue 0
    (1154-1159).  The eigen-decomposition runs on the device (Engine.hermitian_eig), the orders with the same block together.
    Returns (tuple of v_n (Nq,) -- complex, where upstream keeps the eigenvector's dtype, real for a real block; MTIP2D casts them
    on entry either way --, tuple of eigenvalues)."""
    b_coeff = np.asarray(b_coeff)
    n_orders, nq = b_coeff.shape[0], b_coeff.shape[-1]
    if isinstance(q_id_limits, bool):                                              # 1091-1093
        lim = np.zeros((n_orders, 2, 2), dtype=int)
        lim[..., 1] = nq
    else:
        lim = np.array(q_id_limits)
    if not (lim[:, 0, :] == lim[:, 1, :]).all():                                   # 1094-1099
        lim[:, 1] = lim[:, 0]
    pairs = [None] * n_orders
    blocks = {}
    for o in range(n_orders):
        blocks.setdefault((int(lim[o, 0, 0]), int(lim[o, 0, 1])), []).append(o)
    for (lo, hi), orders in blocks.items():
        w, v = deg2_invariant_eigenvalues(engine, b_coeff[orders][:, lo:hi, lo:hi], sort_mode)
        for i, o in enumerate(orders):
            pairs[o] = (w[i], v[i], lo, hi)
    pms, evs = [], []
    for o in range(n_orders):
        w, v, lo, hi = pairs[o]
        if len(w) == 0:
            raise IndexError('order %d: empty block [%d, %d) of the degree-2 invariant (fxs_invariant_tools.py:1149 indexes its first '
                             'eigenvalue)' % (o, lo, hi))
        eig_val, eig_vect = float(w[0]), np.array(v[:, 0])
        if not eig_val >= 0:                                                       # 1154-1159
            eig_val = 0.0
            eig_vect[:] = 0
        full = np.zeros(nq, dtype=eig_vect.dtype)
        full[lo:hi] = eig_vect
        pms.append((full * np.sqrt(eig_val)).astype(complex))
        evs.append(eig_val)
    return tuple(pms), tuple(evs)


def nearest_positive_semidefinite_matrix(engine, A, low_positive_eigenvalues_to_zero=False):
    """mathLibrary.py:872-892 for one matrix or a stack: eigenvalues of the Hermitian part below the limit set to zero.  The
    eigen-decomposition runs on the device; the noise-floor variant needs the spectrum of the unsymmetrised A (numpy, host)."""
    A = np.asarray(A)
    single = A.ndim == 2
    stack = A[None] if single else A.reshape((-1,) + A.shape[-2:])
    B = (stack + np.conj(np.swapaxes(stack, -1, -2))) / 2
    w, v = _batched_eigh(engine, B)
    out = np.empty_like(B)
    for i in range(len(B)):
        limit = 0
        if low_positive_eigenvalues_to_zero:
            limit = np.abs(np.min(np.linalg.eig(stack[i])[0]))
        wi = w[i].copy()
        wi[wi < limit] = 0
        out[i] = (v[i] * wi[None, :]) @ np.conj(v[i]).T
    return out[0] if single else out.reshape(A.shape)


def apply_invariant_constraints(engine, b_coeff, q_id_limits, bl_enforce_psd=True):
    """xframe/projects/fxs/extract.py:418-430: the block q_id_limits[o, 0] of every order replaced by its nearest positive
    semidefinite matrix"""
    out = np.array(b_coeff, copy=True)
    if not bl_enforce_psd:
        return out
    lim = np.array(q_id_limits)
    if not (lim[:, 0, :] == lim[:, 1, :]).all():
        lim[:, 1] = lim[:, 0]
    for o in range(len(out)):
        lo, hi = int(lim[o, 0, 0]), int(lim[o, 0, 1])
        if hi > lo:
            out[o, lo:hi, lo:hi] = nearest_positive_semidefinite_matrix(engine, b_coeff[o, lo:hi, lo:hi])
    return out


# ---- cross-correlation -> B_l -> V_l: the route in front of the functions above ----------------------------------------------------
# xframe/projects/fxs/extract.py:95-168 (extract_bl_from_cc), 332-414 (masks), 496-532 (extract) and
# xframe/projects/fxs/projectLibrary/fxs_invariant_tools.py:374-422 (cross_correlation_to_deg2_invariant), 578-645 (back-substitution),
# 813-839 (2-D), 235-289 (modify_cross_correlation), 1259-1269 (error estimate).  The arithmetic on the cross-correlation runs in
# one kernel (csrc/k_extract.hip, Engine.cc_to_deg2); everything here is settings bookkeeping.  What the reference offers and this
# route does not build raises NotImplementedError with the option and the reference line: no CPU fallback.
_BUILT_MODIFY_CC = ('subtract_average_intensity', 'pi_periodicity', 'q1q2_symmetric')
_REFERENCE_MODES = ('lstsq', 'legendre', 'back_substitution', 'back_substitution_psd', 'back_substitution_qqsym',
                    'back_substitution_memory_hungry')               # the keys of fxs_invariant_tools.py:440


def legendre_table(radial_points, xray_wavelength, max_order, stride):
    """(Nq, n_m (n_m + 1) / 2) table of mtip_op_cc_to_deg2: gsl_sf_legendre_sphPlm(li stride, mi stride, cos theta_q) at
    li (li + 1) / 2 + mi with theta_q = ewald_sphere_theta_pi (physicsLibrary.py:94-95; fxs_invariant_tools.py:602 takes this
    geometry whatever the dataset's pi_in_q says)."""
    from .hostsetup import sph_plm
    qs = np.asarray(radial_points, dtype=float)
    x = np.cos(np.arccos(qs * xray_wavelength / (4 * np.pi)))        # 602, 65
    if not np.isfinite(x).all():
        raise ValueError('q * wavelength / (4 pi) > 1: the radial points do not lie on the Ewald sphere of this wavelength')
    n_m = int(max_order) // int(stride) + 1
    li, mi = np.tril_indices(n_m)                                    # row-major lower triangle: li (li + 1) / 2 + mi
    return np.ascontiguousarray(sph_plm((li * stride)[None, :], (mi * stride)[None, :], x[:, None]))


_NARROW_ENTRY_ORDERS = 64              # what mtip_op_cc_to_deg2 extracts; more go to mtip_op_cc_to_deg2_wide (up to 129, max_order <= 128)


def _wants_wide_entry(max_order, stride):
    return int(max_order) // int(stride) + 1 > _NARROW_ENTRY_ORDERS


def _check_cc_options(metadata, dim):
    mask_type = (metadata.get('cc_mask') or {'type': 'none'}).get('type', 'none')
    if mask_type != 'none':
        raise NotImplementedError('cc_mask.type %r (fxs_invariant_tools.py:205-232): only unmasked data (type none) is built; the masked '
                                  'routes interpolate on the host upstream (605-608)' % (mask_type,))
    for key, value in (metadata.get('modify_cc') or {}).items():
        if key not in _BUILT_MODIFY_CC and not (isinstance(value, (bool, np.bool_)) and not value):
            raise NotImplementedError('modify_cc.%s (fxs_invariant_tools.py:235-289): built are %s' % (key, ', '.join(_BUILT_MODIFY_CC)))
    mode = metadata.get('mode', False)
    if dim == 3 and mode != 'back_substitution':
        if isinstance(mode, (bool, np.bool_)):
            raise NotImplementedError("bl extraction without 'mode' (fxs_invariant_tools.py:414-415 returns the (Nq, Nq, orders) layout of "
                                      "ccd_to_deg2_invariant_3d): the worker always names the mode (extract.py:134)")
        if mode not in _REFERENCE_MODES:
            raise NotImplementedError('bl_extraction_method %r is not a key of the reference\'s mode table and asserts upstream: Given B_l '
                                      'extraction mode "%s" is unknown. Known modes are %s (fxs_invariant_tools.py:440-446; the settings '
                                      'file offers legendre_approx)' % (mode, mode, list(_REFERENCE_MODES)))
        raise NotImplementedError('bl_extraction_method %r (fxs_invariant_tools.py:440): only back_substitution (578-645) is built' % (mode,))


def cross_correlation_to_deg2_invariant(engine, cc, dim, **metadata):
    """fxs_invariant_tools.py:374-422 with the arithmetic on the device.  metadata as the worker builds it (extract.py:134):
    'data_grid' {qs, thetas, phis}, 'orders' (arange(max_order + 1)), 'assume_zero_odd_orders', 'modify_cc', 'cc_mask', 'mode',
    'xray_wavelength' (dim 3), 'average_intensity'.  Returns (b_coeff (max_order + 1, Nq, Nq) complex, odd orders zero when they are
    assumed zero, qq_mask (Nq, Nq) all true: the unmasked case, 136-139, 609)."""
    if dim not in (2, 3):
        raise ValueError('dim must be 2 or 3')
    _check_cc_options(metadata, dim)
    orders = np.asarray(metadata['orders'])
    max_order = int(orders.max())
    if not np.array_equal(orders, np.arange(max_order + 1)):
        raise NotImplementedError('orders other than arange(max_order + 1) (the worker passes these, extract.py:134)')
    n_delta = int(cc.shape[-1])
    if n_delta < 2 * max_order:
        # the worker clamps max_order to n_delta // 2 first (extract.py:112-119); the reference's own fallback is broken (388-391)
        raise ValueError('max_order %d cannot be resolved with %d angular points (need n_delta >= 2 max_order)' % (max_order, n_delta))
    data_grid = metadata['data_grid']
    phis = np.asarray(data_grid['phis'], dtype=float)
    mod = metadata.get('modify_cc') or {}
    avg = metadata.get('average_intensity', False)
    avg = np.asarray(getattr(avg, 'data', avg))
    kw = {}
    if mod.get('subtract_average_intensity', False) and avg.ndim == 1:                                    # 245
        kw['average_intensity'] = avg
    if mod.get('pi_periodicity', False):
        assert n_delta % 2 == 0, 'for odd number of phi symmetry enforcing is not possible since phi+pi is not an existing grid point.'
        assert n_delta == len(phis), 'Cross correlation has {} angular datapoints but only {} angle values are given.'.format(n_delta, len(phis))
        kw['bad_angles'] = (phis < np.pi / 2) | (phis >= 3 * np.pi / 2)                                  # 267
    stride = 2 if metadata['assume_zero_odd_orders'] else 1
    if dim == 3:
        kw['legendre'] = legendre_table(data_grid['qs'], metadata['xray_wavelength'], max_order, stride)
    b = engine.cc_to_deg2(cc, max_order, order_stride=stride, dimensions=dim, q1q2_symmetric=bool(mod.get('q1q2_symmetric', False)),
                          wide=_wants_wide_entry(max_order, stride), **kw)
    if not isinstance(b, np.ndarray):
        b = b.cpu().numpy()
    return b, np.ones(b.shape[1:], dtype=bool)


# ---- masked cross-correlation data ------------------------------------------------------------------------------------------------
# fxs_invariant_tools.py:100-232 (the cc_mask generators), 235-289 with a mask, 335-351 (interpolate), 452-517 (lstsq).  The function
# above stays the unmasked operator and keeps refusing these options; extract_from_cross_correlation sends a data set whose settings
# ask for a mask, for lstsq or for interpolate_masked here.  The masks are settings-derived tables computed once per data set (numpy);
# the arithmetic on C runs in the two kernels of csrc/k_extract_lsq.h.
_MASKED_MODES = ('back_substitution', 'lstsq', 'back_substitution_memory_hungry', 'back_substitution_qqsym', 'back_substitution_psd')
_CM_MODES = ('back_substitution_qqsym', 'back_substitution_psd')      # C_m by the dimensions = 2 entry, then Engine.cm_backsub
_LSTSQ_RCOND_MIN = 1e-12               # about one decade above LAPACK's own cut eps max(M, N) (2e-13 .. 9e-13 for M = 1024 .. 4096)


def _true_cc_mask(data_grid):                                                                          # 136-139
    return np.ones((len(data_grid['qs']),) * 2 + (len(data_grid['phis']),), dtype=bool)


def _ewald_shifted_angles(data_grid, wavelength):
    """what pixel_arc_cc_mask reads of cartesian_to_spherical(spherical_to_cartesian(grid) - (0, 0, 2 pi / lambda)) on the
    uniform_dependent grid (q, theta_q, phi) (115-118; mathLibrary.py:629-698, gridLibrary.py:959-1016): theta of every shell at the
    first phi, and phi along the SECOND shell (sic, 122: index 1)"""
    qs, thetas, phis = (np.asarray(data_grid[k], dtype=float) for k in ('qs', 'thetas', 'phis'))
    r, theta, phi = qs[:, None], thetas[:, None], phis[None, :]
    xy = r * np.sin(theta)
    x, y, z = np.cos(phi) * xy, np.sin(phi) * xy, r * np.cos(theta) + 0 * phi
    z = z - 2 * np.pi / wavelength
    rr = np.sqrt(np.square(x) + np.square(y) + np.square(z))
    new_theta = np.zeros(rr.shape)
    nz = rr != 0
    new_theta[nz] = np.arccos(z[nz] / rr[nz])
    new_phi = np.arctan2(y, x)
    new_phi = np.where(new_phi < 0, new_phi + 2 * np.pi, new_phi)
    return new_theta[:, 0], new_phi[1, :]


def _pixel_arc_cc_mask(data_grid, d):                                                                  # 100-135
    ewald_r = 2 * np.pi / d['xray_wavelength']
    ew_theta, ew_phi = _ewald_shifted_angles(data_grid, d['xray_wavelength'])
    ct, st = np.cos(ew_theta), np.sin(ew_theta)

    def arc(cos_phi):
        return np.abs(ewald_r * np.arccos(ct[:, None, None] * ct[None, :, None] + st[:, None, None] * st[None, :, None] * cos_phi[None, None, :]))
    r_pixel_size = 2 * np.pi / d['pixel_size']
    mask = arc(np.cos(ew_phi)) > r_pixel_size
    if d['mask_at_pi']:
        mask = mask & (arc(np.cos(ew_phi - np.pi)) > r_pixel_size)
    return mask


def _pixel_custom_cc_mask(data_grid, d):                                                               # 140-171
    n_phis, n_qs = len(data_grid['phis']), len(data_grid['qs'])
    n = int(n_phis * d['n_masked_pixels_phi'])
    nq = int(n_qs * d['n_masked_pixels_q'])
    pi_index = int(n_phis / 2)
    ids = list(range(n)) + list(range(n_phis - n, n_phis, 1))
    if d['mask_at_pi']:
        ids = list(range(n)) + list(range(pi_index - (n - 1), pi_index + (n - 1), 1)) + list(range(n_phis - n, n_phis, 1))
    mask = np.full((n_qs, n_qs, n_phis), True)
    mask[..., ids] = False
    mask[np.abs(np.arange(n_qs)[:, None] - np.arange(n_qs)[None, :]) > nq] = True
    return mask


def _pixel_flat_cc_mask(data_grid, d):                                                                 # 172-195
    qs, phis = np.asarray(data_grid['qs'], dtype=float), np.asarray(data_grid['phis'], dtype=float)
    r_pixel_size = 2 * np.pi / d['pixel_size']
    with np.errstate(divide='ignore'):
        phi_min = 2 * np.pi / ((2 * np.pi * qs) / r_pixel_size)
    phi_mask = (phis[None, :] > phi_min[:, None]) & (phis[None, :] < (2 * np.pi - phi_min[:, None]))
    if d['mask_at_pi']:
        phi_mask &= (phis[None, :] > np.pi + phi_min[:, None]) | (phis[None, :] < np.pi - phi_min[:, None])
    phi_mask = phi_mask[None, :, :] & phi_mask[:, None, :]
    radial_mask = np.abs(qs[None, :] - qs[:, None]) > r_pixel_size
    return radial_mask[:, :, None] | phi_mask


def _direct_cc_mask(data_grid, d):                                                                     # 218-219
    return d['mask']


_CC_MASK_TYPES = {'direct': _direct_cc_mask, 'none': _true_cc_mask, 'pixel_arc': _pixel_arc_cc_mask, 'pixel_flat': _pixel_flat_cc_mask,
                  'pixel_custom': _pixel_custom_cc_mask}


def cross_correlation_mask(data_grid, datadict):
    """fxs_invariant_tools.py:221-232: the bool mask (Nq, Nq, n_delta), True = keep, of datadict['cc_mask']['type']; the generator of
    a type reads the merged dict {**cc_mask[type], **datadict} (231)."""
    given_type = datadict['cc_mask']['type']
    generator = _CC_MASK_TYPES.get(given_type, False)
    if isinstance(generator, bool):
        raise AssertionError('Given Cross-Correlation mask type "{}" not known. Known types are {}'.format(given_type, _CC_MASK_TYPES.keys()))
    if given_type == 'none':
        return generator(data_grid)
    return generator(data_grid, {**datadict['cc_mask'][given_type], **datadict})


def _pair_name(flat, nq):
    return '(q1, q2) = (%d, %d)' % (flat // nq, flat % nq)


_CONDITIONING_KEYS = ('low_pass_order_in_q', 'enforce_max_order', 'enforce_zero_odd_harmonics', 'apply_binned_mean')
_RANK_DEFICIENT = ('raise', 'minimum_norm')


def _is_off(value):
    return isinstance(value, (bool, np.bool_)) and not value


def binned_mean_tables(phis, max_order):
    """the host tables of ``Engine.cc_binned_mean`` in the reference's own expressions (binned_mean, fxs_invariant_tools.py:310-323):
    returns (bin_start (n_bins + 1) int32: the runs of the rolled bin ids that numpy.add.reduceat sums, n_roll, new_phis (330)).
    Raises ValueError where the runs are not the bins 0 .. n_bins - 1 in order -- a grid that leaves a bin without a sample (reduceat
    then returns fewer bins than new_phis has entries) or that is not sorted."""
    phis = np.asarray(phis, dtype=float)
    max_order = int(max_order)
    if max_order < 1:
        raise ValueError('apply_binned_mean needs max_order >= 1 (step pi / max_order, fxs_invariant_tools.py:310)')
    step_size = np.pi / max_order                                                                        # 310
    n_bins = 2 * max_order
    ids = (phis + step_size / 2) // step_size                                                            # 312: numpy's floor division
    n_roll = int(np.sum(ids == n_bins))
    ids[ids == n_bins] = 0
    idr = np.roll(ids, n_roll)                                                                           # 319
    split_ids = np.where(np.roll(idr, 1) != idr)[0]                                                      # 323
    if len(split_ids) != n_bins or not np.array_equal(idr[split_ids], np.arange(n_bins)):
        raise ValueError('apply_binned_mean: the %d angles do not put a sample into every one of the 2 max_order = %d bins in '
                         'rising order (%d runs of bin ids; fxs_invariant_tools.py:323-324 would return that many bins for %d new '
                         'angles)' % (len(phis), n_bins, len(split_ids), n_bins))
    bin_start = np.concatenate([split_ids, [len(phis)]]).astype(np.int32)
    return bin_start, n_roll, np.arange(n_bins) * 2 * np.pi / n_bins                                     # 330


def lowpass_sos(value, nq):
    """the second-order section of low_pass_order_in_q (fxs_invariant_tools.py:250): scipy.signal.butter(1, value, 'lp', fs=Nq,
    output='sos'); a cutoff outside (0, Nq / 2) raises ValueError, as scipy does"""
    if isinstance(value, (bool, np.bool_)) or not np.isscalar(value) or not np.isfinite(value) or not 0 < value < nq / 2:
        raise ValueError('low_pass_order_in_q = %r: scipy.signal.butter(1, value, \'lp\', fs=%d) needs 0 < value < fs / 2 = %g'
                         % (value, nq, nq / 2))
    from scipy.signal import butter
    sos = np.asarray(butter(1, value, 'lp', fs=nq, output='sos'), dtype=float)
    assert sos.shape == (1, 6) and sos[0, 3] == 1.0, sos
    return sos


def modify_masked_cross_correlation(engine, cc, cc_mask, phis, max_order, average_intensity=False, **modify_cc):
    """modify_cross_correlation (fxs_invariant_tools.py:235-289) with a mask, every stage on the device, in the reference's order:
    subtract_average_intensity, low_pass_order_in_q (``Engine.cc_lowpass_q``), enforce_max_order / enforce_zero_odd_harmonics
    (``Engine.cc_harmonic_filter``), pi_periodicity, q1q2_symmetric, apply_binned_mean (``Engine.cc_binned_mean``),
    interpolate_masked.  The first stage that runs subtracts the average intensity.  With none of low_pass_order_in_q,
    enforce_max_order, enforce_zero_odd_harmonics, apply_binned_mean it is ONE ``Engine.cc_prepare_masked`` call.  Returns
    (cc', mask', phis'): after a binned mean the 2 max_order new angles, which the interpolation already uses.  Raises ValueError
    for a cutoff outside (0, Nq / 2), for a grid that leaves a bin without an angle, and where scipy's interp1d would raise."""
    mod = modify_cc
    phis = np.asarray(phis, dtype=float)
    nq, n_delta = int(cc.shape[0]), int(cc.shape[-1])
    max_order = int(max_order)
    avg = average_intensity
    avg = np.asarray(getattr(avg, 'data', avg))
    kw = {}
    if mod.get('subtract_average_intensity', False) and avg.ndim == 1:                                    # 245
        kw['average_intensity'] = avg
    if mod.get('pi_periodicity', False):
        assert n_delta % 2 == 0, 'for odd number of phi symmetry enforcing is not possible since phi+pi is not an existing grid point.'
        assert n_delta == len(phis), 'Cross correlation has {} angular datapoints but only {} angle values are given.'.format(n_delta, len(phis))
        kw['bad_angles'] = (phis < np.pi / 2) | (phis >= 3 * np.pi / 2)                                  # 267
    interpolate = bool(mod.get('interpolate_masked', False))
    symmetric = bool(mod.get('q1q2_symmetric', False))
    low_pass = mod.get('low_pass_order_in_q', False)
    sos = None if isinstance(low_pass, (bool, np.bool_)) else lowpass_sos(low_pass, nq)                  # 248: anything but a bool
    cut_orders, zero_odd = bool(mod.get('enforce_max_order', False)), bool(mod.get('enforce_zero_odd_harmonics', False))
    binned = bool(mod.get('apply_binned_mean', False))
    if binned:
        assert n_delta == len(phis), 'Cross correlation has {} angular datapoints but only {} angle values are given.'.format(n_delta, len(phis))
        bin_start, n_roll, new_phis = binned_mean_tables(phis, max_order)
    # the first stage that runs subtracts the average intensity (245-247); every stage up to the bins works on the old angles
    pending = {'average_intensity': kw.pop('average_intensity')} if 'average_intensity' in kw else {}
    if sos is not None:
        cc = engine.cc_lowpass_q(cc, sos, **pending)
        pending = {}
    if cut_orders or zero_odd:
        cc = engine.cc_harmonic_filter(cc, max_order=max_order if cut_orders else None, zero_odd=zero_odd, **pending)
        pending = {}
    if binned:
        if symmetric or 'bad_angles' in kw:
            cc, cc_mask, _ = engine.cc_prepare_masked(cc, cc_mask, q1q2_symmetric=symmetric, **pending, **kw)
            pending = {}
        cc2, mask2 = engine.cc_binned_mean(cc, cc_mask, bin_start, n_roll, **pending)
        phis = new_phis
        status = (0, 0)
        if interpolate:
            cc2, mask2, status = engine.cc_prepare_masked(cc2, mask2, interpolate_phis=phis)
    else:
        if interpolate:
            kw['interpolate_phis'] = phis
        cc2, mask2, status = engine.cc_prepare_masked(cc, cc_mask, q1q2_symmetric=symmetric, **pending, **kw)
    if status[0]:
        raise ValueError('interpolate_masked: %d rows have a masked sample outside the range of their valid ones, the first at %s; scipy\'s '
                         'interp1d raises there (fxs_invariant_tools.py:348) and nothing is extrapolated' % (status[0], _pair_name(status[1], nq)))
    return cc2, mask2, phis


def masked_cross_correlation_to_deg2_invariant(engine, cc, dim, rank_deficient='raise', **metadata):
    """fxs_invariant_tools.py:374-422 for data with a cc_mask, for mode 'lstsq' and for modify_cc.interpolate_masked, three dimensions,
    arithmetic on the device.  metadata as for ``cross_correlation_to_deg2_invariant``; modes: 'back_substitution' (578-645: the masked
    samples are interpolated first, 605-608; qq_mask = mask'.all(-1)) and 'lstsq' (452-517: a fit over the unmasked samples of every
    pair; a pair without any gets zeros; qq_mask = mask'.any(-1)).  Returns (b_coeff (max_order + 1, Nq, Nq) complex, qq_mask).
    The other back-substitutions of the mode table (440) live here too, as 'lstsq' does: 'back_substitution_memory_hungry' (519-576)
    is the same elimination as 'back_substitution', interpolation implied (546-549), and returns that kernel's bits;
    'back_substitution_qqsym' (646-694: Hermitian mean of the harmonics over (q1, q2)) and 'back_substitution_psd' (710-761: every
    C_m and every B_l replaced by its nearest positive-semidefinite matrix inside the elimination) imply no interpolation, take
    qq_mask = mask'.all(-1), zero the masked pairs, and run on the harmonics of ``Engine.cc_to_deg2`` (dimensions 2, stride 1) through
    ``Engine.cm_backsub``; with an odd max_order and zero odd orders the solved system ends at max_order - 1.  For these two modes a
    conditioning stage of modify_cc (low_pass_order_in_q, enforce_max_order, enforce_zero_odd_harmonics, apply_binned_mean) together
    with a mask that removes samples raises NotImplementedError: they transform the masked samples as they are, and what those stages
    leave at masked positions is not pinned to the reference.

    Raises ValueError where scipy's interp1d does (335-351; scipy 1.15.3): a row that has a valid sample and a masked sample outside
    the range of its valid ones -- every mask that removes Delta = 0 or the last angle of such a row, and every row with a single
    valid sample (its other samples lie outside the range of one point).  Rows without a valid sample and rows without a masked one
    are fine.  Nothing is extrapolated.
    Raises NotImplementedError for rank-deficient least-squares problems (0 < n_valid < number of orders, or a reciprocal condition
    estimate min |r_kk| / max |r_kk| of the triangle below 1e-12): LAPACK's gelsd returns the truncated minimum-norm solution there,
    which this route builds as an opt-in: rank_deficient='minimum_norm' (``Engine.cc_lstsq_deg2_minnorm``; the flow reads
    settings['GPU']['lstsq_minimum_norm']) solves those pairs as numpy.linalg.lstsq(..., rcond=None) does and leaves the bits of
    every other pair alone.

    modify_cc runs in the reference's order (235-289): subtract_average_intensity, low_pass_order_in_q (``Engine.cc_lowpass_q``),
    enforce_max_order / enforce_zero_odd_harmonics (``Engine.cc_harmonic_filter``), pi_periodicity, q1q2_symmetric,
    apply_binned_mean (``Engine.cc_binned_mean``), interpolate_masked.  With none of the four conditioning keys it is the one
    ``Engine.cc_prepare_masked`` call.  After a binned mean the interpolation, the fit and data_grid['phis'] use the 2 max_order
    new angles, as upstream (395)."""
    if rank_deficient not in _RANK_DEFICIENT:
        raise ValueError('rank_deficient %r: one of %s' % (rank_deficient, ', '.join(_RANK_DEFICIENT)))
    if dim == 2:
        raise NotImplementedError('masked cross-correlation data with dimensions = 2 (fxs_invariant_tools.py:813-839 drops masked pairs)')
    if dim != 3:
        raise ValueError('dim must be 2 or 3')
    mod = dict(metadata.get('modify_cc') or {})
    built = _BUILT_MODIFY_CC + ('interpolate_masked',) + _CONDITIONING_KEYS
    for key, value in mod.items():
        if key not in built and not _is_off(value):
            raise NotImplementedError('modify_cc.%s (fxs_invariant_tools.py:235-289): built are %s' % (key, ', '.join(built)))
    mode = metadata.get('mode', False)
    if mode not in _MASKED_MODES:
        raise NotImplementedError('bl_extraction_method %r on masked data (fxs_invariant_tools.py:440): built are %s' % (mode, ', '.join(_MASKED_MODES)))
    orders = np.asarray(metadata['orders'])
    max_order = int(orders.max())
    if not np.array_equal(orders, np.arange(max_order + 1)):
        raise NotImplementedError('orders other than arange(max_order + 1) (the worker passes these, extract.py:134)')
    n_delta = int(cc.shape[-1])
    if n_delta < 2 * max_order:
        raise ValueError('max_order %d cannot be resolved with %d angular points (need n_delta >= 2 max_order)' % (max_order, n_delta))
    data_grid = metadata['data_grid']
    qs, phis = np.asarray(data_grid['qs'], dtype=float), np.asarray(data_grid['phis'], dtype=float)
    nq = len(qs)
    cc_mask = np.asarray(cross_correlation_mask(data_grid, metadata), dtype=bool)
    if cc_mask.shape != tuple(cc.shape):
        raise ValueError('cc_mask has shape %r, the cross-correlation %r' % (cc_mask.shape, tuple(cc.shape)))
    # interpolation: the setting, or implied by back_substitution and its memory_hungry twin (605-608, 546-549; a no-op on a mask that
    # is all true).  qqsym and psd transform the masked samples as they are (no interpolation upstream, 677 / 742): what
    # cc_prepare_masked leaves at masked positions is pinned against modify_cross_correlation for subtract_average_intensity,
    # pi_periodicity and q1q2_symmetric (G27 compares whole arrays, G31 the modes on top); the conditioning stages are not
    implied = mode in ('back_substitution', 'back_substitution_memory_hungry')
    if mode in _CM_MODES and not cc_mask.all() and not bool(mod.get('interpolate_masked', False)):
        for key in _CONDITIONING_KEYS:
            if not _is_off(mod.get(key, False)):
                raise NotImplementedError('modify_cc.%s with masked data and bl_extraction_method %r: the mode transforms the masked samples '
                                          'as they are (fxs_invariant_tools.py:677, 742), and what this stage leaves at masked positions is '
                                          'not pinned to the reference' % (key, mode))
    mod['interpolate_masked'] = bool(mod.get('interpolate_masked', False)) or implied
    cc2, mask2, phis = modify_masked_cross_correlation(engine, cc, cc_mask, phis, max_order,
                                                       average_intensity=metadata.get('average_intensity', False), **mod)
    if mod.get('apply_binned_mean', False):
        data_grid['phis'] = phis                                                                         # 395
    stride = 2 if metadata['assume_zero_odd_orders'] else 1
    if mode in ('back_substitution', 'back_substitution_memory_hungry'):                                 # (the same elimination: one kernel)
        leg = legendre_table(qs, metadata['xray_wavelength'], max_order, stride)
        b = engine.cc_to_deg2(cc2, max_order, order_stride=stride, dimensions=3, legendre=leg, wide=_wants_wide_entry(max_order, stride))
        return np.asarray(b), np.asarray(mask2).all(-1)                                                  # 609, 550
    if mode in _CM_MODES:
        # the solved system ends at the highest extracted order (orders[order_mask].max(), 396-399, 675 / 740): max_order - 1 for an
        # odd max_order with zero odd orders; the orders above come back as zeros (417-419)
        l_max = (max_order // stride) * stride
        psd = mode == 'back_substitution_psd'
        qq_mask = np.asarray(mask2).all(-1)                                                              # 677, 742
        cm = engine.cc_to_deg2(cc2, l_max, order_stride=1, dimensions=2, wide=_wants_wide_entry(l_max, 1))
        leg = legendre_table(qs, metadata['xray_wavelength'], l_max, 1 if psd else stride)
        b, _ = engine.cm_backsub(cm, leg, order_stride=stride, mode='psd' if psd else 'plain', hermitian_mean=not psd,
                                 qq_mask=None if qq_mask.all() else qq_mask)
        b = np.asarray(b)
        if b.shape[0] < max_order + 1:
            b = np.concatenate([b, np.zeros((max_order + 1 - b.shape[0],) + b.shape[1:], complex)])
        return b, qq_mask
    extracted = np.arange(0, max_order + 1, stride)                                                      # orders[order_mask], 396-399
    thetas = np.arccos(qs * metadata['xray_wavelength'] / (4 * np.pi))                                   # 471, physicsLibrary.py:94-95
    if not np.isfinite(thetas).all():
        raise ValueError('q * wavelength / (4 pi) > 1: the radial points do not lie on the Ewald sphere of this wavelength')
    if rank_deficient == 'minimum_norm':
        b, n_valid, rcond, _ = engine.cc_lstsq_deg2_minnorm(cc2, mask2, extracted, thetas, phis)
    else:
        b, n_valid, rcond = engine.cc_lstsq_deg2(cc2, mask2, extracted, thetas, phis)
    b, n_valid, rcond = np.asarray(b), np.asarray(n_valid), np.asarray(rcond)
    deficient = (n_valid > 0) & ((n_valid < len(extracted)) | (rcond < _LSTSQ_RCOND_MIN))
    if deficient.any() and rank_deficient == 'raise':
        first = int(np.flatnonzero(deficient)[0])
        raise NotImplementedError('lstsq: %d of %d pairs are rank deficient (fewer valid samples than the %d orders, or a reciprocal '
                                  'condition estimate below %g), the first at %s with %d valid samples, estimate %.1e; LAPACK returns the '
                                  'truncated minimum-norm solution there (fxs_invariant_tools.py:513), which is opt-in: '
                                  "rank_deficient='minimum_norm', or settings['GPU']['lstsq_minimum_norm'] = True in the flow"
                                  % (int(deficient.sum()), deficient.size, len(extracted), _LSTSQ_RCOND_MIN, _pair_name(first, nq),
                                     int(n_valid.flat[first]), float(rcond.flat[first])))
    if b.shape[0] < max_order + 1:                                                                       # (odd max_order at stride 2)
        b = np.concatenate([b, np.zeros((max_order + 1 - b.shape[0],) + b.shape[1:], complex)])
    return b, n_valid > 0                                                                                # 481


def _wants_masked_route(dopt):
    mask_type = (dopt.get('cc_mask') or {'type': 'none'}).get('type', 'none')
    mod = dopt.get('modify_cc') or {}
    return (mask_type != 'none' or dopt.get('bl_extraction_method') in ('lstsq',) + _MASKED_MODES[2:] or bool(mod.get('interpolate_masked', False))
            or any(not _is_off(mod.get(key, False)) for key in _CONDITIONING_KEYS))


def calc_deg_2_invariant_line_mask(radial_points, max_order, line_specifier, invert=False):
    """extract.py:368-414: the side of one line (or, for a tuple, of two lines: q1 and q2) through two (order, q) points"""
    qs = np.asarray(radial_points, dtype=float)
    n_qs = len(qs)
    grid = np.stack(np.meshgrid(np.arange(max_order + 1), qs, indexing='ij'), axis=-1)

    def side(line):                                                  # mathLibrary.py:1131-1137
        p1, p2 = np.array(line)
        rot = np.array([[0, 1], [-1, 0]]) @ (p2 - p1)
        return (-1 * np.sum((grid - p1) * rot[None, None, :], axis=-1)) >= 0
    if isinstance(line_specifier, tuple):
        mask1, mask2 = side(line_specifier[0]), side(line_specifier[1])
        if not invert:
            q1_id, q2_id = np.argmax(mask1, axis=1), np.argmax(mask2, axis=1)
            if not mask1.any():
                q1_id = n_qs - 1
            if not mask2.any():
                q2_id = n_qs - 1
        else:
            mask1, mask2 = ~mask1, ~mask2
            q1_id, q2_id = np.argmin(mask1, axis=1), np.argmin(mask2, axis=1)
            if mask1.all():
                q1_id = n_qs
            if mask1.all():                                          # (sic, 392: the first mask decides for the second line too)
                q2_id = n_qs
        q_id_limits = np.stack(np.broadcast_arrays(q1_id, q2_id), axis=-1)
        mask = mask1[:, :, None] * mask2[:, None, :]
    else:
        mask = side(line_specifier)
        if not invert:
            q_id = np.argmax(mask, axis=1)
            if not mask.any():
                q_id = n_qs - 1
        else:
            mask = ~mask
            q_id = np.argmin(mask, axis=1)
            if mask.all():
                q_id = n_qs
        mask = mask[:, :, None] * mask[:, None, :]
        q_id_limits = np.stack(np.broadcast_arrays(q_id, q_id), axis=-1)
    return mask, q_id_limits


def calc_deg_2_invariant_masks(dopt, bl_shape, q_mask, radial_points, max_order):
    """extract.py:332-364 for bl_q_limits types 'none' and 'line': returns (mask (orders, Nq, Nq), q_id_limits (orders, 2, 2))"""
    lim = dopt['bl_q_limits']
    min_type, max_type = lim['min']['type'], lim['max']['type']
    for t in (min_type, max_type):
        if t not in ('none', 'line'):
            raise NotImplementedError("bl_q_limits type %r (extract.py:342-353 knows 'line'; anything else means none)" % (t,))
    empty_mask = np.ones(bl_shape, dtype=bool)
    q_id_limits = np.zeros((bl_shape[0],) + (2, 2), dtype=int)
    q_id_limits[..., 1] = len(q_mask)
    if min_type == 'line':
        min_mask, q_id_mins = calc_deg_2_invariant_line_mask(radial_points, max_order, lim['min']['line'])
        q_id_limits[:, :, 0] = q_id_mins
    else:
        min_mask = empty_mask.copy()
    if max_type == 'line':
        max_mask, q_id_maxs = calc_deg_2_invariant_line_mask(radial_points, max_order, lim['max']['line'], invert=True)
        q_id_limits[:, :, 1] = q_id_maxs
    else:
        max_mask = empty_mask.copy()
    q_id_min = np.argmax(q_mask)
    q_id_max = len(q_mask) - np.argmax(q_mask[::-1])
    mask = min_mask & max_mask
    mask[:, ~q_mask] = False
    q_id_limits[q_id_limits[:, :, 0] < q_id_min] = q_id_min
    q_id_limits[q_id_limits[:, :, 1] > q_id_max] = q_id_max
    return mask, q_id_limits


def calc_projection_matrix_error_estimate(deg2_invariant, proj_matrices):
    """fxs_invariant_tools.py:1259-1269: |B_l - V_l V_l^+| / |B_l| where B_l != 0, -1 elsewhere"""
    errors = np.full_like(deg2_invariant, -1)
    for b, pr, e in zip(deg2_invariant, proj_matrices, errors):
        if pr.ndim == 1:
            pr = pr[:, None]
        nz = b != 0
        e[nz] = np.abs(b[nz] - (pr @ pr.conj().T)[nz]) / np.abs(b[nz])
    return errors


def extract_from_cross_correlation(engine, ccd, settings):
    """extract.py:95-168 + 496-532 for the dataset I1I1 in three or two dimensions: `ccd` as ``io.load_ccd`` returns it, `settings` the
    extract settings as a plain dict (default_0.01.yaml: dimensions, max_order, bl_eig_sort_mode, optimize_projection_matrices,
    low_resolution_intensity_approximation, cross_correlation.datasets.I1I1 ...).  Returns the `data` dict of the reconstruct worker
    with the key names of ``io.load_invariants`` (what _database_.py:611-646 saves)."""
    opt = settings
    dim = int(opt.get('dimensions', 3))
    if opt.get('extraction_mode', 'cross_correlation') != 'cross_correlation':
        raise NotImplementedError("extraction_mode %r (extract.py:72-77): this is the route 'cross_correlation'" % (opt['extraction_mode'],))
    if opt.get('optimize_projection_matrices', {}).get('use', False):
        raise NotImplementedError('optimize_projection_matrices.use: True (extract.py:446-451, prephase_projection_matrices 479-493)')
    if dim not in (2, 3):
        raise ValueError('dimensions must be 2 or 3')
    cco = opt['cross_correlation']
    to_process = cco.get('datasets_to_process', ['I1I1'])
    cc_arrays = ccd['cross_correlation']
    for name in cc_arrays:
        if name != 'I1I1' and name in cco['datasets'] and (not isinstance(to_process, (list, tuple)) or name in to_process):
            raise NotImplementedError('cross-correlation dataset %r (extract.py:122-159): only I1I1 is built' % (name,))
    dopt = cco['datasets']['I1I1']
    avg = ccd['average_intensity']
    avg = np.array(getattr(avg, 'data', avg), dtype=float)
    qs = np.asarray(ccd['radial_points'], dtype=float)
    phis = np.asarray(ccd['angular_points'], dtype=float)
    max_order = min(int(opt['max_order']), len(phis) // 2)                                               # 112-119
    meta = {**{k: v for k, v in ccd.items() if k != 'cross_correlation'}, **dopt, 'orders': np.arange(max_order + 1),
            'mode': dopt['bl_extraction_method'], 'average_intensity': avg}                              # 134
    if _wants_masked_route(dopt):
        minimum_norm = bool((opt.get('GPU') or {}).get('lstsq_minimum_norm', False))
        b_coeff, q_mask = masked_cross_correlation_to_deg2_invariant(engine, cc_arrays['I1I1'], dim,
                                                                     rank_deficient='minimum_norm' if minimum_norm else 'raise', **meta)
    else:
        b_coeff, q_mask = cross_correlation_to_deg2_invariant(engine, cc_arrays['I1I1'], dim, **meta)
    mask, q_id_limits = calc_deg_2_invariant_masks(dopt, b_coeff.shape, q_mask, qs, max_order)
    b_coeff = apply_invariant_constraints(engine, b_coeff, q_id_limits, dopt.get('bl_enforce_psd', False))
    if dopt.get('modify_cc', {}).get('subtract_average_intensity', False):                               # 160-167
        b_coeff[0] = avg[:, None] * avg[None, :] * (4 * np.pi if dim == 3 else 1)
    sort_mode = 1 if opt.get('bl_eig_sort_mode', 'eigenvalues') == 'median_of_scaled_eigenvector' else 0  # 436-439
    trapz = getattr(np, 'trapezoid', None) or np.trapz
    if dim == 2:
        # 129-130: the 2-D Fourier series whatever bl_extraction_method says (the kernel behind cross_correlation_to_deg2_invariant);
        # one projection vector per order (fxs_invariant_tools.py:1143-1169); 520: the weight q, times 4 pi as written; 526-528: the
        # low-resolution coefficients stay what the worker initialises them to (61)
        pms, _ = deg2_invariant_to_projection_matrices_2d(engine, b_coeff, q_id_limits=q_id_limits, sort_mode=sort_mode)
        errors = calc_projection_matrix_error_estimate(b_coeff, pms)
        return {'dimensions': dim, 'xray_wavelength': ccd['xray_wavelength'], 'average_intensity': avg, 'data_radial_points': qs,
                'data_angular_points': phis, 'data_min_q': float(qs.min()), 'max_order': max_order,
                'data_projection_matrices': np.array(pms), 'data_low_resolution_intensity_coefficients': False,
                'data_projection_matrices_q_id_limits': {'I1I1': q_id_limits[:, 0]},
                'data_projection_matrices_masks': {'I1I1': mask.sum(axis=2)}, 'data_projection_matrix_error_estimates': {'I1I1': errors},
                'integrated_intensity': trapz(avg * qs, x=qs, axis=0) * 4 * np.pi, 'deg_2_invariant': {'I1I1': b_coeff},
                'deg_2_invariant_masks': {'I1I1': mask}, 'deg_2_invariant_q_id_limits': {'I1I1': q_id_limits}, 'b_coeff': {'I1I1': b_coeff}}
    pms, _ = deg2_invariant_to_projection_matrices(engine, b_coeff, q_id_limits=q_id_limits, sort_mode=sort_mode)
    errors = calc_projection_matrix_error_estimate(b_coeff, pms)
    integrated = trapz(avg * qs ** 2, x=qs, axis=0) * 4 * np.pi                                          # 518
    low_order = int(opt.get('low_resolution_intensity_approximation', {}).get('max_order', 20))
    matrices = np.empty(len(pms), object)
    for i, m in enumerate(pms):
        matrices[i] = m
    low = np.empty(len(pms[:low_order + 1]), object)                                                     # 476
    for i, m in enumerate(pms[:low_order + 1]):
        low[i] = m
    return {'dimensions': dim, 'xray_wavelength': ccd['xray_wavelength'], 'average_intensity': avg, 'data_radial_points': qs,
            'data_angular_points': phis, 'data_min_q': float(qs.min()), 'max_order': max_order, 'data_projection_matrices': matrices,
            'data_low_resolution_intensity_coefficients': low, 'data_projection_matrices_q_id_limits': {'I1I1': q_id_limits[:, 0]},
            'data_projection_matrices_masks': {'I1I1': mask.sum(axis=2)}, 'data_projection_matrix_error_estimates': {'I1I1': errors},
            'integrated_intensity': integrated, 'deg_2_invariant': {'I1I1': b_coeff}, 'deg_2_invariant_masks': {'I1I1': mask},
            'deg_2_invariant_q_id_limits': {'I1I1': q_id_limits}, 'b_coeff': {'I1I1': b_coeff}}

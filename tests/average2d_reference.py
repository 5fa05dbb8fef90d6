"""numpy / longdouble restatement of the reference's 2-D averaging (xframe/projects/fxs/average.py:123-358, run_2d) and of the
functions it calls (resolution_metrics.py: _fsc 23-33, FSC_bit_limit 9-21, PRTF 63-79, FQCB_2D 146-187; misk.py:295-312;
fxs_Projections.py:1426-1434; mathLibrary.py:1254-1262; fxs_invariant_tools.py:872-914), written line by line from them: the
yardstick of tests/average2d_cases.py.  The operator references work in longdouble and also return the sum of the magnitudes of
the summed terms, the scale an a-priori rounding bound is stated on; `run_2d_ref` is the flow in double precision on transforms that
are handed in (oracle/polar2d.py in the tests), with the reference's in-place operations kept as in-place operations."""
import numpy as np

from so3_reference import LD, CLD, PI_LD, _cexp

_trapz = getattr(np, 'trapezoid', None) or np.trapz


# ------------------------------------------------------------------------------------------------------------------- operators
def phis_ld(n_phi):
    return 2 * PI_LD * np.arange(n_phi).astype(LD) / n_phi


def polar_integrate(values, rs, phis):
    """PolarIntegrator.integrate (mathLibrary.py:1258-1262), literally, in the precision of its arguments"""
    s_int = _trapz(values, x=phis, axis=1)
    return _trapz(s_int * rs, x=rs, axis=0)


def stats_ref(g, rs):
    """the statistics of k2a_stats for one grid g (Nq, n_phi): (values (9,) longdouble, sum of the magnitudes of the terms (9,)).
      [0] int Re, [1], [2] int Re x, int Re y: the moments of the centre of mass (misk.py:304-308) by the PolarIntegrator
      [3] np.max(g[g > 0].real) (average.py:171; -inf when there is no such entry, where numpy raises), [4] + i [5] their sum and
      [6] their count (178), `>` being numpy's lexicographic order on complex numbers; [7] max Re, [8] min Re (721-727)"""
    g = np.asarray(g)
    re, im = g.real.astype(LD), g.imag.astype(LD)
    rs = np.asarray(rs).astype(LD)
    phi = phis_ld(g.shape[1])
    x, y = rs[:, None] * np.cos(phi)[None, :], rs[:, None] * np.sin(phi)[None, :]
    val, mag = np.zeros(9, LD), np.zeros(9, LD)
    for i, t in enumerate((re, re * x, re * y)):
        val[i], mag[i] = polar_integrate(t, rs, phi), polar_integrate(np.abs(t), rs, phi)
    pos = g > 0
    assert np.array_equal(pos, (g.real > 0) | ((g.real == 0) & (g.imag > 0)))
    val[3] = np.max(g[pos].real) if pos.any() else -np.inf
    val[4], val[5], val[6] = re[pos].sum(), im[pos].sum(), pos.sum()
    mag[4], mag[5] = np.abs(re[pos]).sum(), np.abs(im[pos]).sum()
    val[7], val[8] = np.max(g.real), np.min(g.real)
    return val, mag


def phase_ref(g, center_xy, sign, qs):
    """g exp(-i sign k . c), k = q (cos phi, sin phi) (fxs_Projections.py:1427-1433), clongdouble"""
    g = np.asarray(g)
    phi = phis_ld(g.shape[1])
    q = np.asarray(qs).astype(LD)[:, None]
    kc = q * np.cos(phi)[None, :] * LD(float(center_xy[0])) + q * np.sin(phi)[None, :] * LD(float(center_xy[1]))
    return g.astype(CLD) * _cexp(-LD(float(sign)) * kc)


def inversion_metric_ref(F, F_ref, qs):
    """average.py:216-217: (diff, diff_inv) in longdouble, and the integral of |Im F| + |Im F_ref| as the scale of the terms"""
    a, r = np.asarray(F).imag.astype(LD), np.asarray(F_ref).imag.astype(LD)
    qs = np.asarray(qs).astype(LD)
    phi = phis_ld(a.shape[1])
    return (polar_integrate(np.abs(a - r), qs, phi), polar_integrate(np.abs(a - (-r)), qs, phi),
            polar_integrate(np.abs(a) + np.abs(r), qs, phi))


def combine_ref(op, A, scalars=None):
    """the operations of k2a_combine on a stack A (n, Nq, n_phi) in clongdouble"""
    A = np.asarray(A).astype(CLD)
    if op == 'conj':
        return A.conj()
    s = np.asarray(scalars).astype(CLD)
    if op == 'div':
        return A / s[:, None, None]
    if op == 'mean':
        return A.sum(axis=0) / s[0].real
    if op == 'abs2mean':
        return ((A.real ** 2 + A.imag ** 2).sum(axis=0) / s[0].real).astype(CLD)
    if op == 'affine':
        return (A - s[0].real) / s[1].real
    raise KeyError(op)


def prtf_points(a1, a2, b1, b2):
    """PRTF (resolution_metrics.py:63-71) up to the square root, literally"""
    prtf_nd = np.ones(a1.shape, dtype=complex)
    non_zero = (b1 != 0) & (b2 != 0)
    prtf_nd[non_zero] = (a1[non_zero] * a2[non_zero].conj()) / (b1[non_zero] * b2[non_zero].conj())
    prtf_nd[~non_zero & (a1 != 0) & (a2 != 0)] = 0
    return np.sqrt(prtf_nd)


def prtf_numpy(a1, a2, b1, b2):
    """PRTF (63-79) as numpy evaluates it: (average, std) per shell"""
    nd = prtf_points(a1, a2, b1, b2)
    axes = tuple(range(1, a1.ndim))
    return np.average(nd, axis=axes), np.std(nd, axis=axes)


def prtf_ref(a1, a2, I1, I2):
    """PRTF_fxs (90-101) per shell with the sums in longdouble: (mean (Nq,) clongdouble, std (Nq,) longdouble, sum of |nd| (Nq,))"""
    nd = prtf_points(np.asarray(a1), np.asarray(a2), np.sqrt(np.asarray(I1).real), np.sqrt(np.asarray(I2).real)).astype(CLD)
    n = nd.shape[1]
    mean = nd.sum(axis=1) / LD(n)
    dev = nd - mean[:, None]
    std = np.sqrt((dev.real ** 2 + dev.imag ** 2).sum(axis=1) / LD(n))
    return mean, std, np.sqrt(nd.real ** 2 + nd.imag ** 2).sum(axis=1)


def fsc(a1, a2):
    """_fsc (resolution_metrics.py:23-33), literally, in the precision of its arguments"""
    axes = tuple(range(1, a1.ndim))
    I1 = (a1 * a1.conj()).real
    I2 = (a2 * a2.conj()).real
    nominator = np.sum(a1 * a2.conj(), axis=axes).real
    denominator = np.sqrt(np.sum(I1, axis=axes) * np.sum(I2, axis=axes)).real
    non_zero = denominator != 0
    out = np.ones(nominator.shape, dtype=nominator.dtype)
    out[non_zero] = nominator[non_zero] / denominator[non_zero]
    return out


def fsc_ref(a1, a2):
    """_fsc in longdouble, and the condition scale of the numerator: sum |a1| |a2| / denominator (1 where that vanishes)"""
    a1, a2 = np.asarray(a1).astype(CLD), np.asarray(a2).astype(CLD)
    den = np.sqrt(np.sum(np.abs(a1) ** 2, axis=1) * np.sum(np.abs(a2) ** 2, axis=1))
    mag = np.where(den != 0, np.sum(np.abs(a1) * np.abs(a2), axis=1) / np.where(den != 0, den, 1), 1)
    return fsc(a1, a2), mag


def fsc_bit_limit(target_SNR, grid):
    """FSC_bit_limit (resolution_metrics.py:9-21), literally (line 20 as written)"""
    points_per_shell = np.prod(grid.shape[1:])
    half_dataset_SNR = target_SNR / 2
    x = half_dataset_SNR
    p = points_per_shell
    return (x + 2 * np.sqrt(x / p) + 1 / np.sqrt(p)) / (1 + x + 2 ** np.sqrt(x / p))


def fqcb_2d(bn1, bn2, return_2d_fqcb=False, skip_odd_orders=False, include_zero_order=False):
    """FQCB_2D (resolution_metrics.py:146-187), literally, in the precision of its arguments"""
    if skip_odd_orders:
        o_start, o_step = 2, 2
    else:
        o_start, o_step = 1, 1
    if include_zero_order:
        o_start = 0
    o_stop = min(len(bn1), len(bn2))
    b1 = ((bn1 + np.swapaxes(bn1, -1, -2)) / 2)[o_start:o_stop:o_step]
    b2 = ((bn2 + np.swapaxes(bn2, -1, -2)) / 2)[o_start:o_stop:o_step]
    B1 = (b1 * b1.conj()).real
    B2 = (b2 * b2.conj()).real
    bb_nominator = np.sum(b1 * b2.conj(), axis=0).real
    bb_denominator = np.sqrt(np.sum(B1, axis=0) * np.sum(B2, axis=0)).real
    non_zero = bb_denominator != 0
    bb = np.ones(b1.shape[1:], dtype=bb_nominator.dtype)
    bb[non_zero] = bb_nominator[non_zero] / bb_denominator[non_zero]
    bb = np.abs(bb)
    qq_mask = np.tril(np.ones(bb.shape)).astype(bool)
    fqc = np.mean(bb, axis=1, where=qq_mask)
    std = np.std(bb, axis=1, where=qq_mask)
    if return_2d_fqcb:
        return fqc, std, bb
    return fqc, std


def deg2_from_table(Ims, Ims2=False):
    """harmonic_coeff_to_deg2_invariants_2d (fxs_invariant_tools.py:906-914), literally"""
    if isinstance(Ims2, bool):
        return np.array(tuple(Im[:, None] * Im[None, :].conj() for Im in Ims.T))
    return np.array(tuple(Im1[:, None] * Im2[None, :].conj() for Im1, Im2 in zip(Ims.T, Ims2.T)))


def intensity_to_deg2_invariant(intensity, cht_forward):
    """intensity_to_deg2_invariant for a 2-D grid and the complex transform (fxs_invariant_tools.py:872-888)"""
    harm_coeff = cht_forward(intensity.astype(complex))
    n_orders = intensity.shape[-1] // 2 + 1
    return deg2_from_table(harm_coeff[..., :n_orders])


def averaged_projection_matrices(projection_matrices, average_scaling_factors):
    """get_averaged_projection_matrices (average.py:90-99), literally"""
    averaged_matrices = []
    n_matrices = len(projection_matrices[0])
    N_datasets = len(projection_matrices)
    for i in range(n_matrices):
        temp = projection_matrices[0][i] / average_scaling_factors[0] ** 2
        for j in range(1, N_datasets):
            temp += projection_matrices[j][i] / average_scaling_factors[j] ** 2
        averaged_matrices.append(temp / N_datasets)
    return averaged_matrices


# ------------------------------------------------------------------------------------------------------------------------ flow
class Flow2D:
    """what run_2d takes from its surroundings: the grid pair and the four transforms"""

    def __init__(self, rs, qs, n_phi, ft, ift, cht_forward, phis=None):
        self.rs, self.qs = np.asarray(rs, float), np.asarray(qs, float)
        self.phis = np.arange(n_phi) / n_phi * 2 * np.pi if phis is None else np.asarray(phis, float)
        self.fft, self.ifft, self.cht = ft, ift, cht_forward
        q, p = np.meshgrid(self.qs, self.phis, indexing='ij')
        self.cart_q = np.stack([q * np.cos(p), q * np.sin(p)], -1)           # spherical_to_cartesian of the reciprocal grid
        r, p = np.meshgrid(self.rs, self.phis, indexing='ij')
        self.cart_r = np.stack([r * np.cos(p), r * np.sin(p)], -1)

    def integrate_reciprocal(self, values):
        return polar_integrate(values, self.qs, self.phis)

    def find_center(self, density):
        """generate_calc_center (misk.py:304-311) and cartesian_to_spherical for two dimensions (r, phi in [0, 2 pi))"""
        density_integral = polar_integrate(density.real, self.rs, self.phis)
        if density_integral == 0:
            density_integral = 1
        cx = polar_integrate(self.cart_r[..., 0] * density.real, self.rs, self.phis) / density_integral
        cy = polar_integrate(self.cart_r[..., 1] * density.real, self.rs, self.phis) / density_integral
        phi = np.arctan2(cy, cx)                                         # cartesian_to_spherical, mathLibrary.py:638-644
        return np.array([np.sqrt(np.square(cx) + np.square(cy)), np.where(phi < 0, phi + 2 * np.pi, phi)])

    def negative_shift(self, reciprocal_density, vector):
        """generate_shift_by_operator(opposite_direction=True), dim 2 (fxs_Projections.py:1426-1434): IN PLACE"""
        cart_vect = np.array([vector[0] * np.cos(vector[1]), vector[0] * np.sin(vector[1])])
        phases = np.exp(-1.j * -1 * (self.cart_q * cart_vect).sum(axis=-1))
        reciprocal_density *= phases
        return reciprocal_density

    def shift_to_center(self, density, ft_density):
        """assemble_shift_to_center (average.py:1021-1027): the second argument is shifted in place and handed back"""
        center = self.find_center(density)
        return [self.ifft(self.negative_shift(self.fft(density), center)), self.negative_shift(ft_density, center), center]


def normalize_density(d, d_min=False):
    """average.py:721-727"""
    if isinstance(d_min, bool):
        d_min = d.real.min()
    d_max = np.max(d.real)
    return (d - d_min) / (d_max - d_min)


def run_2d_ref(fl, reconstructions, errors, opt, projection_matrices=None, reconstruction_ids_per_file=None):
    """run_2d (average.py:123-358) for the keys that do not depend on files.  reconstructions: list of [density, ft_density] (copied
    here; the reference edits its inputs).  opt: center_reconstructions, normalize_reconstructions {use, mode},
    pointinvert_reference, selection {n_reconstructions}, resolution_metrics {PRTF, pseudo_FSC, FQCB}.  The FQCB branch is the
    evident intent of 266-301 (upstream its first call cannot run): intensity_to_deg2_invariant(I, cht=cht)."""
    import warnings
    reconstructions = [[np.array(r[0], complex), np.array(r[1], complex)] for r in reconstructions]
    n_in = len(reconstructions)
    if reconstruction_ids_per_file is None:
        reconstruction_ids_per_file = [np.arange(n_in)]
    n_reconstructions = opt.get('selection', {}).get('n_reconstructions', 'all')
    if not isinstance(n_reconstructions, int) or isinstance(n_reconstructions, bool):
        n_reconstructions = n_in
    reference_arg = int(np.argmin(errors))
    fft, ifft = fl.fft, fl.ifft
    if opt.get('center_reconstructions', False):
        for r_id, r in enumerate(reconstructions):
            temp = fl.shift_to_center(*r)
            reconstructions[r_id] = temp[:2]
    scaling_factors = np.ones(n_in)
    norm = opt.get('normalize_reconstructions', {})
    if norm.get('use', False):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            if norm['mode'] == 'max':
                for r_id, r in enumerate(reconstructions):
                    scale = np.max(r[0][r[0] > 0].real)
                    scaling_factors[r_id] = scale
                    reconstructions[r_id] = [r[0] / scale, r[1] / scale]
            elif norm['mode'] == 'mean':
                for r_id, r in enumerate(reconstructions):
                    scale = np.mean(r[0][r[0] > 0])
                    scaling_factors[r_id] = scale
                    reconstructions[r_id] = [r[0] / scale, r[1] / scale]
    average_scaling_factors_per_file = np.ones(len(reconstruction_ids_per_file))
    for file_id, r_ids in enumerate(reconstruction_ids_per_file):
        average_scaling_factors_per_file[file_id] = np.mean(scaling_factors[r_ids])
    integrate = fl.integrate_reciprocal
    reference_reconstruction = reconstructions.pop(reference_arg)
    d_ref = reference_reconstruction[0].copy()
    ft_d_ref = reference_reconstruction[1].copy()
    if opt.get('pointinvert_reference', False):
        ft_d_ref = ft_d_ref.conj()
        d_ref = ifft(fft(d_ref).conj())
    aligned_reconstructions = [[d_ref, ft_d_ref]]
    p_inv_metric = []
    ft_d_ref_pinv = ft_d_ref.conj()
    for i, reconstruction in enumerate(reconstructions):
        d, ft_d = reconstruction
        diff = integrate(np.abs(ft_d.imag - ft_d_ref.imag))
        diff_inv = integrate(np.abs(ft_d.imag - ft_d_ref_pinv.imag))
        point_inverted = diff > diff_inv
        if point_inverted:
            new_ft_d = ft_d.copy().conj()
            new_d = ifft(fft(d).conj())
        else:
            new_ft_d = ft_d
            new_d = d
        aligned_reconstructions.append([new_d, new_ft_d])
        p_inv_metric.append([diff, diff_inv, int(point_inverted)])
    if len(aligned_reconstructions) >= n_reconstructions:
        aligned_reconstructions = aligned_reconstructions[:n_reconstructions]
    average_density = np.mean(np.array(tuple(r[0] for r in aligned_reconstructions)), axis=0)
    average_ft_density = np.mean(np.array(tuple(r[1] for r in aligned_reconstructions)), axis=0)
    aligned_ft_reconstr_ftd = [fft(r[0]) for r in aligned_reconstructions]
    intensity_from_ft_density = np.mean([(r[1] * r[1].conj()).real for r in aligned_reconstructions], axis=0)
    intensity_from_density = np.mean([(r * r.conj()).real for r in aligned_ft_reconstr_ftd], axis=0)
    centered_average = fl.shift_to_center(average_density, average_ft_density)
    resolution_metrics = {}
    mopt = opt.get('resolution_metrics', {})
    if mopt.get('PRTF', False):
        b_d, b_ft = np.sqrt(intensity_from_density), np.sqrt(intensity_from_ft_density)
        a_d = fft(average_density)
        for name, args in (('PRTF', (a_d, average_ft_density, b_d, b_ft)), ('PRTF_from_density', (a_d, a_d, b_d, b_d)),
                           ('PRTF_from_ft_density', (average_ft_density, average_ft_density, b_ft, b_ft)),
                           ('PRTF_ftI', (a_d, a_d, b_ft, b_ft))):
            resolution_metrics[name], resolution_metrics[name + '_std'] = prtf_numpy(*args)
    if mopt.get('FQCB', False):
        ft_d = fft(average_density)
        b_d_rec = intensity_to_deg2_invariant(ft_d * ft_d.conj(), fl.cht)
        b_ftd_rec = intensity_to_deg2_invariant(average_ft_density * average_ft_density.conj(), fl.cht)
        pr_mat = np.squeeze(np.array(averaged_projection_matrices(projection_matrices, average_scaling_factors_per_file)))
        b_target = deg2_from_table(pr_mat.T)
        fqcb_d = fqcb_2d(b_d_rec, b_target, skip_odd_orders=True)
        fqcb_ftd = fqcb_2d(b_ftd_rec, b_target, skip_odd_orders=True)
        fqcb_rec = fqcb_2d(b_ftd_rec, b_d_rec, skip_odd_orders=True)
        fqcb_d_z = fqcb_2d(b_d_rec, b_target, skip_odd_orders=True, include_zero_order=True)
        fqcb_ftd_z = fqcb_2d(b_ftd_rec, b_target, skip_odd_orders=True, include_zero_order=True)
        for name, val in (('FQCB_from_density', fqcb_d), ('FQCB_from_ft_density', fqcb_ftd), ('FQCB_projected_vs_unprojected', fqcb_rec),
                          ('FQCB_from_density_with_zero_order', fqcb_d_z), ('FQCB_from_ft_density_with_zero_order', fqcb_ftd_z)):
            resolution_metrics[name], resolution_metrics[name + '_std'] = val
        resolution_metrics['FQCB_bl_from_density'] = b_d_rec
        resolution_metrics['FQCB_bl_from_ft_density'] = b_ftd_rec
        resolution_metrics['FQCB_bl_target'] = b_target
    if mopt.get('pseudo_FSC', False):
        resolution_metrics['pseudo_FSC'] = fsc(fft(average_density), average_ft_density)
        rgrid = np.zeros(fl.rs.shape + fl.phis.shape + (2,))
        resolution_metrics['FSC_0.5bit_limit'] = fsc_bit_limit(0.5, rgrid)
    return {
        'average': {'real_density': average_density, 'normalized_real_density': normalize_density(average_density),
                    'reciprocal_density': average_ft_density, 'intensity_from_densities': intensity_from_density,
                    'intensity_from_ft_densities': intensity_from_ft_density},
        'resolution_metrics': resolution_metrics,
        'centered_average': {'real_density': centered_average[0], 'normalized_real_density': normalize_density(centered_average[0]),
                             'reciprocal_density': centered_average[1]},
        'aligned': {str(i): {'real_density': r[0], 'reciprocal_density': r[1]} for i, r in enumerate(aligned_reconstructions)},
        'input_meta': {'scaling_factors': np.array(scaling_factors), 'average_scaling_factors_per_file': np.array(average_scaling_factors_per_file)},
        'inversion_metric': {str(i + 1): np.array(m) for i, m in enumerate(p_inv_metric)},
        'reference_arg': reference_arg, 'point_inverted': [bool(m[2]) for m in p_inv_metric],
    }


# --------------------------------------------------------------------------------------------------------- extract, dimensions = 2
def nearest_psd(A):
    """nearest_positive_semidefinite_matrix (mathLibrary.py:872-892) with limit 0"""
    B = (A + np.swapaxes(A, -1, -2).conj()) / 2
    l, v = np.linalg.eigh(B)
    l[l < 0] = 0
    return v * l[..., None, :] @ np.swapaxes(v, -1, -2).conj()


def deg2_eigenvalues(b_matrix, sort_mode=0):
    """deg2_invariant_eigenvalues (fxs_invariant_tools.py:1114-1141), scipy's eigh with the driver 'ev' as there"""
    import scipy.linalg
    b_matrix = (b_matrix + b_matrix.T.conj()) / 2
    if not np.isclose(b_matrix, 0).all():
        eig_vals, eig_vect = scipy.linalg.eigh(b_matrix, driver='ev')
    else:
        eig_vect, eig_vals = np.zeros(b_matrix.shape), np.zeros(b_matrix.shape[0])
    if sort_mode == 0:
        sort_metric = eig_vals
    else:
        sort_metric = np.median(np.abs(np.sqrt(np.abs(eig_vals[None, :])) * eig_vect), axis=0) * np.sign(eig_vals)
    sorted_ids = np.argsort(sort_metric)[::-1]
    return eig_vals[sorted_ids].real, eig_vect[:, sorted_ids]


def projection_vector_2d(b_coeff, q_id_limits, sort_mode=0):
    """deg2_invariant_to_projection_matrices_2d (fxs_invariant_tools.py:1143-1169) for one order: (vector (Nq,), eigenvalue)"""
    q_slice = slice(*q_id_limits[0])
    eig_vals, eig_vect = deg2_eigenvalues(b_coeff[q_slice, q_slice], sort_mode)
    eig_val, eig_vect = eig_vals[0], eig_vect[:, 0].copy()
    if not eig_val >= 0:
        eig_val = 0
        eig_vect[:] = 0
    full = np.zeros(len(b_coeff), dtype=eig_vect.dtype)
    full[q_slice] = eig_vect
    return full * np.sqrt(eig_val), eig_val


def extract_2d_ref(b_coeff, q_id_limits, avg, qs, enforce_psd, subtract_average_intensity, sort_mode=0):
    """extract.py:140-167, 441, 520 for dimensions = 2 after cross_correlation_to_deg2_invariant: (b_coeff, vectors, integrated)"""
    lim = np.array(q_id_limits)
    out = b_coeff.copy()
    if enforce_psd:
        for o in range(len(b_coeff)):
            s = slice(*lim[o, 0])
            out[o, s, s] = nearest_psd(b_coeff[o, s, s])
    if subtract_average_intensity:
        out[0] = avg[:, None] * avg[None, :] * 1
    vectors = [projection_vector_2d(out[o], lim[o], sort_mode)[0] for o in range(len(out))]
    return out, vectors, _trapz(avg * qs, x=qs, axis=0) * 4 * np.pi

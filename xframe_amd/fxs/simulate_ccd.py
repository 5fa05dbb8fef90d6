"""The upstream worker ``fxs simulate_ccd``: a density -> degree-2 invariants B_l -> cross-correlation C(q1, q2, Delta), the data set the
``extract`` worker starts from.  Host mirror of

    xframe/projects/fxs/simulate_ccd.py:92-298                                  InvariantExtractor (shapes, grid, B_l, scalings, cc_data)
    xframe/projects/fxs/projectLibrary/fxs_invariant_tools.py:889-923           density_to_deg2_invariants
                                                              934-1031          deg2_invariant_to_cc_2d / _3d and their workers
    xframe/library/mathLibrary.py:137-167                                       SampleShapeFunctions.get_disk_function

with the arithmetic on the device: the front half on the engine's operators (Fourier transform, forward SHT, B_l = I_l I_l^+), the back
half in the kernels of ``csrc/k_simulate.h`` (``Engine.deg2_to_cc``).  Shapes, grids and tables are set-up arithmetic on the host.  What
the reference offers and this route does not build raises NotImplementedError with the option and the reference line (DESIGN section
6): there is no CPU fallback."""
import numpy as np

from . import hostsetup as hs
from .settings import DictNamespace, reciprocity_coefficient, resolve_simulate_ccd

_CC_MODES = ('lstsq', 'back_substitution', 'legendre')                # the keys of fxs_invariant_tools.py:946


def ewald_thetas(radial_points, xray_wavelength):
    """ewald_sphere_theta_pi (physicsLibrary.py:94-95)"""
    thetas = np.arccos(np.asarray(radial_points, dtype=float) * xray_wavelength / (4 * np.pi))
    if not np.isfinite(thetas).all():
        raise ValueError('q * wavelength / (4 pi) > 1: the radial points do not lie on the Ewald sphere of this wavelength')
    return thetas


def legendre_table_t(radial_points, xray_wavelength, max_order):
    """((L + 1)(L + 2) / 2, Nq) table of mtip_op_deg2_to_cc: gsl_sf_legendre_sphPlm(l, n, cos theta_q) at row l (l + 1) / 2 + n -- the
    table of ``extract.legendre_table`` at stride 1, transposed so that neighbouring shells are neighbours in memory
    (fxs_invariant_tools.py:60-74, 962)."""
    x = np.cos(ewald_thetas(radial_points, xray_wavelength))
    li, ni = np.tril_indices(int(max_order) + 1)
    return np.ascontiguousarray(hs.sph_plm(li[:, None], ni[:, None], x[None, :]))


def _check_orders(orders, n_orders):
    if orders is None or isinstance(orders, (bool, np.bool_)):
        return
    if not np.array_equal(np.asarray(orders), np.arange(n_orders)):
        raise NotImplementedError('orders other than arange(len(bl)) (fxs_invariant_tools.py:951-952 is what the worker uses)')


def _check_mode(mode):
    if mode not in _CC_MODES:
        raise ValueError('Given cc creation mode "{}" is unknown. Known modes are {}" (fxs_invariant_tools.py:946-950, where the lookup '
                         'then fails)'.format(mode, list(_CC_MODES)))
    if mode == 'legendre':
        raise NotImplementedError("cross_correlation.method 'legendre' (fxs_invariant_tools.py:1028-1031 cc_3d_legendre_worker): it needs "
                                  "the fast Legendre transform plugin `flt`; built are back_substitution and lstsq")


def deg2_invariant_to_cc(engine, bl, xray_wavelength, data_grid, orders=None, mode='back_substitution'):
    """fxs_invariant_tools.py:941-990 with the arithmetic on the device.  bl (L + 1, Nq, Nq), a numpy array or a tensor on the engine's
    device; data_grid {'qs', 'phis'}.
    'back_substitution' (979-988): (Nq, Nq, 2L) float64 whatever data_grid['phis'] holds, as upstream.
    'lstsq' (963-971): (Nq, Nq, len(phis)) complex128.  The reference evaluates the samples phis <= pi and assigns their mirror
    [1:-1][::-1] to the samples above: that only fits a grid whose samples <= pi come first and outnumber the others by two (a
    uniform grid of even length with pi on it); any other grid raises ValueError here, before anything is launched (upstream it is
    numpy's shape error at 971).
    'legendre' (1028-1031) needs the `flt` plugin and is not built."""
    _check_mode(mode)
    _check_orders(orders, int(bl.shape[0]))
    if int(bl.shape[0]) < 2:
        raise ValueError('deg2_invariant_to_cc: max_order = 0 (a single order has no angular dependence; the inverse transform of '
                         'size 0 fails upstream too)')
    qs = np.asarray(data_grid['qs'], dtype=float)
    thetas = ewald_thetas(qs, xray_wavelength)                                                           # 962
    if mode == 'back_substitution':
        return engine.deg2_to_cc(bl, 'back_substitution', 3, legendre_t=legendre_table_t(qs, xray_wavelength, int(bl.shape[0]) - 1))
    phis = np.asarray(data_grid['phis'], dtype=float)
    low = phis <= np.pi                                                                                  # 965
    n_low = int(low.sum())
    if n_low < 2 or not low[:n_low].all() or len(phis) - n_low != n_low - 2:
        raise ValueError('lstsq: the angular grid has %d samples <= pi and %d above; the mirror [1:-1][::-1] of the first onto the second '
                         '(fxs_invariant_tools.py:970-971) needs the samples <= pi first and two more of them than of the others, i.e. a '
                         'uniform grid of even length that contains pi' % (n_low, len(phis) - n_low))
    return engine.deg2_to_cc(bl, 'lstsq', 3, cos_sin_theta=np.stack([np.cos(thetas), np.sin(thetas)]), cos_delta=np.cos(phis[:n_low]))


def deg2_invariant_to_cc_2d(engine, bl):
    """fxs_invariant_tools.py:934-939: irfft(B_m size, size) along the order axis, size = 2 (M - 1); (Nq, Nq, size) float64"""
    if int(bl.shape[0]) < 2:
        raise ValueError('deg2_invariant_to_cc_2d: max_order = 0 (an inverse transform of size 0)')
    return engine.deg2_to_cc(bl, 'back_substitution', 2)


def density_to_deg2_invariants(engine, density):
    """fxs_invariant_tools.py:889-923 in three dimensions on the engine's operators: I = |FT rho|^2, I_lm = SHT(I), B_l = I_l I_l^+ --
    (L + 1, N, N) complex128 exactly as the reference forms it: no 1/4 and no symmetrisation (those belong to the stored convention of
    ``synthetic.invariants_from_intensity_coefficients``)."""
    rho = np.asarray(density).astype(complex)
    if rho.shape != engine.shape:
        raise ValueError('density_to_deg2_invariants: the density has shape %r, the engine\'s grid %r' % (rho.shape, engine.shape))
    ft = engine.fourier_transform(rho)
    intensity = ft * ft.conj()                                                                          # 892
    return engine.deg2_invariants(engine.sht_forward(intensity))[0]


def spherical_to_cartesian(points):
    """mathLibrary.py:673-698 for (.., 3) points (r, theta, phi)"""
    p = np.asarray(points, dtype=float)
    r, theta, phi = p[..., 0], p[..., 1], p[..., 2]
    xy = r * np.sin(theta)
    return np.stack([np.cos(phi) * xy, np.sin(phi) * xy, r * np.cos(theta)], axis=-1)


def _check_shapes(shapes):
    for t in np.asarray(shapes['types']).tolist():
        if t != 'sphere':
            raise NotImplementedError("shapes.types %r (simulate_ccd.py:154-165: tetrahedron, cube and the max-norm fallback): only "
                                      "'sphere' (151-153) is built" % (t,))
    if np.asarray(shapes['random_orientation']).any():
        raise NotImplementedError('shapes.random_orientation: True (mathLibrary.py:159-160 draws a rotation from '
                                  'scipy.stats.special_ortho_group per call): only False is built')


def shape_density(grid, shapes):
    """simulate_ccd.py:148-167 for shapes of type 'sphere': the sum over the shapes of density * [|x - centre| < size] on the points of
    `grid` (.., 3) in spherical coordinates (SampleShapeFunctions.get_disk_function, mathLibrary.py:137-167, coordSys 'spherical',
    norm 'standard': centres in spherical coordinates, strict <)."""
    _check_shapes(shapes)
    centers = np.asarray(shapes['centers'], dtype=float).reshape(len(shapes['types']), -1)               # 103: one float array
    sizes, values = np.asarray(shapes['sizes'], dtype=float), np.asarray(shapes['densities'], dtype=float)
    cart = spherical_to_cartesian(grid)
    density = np.zeros(cart.shape[:-1], dtype=float)
    for center, size, value in zip(centers, sizes, values):                                              # 149 (zip: the shortest list)
        inside = np.linalg.norm(cart - spherical_to_cartesian(center), axis=-1) < size                   # 158, 163
        density += np.where(inside, value, 0.0)
    return density


def simulation_grid(opt):
    """simulate_ccd.py:103-123: (max_q, n_radial_points, max_r) from grid.max_q, or from grid.oversampling and the extent of the shapes"""
    kappa = float(reciprocity_coefficient(opt['fourier_transform']))
    n = int(opt['grid']['n_radial_points'])
    max_q = opt['grid']['max_q']
    if isinstance(max_q, (bool, np.bool_)):
        radius = opt.get('shape_size', 'not given')
        if not isinstance(radius, (float, int)) or isinstance(radius, bool):
            radius = np.max(np.asarray(opt['shapes']['centers'], dtype=float)[:, 0] + np.asarray(opt['shapes']['sizes'], dtype=float))
        else:
            radius = radius / 2
        max_r = opt['grid']['oversampling'] * radius
        max_q = kappa * n / max_r                                                                        # mathLibrary.py:1169-1176
    else:
        max_r = kappa * n / max_q
    return float(max_q), n, float(max_r)


def simulate_ccd(settings=None, density=None, lib_path=None, device=0):
    """The worker's flow (simulate_ccd.py:271-298, 92-172, 194-230, 256-266) for dimensions 3.  `settings`: overrides on
    ``settings.simulate_ccd_default_settings()``; `density`: a density on the engine's real grid instead of the shapes.  Returns a
    namespace (cc_data, density, grid, integrated_intensity (281)): cc_data with exactly the keys of 285-292 -- 'radial_points', 'angular_points' (arange(2L) pi / L),
    'xray_wavelength', 'cross_correlation' {'I1I1'}, 'average_intensity', 'deg_2_invariant' {'I1I1'}, 'number_of_particles' -- which
    ``io.load_ccd(cc_data, 'direct')`` and ``extract_from_cross_correlation`` take as it is; the density and the real grid
    (N, n_theta, n_phi, 3) are what the reference saves beside it (46).

    One fact of the reference is reproduced on purpose: number_of_particles is the constant 1 of InvariantExtractor.__init__ (71); the
    setting n_particles is read (208) and never used, so the scaling of 211-212 multiplies by 1 and cc_data['number_of_particles']
    is 1 whatever the settings say.
    Sizes beyond the limits of a transforms-only engine (max_order > 128, n_phi > 512) raise from the engine's constructor.  At the
    reference's tutorial size (settings/simulate_ccd/tutorial.yaml: 512 shells, max_order 128, a 256 x 512 angular grid) the engine holds
    about 13 GB of device memory (ten grids of 1.07 GB and the tables), every host array of grid size is 1 GB, and the one-off Hankel
    weights (hostsetup.hankel_raw_weights(128, 512, ..)) take 32 s of one core on the CPU-only host the code was developed on and about
    12 s on the host of the MI355X it was measured on, before the first kernel runs: the first call is not hung.  There the first call took
    26 s and the next, with the weights cached, 14 s (profiles/simulate_timing.txt section 5)."""
    from .engine import Engine
    opt = resolve_simulate_ccd(settings)
    if int(opt['dimensions']) != 3:
        raise NotImplementedError('simulate_ccd with dimensions = %r (simulate_ccd.py:139-141, 264-265): the flow is built for 3; the '
                                  '2-D operator itself is deg2_invariant_to_cc_2d' % (opt['dimensions'],))
    method = opt['cross_correlation']['method']
    _check_mode(method)                                                                                  # (before anything runs)
    if density is None:
        _check_shapes(opt['shapes'])
    max_q, n, _ = simulation_grid(opt)
    L = int(opt['grid']['max_order'])
    engine = Engine({'grid': {k: opt['grid'][k] for k in ('max_order', 'n_phi', 'n_theta', 'n_radial_points')},
                     'fourier_transform': opt['fourier_transform']}, None, n_batch=1, device=device, lib_path=lib_path, max_q=max_q)
    try:
        grid = np.stack(np.meshgrid(engine.rs, engine.theta, engine.phi, indexing='ij'), axis=-1)
        if density is None:
            density = shape_density(grid, opt['shapes'])
        number_of_particles = 1                                                                          # 71 (n_particles: 208, unused)
        bl = density_to_deg2_invariants(engine, density)                                                 # 210
        bl *= number_of_particles                                                                        # 211
        bl[0] *= number_of_particles                                                                     # 212
        average_intensity = np.sqrt(np.diag(bl[0]).real / (4 * np.pi))                                   # 230
        qs = np.array(engine.qs)                                                                         # 136
        phis = np.arange(0, L * 2) * np.pi / L                                                           # 138, ft_grid_pairs.py:557-558
        wavelength = opt['cross_correlation']['xray_wavelength']
        cc = deg2_invariant_to_cc(engine, bl, wavelength, {'qs': qs, 'phis': phis}, mode=method)         # 256-263
    finally:
        engine.close()
    trapz = getattr(np, 'trapezoid', None) or np.trapz
    integrated_intensity = trapz(average_intensity * qs ** 2, x=qs, axis=0) * 4 * np.pi                  # 281
    cc_data = {'radial_points': qs, 'angular_points': phis, 'xray_wavelength': wavelength, 'cross_correlation': {'I1I1': cc},
               'average_intensity': average_intensity, 'deg_2_invariant': {'I1I1': bl}, 'number_of_particles': number_of_particles}
    return DictNamespace(cc_data=cc_data, density=density, grid=grid, integrated_intensity=integrated_intensity)

#!/usr/bin/env python3
"""tests/golden/simulate_ccd.npz (G28): the reference's worker `simulate_ccd` on seeded data.

Run:  python tests/golden/make_golden_simulate.py   (build container only: needs the reference checkout make_golden.py names)

Outputs of the reference's OWN functions:
  * deg2_invariant_to_cc_3d (fxs_invariant_tools.py:941-990) in the modes back_substitution and lstsq, and deg2_invariant_to_cc_2d
    (934-939), each on a seeded real B_l and a seeded complex non-Hermitian B_l (simulate_cases.seeded_bl) at 16 shells x L = 8 and at
    5 shells x L = 7 (odd L: 14 angles), on the angular grid of the worker, arange(2L) pi / L (ft_grid_pairs.py:557-558);
  * ccd_associated_legendre_matrices_single_l (60-74) of the highest order;
  * SampleShapeFunctions.get_disk_function (mathLibrary.py:137-167) for two off-centre spheres on a small spherical grid;
  * the worker's flow at 12 shells x L = 6 (simulate_cases.FLOW), pieced together from the functions InvariantExtractor calls
    (simulate_ccd.py:103-166 grid and density, 191 generate_ft, 210-212 density_to_deg2_invariants and the particle-number scaling,
    230 average_intensity, 263 the cross-correlation, 281 integrated_intensity), with the Fourier transform built as make_golden.py
    builds it for G2.
pygsl and shtns are absent: `mathLibrary.gsl` gets make_golden_cc.gsl_double(), `mathLibrary.shtns` make_golden.ShAdapter.  The worker
processes of Multiprocessing.comm_module.request_mp_evaluation are replaced by one call of the worker function on the flattened
meshgrid of the two index arrays, reshaped to (n_q, n_q, ...) (the lstsq worker indexes whole arrays, fxs_invariant_tools.py:997-1000).
Only inputs and outputs (data) are written; no reference source is copied."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..'))

import make_golden as MG                                              # noqa: E402  (bootstrap, ShAdapter; puts the repository on sys.path)
import make_golden_cc as MGC                                          # noqa: E402  (the gsl stand-in)


class OneCall:
    @staticmethod
    def request_mp_evaluation(func, input_arrays=(), const_inputs=(), **kw):
        a, b = input_arrays
        ia, ib = np.meshgrid(a, b, indexing='ij')
        out = np.asarray(func(ia.ravel(), ib.ravel(), *const_inputs))
        return out.reshape(ia.shape + out.shape[1:])


def main():
    mods = MG.bootstrap()
    ml = mods['xframe.library.mathLibrary']
    mp = mods['xframe.Multiprocessing']
    ml.shtns = MG.ShAdapter
    ml.gsl = MGC.gsl_double()
    mp.comm_module = OneCall
    pre = 'xframe.projects.fxs.projectLibrary.'
    it = importlib.import_module(pre + 'fxs_invariant_tools')
    import simulate_cases as SC
    from xframe_amd.fxs import settings as ST, simulate_ccd as SIM
    if not hasattr(np, 'trapz'):
        np.trapz = np.trapezoid

    out = {'G28_wavelength': np.array(SC.WAVELENGTH)}
    for nq, L in SC.GOLDEN_SIZES:
        qs = SC.CC.radial_points(nq)
        phis = np.arange(0, L * 2) * np.pi / L                         # get_polar_fft_angles_from_max_order
        assert (phis <= np.pi).sum() == L + 1
        thetas = np.arccos(qs * SC.WAVELENGTH / (4 * np.pi))
        out[f'G28_qs_{nq}'], out[f'G28_phis_{nq}'] = qs, phis
        out[f'G28_qq_matrix_{nq}'] = it.ccd_associated_legendre_matrices_single_l(thetas, L, L)
        for kind in ('real', 'cplx'):
            bl = SC.seeded_bl(nq, L, 2800 + nq, kind)
            out[f'G28_bl_{kind}_{nq}'] = bl
            grid = {'qs': qs, 'phis': phis}
            out[f'G28_cc_bs_{kind}_{nq}'] = it.deg2_invariant_to_cc_3d(bl.copy(), SC.WAVELENGTH, grid, mode='back_substitution')
            out[f'G28_cc_ls_{kind}_{nq}'] = it.deg2_invariant_to_cc_3d(bl.copy(), SC.WAVELENGTH, grid, mode='lstsq')
            out[f'G28_cc_2d_{kind}_{nq}'] = it.deg2_invariant_to_cc_2d(bl.copy(), None)
            for k in ('bs', 'ls', '2d'):
                a = out[f'G28_cc_{k}_{kind}_{nq}']
                print(nq, L, kind, k, a.shape, a.dtype, np.abs(a).max())
    # shapes
    disk = np.zeros(SC.disk_grid().shape[:-1])
    sh = SC.DISK_SHAPES
    for center, size, dval in zip(np.asarray(sh['centers']), np.asarray(sh['sizes']), np.asarray(sh['densities'])):
        f = ml.SampleShapeFunctions.get_disk_function(size, lambda points, dval=dval: np.full(points.shape[:-1], dval), center=center,
                                                      norm='standard', random_orientation=False, coordSys='spherical')
        disk += f(SC.disk_grid())
    out['G28_disk_density'] = disk
    print('disk density: nonzero', np.count_nonzero(disk), 'of', disk.size)
    # the flow
    opt = ST.resolve_simulate_ccd(SC.FLOW)
    hts = importlib.import_module(pre + 'harmonic_transforms')
    fts = importlib.import_module(pre + 'fourier_transforms')
    gp = importlib.import_module(pre + 'ft_grid_pairs')
    ht = importlib.import_module(pre + 'hankel_transforms')
    kappa = opt['fourier_transform']['reciprocity_coefficient']
    L, N = opt['grid']['max_order'], opt['grid']['n_radial_points']
    centers, sizes = np.asarray(opt['shapes']['centers']), np.asarray(opt['shapes']['sizes'])
    max_r = opt['grid']['oversampling'] * np.max(centers[:, 0] + sizes)                                   # 111-117
    max_q = ml.polar_spherical_dft_reciprocity_relation_radial_cutoffs(max_r, N, reciprocity_coefficient=kappa)
    cht = hts.HarmonicTransform('complex', {'dimensions': 3, 'max_order': L, **opt['grid']})              # 127-129
    grid_pair = gp.get_grid({'dimensions': 3, 'type': 'midpoint', 'max_q': max_q, 'n_radial_points': N, **cht.grid_param,
                             'reciprocity_coefficient': kappa})                                           # 132-133
    real_grid = np.array(grid_pair.realGrid[:])
    qs = np.array(grid_pair.reciprocalGrid[:, 0, 0, 0])
    density = np.zeros(real_grid.shape[:-1], dtype=float)
    for center, size, dval in zip(centers, sizes, np.asarray(opt['shapes']['densities'])):               # 149-166
        f = ml.SampleShapeFunctions.get_disk_function(size, lambda points, dval=dval: np.full(points.shape[:-1], dval), center=center,
                                                      norm='standard', random_orientation=False, coordSys='spherical')
        density += f(real_grid)
    wd = {'weights': ht.calc_spherical_mid_weights(np.arange(L + 1), N, kappa), 'posHarmOrders': np.arange(L + 1)}
    r_max = real_grid[:, 0, 0, 0].max()                                                                   # 178
    ft, _ = fts.generate_ft(r_max, wd, cht, 3, pos_orders=np.arange(L + 1), reciprocity_coefficient=kappa, use_gpu=False, mode='midpoint')
    number_of_particles = 1                                                                               # 71
    bl = it.density_to_deg2_invariants(density.astype(complex), ft, 3, cht=cht)                           # 210
    bl *= number_of_particles
    bl[0] *= number_of_particles
    avg = np.sqrt(np.diag(bl[0]).real / (4 * np.pi))                                                      # 230
    phis = gp.get_polar_fft_angles_from_max_order(L)                                                      # 138
    cc = it.deg2_invariant_to_cc_3d(bl, opt['cross_correlation']['xray_wavelength'], {'qs': qs, 'phis': phis},
                                    mode=opt['cross_correlation']['method'], n_processes=True)             # 263
    integrated = np.trapz(avg.data * qs ** 2, x=qs, axis=0) * 4 * np.pi                                   # 281
    out.update({'G28_flow_rs': real_grid[:, 0, 0, 0], 'G28_flow_qs': qs, 'G28_flow_grid': real_grid, 'G28_flow_density': density,
                'G28_flow_bl': bl, 'G28_flow_cc': cc, 'G28_flow_average_intensity': avg, 'G28_flow_angular_points': phis,
                'G28_flow_integrated_intensity': np.array(integrated), 'G28_flow_number_of_particles': np.array(number_of_particles),
                'G28_flow_wavelength': np.array(opt['cross_correlation']['xray_wavelength'])})
    print('flow: grid', real_grid.shape, 'max_q', max_q, 'density nonzero', np.count_nonzero(density), 'of', density.size, '|B_l| per order',
          [float(np.linalg.norm(b)) for b in bl], 'cc', cc.shape, cc.dtype, 'integrated', integrated)
    assert np.array_equal(SIM.shape_density(real_grid, opt['shapes']), density)
    path = os.path.join(HERE, 'simulate_ccd.npz')
    np.savez_compressed(path, **out)
    print('simulate_ccd fixture:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

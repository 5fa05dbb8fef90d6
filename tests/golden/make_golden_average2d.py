#!/usr/bin/env python3
"""Golden vectors of the 2-D averaging and the 2-D extract rules: outputs of the REFERENCE's own functions on seeded inputs at
12 shells x M = 6 (build container only; needs /root/reference, never runs on the GPU box).

Run:  python tests/golden/make_golden_average2d.py      -> tests/golden/average2d.npz

resolution_metrics.py: FQCB_2D in the five argument combinations of average.py:282-286, FSC_single_fxs, FSC_bit_limit, PRTF_fxs in
both forms; fxs_invariant_tools.py: harmonic_coeff_to_deg2_invariants_2d, intensity_to_deg2_invariant (called as evidently meant,
with cht as keyword), deg2_invariant_to_projection_matrices_2d (a negative definite block included); misk.generate_calc_center,
fxs_Projections.generate_shift_by_operator and PolarIntegrator.integrate on the polar midpoint grid pair.
Only inputs and outputs (data) are written; no reference source is copied."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..'))

import make_golden as MG                                              # noqa: E402  (bootstrap; puts the repository on sys.path)


def main():
    mods = MG.bootstrap()
    ml = mods['xframe.library.mathLibrary']
    ml.shtns = MG.ShAdapter
    pl = mods['xframe.library.pythonLibrary']
    st = mods['xframe.settings']
    import types as _t

    class _Any:
        def __init__(s, *a, **k):
            pass

        def __getattr__(s, n):
            return _Any()

        def __call__(s, *a, **k):
            return _Any()

    class AnyModule(_t.ModuleType):
        def __getattr__(s, n):
            if n.startswith('__'):
                raise AttributeError(n)
            return _Any()
    for name in ('xframe.presenters', 'xframe.presenters.matplotlibPresenter', 'xframe.presenters.openCVPresenter'):
        sys.modules[name] = AnyModule(name)
    from oracle import mtip as OM
    from xframe_amd.fxs import synthetic as S
    o = OM.deep_update(OM.default_settings(), S.config_overrides(1))
    st.project = pl.DictNamespace.dict_to_dictnamespace(o)
    pre = 'xframe.projects.fxs.projectLibrary.'
    rm = importlib.import_module(pre + 'resolution_metrics')
    it = importlib.import_module(pre + 'fxs_invariant_tools')
    misk = importlib.import_module(pre + 'misk')
    fpj = importlib.import_module(pre + 'fxs_Projections')
    gp = importlib.import_module(pre + 'ft_grid_pairs')
    hts = importlib.import_module(pre + 'harmonic_transforms')
    rng = np.random.default_rng(3030)
    N, M, max_q = 12, 6, 2.0
    n_phi = 2 * M + 1
    out = {'N': np.array(N), 'M': np.array(M), 'max_q': np.array(max_q)}
    grid = gp.get_grid({**o['fourier_transform'], 'type': 'midpoint', 'dimensions': 2, 'n_radial_points': N, 'max_q': max_q,
                        'phis': np.arange(n_phi) / n_phi * 2 * np.pi})
    out['rs'], out['qs'] = np.asarray(grid.realGrid[:, 0, 0]), np.asarray(grid.reciprocalGrid[:, 0, 0])
    out['grid_shape'] = np.array(grid.reciprocalGrid[:].shape)
    out['phis'], out['phis_reciprocal'] = np.asarray(grid.realGrid[0, :, 1]), np.asarray(grid.reciprocalGrid[0, :, 1])
    # ---- curves
    a1, a2 = MG.cplx(rng, (N, n_phi)), MG.cplx(rng, (N, n_phi))
    I1, I2 = np.abs(MG.cplx(rng, (N, n_phi))) ** 2, np.abs(MG.cplx(rng, (N, n_phi))) ** 2
    I1[rng.random((N, n_phi)) < 0.1] = 0
    I2[rng.random((N, n_phi)) < 0.1] = 0
    I1[1] = 0
    I2[2] = 0
    a1[2, ::2] = 0
    a1[3] = 0
    out.update(a1=a1, a2=a2, I1=I1, I2=I2)
    p = rm.PRTF_fxs(a1, I1, averaged_projected_scattering_amplitude=a2, averaged_projected_intensity=I2)
    out['prtf_mean'], out['prtf_std'] = p[0], p[1]
    p = rm.PRTF_fxs(a1, I1)
    out['prtf_single_mean'], out['prtf_single_std'] = p[0], p[1]
    out['fsc'] = rm.FSC_single_fxs(a1, a2)
    out['fsc_limit'] = np.array(rm.FSC_bit_limit(0.5, grid.reciprocalGrid[:]))
    # ---- invariants and FQCB
    cht = hts.HarmonicTransform('complex', {'dimensions': 2, 'max_order': M})
    Id, Iftd = np.abs(MG.cplx(rng, (N, n_phi))) ** 2, np.abs(MG.cplx(rng, (N, n_phi))) ** 2
    Iftd[N // 2] = 0
    out['Id'], out['Iftd'] = Id, Iftd
    out['cht_Id'] = np.array(cht.forward(Id.astype(complex)))
    b_d = it.intensity_to_deg2_invariant(Id, cht=cht)
    b_ftd = it.intensity_to_deg2_invariant(Iftd, cht=cht)
    pr_mat = MG.cplx(rng, (M, N))                                     # one order fewer than the reconstructions: o_stop = min(...)
    b_t = it.harmonic_coeff_to_deg2_invariants(2, pr_mat.T)
    out.update(b_d=b_d, b_ftd=b_ftd, pr_mat=pr_mat, b_target=b_t)
    for name, args, kw in (('d', (b_d, b_t), {}), ('ftd', (b_ftd, b_t), {}), ('rec', (b_ftd, b_d), {}),
                           ('d_z', (b_d, b_t), {'include_zero_order': True}), ('ftd_z', (b_ftd, b_t), {'include_zero_order': True})):
        f = rm.FQCB_2D(*args, skip_odd_orders=True, **kw)
        out['fqcb_' + name], out['fqcb_' + name + '_std'] = f[0], f[1]
    f = rm.FQCB_2D(b_d, b_t)
    out['fqcb_all_orders'], out['fqcb_all_orders_std'] = f[0], f[1]
    # ---- projection vectors
    v = MG.cplx(rng, (3, N))
    B = np.array([v[0][:, None] * v[0][None, :].conj() + 0.01 * np.eye(N), v[1][:, None] * v[1][None, :].conj(),
                  -(v[2][:, None] * v[2][None, :].conj() + 0.05 * np.eye(N))])
    lim = np.array([[[0, N], [0, N]], [[3, N], [3, N]], [[0, N], [0, N]]])
    out['pv_B'], out['pv_lim'] = B, lim
    for i in range(3):
        pm, ev = it.deg2_invariant_to_projection_matrices_2d(B[i].copy(), lim[i], i, 0)
        out[f'pv_{i}'], out[f'pv_eig_{i}'] = np.asarray(pm), np.array(ev)
    # ---- centre, shift, integrator
    r, ph = np.asarray(grid.realGrid[..., 0]), np.asarray(grid.realGrid[..., 1])
    dens = (np.exp(-((r * np.cos(ph) - 0.2 * r.max()) ** 2 + (r * np.sin(ph) + 0.3 * r.max()) ** 2) / (0.25 * r.max()) ** 2)
            * (1 + 0.1 * rng.random((N, n_phi)))).astype(complex) + 0.05j * rng.normal(size=(N, n_phi))
    F = MG.cplx(rng, (N, n_phi))
    out['dens'], out['F'] = dens, F
    center = misk.generate_calc_center(grid.realGrid)(dens)
    out['center'] = np.asarray(center)
    out['F_negative_shift'] = fpj.generate_shift_by_operator(grid.reciprocalGrid, opposite_direction=True)(F.copy(), center)
    out['F_shift'] = fpj.generate_shift_by_operator(grid.reciprocalGrid)(F.copy(), center)
    out['integral_real'] = np.array(ml.PolarIntegrator(grid.realGrid[:]).integrate(dens.real))
    out['integral_reciprocal'] = np.array(ml.PolarIntegrator(grid.reciprocalGrid[:]).integrate(np.abs(F.imag)))
    path = os.path.join(HERE, 'average2d.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

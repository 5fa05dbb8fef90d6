#!/usr/bin/env python3
"""tests/golden/correlate.npz (G25): the reference's `correlate` stage after the polar resampling, on seeded data.

Run:  python tests/golden/make_golden_correlate.py   (build container only: needs the reference checkout make_golden.py names)

Outputs of the reference's OWN functions at 4 rings x 16 angles:
  * ccf_analysis.ccf_twopoint_q1_q2_mask_corrected, symmetrize_ccf (positions of correlate.py:262-264 on an even and on an awkward
    phi offset) and ccf_fcs (projectLibrary/cross_correlation.py);
  * DataReader.process_image (correlate.py:377-452) on a stand-in `self` that holds exactly the attributes it reads, for every
    entry of correlate_cases.SWITCHES (each switch alone and all together) and four patterns: a plain one, a fully masked one, a
    ten times brighter one (rejected where the ROI mean filter is on) and one with a fully masked ring.  cart_x / cart_y are the
    index grid of an (n_q, n_phi) array and interp_order = 0, so the reference's map_coordinates is the identity and lines 401-452
    run on polar data; then ccf_twopoint_q1_q2_mask_corrected on what it returns;
  * DataReader._prepare_polar_representation (489-559) for the phi_range modes exact / max / min, and the correction tables of
    _determine_polarization_correction / _determine_solid_angle_correction (565-591).
Only inputs and outputs (data) are written; no reference source is copied."""
import functools
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..'))

import make_golden as MG                                              # noqa: E402  (bootstrap; puts the repository on sys.path)


def main():
    cwd = os.getcwd()
    MG.bootstrap()
    # the worker module pulls in the framework's interfaces and database at import: stand-ins with the names it reads
    for name, attrs in (('xframe.interfaces', {'ProjectWorkerInterface': object}), ('xframe.database', {'project': None})):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
            setattr(sys.modules['xframe'], name.split('.')[-1], m)
    co = importlib.import_module('xframe.projects.fxs.correlate')
    xc = importlib.import_module('xframe.projects.fxs.projectLibrary.cross_correlation')
    os.chdir(cwd)
    import correlate_cases as CC
    from xframe_amd.fxs import correlate as CR
    DR = co.DataReader

    n_q, n_phi, P = 4, 16, 4
    images, masks = CC.make_patterns(n_q, n_phi, P, 2525, masked_pattern=1, rejected_pattern=2, masked_ring=(3, 1))
    out = {'G25_n_q': np.array(n_q), 'G25_n_phi': np.array(n_phi), 'G25_images': images, 'G25_masks': masks}

    def stand_in(settings):
        opt = CR.resolve_correlate(settings)
        me = types.SimpleNamespace(pixelsize=opt['pixel_size'], det_sam=opt['sample_distance'], wavelng=opt['wavelength'],
                                   dpcenter=opt['detector_origin'])
        DR._prepare_polar_representation(me, opt['qrange'], opt['qrange_xcca'], opt['phi_range'])
        return me, opt

    # ---- process_image, every switch set
    for name, sw in CC.SWITCHES.items():
        settings = CC.make_settings(n_q, n_phi, **sw)
        me, opt = stand_in(settings)
        assert me.n_q == n_q and me.n_phi == n_phi
        me.compute = ['is_good', 'waxs', 'xcca']
        me.intensity_pixel_threshold = [False, 0, 0]
        me.mask_binary_inp = False
        me.background_subtraction = False
        me.interp_order = 0
        gx, gy = np.meshgrid(np.arange(n_q), np.arange(n_phi), indexing='ij')
        me.cart_x, me.cart_y = gx.astype(float), gy.astype(float)
        me.intensity_radial_pixel_filter = opt['intensity_radial_pixel_filter']
        me.ROInormalization, me.ROImeanfilter = opt['ROI_normalization'], opt['ROI_mean_filter']
        me.ROInorm_qpos1 = np.abs(me.qvals - me.ROInormalization[1]).argmin()            # correlate.py:187-188
        me.ROInorm_qpos2 = np.abs(me.qvals - me.ROInormalization[2]).argmin()
        me.xpolarization = opt['polarization_correction']
        me.solid_angle_correction = opt['solid_angle_correction']
        if me.xpolarization[0]:
            DR._determine_polarization_correction(me)
        if me.solid_angle_correction is True:
            DR._determine_solid_angle_correction(me)
        for f in ('i_average_and_sigma_azimuthal', 'i_average_azimuthal', 'i_median_and_mad'):
            setattr(me, f, functools.partial(getattr(DR, f), me))
        xcca = xc.ccf_analysis(me.n_q1, me.n_q2, n_phi, me.q1vals_pos, me.q2vals_pos)
        for p in range(P):
            v = DR.process_image(me, images[p].copy(), masks[p].copy())
            tag = f'G25_{name}_p{p}_'
            out[tag + 'is_good'] = np.array(int(v['is_good']))
            out[tag + 'waxs'] = np.asarray(v['waxs'], dtype=float) * np.ones(n_q)
            if isinstance(v.get('image_polar', 0), np.ndarray):
                out[tag + 'image'], out[tag + 'mask'] = np.asarray(v['image_polar'], float), np.asarray(v['mask_polar']).astype(np.int64)
                ccf, valid = xcca.ccf_twopoint_q1_q2_mask_corrected(v['image_polar'], v['mask_polar'])
                out[tag + 'ccf'], out[tag + 'ccf_valid'] = np.array(ccf), np.array(valid)
            print(name, p, 'is_good', int(v['is_good']), 'waxs', np.round(out[tag + 'waxs'], 2))

    # ---- ccf_analysis alone: rectangular, strided selection
    me, _ = stand_in(CC.make_settings(n_q, n_phi, (0, n_q - 1, 1), (0, n_q - 1, 2)))
    xcca = xc.ccf_analysis(me.n_q1, me.n_q2, n_phi, me.q1vals_pos, me.q2vals_pos)
    img, msk = CC.make_patterns(n_q, n_phi, 1, 2526, masked_ring=(0, 2))
    ccf, valid = xcca.ccf_twopoint_q1_q2_mask_corrected(img[0], msk[0])
    ccf = np.array(ccf)
    out.update({'G25_q1': np.asarray(me.q1vals_pos), 'G25_q2': np.asarray(me.q2vals_pos), 'G25_ccf_image': img[0], 'G25_ccf_mask': msk[0],
                'G25_ccf': ccf, 'G25_ccf_valid': np.array(valid), 'G25_fcs': xcca.ccf_fcs(ccf)})
    for tag, phi_min in (('even', 0.0), ('awkward', 0.37)):
        phi = np.arange(n_phi) * 2 * np.pi / n_phi + phi_min
        pos = (np.abs(phi - np.pi / 2.0).argmin(), np.abs(phi - np.pi).argmin(), np.abs(phi - 3 * np.pi / 2.0).argmin())
        out[f'G25_sym_{tag}_phi'], out[f'G25_sym_{tag}'] = phi, xcca.symmetrize_ccf(ccf, *pos)

    # ---- geometry and correction tables
    for mode in ('exact', 'max', 'min'):
        me, _ = stand_in(dict(CC.g25_geometry_settings(), phi_range=(0.1, 0.1 + 2 * np.pi, 64, mode)))
        for k in ('qvals', 'theta', 'phi', 'cart_x', 'cart_y', 'q1vals_pos', 'q2vals_pos'):
            out[f'G25_geo_{mode}_{k}'] = np.asarray(getattr(me, k))
        out[f'G25_geo_{mode}_n_phi'] = np.array(me.n_phi)
    me, _ = stand_in(CC.make_settings(n_q, n_phi))
    for kind in ('h', 'v'):
        me.xpolarization = [True, kind]
        DR._determine_polarization_correction(me)
        out[f'G25_pfactor_{kind}'] = me.Pfactor.copy()
    DR._determine_solid_angle_correction(me)
    out['G25_solang'] = me.SolAngCorr.copy()

    path = os.path.join(HERE, 'correlate.npz')
    np.savez_compressed(path, **out)
    print('correlate fixture:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

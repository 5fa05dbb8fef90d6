#!/usr/bin/env python3
"""tests/golden/correlate_median_mad.npz (G29): the reference's median_mad radial pixel filter on seeded data.

Run:  python tests/golden/make_golden_median_mad.py   (build container only: needs the reference checkout make_golden.py names)

Outputs of the reference's OWN functions:
  * DataReader.i_median_and_mad (correlate.py:471-474) on a 3 x 700 array: a row at 70 % valid samples, a fully masked row (NaN, NaN)
    and a row with more than half of its samples equal (mad = 0);
  * DataReader.process_image (377-452) at 4 rings x 16 angles on the stand-in `self` of make_golden_correlate.py (index-grid
    coordinates and interp_order = 0, so lines 401-452 run on polar data), for intensity_radial_pixel_filter ['median_mad', 3] and
    ['median_mad', 1.5], alone and with every other switch of correlate_cases.SWITCHES['all'] on, and four patterns: a plain one, a
    fully masked one, a ten times brighter one (rejected where the ROI mean filter is on) and one with a fully masked ring; then
    ccf_analysis.ccf_twopoint_q1_q2_mask_corrected on what it returns.
The reference's module calls `spst.median_abs_deviation` (473) and never imports `spst`, so upstream the option ends in a NameError;
the name is bound here to scipy.stats, its evident meaning, and nothing else is changed.
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
    if not hasattr(co, 'spst'):                                       # line 473 reads a module global `spst` that no line binds
        co.spst = importlib.import_module('scipy.stats')
    os.chdir(cwd)
    import correlate_cases as CC
    import ringfilter_cases as RF
    from xframe_amd.fxs import correlate as CR
    DR = co.DataReader

    # ---- i_median_and_mad alone
    rng = np.random.default_rng(2929)
    rows = 200.0 * (1.0 + 0.4 * rng.random((3, 700)))
    rows[rng.random(rows.shape) < 0.04] *= 2.5
    rows_mask = np.ones((3, 700), np.int64)
    rows_mask[0] = rng.random(700) < 0.7
    rows_mask[1] = 0
    rows[2, rng.permutation(700)[:400]] = 211.5
    med, mad = DR.i_median_and_mad(None, rows, rows_mask)
    out = {'G29_rows': rows, 'G29_rows_mask': rows_mask, 'G29_rows_median': np.asarray(med, float), 'G29_rows_mad': np.asarray(mad, float)}
    print('i_median_and_mad:', med, mad)

    # ---- process_image
    n_q, n_phi, P = 4, 16, 4
    images, masks = CC.make_patterns(n_q, n_phi, P, 2929, masked_pattern=1, rejected_pattern=2, masked_ring=(3, 1))
    out.update({'G29_n_q': np.array(n_q), 'G29_n_phi': np.array(n_phi), 'G29_images': images, 'G29_masks': masks})
    for k in RF.G29_KS:
        for name, sw in RF.G29_SWITCHES.items():
            opt = CR.resolve_correlate(RF.mad_settings(n_q, n_phi, k, **sw))
            me = types.SimpleNamespace(pixelsize=opt['pixel_size'], det_sam=opt['sample_distance'], wavelng=opt['wavelength'],
                                       dpcenter=opt['detector_origin'])
            DR._prepare_polar_representation(me, opt['qrange'], opt['qrange_xcca'], opt['phi_range'])
            assert me.n_q == n_q and me.n_phi == n_phi
            me.compute = ['is_good', 'waxs', 'xcca']
            me.intensity_pixel_threshold = [False, 0, 0]
            me.mask_binary_inp = False
            me.background_subtraction = False
            me.interp_order = 0
            gx, gy = np.meshgrid(np.arange(n_q), np.arange(n_phi), indexing='ij')
            me.cart_x, me.cart_y = gx.astype(float), gy.astype(float)
            me.intensity_radial_pixel_filter = opt['intensity_radial_pixel_filter']
            assert me.intensity_radial_pixel_filter == [True, ['median_mad', k]]
            me.ROInormalization, me.ROImeanfilter = opt['ROI_normalization'], opt['ROI_mean_filter']
            me.ROInorm_qpos1 = np.abs(me.qvals - me.ROInormalization[1]).argmin()        # correlate.py:187-188
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
                tag = f'G29_k{k}_{name}_p{p}_'
                out[tag + 'is_good'] = np.array(int(v['is_good']))
                out[tag + 'waxs'] = np.asarray(v['waxs'], dtype=float) * np.ones(n_q)
                if isinstance(v.get('image_polar', 0), np.ndarray):
                    out[tag + 'image'], out[tag + 'mask'] = np.asarray(v['image_polar'], float), np.asarray(v['mask_polar']).astype(np.int64)
                    ccf, valid = xcca.ccf_twopoint_q1_q2_mask_corrected(v['image_polar'], v['mask_polar'])
                    out[tag + 'ccf'], out[tag + 'ccf_valid'] = np.array(ccf), np.array(valid)
                    print(tag, 'is_good', int(v['is_good']), 'kept', int(out[tag + 'mask'].sum()), 'of', int(masks[p].sum()))
                else:
                    print(tag, 'is_good', int(v['is_good']))
            # the condition the device comparison needs: every exact pair count >= 1, or 0 because a whole ring is masked
            x = CC.x_correlate(*RF.filtered(images, masks, k), CC.params(CC.make_settings(n_q, n_phi, **sw)))
            assert x['holes'] == 0 and x['roi_margin'] > 1e-9, (k, name, x['holes'], x['roi_margin'])

    path = os.path.join(HERE, 'correlate_median_mad.npz')
    np.savez_compressed(path, **out)
    print('median_mad fixture:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

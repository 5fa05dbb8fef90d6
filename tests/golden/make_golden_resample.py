#!/usr/bin/env python3
"""tests/golden/resample.npz (G26): the Cartesian stage of the reference's `correlate`, on seeded data.

Run:  python tests/golden/make_golden_resample.py   (build container only: needs the reference checkout make_golden.py names)

Outputs of the reference's OWN DataReader.process_image (correlate.py:377-452) on the stand-in `self` of make_golden_correlate.py:
three frames of 24 x 20 with values up to 1000 and initial masks (random dead pixels, a dead rectangle, a dead column), real
cart_x / cart_y of DataReader._prepare_polar_representation (8 rings x 16 angles whose outer rings leave the frame), at
interp_order 0, 2, 3 and 5, with the intensity threshold on and off, with a background, with an integer-typed mask_binary (so that
line 385 runs), and with all of them.  The radial pixel filter, the ROI switches and the correction tables are off, so image_polar
and mask_polar are what lines 395-398 produce.  Only inputs and outputs (data) are written; no reference source is copied."""
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
    for name, attrs in (('xframe.interfaces', {'ProjectWorkerInterface': object}), ('xframe.database', {'project': None})):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__dict__.update(attrs)
            sys.modules[name] = m
            setattr(sys.modules['xframe'], name.split('.')[-1], m)
    co = importlib.import_module('xframe.projects.fxs.correlate')
    os.chdir(cwd)
    import resample_cases as RC
    from xframe_amd.fxs import correlate as CR
    DR = co.DataReader

    H, W, n_q, n_phi, P = 24, 20, 8, 16, 3
    images, masks, binary, background = RC.make_frames(H, W, P, 2626)
    threshold = np.array(RC.THRESHOLD)
    settings = RC.detector_settings(H, W, n_q, n_phi)
    opt = CR.resolve_correlate(settings)
    me = types.SimpleNamespace(pixelsize=opt['pixel_size'], det_sam=opt['sample_distance'], wavelng=opt['wavelength'],
                               dpcenter=opt['detector_origin'])
    DR._prepare_polar_representation(me, opt['qrange'], opt['qrange_xcca'], opt['phi_range'])
    assert (me.n_q, me.n_phi) == (n_q, n_phi)
    out = {'G26_images': images, 'G26_masks': masks, 'G26_binary': binary, 'G26_background': background, 'G26_threshold': threshold,
           'G26_cart_x': np.asarray(me.cart_x), 'G26_cart_y': np.asarray(me.cart_y), 'G26_q_max': np.array(opt['qrange'][1]),
           'G26_q_step': np.array(opt['qrange'][2]), 'G26_origin': np.array(opt['detector_origin']),
           'G26_pixel_size': np.array(opt['pixel_size']), 'G26_sample_distance': np.array(opt['sample_distance']),
           'G26_wavelength': np.array(opt['wavelength'])}
    outside = np.mean((me.cart_x < 0) | (me.cart_x > H - 1) | (me.cart_y < 0) | (me.cart_y > W - 1))
    print('points outside the frame:', outside)
    assert 0.2 < outside < 0.5

    me.compute = ['is_good', 'waxs', 'xcca']
    me.intensity_radial_pixel_filter = [False, ['average_sigma', 3]]
    me.ROInormalization, me.ROImeanfilter = [False, 0.0, 0.0], [False, 0.0, 0.0]
    me.xpolarization, me.solid_angle_correction = [False, 'h'], False
    me.mask_binary = binary.astype(np.int64)
    me.background_data = background
    for f in ('i_average_and_sigma_azimuthal', 'i_average_azimuthal', 'i_median_and_mad'):
        setattr(me, f, functools.partial(getattr(DR, f), me))
    for order in RC.G26_ORDERS:
        me.interp_order = order
        for name, sw in RC.G26_SETS.items():
            me.intensity_pixel_threshold = [bool(sw.get('thr')), threshold[0], threshold[1]]
            me.mask_binary_inp = bool(sw.get('bin'))
            me.background_subtraction = bool(sw.get('bg'))
            for p in range(P):
                v = DR.process_image(me, images[p].copy(), masks[p].copy())
                tag = f'G26_o{order}_{name}_p{p}_'
                assert v['mask_polar'].dtype.kind == 'i'
                out[tag + 'image'] = np.asarray(v['image_polar'], float)
                out[tag + 'mask'] = np.asarray(v['mask_polar']).astype(np.int8)
    path = os.path.join(HERE, 'resample.npz')
    np.savez_compressed(path, **out)
    print('resample fixture:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

"""Cases of the route patterns -> C(q1, q2, Delta) (csrc/k_correlate.h, fxs/correlate.py), shared by tests/test_emul_correlate.py (CPU
emulator, toy sizes) and tests/test_gpu_correlate.py (MI355X).

Three yardsticks:
  * G25 (tests/golden/correlate.npz): outputs of the reference's own ccf_analysis functions and of DataReader.process_image /
    _prepare_polar_representation / the correction tables on seeded data (tests/golden/make_golden_correlate.py);
  * the numpy restatement below (each function cites its reference lines), held to G25 by a CPU test;
  * an independent longdouble direct-sum correlation with exact integer pair counts.

Conditions on the inputs, asserted by the case builder (reference()):
  * wherever a case is compared with the restatement every exact pair count is >= 1, or 0 because a whole ring is masked: the
    reference's test M != 0 is deterministic there and equals the device's |M| >= 0.5;
  * no pixel sits within 1e-12 sigma of the average_sigma threshold, no ROI mean within 1e-9 of its limits.
Tolerances: count, is_good exact; sum per element  4 eps log2(n_phi) sum_p |I_p(q1)|_2 |I_p(q2)|_2 / M_p + P eps |sum|  (a-priori:
numpy's own error is 0.13-0.28 of it without the factor 4, which is the margin for another radix plan and twiddle table); ring
statistics (waxs) relative 1e-13 against longdouble."""
import functools
import os
import warnings

import numpy as np

from helpers import rel_l2
from xframe_amd.fxs import _lib, correlate as CR, extract as X, io as IO
from ccextract_cases import small_engine

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'correlate.npz')
EPS = np.finfo(float).eps
TOL_STAT = 1e-13
TOL_GOLDEN = 1e-14
WAVES = 4                 # COR_WAVES: pairs per workgroup
CHUNK = 32                # COR_CHUNK: patterns per pass over the accumulators
Q_STEP, Q_MIN = 0.0625, 0.125

# the switch sets of G25: each alone and all together (make_golden_correlate.py runs process_image on exactly these)
SWITCHES = {
    'plain': {},
    'filter': {'filter': 1.5},
    'roi_filter': {'roi_filter': (80.0, 400.0)},
    'roi_norm': {'roi_norm': True},
    'pol_h': {'pol': 'h'},
    'pol_v': {'pol': 'v'},
    'solid': {'solid': True},
    'all': {'filter': 1.5, 'roi_filter': (80.0, 400.0), 'roi_norm': True, 'pol': 'h', 'solid': True},
}


# ---- settings --------------------------------------------------------------------------------------------------------------------------
def make_settings(n_q, n_phi, sel1=None, sel2=None, filter=None, roi_filter=None, roi_norm=False, pol=None, solid=False, phi_min=0.0,
                  q_step=Q_STEP, q_min=Q_MIN, **top):
    """settings of the correlate worker for n_q rings (binary-exact q values, so that n_q and the selections come out as asked);
    sel = (first ring, last ring, step)"""
    qvals = np.arange(n_q) * q_step + q_min
    sel1 = sel1 or (0, n_q - 1, 1)
    sel2 = sel2 or sel1
    s = {'compute': ['is_good', 'waxs_aver', 'ccf_q1q2'], 'qrange': [q_min, qvals[-1], q_step],
         'qrange_xcca': [[qvals[sel1[0]], qvals[sel1[1]], sel1[2]], [qvals[sel2[0]], qvals[sel2[1]], sel2[2]]],
         'phi_range': (phi_min, phi_min + 2 * np.pi, n_phi, 'exact'),
         'intensity_radial_pixel_filter': [filter is not None, ['average_sigma', 3 if filter is None else filter]],
         'ROI_normalization': [bool(roi_norm), qvals[min(1, n_q - 1)], qvals[n_q - 1]],
         'ROI_mean_filter': [roi_filter is not None] + list(roi_filter or (1e2, 1e4)),
         'polarization_correction': [pol is not None, pol or 'h'], 'solid_angle_correction': bool(solid)}
    s.update(top)
    return s


def params(settings):
    """what process_image reads, from the settings (the tables through fxs.correlate, which a test holds to G25)"""
    opt = CR.resolve_correlate(settings)
    g = CR.polar_geometry(opt)
    filt, rn, rf, pol = opt['intensity_radial_pixel_filter'], opt['ROI_normalization'], opt['ROI_mean_filter'], opt['polarization_correction']
    q = g['qvals']
    return {'filter': filt[1][1] if filt[0] else None, 'roi': (int(np.abs(q - rn[1]).argmin()), int(np.abs(q - rn[2]).argmin())),
            'roi_filter': (rf[1], rf[2]) if rf[0] else None, 'roi_norm': bool(rn[0]),
            'pfactor': CR.polarization_factor(g['theta'], g['phi'], pol[1]) if pol[0] else None,
            'solang': CR.solid_angle_factor(g['theta'], g['n_phi']) if opt['solid_angle_correction'] is True else None,
            'q1': g['q1vals_pos'], 'q2': g['q2vals_pos'], 'phi': g['phi'], 'n_q': g['n_q'], 'n_phi': g['n_phi']}


# ---- numpy restatement (dtype float64: the reference's route; longdouble: the ring statistics' yardstick) ----------------------------------
def r_process_image(image, mask, prm, dtype=np.float64):
    """process_image after the resampling (correlate.py:401-452): {'is_good', 'waxs', 'image', 'mask', 'margin', 'roi_mean'}"""
    image = np.array(image, dtype=dtype)
    mask = np.array(mask, dtype=int)
    out = {'is_good': 0, 'waxs': np.zeros(image.shape[0], dtype=dtype), 'image': None, 'mask': None, 'margin': np.inf, 'roi_mean': None}
    with np.errstate(invalid='ignore', divide='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)                                  # (numpy announces the mean of an empty ring)
        if prm['filter'] is not None:                                                    # 402-413
            av = np.mean(image, axis=1, where=(mask == 1))                               # 458-461
            sig = np.std(image, axis=1, where=(mask == 1))
            dev, thr = np.abs(image - av[:, None]), prm['filter'] * sig[:, None]
            m = np.abs(dev - thr) / sig[:, None]
            sel = (mask == 1) & np.isfinite(m)
            if sel.any():
                out['margin'] = float(m[sel].min())
            mask[dev > thr] = 0
            image = image * mask
        if np.sum(mask) == 0:                                                            # 418-421
            return out
        is_good = 1
        lo, hi = prm['roi']
        if prm['roi_filter'] is not None or prm['roi_norm']:
            roi = np.mean(image[lo:hi], where=(mask[lo:hi] == 1))                        # 425
            out['roi_mean'] = roi
        if prm['roi_filter'] is not None and (roi < prm['roi_filter'][0] or roi > prm['roi_filter'][1]):
            is_good = 0                                                                  # 427-429
        if prm['roi_norm']:
            image = np.divide(image, roi)                                                # 431-432
        if prm['pfactor'] is not None:
            image = np.multiply(image, prm['pfactor'].astype(dtype))                     # 434-435
        if prm['solang'] is not None:
            image = np.multiply(image, prm['solang'].astype(dtype))                      # 437-438
        out.update(is_good=is_good, waxs=np.mean(image, axis=1, where=(mask == 1)), image=image, mask=mask)   # 446, 465-467
    return out


def r_ccf(image, mask, q1, q2):
    """ccf_twopoint_q1_q2_mask_corrected (cross_correlation.py:29-62): (corrected ccf, valid)"""
    n = image.shape[-1]
    f, g = np.fft.rfft(image), np.fft.rfft(mask)
    d = np.fft.irfft(np.conjugate(f[q1, None, :]) * f[None, q2, :], n)
    m = np.fft.irfft(np.conjugate(g[q1, None, :]) * g[None, q2, :], n)
    valid = m != 0
    np.divide(d, m, out=d, where=valid)
    return d, valid


def r_symmetrize(ccf, phi):
    """symmetrize_ccf (cross_correlation.py:67-78) with the positions of correlate.py:262-264"""
    p2, p1, p3 = np.abs(phi - np.pi / 2).argmin(), np.abs(phi - np.pi).argmin(), np.abs(phi - 3 * np.pi / 2).argmin()
    out = ccf.copy()
    n = ccf.shape[-1]
    out[..., 0:p2] = ccf[..., p1:p1 + p2]
    out[..., p3 + 1:n] = ccf[..., p3 + 1 - p1:n - p1]
    return out


def r_correlate(images, masks, prm):
    """process_batch / run_processing_in_parallel (correlate.py:329-355, 249-259) with a pattern's own flag: sum, count, is_good, waxs"""
    q1, q2 = prm['q1'], prm['q2']
    P = len(images)
    acc = np.zeros((len(q1), len(q2), prm['n_phi']))
    cnt = np.zeros(acc.shape, dtype=int)
    good, waxs = np.zeros(P, dtype=int), np.zeros((P, prm['n_q']))
    for p in range(P):
        r = r_process_image(images[p], masks[p], prm)
        good[p], waxs[p] = r['is_good'], r['waxs']
        if r['is_good'] == 1:
            v, valid = r_ccf(r['image'], r['mask'], q1, q2)
            np.add(acc, v, out=acc, where=valid)
            np.add(cnt, 1, out=cnt, where=valid)
    return {'sum': acc, 'count': cnt, 'is_good': good, 'waxs': waxs}


def r_finalize(part, prm, symmetrize=False, fc_n=None):
    """correlate.py:249-270"""
    with np.errstate(invalid='ignore', divide='ignore'), warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        ccf = np.where(part['count'] != 0, part['sum'] / np.where(part['count'] != 0, part['count'], 1), np.nan)
        if symmetrize:
            ccf = r_symmetrize(ccf, prm['phi'])
        aver = np.mean(part['waxs'], axis=0, where=(part['is_good'][:, None] == 1))
        fc = None if fc_n is None else np.fft.fft(ccf)[..., :fc_n]
    return ccf, fc, aver


# ---- longdouble direct sums ------------------------------------------------------------------------------------------------------------
def x_circ(a, b):
    """sum_phi a[phi] b[(phi + Delta) mod n] for every Delta, in the arrays' own type (longdouble or integer)"""
    n = len(a)
    idx = (np.arange(n)[None, :] + np.arange(n)[:, None]) % n
    return (b[idx] * a[None, :]).sum(axis=1)


def x_correlate(images, masks, prm):
    """the exact-count reference: per good pattern D by longdouble direct sums, M by integer sums, sum += D / M where M > 0;
    the a-priori bound per element; the longdouble ring statistics; the input margins"""
    q1, q2, n = prm['q1'], prm['q2'], prm['n_phi']
    P = len(images)
    shape = (len(q1), len(q2), n)
    acc, cnt = np.zeros(shape, np.longdouble), np.zeros(shape, dtype=int)
    bound, min_count, holes = np.zeros(shape), np.iinfo(int).max, 0
    good, waxs, margin, roi_margin = np.zeros(P, dtype=int), np.zeros((P, prm['n_q']), np.longdouble), np.inf, np.inf
    for p in range(P):
        r = r_process_image(images[p], masks[p], prm, np.longdouble)
        good[p], waxs[p] = r['is_good'], r['waxs']
        margin = min(margin, r['margin'])
        if prm['roi_filter'] is not None and r['roi_mean'] is not None:
            roi_margin = min(roi_margin, float(min(abs(r['roi_mean'] - prm['roi_filter'][0]), abs(r['roi_mean'] - prm['roi_filter'][1]))))
        if r['is_good'] != 1:
            continue
        img, msk = r['image'], r['mask']
        norm = np.sqrt((img.astype(float) ** 2).sum(axis=1))
        ring_empty = msk.sum(axis=1) == 0
        for i, a in enumerate(q1):
            for j, b in enumerate(q2):
                m = x_circ(msk[a], msk[b])
                d = x_circ(img[a], img[b])
                ok = m > 0
                acc[i, j, ok] += d[ok] / m[ok]
                cnt[i, j, ok] += 1
                bound[i, j, ok] += 4 * EPS * np.log2(n) * norm[a] * norm[b] / m[ok]
                if not (ring_empty[a] or ring_empty[b]):
                    holes += int((~ok).sum())
                    min_count = min(min_count, int(m.min()))
    bound += P * EPS * np.abs(acc.astype(float))
    return {'sum': acc, 'count': cnt, 'bound': bound, 'is_good': good, 'waxs': waxs, 'margin': margin, 'roi_margin': roi_margin,
            'holes': holes, 'min_count': min_count}


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------------
def make_patterns(n_q, n_phi, P, seed, density=0.85, masked_pattern=None, rejected_pattern=None, masked_ring=None, dtype=np.float64,
                  outliers=True):
    """P patterns around 200 counts with a ring envelope and a few outliers (for the pixel filter), masks of the given density;
    masked_pattern: fully masked; rejected_pattern: ten times brighter (the ROI mean filter of SWITCHES rejects it);
    masked_ring = (pattern, ring): that ring fully masked.  Images are multiplied by their masks, as upstream's are at line 392."""
    rng = np.random.default_rng(seed)
    env = 200.0 * np.exp(-np.arange(n_q) / n_q)[None, :, None]
    images = env * (1.0 + 0.4 * rng.random((P, n_q, n_phi)))
    if outliers:
        images[rng.random(images.shape) < 0.04] *= 2.5
    masks = (rng.random((P, n_q, n_phi)) < density).astype(np.int64)
    if masked_pattern is not None:
        masks[masked_pattern] = 0
    if rejected_pattern is not None:
        images[rejected_pattern] *= 10.0
    if masked_ring is not None:
        masks[masked_ring[0], masked_ring[1]] = 0
    return (images * masks).astype(dtype), masks


# name -> (n_q, n_phi, sel1, sel2, P, switches, pattern options); the docstring of each boundary case names the boundary
CASES = {
    # every supported length, P = 1, 2, 5, steps 1 and 2, n_q1 != n_q2, every switch somewhere
    'n16': (4, 16, (0, 3, 1), (0, 2, 2), 5, 'all', {'masked_pattern': 1, 'rejected_pattern': 2, 'masked_ring': (3, 1)}),
    'n32': (3, 32, (0, 2, 1), (1, 2, 1), 1, 'plain', {}),
    'n64': (5, 64, (0, 4, 2), (0, 4, 1), 2, 'filter', {'dtype': np.float32}),
    'n128': (4, 128, (1, 3, 1), (0, 3, 1), 5, 'roi_filter', {'masked_pattern': 2, 'rejected_pattern': 3, 'masked_ring': (4, 0)}),
    'n256': (3, 256, (0, 2, 2), (0, 2, 1), 2, 'roi_norm', {}),
    'n512': (3, 512, (0, 2, 1), (0, 1, 1), 1, 'pol_v', {}),
    'n1024': (3, 1024, (0, 2, 1), (0, 2, 2), 2, 'all', {'masked_ring': (1, 2)}),
    'n1024_plain': (3, 1024, (0, 1, 1), (0, 2, 1), 5, 'solid', {'masked_pattern': 3}),
    # boundary: pairs per workgroup (COR_WAVES = 4): 5 pairs leave the second workgroup with one busy wave
    'pairs_per_wg': (5, 16, (0, 0, 1), (0, 4, 1), 2, 'plain', {}),
    # boundary: patterns per in-kernel chunk (COR_CHUNK = 32): 33 patterns make a second pass over the accumulators
    'chunk': (3, 16, (0, 2, 1), (0, 2, 1), CHUNK + 1, 'plain', {'masked_pattern': CHUNK - 1}),
}


def grid_stride_case(engine):
    """boundary: a second grid-stride trip over pairs -- the pair kernel's grid is capped at 8 workgroups per compute unit, 4 pairs
    each: 2 units under the emulator (64 pairs: 9 x 9 rings), 256 on the MI355X (8192 pairs: 91 x 91 rings)"""
    n_q = 9 if engine.emulated else 91
    return (n_q, 16, (0, n_q - 1, 1), (0, n_q - 1, 1), 1, 'plain', {})


@functools.lru_cache(maxsize=None)
def _reference(key):
    n_q, n_phi, sel1, sel2, P, sw, popt = key
    settings = make_settings(n_q, n_phi, sel1, sel2, **SWITCHES[sw])
    prm = params(settings)
    images, masks = make_patterns(n_q, n_phi, P, 1000 + n_phi + P, **dict(popt))
    x = x_correlate(images, masks, prm)
    r = r_correlate(images, masks, prm)
    # the conditions on the inputs
    assert x['holes'] == 0 and x['min_count'] >= 1, (x['holes'], x['min_count'])
    assert x['margin'] > 1e-12, x['margin']
    assert x['roi_margin'] > 1e-9, x['roi_margin']
    assert np.array_equal(r['count'], x['count']) and np.array_equal(r['is_good'], x['is_good'])
    for v in (images, masks, *x.values(), *r.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return settings, prm, images, masks, x, r


def reference(case):
    n_q, n_phi, sel1, sel2, P, sw, popt = case
    return _reference((n_q, n_phi, sel1, sel2, P, sw, tuple(sorted(popt.items(), key=lambda kv: kv[0]))))


def compare_partial(part, x, tag, r=None):
    """count / is_good exact, sum inside the per-element bound, waxs 1e-13 against longdouble; returns the worst ratio to the bound"""
    assert np.array_equal(part['count'], x['count']), tag
    assert np.array_equal(part['is_good'], x['is_good']), (tag, part['is_good'], x['is_good'])
    err = np.abs((part['sum'].astype(np.longdouble) - x['sum']).astype(float))
    pos = x['bound'] > 0
    assert not np.any(part['sum'][~pos]), tag                                            # nothing counted: nothing summed
    ratio = float((err[pos] / x['bound'][pos]).max()) if pos.any() else 0.0
    msg = f'{tag}: sum worst ratio to the bound {ratio:.3f}'
    if r is not None:
        er = np.abs((r['sum'].astype(np.longdouble) - x['sum']).astype(float))
        msg += f' (numpy restatement {float((er[pos] / x["bound"][pos]).max()) if pos.any() else 0.0:.3f})'
    wx = x['waxs'].astype(float)
    assert np.array_equal(np.isnan(part['waxs']), np.isnan(wx)), tag
    fin = ~np.isnan(wx)
    wd = float(np.max(np.abs((part['waxs'][fin].astype(np.longdouble) - x['waxs'][fin]).astype(float)) / np.maximum(np.abs(wx[fin]), 1e-300),
                      initial=0.0))
    print(msg + f'; waxs {wd:.2e}')
    assert ratio <= 1.0, (tag, ratio)
    assert wd <= TOL_STAT, (tag, wd)
    return ratio


def run(engine, settings, images, masks, splits=None, shared_mask=False):
    c = CR.Correlator(engine, settings, shared_mask=shared_mask)
    P = len(images)
    start = 0
    for n in (splits or [P]):
        c.add(images[start:start + n], masks if shared_mask else masks[start:start + n])
        start += n
    assert start == P and c.num_patterns == P
    return c


# ---- checks ------------------------------------------------------------------------------------------------------------------------------
def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def check_restatement_golden(g):
    """the restatement and the host tables against the reference's own functions (G25)"""
    n_q, n_phi = int(g['G25_n_q']), int(g['G25_n_phi'])
    for name, sw in SWITCHES.items():
        prm = params(make_settings(n_q, n_phi, **sw))
        for p in range(len(g['G25_images'])):
            r = r_process_image(g['G25_images'][p], g['G25_masks'][p], prm)
            tag = f'G25_{name}_p{p}_'
            assert r['is_good'] == int(g[tag + 'is_good']), tag
            assert np.allclose(r['waxs'], g[tag + 'waxs'], rtol=TOL_GOLDEN, atol=0, equal_nan=True), tag
            if tag + 'image' in g:
                assert np.allclose(r['image'], g[tag + 'image'], rtol=TOL_GOLDEN, atol=0), tag
                assert np.array_equal(r['mask'], g[tag + 'mask']), tag
            else:
                assert r['image'] is None, tag
    prm = params(make_settings(n_q, n_phi, (0, n_q - 1, 1), (0, n_q - 1, 2)))
    assert np.array_equal(prm['q1'], g['G25_q1']) and np.array_equal(prm['q2'], g['G25_q2'])
    v, valid = r_ccf(g['G25_ccf_image'], g['G25_ccf_mask'], prm['q1'], prm['q2'])
    assert np.array_equal(valid, g['G25_ccf_valid'])
    assert np.allclose(v[valid], g['G25_ccf'][valid], rtol=0, atol=TOL_GOLDEN * np.abs(g['G25_ccf'][valid]).max())
    for tag in ('even', 'awkward'):
        phi = g[f'G25_sym_{tag}_phi']
        assert np.array_equal(r_symmetrize(g['G25_ccf'], phi), g[f'G25_sym_{tag}'], equal_nan=True), tag
    assert np.allclose(np.fft.fft(g['G25_ccf']), g['G25_fcs'], rtol=0, atol=TOL_GOLDEN * np.abs(g['G25_fcs']).max())
    # geometry and correction tables
    for mode in ('exact', 'max', 'min'):
        s = dict(g25_geometry_settings(), phi_range=(0.1, 0.1 + 2 * np.pi, 64, mode))
        geo = CR.polar_geometry(s)
        for k in ('qvals', 'theta', 'phi', 'cart_x', 'cart_y'):
            assert np.allclose(geo[k], g[f'G25_geo_{mode}_{k}'], rtol=TOL_GOLDEN, atol=0), (mode, k)
        for k in ('q1vals_pos', 'q2vals_pos'):
            assert np.array_equal(geo[k], g[f'G25_geo_{mode}_{k}']), (mode, k)
        assert geo['n_phi'] == int(g[f'G25_geo_{mode}_n_phi'])
    geo = CR.polar_geometry(make_settings(n_q, n_phi))
    for kind in ('h', 'v'):
        assert np.allclose(CR.polarization_factor(geo['theta'], geo['phi'], kind), g[f'G25_pfactor_{kind}'], rtol=TOL_GOLDEN, atol=0)
    assert np.allclose(CR.solid_angle_factor(geo['theta'], n_phi), g['G25_solang'], rtol=TOL_GOLDEN, atol=0)
    assert CR.analyse_dependencies(['ccf_q1q2', 'waxs_aver']) == ['ccf_q1q2', 'waxs_aver', 'xcca', 'waxs']


def g25_geometry_settings():
    return {'qrange': [0.05, 0.1, 0.0125], 'qrange_xcca': [[0.06, 0.09, 1], [0.05, 0.1, 2]], 'pixel_size': 200.0, 'sample_distance': 620.0,
            'wavelength': 1.23984, 'detector_origin': [255.2, 255.5]}


def check_device_golden(g, lib_path=None):
    """every switch set of G25 on the device: is_good and count exact, waxs and the accumulated sum against the reference's own
    outputs (the sum of its mask-corrected ccfs over its good patterns)"""
    e = small_engine(lib_path)
    n_q, n_phi = int(g['G25_n_q']), int(g['G25_n_phi'])
    images, masks = g['G25_images'], g['G25_masks']
    for name, sw in SWITCHES.items():
        settings = make_settings(n_q, n_phi, **sw)
        prm = params(settings)
        c = run(e, settings, images, masks)
        part = c.partial()
        c.close()
        x = x_correlate(images, masks, prm)
        assert x['holes'] == 0 and x['margin'] > 1e-12 and x['roi_margin'] > 1e-9
        acc, cnt = np.zeros(part['sum'].shape), np.zeros(part['sum'].shape, int)
        for p in range(len(images)):
            tag = f'G25_{name}_p{p}_'
            assert part['is_good'][p] == int(g[tag + 'is_good']), tag
            assert np.allclose(part['waxs'][p], g[tag + 'waxs'], rtol=TOL_STAT, atol=0, equal_nan=True), tag
            if int(g[tag + 'is_good']) == 1:
                acc += np.where(g[tag + 'ccf_valid'], g[tag + 'ccf'], 0.0)
                cnt += g[tag + 'ccf_valid']
        assert np.array_equal(part['count'], cnt), name
        assert np.all(np.abs(part['sum'] - acc) <= x['bound'] + len(images) * EPS * np.abs(acc)), name
        compare_partial(part, x, 'G25 ' + name)
    e.close()


def check_case(lib_path, name):
    """one entry of CASES (or the grid-stride case) against the exact-count longdouble reference; returns the worst ratio to the bound"""
    e = small_engine(lib_path)
    case = grid_stride_case(e) if name == 'grid_stride' else CASES[name]
    settings, prm, images, masks, x, r = reference(case)
    c = run(e, settings, images, masks)
    part = c.partial()
    res = c.result()
    c.close()
    e.close()
    ratio = compare_partial(part, x, name, r)
    assert res['num_images_good'] == int(x['is_good'].sum()) and res['num_images_processed'] == len(images)
    ccf_r, _, aver_r = r_finalize(r, prm)
    assert np.array_equal(np.isnan(res['cross_correlation']['I1I1']), np.isnan(ccf_r))
    assert np.allclose(res['average_intensity'], aver_r, rtol=TOL_STAT, atol=0, equal_nan=True)
    return ratio


def check_sparse(lib_path):
    """sparse masks with truly empty (q1, q2, Delta) elements, compared with the exact integer reference only: count equals the number
    of patterns with a non-zero exact pair count, NaN where that is zero"""
    n_q, n_phi, P = 4, 32, 5
    settings = make_settings(n_q, n_phi)
    prm = params(settings)
    images, masks = make_patterns(n_q, n_phi, P, 77, density=0.12)
    x = x_correlate(images, masks, prm)
    assert x['holes'] > 0 and (x['count'] == 0).any() and (x['count'] == P).any()
    e = small_engine(lib_path)
    c = run(e, settings, images, masks)
    part, res = c.partial(), c.result()
    c.close()
    e.close()
    compare_partial(part, x, 'sparse')
    assert np.array_equal(np.isnan(res['cross_correlation']['I1I1']), x['count'] == 0)


def check_shared_mask(lib_path):
    """one shared mask against per-pattern copies of it: counts equal, sums inside the bound of both (here: bit-identical, the same
    code computes M); the shared M is computed once per handle (the launch log of the emulator)"""
    import parity_cases as PC
    n_q, n_phi, P = 4, 64, 5
    settings = make_settings(n_q, n_phi, (0, 3, 1), (0, 3, 2), roi_norm=True)
    prm = params(settings)
    images, masks = make_patterns(n_q, n_phi, P, 5, masked_ring=(0, 2))
    masks = np.broadcast_to(masks[0], masks.shape).copy()
    images = images * masks
    x = x_correlate(images, masks, prm)
    assert x['holes'] == 0
    e = small_engine(lib_path)
    a = run(e, settings, images, masks).partial()
    PC.launched_kernels(e, ('k_corr',))
    c = run(e, settings, images, masks[0], splits=[2, 3], shared_mask=True)
    log = PC.launched_kernels(e, ('k_corr',))
    b = c.partial()
    c.close()
    with_filter = CR.Correlator(e, make_settings(n_q, n_phi, filter=2.0), shared_mask=True)
    assert with_filter.shared_mask is False                                              # the filter makes masks per pattern
    with_filter.close()
    e.close()
    compare_partial(a, x, 'per-pattern copies')
    compare_partial(b, x, 'shared mask')
    assert np.array_equal(a['count'], b['count'])
    assert np.array_equal(a['sum'], b['sum'])
    if log is not None:
        assert log == ('k_corr_ring', 'k_corr_pair', 'k_corr_stats', 'k_corr_ring', 'k_corr_pair', 'k_corr_stats', 'k_corr_ring',
                       'k_corr_pair'), log


def check_batch_independence(lib_path):
    """the same 7 patterns added as 7, as 3 + 4 and as 1 x 7: bit-identical sum and count"""
    n_q, n_phi, P = 3, 32, 7
    settings = make_settings(n_q, n_phi, **SWITCHES['all'])
    images, masks = make_patterns(n_q, n_phi, P, 9, masked_pattern=2, rejected_pattern=4)
    e = small_engine(lib_path)
    parts = [run(e, settings, images, masks, splits=s).partial() for s in ([7], [3, 4], [1] * 7)]
    e.close()
    assert parts[0]['is_good'].tolist() == [1, 1, 0, 1, 0, 1, 1]
    for p in parts[1:]:
        for k in ('sum', 'count', 'is_good', 'waxs'):
            assert np.array_equal(p[k], parts[0][k], equal_nan=True), k


def check_merge(lib_path):
    """partial / merge of two handles: count and flags equal those of one handle exactly, sum agrees within the accumulation bound
    P eps (sum of |terms|)"""
    n_q, n_phi, P = 4, 32, 6
    settings = make_settings(n_q, n_phi, (0, 3, 1), (1, 3, 1), roi_filter=(80.0, 400.0))
    prm = params(settings)
    images, masks = make_patterns(n_q, n_phi, P, 21, rejected_pattern=1, masked_pattern=4)
    x = x_correlate(images, masks, prm)
    e = small_engine(lib_path)
    one = run(e, settings, images, masks).partial()
    a, b = run(e, settings, images[:2], masks[:2]), run(e, settings, images[2:], masks[2:])
    a.merge(b.partial())
    both = a.partial()
    res = a.result()
    assert a.num_patterns == P
    e.close()
    for k in ('count', 'is_good', 'waxs'):
        assert np.array_equal(both[k], one[k], equal_nan=True), k
    assert np.all(np.abs(both['sum'] - one['sum']) <= P * EPS * np.abs(one['sum'])) and res['num_images_good'] == 4   # (positive terms)
    compare_partial(both, x, 'merged')


def check_finalize(lib_path):
    """NaN placement, symmetrisation on an even and on an awkward phi offset, fc truncation, the result dict's keys"""
    n_q, n_phi, P = 3, 64, 3
    e = small_engine(lib_path)
    for phi_min, sparse in ((0.0, False), (0.37, False), (0.0, True)):
        for sym in (False, True):
            settings = make_settings(n_q, n_phi, (0, 2, 1), (0, 2, 2), phi_min=phi_min, ccf_2p_symmetrize=sym, fc_n_max=11,
                                     compute=['is_good', 'waxs_aver', 'ccf_q1q2'])
            prm = params(settings)
            images, masks = make_patterns(n_q, n_phi, P, 31, density=0.1 if sparse else 0.85)
            c = run(e, settings, images, masks)
            part, res = c.partial(), c.result()
            ccf_r, fc_r, aver_r = r_finalize(part, prm, sym, 11)                         # the restatement on the device's own partials
            ccf = res['cross_correlation']['I1I1']
            assert set(res) == {'cross_correlation', 'average_intensity', 'radial_points', 'angular_points', 'num_images_processed',
                                'num_images_good', 'xray_wavelength'}
            assert np.array_equal(np.isnan(ccf), np.isnan(ccf_r)) and np.isnan(ccf).any() == sparse
            assert np.allclose(ccf, ccf_r, rtol=4 * EPS, atol=0, equal_nan=True)
            assert np.allclose(res['average_intensity'], aver_r, rtol=TOL_STAT, atol=0, equal_nan=True)
            c2 = run(e, dict(settings, compute=['is_good', 'waxs_aver', 'xcca', 'ccf_q1q2_fc']), images, masks)
            fc = c2.result()['cross_correlation']['I1I1_fc']
            assert fc.shape == ccf.shape[:2] + (11,) and fc.dtype == np.complex128
            rows = ~np.isnan(ccf_r).any(axis=-1)
            scale = np.sqrt((ccf_r[rows] ** 2).sum(axis=-1))[:, None] if rows.any() else 1.0
            assert np.all(np.abs(fc[rows] - fc_r[rows]) <= 4 * EPS * np.log2(n_phi) * scale)
            assert np.isnan(fc[~rows]).all()                                             # a NaN poisons its row, as in numpy
            c.close()
            c2.close()
    e.close()


def check_device_tensor(lib_path):
    """torch tensors on the engine's device (float32 images, bool masks) against the numpy route: bit-identical"""
    import torch
    n_q, n_phi, P = 4, 128, 3
    settings = make_settings(n_q, n_phi, filter=2.0)
    images, masks = make_patterns(n_q, n_phi, P, 41, dtype=np.float32)
    e = small_engine(lib_path)
    a = run(e, settings, images, masks).partial()
    dev = e.torch_device()
    c = CR.Correlator(e, settings)
    c.add(torch.from_numpy(images).to(dev), torch.from_numpy(masks.astype(bool)).to(dev))
    b = c.partial()
    c.close()
    e.close()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def synthetic_patterns(n_q, L, n_phi, P, seed):
    """patterns whose expected cross-correlation is the C of a known B_l (ccextract_cases.synthetic_bl / cc_from_bl): per pattern the
    harmonics a_m(q) of I(q, phi) = sum_m a_m e^{i m phi} are Gaussian with covariance E[conj a_m(q1) a_m(q2)] = C_m(q1, q2)"""
    import ccextract_cases as CC
    qs = (np.arange(n_q) + 0.5) * 0.03125
    assert qs.max() * CC.WAVELENGTH / (4 * np.pi) <= 0.1
    bl = CC.synthetic_bl(n_q, L, seed, decay=0.3, stride=2)
    rng = np.random.default_rng(seed + 7)
    spec = np.zeros((P, n_q, n_phi // 2 + 1), complex)
    for m in range(L + 1):
        cm = np.zeros((n_q, n_q))
        for l in range(m + (m % 2), L + 1, 2):
            cm += bl[l] * CC.legendre_products(qs, l, 1)[..., m]
        w, v = np.linalg.eigh(cm)
        root = v * np.sqrt(np.clip(w, 0, None))[None, :]
        z = rng.normal(size=(P, n_q)) if m == 0 else (rng.normal(size=(P, n_q)) + 1j * rng.normal(size=(P, n_q))) / np.sqrt(2)
        spec[:, :, m] = z @ root.T
    return qs, bl, np.fft.irfft(spec * n_phi, n_phi, axis=-1)


def check_end_to_end(lib_path, n_q=32, L=8, n_phi=64, P=12):
    """patterns synthesised from a known C -> Correlator.result() -> io.load_ccd -> extract_from_cross_correlation: it runs, and its
    B_l (l = 2, 4, .. L) is the synthetic model's within the statistical error of P patterns.  That error is stated from the numpy
    restatement on the same patterns, through the numpy back-substitution: e_l = |B_l(restatement) - B_l(model)| / |B_l(model)|; the
    device has to stay within 1.05 e_l + 1e-9 (it differs from the restatement by rounding only)."""
    import ccextract_cases as CC
    qs, bl, images = synthetic_patterns(n_q, L, n_phi, P, 2025)
    settings = make_settings(n_q, n_phi, q_step=0.03125, q_min=0.015625, wavelength=CC.WAVELENGTH)
    prm = params(settings)
    assert np.array_equal(CR.polar_geometry(settings)['qvals'], qs)
    mask = np.ones((n_q, n_phi), np.int64)
    r = r_correlate(images, np.broadcast_to(mask, images.shape), prm)
    ccf_r, _, aver_r = r_finalize(r, prm)
    b_r, _ = CC.r_cc_to_deg2(ccf_r, 3, qs, prm['phi'], L, True, {}, aver_r)
    e = small_engine(lib_path)
    c = run(e, settings, images, mask, shared_mask=True)
    res = c.result()
    c.close()
    ccd = IO.load_ccd(res, 'direct')
    data = X.extract_from_cross_correlation(e, ccd, CC.flow_settings(L, CC.MASK_CASES['none'], modify_cc={}, enforce_psd=False))
    e.close()
    b_d = data['deg_2_invariant']['I1I1']
    assert res['num_images_good'] == P and len(data['data_projection_matrices']) == L + 1
    for l in range(2, L + 1, 2):
        e_r, e_d = rel_l2(b_r[l], bl[l]), rel_l2(b_d[l], bl[l])
        print(f'end to end l = {l}: statistical error of {P} patterns {e_r:.3e}, device {e_d:.3e}')
        assert e_d <= 1.05 * e_r + 1e-9, (l, e_d, e_r)
    return data


def check_raises(lib_path):
    """what is not built raises and names itself; bad inputs raise before anything is accumulated"""
    import pytest
    e = small_engine(lib_path)
    with pytest.raises(NotImplementedError, match='median_mad.*405'):
        CR.Correlator(e, dict(make_settings(3, 16), intensity_radial_pixel_filter=[True, ['median_mad', 3]]))
    for n in (8, 24, 2048):
        with pytest.raises(NotImplementedError, match='16, 32, 64, 128, 256, 512, 1024'):
            CR.Correlator(e, make_settings(3, n))
    c = CR.Correlator(e, make_settings(3, 16))
    images, masks = make_patterns(3, 16, 2, 1)
    for bad in (masks * 2, masks - 1, masks + 0.5):
        with pytest.raises(ValueError, match='0 / 1'):
            c.add(images, bad)
    with pytest.raises(ValueError, match='shape'):
        c.add(images[:, :2], masks[:, :2])
    with pytest.raises(TypeError):
        c.add(images.astype(np.int32), masks)
    assert c.num_patterns == 0 and not np.any(c.partial()['count'])
    c.close()
    with pytest.raises(MemoryError, match=r'8192 x 8192 pairs x 1024 angles needs 824\.6\d\d GB'):   # 8192^2 x 1024 x 12 B
        CR.Correlator(e, make_settings(8192, 1024, q_step=2.0 ** -13, q_min=2.0 ** -13))
    cfg = _lib.MtipCorrelateCfg(3, 48, 3, 3, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0)
    sel = np.arange(3, dtype=np.int32)
    import ctypes
    assert not e.lib.mtip_correlate_create(e.ctx, ctypes.byref(cfg), _lib.ptr(sel), _lib.ptr(sel), None)
    assert '16, 32, 64, 128, 256, 512, 1024' in e.lib.mtip_last_error(e.ctx).decode()
    e.close()

"""Cases of the median_mad radial pixel filter (csrc/k_ringfilter.h: k_corr_stats_mad; ``mtip_op_ring_median_mad``,
``correlate.ring_median_mad``, ``Correlator(..., median_mad=True)`` = mtip_correlate_cfg.filter_kind 2), shared by
tests/test_emul_ringfilter.py (CPU emulator) and tests/test_gpu_ringfilter.py (MI355X).

Yardsticks:
  * the sort-based restatement below of the rule  median = v[n / 2] (n odd), (v[n / 2 - 1] + v[n / 2]) / 2 (n even), v the sorted valid
    samples (mask != 0, not NaN), mad the same rule on |x - median|, NaN for n = 0.  A CPU test holds it to np.nanmedian and
    scipy.stats.median_abs_deviation(nan_policy='omit') -- the reference's two calls (correlate.py:471-474) -- bit for bit on every
    operator case, and to the reference's own i_median_and_mad / process_image (G29, tests/golden/correlate_median_mad.npz);
  * for a handle: a no-filter handle fed (where(W, I, 0), W) with W the restatement's filtered mask.  That route is pinned by the
    longdouble references of tests/correlate_cases.py; the comparison is bit for bit.
The statistics are elements of the data or the mean of two of them, so the device is held to the restatement with no tolerance and
no decision margin: median and mad numerically equal (the sign of a zero is free), the filtered mask exactly equal."""
import ctypes
import functools
import os
import warnings

import numpy as np
import pytest

import correlate_cases as CO
import resample_cases as RS
from correlate_cases import EPS, TOL_STAT, TOL_GOLDEN, CHUNK, make_patterns, make_settings, params, small_engine
from xframe_amd.fxs import _lib, correlate as CR

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'correlate_median_mad.npz')

# both sides of a wave (64) and of the workgroup (256), numpy's internal switch at 600, the default settings' 1536, the last register
# slot of a thread (2047, 2048 = 8 x 256)
LENGTHS = (1, 2, 3, 16, 18, 63, 64, 65, 255, 256, 257, 600, 1536, 2047, 2048)
KS = (0, 1.5, 3)
ROWS = ('full', 'valid70', 'valid10', 'empty', 'one', 'two', 'all_equal', 'most_equal', 'ties', 'signs', 'denormals', 'nan',
        'all_nan')
G29_KS = (3, 1.5)
# the other switches of correlate_cases.SWITCHES['all']
G29_SWITCHES = {'alone': {}, 'all': {k: v for k, v in CO.SWITCHES['all'].items() if k != 'filter'}}


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _middle(v):
    """the rule on a sorted 1-D array"""
    n = len(v)
    if n == 0:
        return np.nan
    return v[n // 2] if n % 2 else (v[n // 2 - 1] + v[n // 2]) / 2


def y_median_mad(images, masks):
    """(median, mad) per row of images (n_rows, n_phi) over the samples with mask != 0 that are not NaN"""
    images = np.asarray(images, dtype=np.float64)
    med, mad = np.empty(len(images)), np.empty(len(images))
    for i, (x, m) in enumerate(zip(images, np.asarray(masks) != 0)):
        v = np.sort(x[m & ~np.isnan(x)])
        med[i] = _middle(v)
        mad[i] = _middle(np.sort(np.abs(v - med[i])))
    return med, mad


def y_filter(images, masks, k):
    """(median, mad, W): W = mask & ~(|x - median| > k mad), correlate.py:412; uint8"""
    med, mad = y_median_mad(images, masks)
    with np.errstate(invalid='ignore'):
        out = np.abs(np.asarray(images, dtype=np.float64) - med[:, None]) > k * mad[:, None]
    return med, mad, ((np.asarray(masks) != 0) & ~out).astype(np.uint8)


def reference_median_mad(images, masks):
    """the reference's two calls (correlate.py:472-473)"""
    import scipy.stats as spst
    data = np.where(np.asarray(masks) == 1, images, np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)                                  # (numpy announces an all-NaN row)
        return np.nanmedian(data, axis=1), spst.median_abs_deviation(data, axis=1, nan_policy='omit')


# ---- operator cases --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_rows(n_phi):
    """the rows of ROWS at one length: (images (13, n_phi), masks (13, n_phi) uint8), read-only"""
    rng = np.random.default_rng(7000 + n_phi)
    n = len(ROWS)
    x = 200.0 * (1.0 + 0.4 * rng.random((n, n_phi)))
    x[rng.random(x.shape) < 0.04] *= 2.5
    m = np.ones((n, n_phi), np.uint8)
    r = ROWS.index
    m[r('valid70')] = rng.random(n_phi) < 0.7
    m[r('valid10')] = rng.random(n_phi) < 0.1
    m[r('empty')] = 0
    m[r('one')] = 0
    m[r('one'), rng.integers(n_phi)] = 1
    m[r('two')] = 0
    m[r('two'), rng.permutation(n_phi)[:2]] = 1
    x[r('all_equal')] = 173.25
    x[r('most_equal'), rng.permutation(n_phi)[:n_phi // 2 + 1]] = 211.5                   # mad = 0: the filter masks the rest
    x[r('ties')] = rng.poisson(3.0, n_phi)                                               # integer counts
    m[r('ties')] = rng.random(n_phi) < 0.9
    x[r('signs')] = rng.normal(size=n_phi) * rng.choice([1.0, 1e-3, 1e3], n_phi)
    x[r('signs'), rng.random(n_phi) < 0.2] = 0.0
    x[r('signs'), rng.random(n_phi) < 0.2] = -0.0
    x[r('denormals')] = rng.choice([5e-324, 3e-310, -2e-308, 1e299, -1e299, 9.9e299, 1.0], n_phi) * rng.choice([1.0, 0.5], n_phi)
    x[r('nan'), rng.permutation(n_phi)[:max(1, n_phi // 7)]] = np.nan                     # NaN where the mask is 1
    x[r('all_nan')] = np.nan                                                             # no valid sample under a mask of ones
    for a in (x, m):
        a.setflags(write=False)
    return x, m


@functools.lru_cache(maxsize=None)
def make_many_rows(n_rows=300, n_phi=65):
    rng = np.random.default_rng(7300)
    x = rng.poisson(40.0, (n_rows, n_phi)) * rng.choice([1.0, 0.25], (n_rows, 1))
    m = (rng.random((n_rows, n_phi)) < rng.random((n_rows, 1))).astype(np.uint8)
    for a in (x, m):
        a.setflags(write=False)
    return x, m


def compare_rows(got, images, masks, k, tag):
    """median and mad numerically equal to the restatement's (NaN = NaN), the filtered mask exactly"""
    med, mad, w = y_filter(images, masks, k)
    assert np.array_equal(np.asarray(got[0]), med, equal_nan=True), (tag, 'median')
    assert np.array_equal(np.asarray(got[1]), mad, equal_nan=True), (tag, 'mad')
    out = np.asarray(got[2])
    assert out.dtype == np.uint8 and np.array_equal(out, w), (tag, 'mask', np.argwhere(out != w)[:4])
    return med, mad, w


def check_operator(lib_path, n_phi):
    """the rows of ROWS at one length, every k; host buffers"""
    images, masks = make_rows(n_phi)
    e = small_engine(lib_path)
    for k in KS:
        med, mad, w = compare_rows(CR.ring_median_mad(e, images, masks, k), images, masks, k, (n_phi, k))
        r = ROWS.index
        assert np.isnan(med[r('empty')]) and np.isnan(mad[r('empty')]) and not w[r('empty')].any()
        assert mad[r('all_equal')] == 0 and mad[r('most_equal')] == 0 and np.array_equal(w[r('all_equal')], masks[r('all_equal')])
        assert w[r('most_equal')].sum() == n_phi // 2 + 1
        assert np.all(w[r('nan')][np.isnan(images[r('nan')])] == 1)                      # a NaN sample is kept by the filter
        assert np.isnan(med[r('all_nan')]) and w[r('all_nan')].all()                     # a NaN threshold keeps the mask
    # a NULL output is skipped: the mask alone, the statistics alone
    out = np.empty(images.shape, np.uint8)
    med = np.empty(len(images))
    e._ck(e.lib.mtip_op_ring_median_mad(e.ctx, len(images), n_phi, _lib.ptr(images), _lib.ptr(masks), 3.0, None, None, _lib.ptr(out)))
    e._ck(e.lib.mtip_op_ring_median_mad(e.ctx, len(images), n_phi, _lib.ptr(images), _lib.ptr(masks), 3.0, _lib.ptr(med), None, None))
    y = y_filter(images, masks, 3.0)
    assert np.array_equal(out, y[2]) and np.array_equal(med, y[0], equal_nan=True)
    e.close()


def check_many_rows(lib_path):
    """one call with 300 rows (more workgroups than compute units on the emulator, more than one per unit on the MI355X), and the
    same through tensors on the engine's device"""
    import torch
    images, masks = make_many_rows()
    e = small_engine(lib_path)
    compare_rows(CR.ring_median_mad(e, images, masks, 1.5), images, masks, 1.5, 'rows300')
    dev = e.torch_device()
    got = CR.ring_median_mad(e, torch.from_numpy(images.copy()).to(dev), torch.from_numpy(masks.copy()).to(dev), 1.5)
    assert all(t.device.type == dev.type for t in got)
    compare_rows([t.cpu().numpy() for t in got], images, masks, 1.5, 'rows300 tensors')
    e.close()


def check_restatement_numpy_scipy():
    """the restatement against np.nanmedian / scipy.stats.median_abs_deviation on every operator case, bit for bit"""
    pytest.importorskip('scipy.stats')
    for images, masks in [make_rows(n) for n in LENGTHS] + [make_many_rows()]:
        med, mad = y_median_mad(images, masks)
        med_r, mad_r = reference_median_mad(images, masks)
        assert np.array_equal(med, med_r, equal_nan=True) and np.array_equal(mad, mad_r, equal_nan=True), images.shape


# ---- handle cases ----------------------------------------------------------------------------------------------------------------------
def mad_settings(n_q, n_phi, k, *sel, **sw):
    return dict(make_settings(n_q, n_phi, *sel, **sw), intensity_radial_pixel_filter=[True, ['median_mad', k]])


def filtered(images, masks, k):
    """(where(W, I, 0), W) of patterns (P, n_q, n_phi)"""
    shape = images.shape
    w = y_filter(images.reshape(-1, shape[-1]), masks.reshape(-1, shape[-1]), k)[2].reshape(shape)
    return np.where(w != 0, images, 0.0), w


def run(engine, settings, images, masks, splits=None, **kw):
    c = CR.Correlator(engine, settings, **kw)
    start = 0
    for n in (splits or [len(images)]):
        c.add(images[start:start + n], masks[start:start + n])
        start += n
    assert start == len(images) and c.num_patterns == len(images)
    part = c.partial()
    c.close()
    return part


# name -> (n_q, n_phi, P, general_n_phi, k, switches, holes): with holes the last pattern and the last ring of pattern 0 are fully masked
EQUIVALENCE = {
    'n64': (5, 64, 5, False, 3, {'roi_filter': (80.0, 400.0), 'roi_norm': True, 'pol': 'h', 'solid': True}, True),
    'chunk16': (3, 16, CHUNK + 1, False, 1.5, {}, True),                                 # 33 patterns cross COR_CHUNK
    'n18': (4, 18, 4, True, 3, {'roi_norm': True}, True),
    'n1536': (2, 1536, 2, True, 1.5, {'roi_norm': True}, False),                         # the default settings' length
}


def check_equivalence(lib_path, name):
    """a median_mad handle fed (I, M) against a no-filter handle fed (where(W, I, 0), W): sum, count, is_good, waxs bit-identical"""
    n_q, n_phi, P, general, k, sw, holes = EQUIVALENCE[name]
    popt = {'masked_pattern': P - 1, 'masked_ring': (0, n_q - 1)} if holes else {}
    if 'roi_filter' in sw:
        popt['rejected_pattern'] = 1
    images, masks = make_patterns(n_q, n_phi, P, 2900 + n_phi, **popt)
    fi, w = filtered(images, masks, k)
    removed = int(masks.sum() - w.sum())
    assert 0 < removed < 0.5 * masks.sum(), removed                                      # the filter does something, not everything
    e = small_engine(lib_path)
    a = run(e, mad_settings(n_q, n_phi, k, **sw), images, masks, general_n_phi=general, median_mad=True)
    b = run(e, make_settings(n_q, n_phi, **sw), fi, w, general_n_phi=general)
    e.close()
    assert a['is_good'].sum() == P - holes - ('roi_filter' in sw) and a['count'].any()
    assert not holes or (a['is_good'][P - 1] == 0 and np.isnan(a['waxs'][0, n_q - 1]))
    for key in ('sum', 'count', 'is_good', 'waxs'):
        assert np.array_equal(a[key], b[key], equal_nan=True), (name, key)
    print(f'{name}: the filter removed {removed} of {int(masks.sum())} samples')


def check_settings_key(lib_path):
    """settings['GPU']['median_mad'] is the keyword's default; with a shared_mask request the filter still makes masks per pattern"""
    n_q, n_phi, P = 3, 16, 2
    images, masks = make_patterns(n_q, n_phi, P, 2950)
    e = small_engine(lib_path)
    s = mad_settings(n_q, n_phi, 3)
    c = CR.Correlator(e, dict(s, GPU={'median_mad': True}), shared_mask=True)
    assert c.median_mad and c.filter and c.shared_mask is False
    c.close()
    a = run(e, dict(s, GPU={'median_mad': True}), images, masks)
    b = run(e, s, images, masks, median_mad=True)
    e.close()
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def check_batch_independence(lib_path):
    """the same 6 patterns in one call and split 1 + 5: bit-identical partials"""
    n_q, n_phi, P = 3, 32, 6
    settings = mad_settings(n_q, n_phi, 3, roi_filter=(80.0, 400.0), roi_norm=True, pol='h', solid=True)
    images, masks = make_patterns(n_q, n_phi, P, 2909, masked_pattern=2, rejected_pattern=4)
    e = small_engine(lib_path)
    parts = [run(e, settings, images, masks, splits=s, median_mad=True) for s in ([P], [1, P - 1])]
    e.close()
    assert parts[0]['is_good'].tolist() == [1, 1, 0, 1, 0, 1]
    for key in ('sum', 'count', 'is_good', 'waxs'):
        assert np.array_equal(parts[0][key], parts[1][key], equal_nan=True), key


def check_add_detector(lib_path):
    """Correlator.add_detector with the filter is bit-identical to Resampler.run followed by add: one frame of 37 x 53 at
    interpolation order 1 onto 8 rings x 32 angles"""
    H, W, n_q, n_phi = 37, 53, 8, 32
    images, masks, _, _ = RS.make_frames(H, W, 1, 11, np.float64)
    images += 50.0
    settings = RS.detector_settings(H, W, n_q, n_phi, interpolation_order=1, intensity_radial_pixel_filter=[True, ['median_mad', 1.5]])
    e = small_engine(lib_path)
    a = CR.Correlator(e, settings, median_mad=True)
    a.add_detector(images, masks)
    rs = CR.Resampler(e, settings)
    pol_i, pol_m = rs.run(images, masks)
    rs.close()
    b = CR.Correlator(e, settings, median_mad=True)
    b.add(pol_i, pol_m)
    pa, pb = a.partial(), b.partial()
    a.close()
    b.close()
    e.close()
    w = filtered(pol_i, pol_m, 1.5)[1]
    assert 0 < pol_m.sum() - w.sum() < pol_m.sum() and pa['count'].any() and pa['is_good'].tolist() == [1]
    for key in pa:
        assert np.array_equal(pa[key], pb[key], equal_nan=True), key


def check_raises(lib_path):
    """without the opt-in the message names it; filter_kind 3 is refused by both create entries, naming 0, 1 and 2; the operator
    refuses n_phi = 0 and 2049 and n_rows = 0 with its limits"""
    e = small_engine(lib_path)
    s = mad_settings(3, 16, 3)
    for kw in ({}, {'median_mad': False}):
        with pytest.raises(NotImplementedError, match=r"median_mad.*405.*median_mad=True.*settings\['GPU'\]\['median_mad'\]"):
            CR.Correlator(e, s, **kw)
    with pytest.raises(NotImplementedError, match='median_mad.*405'):
        CR.Correlator(e, dict(s, GPU={'median_mad': False}))
    with pytest.raises(ValueError, match='unknown intensity_radial_pixel_filter'):
        CR.Correlator(e, dict(s, intensity_radial_pixel_filter=[True, ['median', 3]]), median_mad=True)
    sel = np.arange(3, dtype=np.int32)
    for kind in (3, -1):
        cfg = _lib.MtipCorrelateCfg(3, 16, 3, 3, kind, 0, 0, 0, 0, 0, 3.0, 0.0, 0.0)
        for create, extra in ((e.lib.mtip_correlate_create, ()), (e.lib.mtip_correlate_create_ex, (_lib.MTIP_CORRELATE_GENERAL_NPHI,))):
            assert not create(e.ctx, ctypes.byref(cfg), _lib.ptr(sel), _lib.ptr(sel), None, *extra)
            msg = e.lib.mtip_last_error(e.ctx).decode()
            assert f'filter_kind = {kind}' in msg and '0 (none), 1 (average_sigma) or 2 (median_mad)' in msg, msg
    x, m = np.ones((1, 2049)), np.ones((1, 2049), np.uint8)
    with pytest.raises(_lib.MtipError, match='1 <= n_phi <= 2048.*n_phi = 2049'):
        CR.ring_median_mad(e, x, m, 3)
    out = np.full(4, 7, np.uint8)
    for n_rows, n_phi in ((1, 0), (0, 4), (-1, 4)):
        rc = e.lib.mtip_op_ring_median_mad(e.ctx, n_rows, n_phi, _lib.ptr(x), _lib.ptr(m), 3.0, None, None, _lib.ptr(out))
        msg = e.lib.mtip_last_error(e.ctx).decode()
        assert rc != 0 and 'n_rows >= 1' in msg and '1 <= n_phi <= 2048' in msg and f'n_rows = {n_rows}, n_phi = {n_phi}' in msg, msg
    assert np.all(out == 7)
    e.close()


# ---- the reference itself (G29) -----------------------------------------------------------------------------------------------------------
def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def r_process_image(image, mask, k, prm):
    """process_image (correlate.py:401-452) with the median_mad filter: the restatement's filter, then correlate_cases.r_process_image
    (whose prm has no filter) on (image * W, W), which is what lines 412-413 leave"""
    w = y_filter(image, mask, k)[2].astype(np.int64)
    return CO.r_process_image(np.asarray(image, dtype=np.float64) * w, w, prm)


def g29_cases(g):
    """(tag, settings with the filter, settings without, k) of every process_image run of the fixture"""
    n_q, n_phi = int(g['G29_n_q']), int(g['G29_n_phi'])
    for k in G29_KS:
        for name, sw in G29_SWITCHES.items():
            yield f'G29_k{k}_{name}_', mad_settings(n_q, n_phi, k, **sw), make_settings(n_q, n_phi, **sw), k


def check_restatement_golden(g):
    """the restatement against the reference's own i_median_and_mad (bit for bit) and process_image"""
    med, mad = y_median_mad(g['G29_rows'], g['G29_rows_mask'])
    assert np.array_equal(med, g['G29_rows_median'], equal_nan=True) and np.array_equal(mad, g['G29_rows_mad'], equal_nan=True)
    assert np.isnan(med).sum() == 1 and (mad == 0).sum() == 1
    for tag, _, plain, k in g29_cases(g):
        prm = params(plain)
        for p in range(len(g['G29_images'])):
            r = r_process_image(g['G29_images'][p], g['G29_masks'][p], k, prm)
            t = f'{tag}p{p}_'
            assert r['is_good'] == int(g[t + 'is_good']), t
            assert np.allclose(r['waxs'], g[t + 'waxs'], rtol=TOL_GOLDEN, atol=0, equal_nan=True), t
            if t + 'image' in g:
                assert np.allclose(r['image'], g[t + 'image'], rtol=TOL_GOLDEN, atol=0), t
                assert np.array_equal(r['mask'], g[t + 'mask']), t
            else:
                assert r['image'] is None, t


def check_device_golden(g, lib_path=None):
    """every run of G29 on the device, as correlate_cases.check_device_golden holds it to G25: is_good and count exact, waxs at
    TOL_STAT, the accumulated sum against the reference's own mask-corrected ccfs within x_correlate's bound"""
    e = small_engine(lib_path)
    images, masks = g['G29_images'], g['G29_masks']
    for tag, settings, plain, k in g29_cases(g):
        prm = params(plain)
        part = run(e, settings, images, masks, median_mad=True)
        x = CO.x_correlate(*filtered(images, masks, k), prm)                             # (the filter is exact: no margin to assert)
        assert x['holes'] == 0 and x['roi_margin'] > 1e-9, tag
        acc, cnt = np.zeros(part['sum'].shape), np.zeros(part['sum'].shape, int)
        for p in range(len(images)):
            t = f'{tag}p{p}_'
            assert part['is_good'][p] == int(g[t + 'is_good']), t
            assert np.allclose(part['waxs'][p], g[t + 'waxs'], rtol=TOL_STAT, atol=0, equal_nan=True), t
            if int(g[t + 'is_good']) == 1:
                acc += np.where(g[t + 'ccf_valid'], g[t + 'ccf'], 0.0)
                cnt += g[t + 'ccf_valid']
        assert np.array_equal(part['count'], cnt), tag
        assert np.all(np.abs(part['sum'] - acc) <= x['bound'] + len(images) * EPS * np.abs(acc)), tag
        CO.compare_partial(part, x, tag)
    e.close()

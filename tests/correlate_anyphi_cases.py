"""Cases of the correlate route at the angular lengths of mtip_correlate_create_ex with MTIP_CORRELATE_ANY_NPHI
(``Correlator(..., any_n_phi=True)``: every even n_phi in 16 .. 2048; a length with a prime factor above 5 runs the chirp-z transforms
of csrc/k_correlate_bs.h), shared by tests/test_emul_correlate_anyphi.py (CPU emulator, toy sizes) and
tests/test_gpu_correlate_anyphi.py (MI355X).

Yardsticks, input conditions and tolerances are those of tests/correlate_cases.py, unchanged: count and is_good exact, sum per
element inside  4 eps log2(n_phi) sum_p |I_p(q1)|_2 |I_p(q2)|_2 / M_p + P eps |sum|  of the longdouble direct sum, waxs relative 1e-13.
np.fft takes any length, so the numpy restatement serves here as it does there; beside it stands a double-precision chirp-z
restatement (b_correlate: numpy transforms of the convolution's length Mc, the chirp with j^2 reduced mod n_phi in integers), whose
ratio to the bound is printed with the device's: on the eleven lengths below it stays at <= 0.23 (0.35 in the grid-stride case of
91 x 91 rings, a maximum over 180 000 elements), numpy's own transform at <= 0.16 (0.18), the MI355X at <= 0.19 (0.27)."""
import ctypes
import functools

import numpy as np
import pytest

import correlate_cases as CO
import correlate_nphi_cases as CN
import parity_cases as PC
import resample_cases as RS
from xframe_amd.fxs import _lib, correlate as CR
from correlate_cases import EPS, TOL_STAT, CHUNK, SWITCHES, make_patterns, make_settings, params, small_engine

# name -> (n_q, n_phi, sel1, sel2, P, switches, pattern options); m = n_phi / 2 is the length of the transform, Mc that of its convolution
CASES = {
    # m = 11, Mc = 24: a partial row of lanes, every switch
    'n22': (4, 22, (0, 3, 1), (0, 2, 2), 5, 'all', {'masked_pattern': 1, 'rejected_pattern': 2, 'masked_ring': (3, 1)}),
    # m = 13, Mc = 25 = 5 x 5: an odd convolution length
    'n26': (3, 26, (0, 2, 1), (1, 2, 1), 1, 'plain', {}),
    # m = 14, Mc = 27 = 3^3
    'n28': (3, 28, (0, 2, 1), (0, 2, 1), 2, 'roi_norm', {}),
    # m = 17, Mc = 36
    'n34': (5, 34, (0, 4, 2), (0, 4, 1), 2, 'filter', {'dtype': np.float32}),
    # m = 31, Mc = 64
    'n62': (4, 62, (1, 3, 1), (0, 3, 1), 5, 'roi_filter', {'masked_pattern': 2, 'rejected_pattern': 3, 'masked_ring': (4, 0)}),
    # m = 67, Mc = 135: more than 64 lanes, a partial second row
    'n134': (3, 134, (0, 2, 2), (0, 2, 1), 2, 'pol_v', {}),
    # m = 77 = 7 x 11, Mc = 160
    'n154': (3, 154, (0, 2, 2), (0, 2, 1), 2, 'solid', {}),
    # m = 523 (prime), Mc = 1080: no power of two
    'n1046': (3, 1046, (0, 1, 1), (0, 2, 1), 2, 'plain', {}),
    # m = 628, Mc = 1280: phi_range's 'max' mode at a ring of 200 pixels radius
    'n1256': (3, 1256, (0, 1, 1), (0, 2, 1), 2, 'all', {'masked_ring': (1, 2)}),
    # m = 1021 (prime), Mc = 2048: the largest LDS
    'n2042': (3, 2042, (0, 1, 1), (0, 1, 1), 1, 'plain', {}),
    # m = 1023 = 3 x 11 x 31, Mc = 2048
    'n2046': (3, 2046, (0, 1, 1), (0, 2, 1), 1, 'filter', {}),
    # boundary: 33 patterns make a second pass over the accumulators (COR_CHUNK = 32)
    'chunk22': (3, 22, (0, 2, 1), (0, 2, 1), CHUNK + 1, 'plain', {'masked_pattern': CHUNK - 1}),
    # boundary: 5 pairs leave the second workgroup with one busy wave (COR_WAVES = 4 at every length: the pair kernel's waves per
    # workgroup do not depend on Mc)
    'pairs22': (5, 22, (0, 0, 1), (0, 4, 1), 2, 'plain', {}),
}
TOY = ('n22', 'n26', 'n28', 'n34', 'n62', 'n134', 'n154', 'chunk22', 'pairs22')        # what the emulator file runs
MC = {22: 24, 26: 25, 28: 27, 34: 36, 62: 64, 134: 135, 154: 160, 1046: 1080, 1256: 1280, 2042: 2048, 2046: 2048}

B_KERNELS = ('k_corr_ring_b', 'k_corr_pair_b', 'k_corr_final_b')


def grid_stride_case(engine):
    """correlate_nphi_cases.grid_stride_case at n_phi = 22"""
    n_q, _, sel1, sel2, P, sw, popt = CN.grid_stride_case(engine)
    return (n_q, 22, sel1, sel2, P, sw, popt)


def run(engine, settings, images, masks, splits=None, shared_mask=False, any_n_phi=True, **kw):
    """correlate_cases.run with the flag"""
    c = CR.Correlator(engine, settings, shared_mask=shared_mask, any_n_phi=any_n_phi, **kw)
    P = len(images)
    start = 0
    for n in (splits or [P]):
        c.add(images[start:start + n], masks if shared_mask else masks[start:start + n])
        start += n
    assert start == P and c.num_patterns == P
    return c


# ---- the chirp-z restatement (double precision, numpy transforms of length Mc) -----------------------------------------------------------
def bs_length(m):
    """the smallest length >= 2 m - 1 with prime factors 2, 3, 5 only"""
    def smooth(k):
        for p in (2, 3, 5):
            while k % p == 0:
                k //= p
        return k == 1
    return next(k for k in range(2 * m - 1, 4 * m) if smooth(k))


def bs_dft(x, sign=-1):
    """sum_j x[j] exp(sign 2 pi i j k / m) along the last axis as a circular convolution of length Mc"""
    m = x.shape[-1]
    Mc = bs_length(m)
    j = np.arange(m)
    c = np.exp(sign * 1j * np.pi * ((j * j) % (2 * m)) / m)
    h = np.zeros(Mc, complex)
    h[:m] = np.conj(c)
    h[Mc - m + 1:] = np.conj(c[:0:-1])
    a = np.zeros(x.shape[:-1] + (Mc,), complex)
    a[..., :m] = x * c
    return np.fft.ifft(np.fft.fft(a) * np.fft.fft(h))[..., :m] * c


def bs_rfft(x):
    """np.fft.rfft of real rows of n = 2 m points through one m-point chirp-z transform (even samples real, odd ones imaginary)"""
    n = x.shape[-1]
    z = bs_dft(x[..., 0::2] + 1j * x[..., 1::2])
    z = np.concatenate([z, z[..., :1]], axis=-1)
    zr = np.conj(z[..., ::-1])
    return 0.5 * (z + zr) - 0.5j * np.exp(-2j * np.pi * np.arange(n // 2 + 1) / n) * (z - zr)


def bs_irfft(X, n):
    """np.fft.irfft(X, n) through one m-point chirp-z transform: the fold E + i O of the pair kernel"""
    m = n // 2
    Xr = np.conj(X[..., ::-1])
    y = 0.5 * ((X + Xr) + 1j * np.exp(2j * np.pi * np.arange(m + 1) / n) * (X - Xr))[..., :m]
    z = bs_dft(y, +1) / m
    out = np.empty(X.shape[:-1] + (n,))
    out[..., 0::2], out[..., 1::2] = z.real, z.imag
    return out


def b_correlate(images, masks, prm):
    """correlate_cases.r_correlate with the transforms above: the sum alone (the counts are the exact ones' business)"""
    q1, q2, n = prm['q1'], prm['q2'], prm['n_phi']
    acc = np.zeros((len(q1), len(q2), n))
    for p in range(len(images)):
        r = CO.r_process_image(images[p], masks[p], prm)
        if r['is_good'] == 1:
            f, g = bs_rfft(r['image']), bs_rfft(r['mask'].astype(float))
            d = bs_irfft(np.conjugate(f[q1, None, :]) * f[None, q2, :], n)
            m = bs_irfft(np.conjugate(g[q1, None, :]) * g[None, q2, :], n)
            valid = np.abs(m) >= 0.5
            acc += np.divide(d, m, out=np.zeros_like(d), where=valid)
    return acc


@functools.lru_cache(maxsize=None)
def _restatement_ratio(key):
    settings, prm, images, masks, x, r = CO.reference(key[:6] + (dict(key[6]),))
    err = np.abs((b_correlate(images, masks, prm).astype(np.longdouble) - x['sum']).astype(float))
    pos = x['bound'] > 0
    return float((err[pos] / x['bound'][pos]).max()) if pos.any() else 0.0


# ---- checks ------------------------------------------------------------------------------------------------------------------------------
def check_case(lib_path, name):
    """one entry of CASES (or the grid-stride case) against the exact-count longdouble reference; returns the worst ratio to the bound"""
    e = small_engine(lib_path)
    case = grid_stride_case(e) if name == 'grid_stride' else CASES[name]
    settings, prm, images, masks, x, r = CO.reference(case)
    if case[1] in MC:
        assert bs_length(case[1] // 2) == MC[case[1]]
    PC.launched_kernels(e, ('k_corr',))                                                  # (resets the emulator's launch log)
    c = run(e, settings, images, masks)
    part = c.partial()
    res = c.result()
    log = PC.launched_kernels(e, ('k_corr',))
    c.close()
    e.close()
    print(f'{name}: chirp-z restatement in double precision: sum worst ratio to the bound {_restatement_ratio(case[:6] + (tuple(sorted(case[6].items())),)):.3f}')
    ratio = CO.compare_partial(part, x, name, r)
    assert res['num_images_good'] == int(x['is_good'].sum()) and res['num_images_processed'] == len(images)
    ccf_r, _, aver_r = CO.r_finalize(r, prm)
    assert np.array_equal(np.isnan(res['cross_correlation']['I1I1']), np.isnan(ccf_r))
    assert np.allclose(res['average_intensity'], aver_r, rtol=TOL_STAT, atol=0, equal_nan=True)
    if log is not None:
        assert set(log) == {'k_corr_stats', *B_KERNELS}, log
    return ratio


def check_shared_mask(lib_path):
    """n_phi = 34: one shared mask against per-pattern copies of it: bit-identical counts and sums; the shared M is computed once per
    handle (the launch log of the emulator)"""
    n_q, n_phi, P = 4, 34, 5
    settings = make_settings(n_q, n_phi, (0, 3, 1), (0, 3, 2), roi_norm=True)
    prm = params(settings)
    images, masks = make_patterns(n_q, n_phi, P, 5, masked_ring=(0, 2))
    masks = np.broadcast_to(masks[0], masks.shape).copy()
    images = images * masks
    x = CO.x_correlate(images, masks, prm)
    assert x['holes'] == 0
    e = small_engine(lib_path)
    a = run(e, settings, images, masks).partial()
    PC.launched_kernels(e, ('k_corr',))
    c = run(e, settings, images, masks[0], splits=[2, 3], shared_mask=True)
    log = PC.launched_kernels(e, ('k_corr',))
    b = c.partial()
    c.close()
    e.close()
    CO.compare_partial(a, x, 'n34 per-pattern copies')
    CO.compare_partial(b, x, 'n34 shared mask')
    assert np.array_equal(a['count'], b['count'])
    assert np.array_equal(a['sum'], b['sum'])
    if log is not None:
        assert log == ('k_corr_ring_b', 'k_corr_pair_b', 'k_corr_stats', 'k_corr_ring_b', 'k_corr_pair_b', 'k_corr_stats',
                       'k_corr_ring_b', 'k_corr_pair_b'), log


def check_batch_independence(lib_path):
    """n_phi = 62: the same 7 patterns added as 7, as 3 + 4 and as 7 x 1: bit-identical sum, count, is_good and waxs"""
    n_q, n_phi, P = 3, 62, 7
    settings = make_settings(n_q, n_phi, **SWITCHES['all'])
    images, masks = make_patterns(n_q, n_phi, P, 9, masked_pattern=2, rejected_pattern=4)
    e = small_engine(lib_path)
    parts = [run(e, settings, images, masks, splits=s).partial() for s in ([7], [3, 4], [1] * 7)]
    e.close()
    assert parts[0]['is_good'].tolist() == [1, 1, 0, 1, 0, 1, 1]
    assert parts[0]['count'].max() == 5
    for p in parts[1:]:
        for k in ('sum', 'count', 'is_good', 'waxs'):
            assert np.array_equal(p[k], parts[0][k], equal_nan=True), k


def check_merge(lib_path):
    """n_phi = 22: partial / merge of two handles, as correlate_cases.check_merge"""
    n_q, n_phi, P = 4, 22, 6
    settings = make_settings(n_q, n_phi, (0, 3, 1), (1, 3, 1), roi_filter=(80.0, 400.0))
    prm = params(settings)
    images, masks = make_patterns(n_q, n_phi, P, 21, rejected_pattern=1, masked_pattern=4)
    x = CO.x_correlate(images, masks, prm)
    e = small_engine(lib_path)
    one = run(e, settings, images, masks).partial()
    a, b = run(e, settings, images[:2], masks[:2]), run(e, settings, images[2:], masks[2:])
    a.merge(b.partial())
    both = a.partial()
    res = a.result()
    assert a.num_patterns == P
    a.close()                                                                             # (handles go before their engine's context)
    b.close()
    e.close()
    for k in ('count', 'is_good', 'waxs'):
        assert np.array_equal(both[k], one[k], equal_nan=True), k
    assert np.all(np.abs(both['sum'] - one['sum']) <= P * EPS * np.abs(one['sum'])) and res['num_images_good'] == 4   # (positive terms)
    CO.compare_partial(both, x, 'n22 merged')


def check_finalize(lib_path):
    """n_phi = 22 and 134 (no multiple of 4: pi / 2 is not on the grid): NaN placement, symmetrisation at two phi offsets, fc against
    numpy's transform of the device's own ccf within the bound correlate_nphi_cases.check_finalize uses, a NaN row, and fc_n_max
    beyond n_phi, which the host clamps.  The chirp-z restatement of that transform (bs_rfft on the same rows) is printed beside the
    device: it stays inside the bound too (worst 0.52 at 22, 0.74 .. 0.83 at 134 depending on the numpy build, whose own transform of
    67 points is a chirp-z one as well; the MI355X: 0.40 and 0.74), so the bound is not widened."""
    n_q, P = 3, 3
    # sparse masks: with density d a pair count has mean n_phi d^2 -- 0.22 at (22, 0.1), 0.34 at (134, 0.05) -- so about 0.5 resp. 0.35
    # of the elements are empty in all three patterns and NaN
    sparse_density = {22: 0.1, 134: 0.05}
    e = small_engine(lib_path)
    for n_phi in (22, 134):
        for phi_min, sparse in ((0.0, False), (0.37, False), (0.0, True)):
            for sym in (False, True):
                settings = make_settings(n_q, n_phi, (0, 2, 1), (0, 2, 2), phi_min=phi_min, ccf_2p_symmetrize=sym, fc_n_max=11,
                                         compute=['is_good', 'waxs_aver', 'ccf_q1q2'])
                prm = params(settings)
                images, masks = make_patterns(n_q, n_phi, P, 31, density=sparse_density[n_phi] if sparse else 0.85)
                c = run(e, settings, images, masks)
                part, res = c.partial(), c.result()
                ccf_r, fc_r, aver_r = CO.r_finalize(part, prm, sym, 11)                  # the restatement on the device's own partials
                ccf = res['cross_correlation']['I1I1']
                assert np.array_equal(np.isnan(ccf), np.isnan(ccf_r)) and np.isnan(ccf).any() == sparse
                assert np.allclose(ccf, ccf_r, rtol=4 * EPS, atol=0, equal_nan=True)
                assert np.allclose(res['average_intensity'], aver_r, rtol=TOL_STAT, atol=0, equal_nan=True)
                c2 = run(e, dict(settings, compute=['is_good', 'waxs_aver', 'xcca', 'ccf_q1q2_fc']), images, masks)
                fc = c2.result()['cross_correlation']['I1I1_fc']
                assert fc.shape == ccf.shape[:2] + (11,) and fc.dtype == np.complex128
                rows = ~np.isnan(ccf_r).any(axis=-1)
                scale = np.sqrt((ccf_r[rows] ** 2).sum(axis=-1))[:, None] if rows.any() else 1.0
                bound = 4 * EPS * np.log2(n_phi) * scale
                worst = float(np.max(np.abs(fc[rows] - fc_r[rows]) / bound, initial=0.0))
                worst_b = float(np.max(np.abs(bs_rfft(ccf_r[rows])[..., :11] - fc_r[rows]) / bound, initial=0.0))
                print(f'finalize n_phi = {n_phi}, phi_min = {phi_min}, sparse = {sparse}, symmetrize = {sym}: fc worst ratio {worst:.3f} '
                      f'(chirp-z restatement {worst_b:.3f})')
                assert worst <= 1.0
                assert np.isnan(fc[~rows]).all()                                         # a NaN poisons its row, as in numpy
                c.close()
                c2.close()
        settings = make_settings(n_q, n_phi, fc_n_max=n_phi + 22, compute=['is_good', 'waxs_aver', 'xcca', 'ccf_q1q2_fc'])
        images, masks = make_patterns(n_q, n_phi, P, 31)
        c = run(e, settings, images, masks)
        fc = c.result()['cross_correlation']['I1I1_fc']
        ccf_r, fc_r, _ = CO.r_finalize(c.partial(), params(settings), False, n_phi)
        c.close()
        assert fc.shape == (n_q, n_q, n_phi)
        assert np.all(np.abs(fc - fc_r) <= 4 * EPS * np.log2(n_phi) * np.sqrt((ccf_r ** 2).sum(axis=-1))[..., None])
    e.close()


def check_route_unchanged(lib_path):
    """an any-flag handle at n_phi = 64 launches the radix-2 kernels and returns the bits of an unflagged handle; at n_phi = 30 it
    launches the mixed-radix kernels and returns the bits of a general-flag handle; at n_phi = 22 it launches the chirp-z kernels"""
    n_q, P = 4, 5
    e = small_engine(lib_path)
    expect = {64: ('k_corr_ring', 'k_corr_pair', 'k_corr_final'), 30: ('k_corr_ring_g', 'k_corr_pair_g', 'k_corr_final_g'), 22: B_KERNELS}
    for n_phi, other in ((64, {}), (30, {'general_n_phi': True}), (22, None)):
        settings = make_settings(n_q, n_phi, (0, 3, 1), (0, 3, 2), roi_norm=True, fc_n_max=9)
        images, masks = make_patterns(n_q, n_phi, P, 5, masked_ring=(0, 2))
        for shared in (False, True):
            out = []
            for kw in ([other, {'any_n_phi': True}, {'any_n_phi': True, 'general_n_phi': True}] if other is not None else [{'any_n_phi': True}]):
                PC.launched_kernels(e, ('k_corr',))
                c = CR.Correlator(e, settings, shared_mask=shared, **kw)
                c.add(images[:2] * masks[0] if shared else images[:2], masks[0] if shared else masks[:2])
                c.add(images[2:] * masks[0] if shared else images[2:], masks[0] if shared else masks[2:])
                ccf, fc = c.finalize(True, True)
                out.append((c.partial(), ccf, fc, PC.launched_kernels(e, ('k_corr',))))
                c.close()
            for pb, ccf_b, fc_b, log_b in out[1:]:
                for k in pb:
                    assert np.array_equal(out[0][0][k], pb[k], equal_nan=True), (n_phi, shared, k)
                assert np.array_equal(out[0][1], ccf_b, equal_nan=True) and np.array_equal(out[0][2], fc_b, equal_nan=True)
                assert out[0][3] == log_b
            ring, pair, final = expect[n_phi]
            if shared and out[0][3] is not None:
                assert out[0][3] == (ring, pair, 'k_corr_stats', ring, pair, 'k_corr_stats', ring, pair, final), out[0][3]
    e.close()


def check_max_mode(lib_path):
    """phi_range in 'max' mode, end to end: frames of 37 x 53 whose outermost ring has a radius of 33 pixels, so that a requested
    n_phi of 4096 comes out as the ring's 208 = 2^4 x 13 pixels.  Without the opt-in the Correlator raises; with it add_detector is
    bit-identical to add of Resampler.run's output and stays inside the bound of x_correlate"""
    H, W, n_q, P = 37, 53, 8, 4
    images, masks, binary, background = RS.make_frames(H, W, P, 11, np.float64)
    images += 50.0                                                                        # (keeps every ring's pair counts positive)
    settings = RS.detector_settings(H, W, n_q, 4096, phi_range=(0.0, 2 * np.pi, 4096, 'max'), interpolation_order=2,
                                    intensity_pixel_threshold=[True, 80.0, 1e4], use_binary_mask=True, subtract_background=True)
    geo = CR.polar_geometry(settings)
    n_phi = geo['n_phi']
    assert (geo['n_q'], n_phi, geo['maxpix']) == (n_q, 208, 208)
    assert CR.any_n_phi_ok(n_phi) and not CR.general_n_phi_ok(n_phi) and n_phi % 13 == 0
    e = small_engine(lib_path)
    with pytest.raises(NotImplementedError, match='n_phi = 208 is not built; supported lengths'):
        CR.Correlator(e, settings, binary_mask=binary, background=background)
    with pytest.raises(NotImplementedError, match='n_phi = 208 is not built.*2, 3 and 5.*below: 200, above: 216'):
        CR.Correlator(e, settings, binary_mask=binary, background=background, general_n_phi=True)
    a = CR.Correlator(e, dict(settings, GPU={'any_n_phi': True}), binary_mask=binary, background=background)
    a.add_detector(images[:1], masks[:1]).add_detector(images[1:], masks[1:])
    rs = CR.Resampler(e, settings, binary_mask=binary, background=background)
    pol_i, pol_m = rs.run(images, masks)
    rs.close()
    assert 0.05 < np.mean(pol_m == 0) < 0.6
    b = CR.Correlator(e, settings, any_n_phi=True)
    b.add(pol_i, pol_m)
    pa, pb = a.partial(), b.partial()
    a.close()
    b.close()
    e.close()
    assert pa['count'].any() and np.all(pa['is_good'] == 1)
    for k in pa:
        assert np.array_equal(pa[k], pb[k], equal_nan=True), k
    CO.compare_partial(pa, CO.x_correlate(pol_i, pol_m, params(settings)), 'n208 add_detector')


def check_ok():
    """any_n_phi_ok over 0 .. 2100: exactly the even lengths 16 .. 2048"""
    assert [n for n in range(0, 2101) if CR.any_n_phi_ok(n)] == list(range(16, 2049, 2))
    assert all(CR.any_n_phi_ok(n) for n in range(0, 2101) if CR.general_n_phi_ok(n) or n in CR.SUPPORTED_N_PHI)


def check_raises(lib_path):
    """refusals with the flag: odd, below 16, above 2048 (the message states the rule and the value), an unknown flag bit (the
    message names the field) -- each before anything is allocated: the handles asked for here have 8192 x 8192 pairs; flags 4 and 5
    take n_phi = 22; flags 0 and 1 refuse what they refused, in the words they used"""
    e = small_engine(lib_path)
    sel = np.arange(3, dtype=np.int32)
    big = np.arange(8192, dtype=np.int32)
    for n in (17, 14, 2050, 4096):
        for kw in ({'any_n_phi': True}, {'any_n_phi': True, 'general_n_phi': True}):
            with pytest.raises(NotImplementedError, match=f'n_phi = {n} is not built; any_n_phi takes every even length 16 .. 2048'):
                CR.Correlator(e, make_settings(3, n), **kw)
        with pytest.raises(NotImplementedError, match=f'n_phi = {n} is not built; any_n_phi'):
            CR.Correlator(e, dict(make_settings(3, n), GPU={'any_n_phi': True}))
        for flags in (4, 5):
            cfg = _lib.MtipCorrelateCfg(8192, n, 8192, 8192, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0)
            assert not e.lib.mtip_correlate_create_ex(e.ctx, ctypes.byref(cfg), _lib.ptr(big), _lib.ptr(big), None, flags)
            msg = e.lib.mtip_last_error(e.ctx).decode()
            assert f'n_phi = {n} is not built' in msg and 'MTIP_CORRELATE_ANY_NPHI: every even length 16 .. 2048' in msg, msg
            assert 'GB' not in msg, msg
    for flags in (2, 3, 8, 0x80000000):
        cfg = _lib.MtipCorrelateCfg(8192, 22, 8192, 8192, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0)
        assert not e.lib.mtip_correlate_create_ex(e.ctx, ctypes.byref(cfg), _lib.ptr(big), _lib.ptr(big), None, flags)
        msg = e.lib.mtip_last_error(e.ctx).decode()
        assert 'flags' in msg and 'MTIP_CORRELATE_GENERAL_NPHI' in msg and 'MTIP_CORRELATE_ANY_NPHI' in msg and 'GB' not in msg, msg
    for flags in (4, 5):
        cfg = _lib.MtipCorrelateCfg(3, 22, 3, 3, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0)
        h = e.lib.mtip_correlate_create_ex(e.ctx, ctypes.byref(cfg), _lib.ptr(sel), _lib.ptr(sel), None, flags)
        assert h, e.lib.mtip_last_error(e.ctx).decode()
        e.lib.mtip_correlate_destroy(h)
    # flag 1 still refuses 22 and 1534 with today's text
    for n in (22, 1534):
        below, above = CR.general_n_phi_near(n)
        cfg = _lib.MtipCorrelateCfg(8192, n, 8192, 8192, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0)
        assert not e.lib.mtip_correlate_create_ex(e.ctx, ctypes.byref(cfg), _lib.ptr(big), _lib.ptr(big), None, 1)
        assert e.lib.mtip_last_error(e.ctx).decode() == (
            f'correlate_create: n_phi = {n} is not built; with MTIP_CORRELATE_GENERAL_NPHI: even lengths 16 .. 2048 whose only prime '
            f'factors are 2, 3 and 5; the nearest below: {below}, above: {above}')
        assert not e.lib.mtip_correlate_create_ex(e.ctx, ctypes.byref(cfg), _lib.ptr(big), _lib.ptr(big), None, 0)
        assert e.lib.mtip_last_error(e.ctx).decode() == (
            f'correlate_create: n_phi = {n} is not built; supported: 16, 32, 64, 128, 256, 512, 1024')
        with pytest.raises(NotImplementedError) as info:
            CR.Correlator(e, make_settings(3, n), general_n_phi=True)
        assert str(info.value).startswith(
            f'correlate: n_phi = {n} is not built; general_n_phi takes even lengths 16 .. 2048 whose only prime factors are 2, 3 and 5; '
            f'the nearest below: {below}, above: {above}') and 'any_n_phi=True' in str(info.value)
        with pytest.raises(NotImplementedError) as info:
            CR.Correlator(e, make_settings(3, n))
        assert str(info.value).startswith(f'correlate: n_phi = {n} is not built; supported lengths: {CR.SUPPORTED_N_PHI}')
    e.close()

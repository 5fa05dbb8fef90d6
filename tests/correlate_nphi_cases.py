"""Cases of the correlate route at the angular lengths of mtip_correlate_create_ex with MTIP_CORRELATE_GENERAL_NPHI
(``Correlator(..., general_n_phi=True)``: every even n_phi in 16 .. 2048 with prime factors 2, 3, 5; csrc/k_correlate_mr.h), shared by
tests/test_emul_correlate_nphi.py (CPU emulator, toy sizes) and tests/test_gpu_correlate_nphi.py (MI355X).

Yardsticks, input conditions and tolerances are those of tests/correlate_cases.py, unchanged: count and is_good exact, sum per
element inside  4 eps log2(n_phi) sum_p |I_p(q1)|_2 |I_p(q2)|_2 / M_p + P eps |sum|  of the longdouble direct sum, waxs relative 1e-13.
np.fft takes any length, so the numpy restatement serves here as it does there."""
import ctypes

import numpy as np
import pytest

import correlate_cases as CO
import parity_cases as PC
import resample_cases as RS
from helpers import rel_l2
from xframe_amd.fxs import _lib, correlate as CR, extract as X, io as IO
from correlate_cases import EPS, TOL_STAT, CHUNK, SWITCHES, make_patterns, make_settings, params, small_engine

# name -> (n_q, n_phi, sel1, sel2, P, switches, pattern options); m = n_phi / 2 is the length of the pair kernel's transform
CASES = {
    # m = 9 = 3 x 3: an odd m, every switch
    'n18': (4, 18, (0, 3, 1), (0, 2, 2), 5, 'all', {'masked_pattern': 1, 'rejected_pattern': 2, 'masked_ring': (3, 1)}),
    # m = 10 = 2 x 5
    'n20': (3, 20, (0, 2, 1), (1, 2, 1), 1, 'plain', {}),
    # m = 12 = 4 x 3: the length the unflagged entry's test refuses
    'n24': (3, 24, (0, 2, 1), (0, 2, 1), 2, 'roi_norm', {}),
    # m = 15 = 3 x 5: no factor 2 in m
    'n30': (5, 30, (0, 4, 2), (0, 4, 1), 2, 'filter', {'dtype': np.float32}),
    # m = 25 = 5 x 5
    'n50': (4, 50, (1, 3, 1), (0, 3, 1), 5, 'roi_filter', {'masked_pattern': 2, 'rejected_pattern': 3, 'masked_ring': (4, 0)}),
    # m = 75: odd, more than 64 lanes, a partial second row
    'n150': (3, 150, (0, 2, 2), (0, 2, 1), 2, 'pol_v', {}),
    # m = 192: three full rows of lanes
    'n384': (3, 384, (0, 2, 1), (0, 1, 1), 1, 'solid', {}),
    # the default settings' length
    'n1536': (3, 1536, (0, 2, 1), (0, 2, 2), 2, 'all', {'masked_ring': (1, 2)}),
    # m = 960 = 2^6 x 3 x 5: every radix in one plan
    'n1920': (3, 1920, (0, 1, 1), (0, 2, 1), 2, 'plain', {}),
    # m = 1000 = 2^3 x 5^3: a partial 16th row
    'n2000': (3, 2000, (0, 1, 1), (0, 2, 1), 3, 'filter', {'masked_pattern': 1}),
    # a power of two beyond the radix-2 kernels' 1024: the largest dynamic LDS
    'n2048': (3, 2048, (0, 2, 1), (0, 1, 1), 1, 'plain', {}),
    # boundary: 33 patterns make a second pass over the accumulators (COR_CHUNK = 32)
    'chunk18': (3, 18, (0, 2, 1), (0, 2, 1), CHUNK + 1, 'plain', {'masked_pattern': CHUNK - 1}),
    # boundary: 5 pairs leave the second workgroup with one busy wave (COR_WAVES = 4)
    'pairs18': (5, 18, (0, 0, 1), (0, 4, 1), 2, 'plain', {}),
}
TOY = ('n18', 'n20', 'n24', 'n30', 'n50', 'n150', 'n384', 'chunk18', 'pairs18')   # what the emulator file runs (n384: 2 s there)

FLAG = _lib.MTIP_CORRELATE_GENERAL_NPHI


def grid_stride_case(engine):
    """a second grid-stride trip over pairs at n_phi = 18, with the ring counts of correlate_cases.grid_stride_case"""
    n_q = 9 if engine.emulated else 91
    return (n_q, 18, (0, n_q - 1, 1), (0, n_q - 1, 1), 1, 'plain', {})


def run(engine, settings, images, masks, splits=None, shared_mask=False, general_n_phi=True, **kw):
    """correlate_cases.run with the flag"""
    c = CR.Correlator(engine, settings, shared_mask=shared_mask, general_n_phi=general_n_phi, **kw)
    P = len(images)
    start = 0
    for n in (splits or [P]):
        c.add(images[start:start + n], masks if shared_mask else masks[start:start + n])
        start += n
    assert start == P and c.num_patterns == P
    return c


def check_case(lib_path, name):
    """one entry of CASES (or the grid-stride case) against the exact-count longdouble reference; returns the worst ratio to the bound"""
    e = small_engine(lib_path)
    case = grid_stride_case(e) if name == 'grid_stride' else CASES[name]
    settings, prm, images, masks, x, r = CO.reference(case)
    c = run(e, settings, images, masks)
    part = c.partial()
    res = c.result()
    c.close()
    e.close()
    ratio = CO.compare_partial(part, x, name, r)
    assert res['num_images_good'] == int(x['is_good'].sum()) and res['num_images_processed'] == len(images)
    ccf_r, _, aver_r = CO.r_finalize(r, prm)
    assert np.array_equal(np.isnan(res['cross_correlation']['I1I1']), np.isnan(ccf_r))
    assert np.allclose(res['average_intensity'], aver_r, rtol=TOL_STAT, atol=0, equal_nan=True)
    return ratio


def check_shared_mask(lib_path):
    """n_phi = 30: one shared mask against per-pattern copies of it: bit-identical counts and sums; the shared M is computed once per
    handle (the launch log of the emulator)"""
    n_q, n_phi, P = 4, 30, 5
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
    CO.compare_partial(a, x, 'n30 per-pattern copies')
    CO.compare_partial(b, x, 'n30 shared mask')
    assert np.array_equal(a['count'], b['count'])
    assert np.array_equal(a['sum'], b['sum'])
    if log is not None:
        assert log == ('k_corr_ring_g', 'k_corr_pair_g', 'k_corr_stats', 'k_corr_ring_g', 'k_corr_pair_g', 'k_corr_stats',
                       'k_corr_ring_g', 'k_corr_pair_g'), log


def check_batch_independence(lib_path):
    """n_phi = 50: the same 7 patterns added as 7, as 3 + 4 and as 1 x 7: bit-identical sum, count, is_good and waxs"""
    n_q, n_phi, P = 3, 50, 7
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
    """n_phi = 18: partial / merge of two handles, as correlate_cases.check_merge"""
    n_q, n_phi, P = 4, 18, 6
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
    CO.compare_partial(both, x, 'n18 merged')


def check_finalize(lib_path):
    """n_phi = 18 and 150 (no multiple of 4: pi / 2 is not on the grid): NaN placement, symmetrisation at two phi offsets, fc against
    numpy's transform of the device's own ccf, a NaN row, and fc_n_max beyond n_phi, which the host clamps"""
    n_q, P = 3, 3
    # sparse masks: with density d a pair count has mean n_phi d^2 -- 0.18 at (18, 0.1), 0.4 at (150, 0.05) -- so about 0.6 resp. 0.3 of
    # the elements are empty in all three patterns and NaN (0.1 at 150 leaves a mean of 1.5 and may leave none)
    sparse_density = {18: 0.1, 150: 0.05}
    e = small_engine(lib_path)
    for n_phi in (18, 150):
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
                worst = float(np.max(np.abs(fc[rows] - fc_r[rows]) / (4 * EPS * np.log2(n_phi) * scale), initial=0.0))
                print(f'finalize n_phi = {n_phi}, phi_min = {phi_min}, sparse = {sparse}, symmetrize = {sym}: fc worst ratio {worst:.3f}')
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


def check_add_detector(lib_path):
    """n_phi = 24: Correlator.add_detector is bit-identical to add of Resampler.run's output (frames of 37 x 53, 8 rings)"""
    H, W, n_q, n_phi, P = 37, 53, 8, 24, 4
    images, masks, binary, background = RS.make_frames(H, W, P, 11, np.float64)
    images += 50.0                                                                        # (keeps every ring's pair counts positive)
    e = small_engine(lib_path)
    settings = RS.detector_settings(H, W, n_q, n_phi, interpolation_order=2, intensity_pixel_threshold=[True, 80.0, 1e4],
                                    use_binary_mask=True, subtract_background=True)
    geo = CR.polar_geometry(settings)
    assert (geo['n_q'], geo['n_phi']) == (n_q, n_phi)
    a = CR.Correlator(e, settings, binary_mask=binary, background=background, general_n_phi=True)
    a.add_detector(images[:1], masks[:1]).add_detector(images[1:], masks[1:])
    rs = CR.Resampler(e, settings, binary_mask=binary, background=background)
    pol_i, pol_m = rs.run(images, masks)
    rs.close()
    assert 0.05 < np.mean(pol_m == 0) < 0.6
    b = CR.Correlator(e, settings, general_n_phi=True)
    b.add(pol_i, pol_m)
    pa, pb = a.partial(), b.partial()
    a.close()
    b.close()
    e.close()
    assert pa['count'].any() and np.all(pa['is_good'] == 1)
    for k in pa:
        assert np.array_equal(pa[k], pb[k], equal_nan=True), k
    CO.compare_partial(pa, CO.x_correlate(pol_i, pol_m, params(settings)), 'n24 add_detector')


def check_end_to_end(lib_path, n_q=32, L=8, n_phi=96, P=12):
    """correlate_cases.check_end_to_end at n_phi = 96 through a flagged handle, with its acceptance: per order the device's error
    against the synthetic model stays within 1.05 x the restatement's statistical error + 1e-9"""
    import ccextract_cases as CC
    qs, bl, images = CO.synthetic_patterns(n_q, L, n_phi, P, 2025)
    settings = make_settings(n_q, n_phi, q_step=0.03125, q_min=0.015625, wavelength=CC.WAVELENGTH)
    prm = params(settings)
    assert np.array_equal(CR.polar_geometry(settings)['qvals'], qs)
    mask = np.ones((n_q, n_phi), np.int64)
    r = CO.r_correlate(images, np.broadcast_to(mask, images.shape), prm)
    ccf_r, _, aver_r = CO.r_finalize(r, prm)
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
        print(f'end to end n_phi = {n_phi}, l = {l}: statistical error of {P} patterns {e_r:.3e}, device {e_d:.3e}')
        assert e_d <= 1.05 * e_r + 1e-9, (l, e_d, e_r)


def check_flag_changes_nothing(lib_path):
    """n_phi = 64: a flagged handle launches the radix-2 kernels (the names correlate_cases.check_shared_mask expects) and returns the
    bits of an unflagged one, per-pattern and shared masks alike"""
    n_q, n_phi, P = 4, 64, 5
    settings = make_settings(n_q, n_phi, (0, 3, 1), (0, 3, 2), roi_norm=True, fc_n_max=9)
    images, masks = make_patterns(n_q, n_phi, P, 5, masked_ring=(0, 2))
    e = small_engine(lib_path)
    for shared in (False, True):
        out = []
        for flagged in (False, True):
            PC.launched_kernels(e, ('k_corr',))
            c = run(e, settings, images * masks[0] if shared else images, masks[0] if shared else masks, splits=[2, 3], shared_mask=shared,
                    general_n_phi=flagged)
            ccf, fc = c.finalize(True, True)
            out.append((c.partial(), ccf, fc, PC.launched_kernels(e, ('k_corr',))))
            c.close()
        (pa, ccf_a, fc_a, log_a), (pb, ccf_b, fc_b, log_b) = out
        for k in pa:
            assert np.array_equal(pa[k], pb[k], equal_nan=True), (shared, k)
        assert np.array_equal(ccf_a, ccf_b, equal_nan=True) and np.array_equal(fc_a, fc_b, equal_nan=True)
        assert log_a == log_b
        if shared and log_b is not None:
            assert log_b == ('k_corr_ring', 'k_corr_pair', 'k_corr_stats', 'k_corr_ring', 'k_corr_pair', 'k_corr_stats', 'k_corr_ring',
                             'k_corr_pair', 'k_corr_final'), log_b
    e.close()


def check_near():
    """general_n_phi_near: the nearest accepted lengths on either side"""
    assert CR.general_n_phi_near(22) == (20, 24)
    assert CR.general_n_phi_near(1534) == (1500, 1536)
    assert CR.general_n_phi_near(17) == (16, 18)
    assert CR.general_n_phi_near(1536) == (1500, 1600)
    assert CR.general_n_phi_near(14) == (None, 16)
    assert CR.general_n_phi_near(2050) == (2048, None) and CR.general_n_phi_near(4096) == (2048, None)
    ok = [n for n in range(0, 2100) if CR.general_n_phi_ok(n)]
    assert ok[0] == 16 and ok[-1] == 2048 and all(n % 2 == 0 for n in ok) and {18, 20, 24, 30, 1536, 1920, 2000, 2048} <= set(ok)
    assert not {22, 26, 28, 34, 1534, 2046} & set(ok)


def check_raises(lib_path):
    """refusals with the flag: odd, below 16, above 2048, a prime factor above 5 (the message names general_n_phi_near's lengths), an
    unknown flag bit (the message names the field) -- each before anything is allocated: the handles asked for here would need 824 GB"""
    e = small_engine(lib_path)
    sel = np.arange(3, dtype=np.int32)
    big = np.arange(8192, dtype=np.int32)
    for n in (17, 14, 2050, 4096, 22, 1534):
        below, above = CR.general_n_phi_near(n)
        with pytest.raises(NotImplementedError, match=f'n_phi = {n} is not built.*2, 3 and 5.*below: {below}, above: {above}'):
            CR.Correlator(e, make_settings(3, n), general_n_phi=True)
        with pytest.raises(NotImplementedError, match=f'n_phi = {n} is not built'):
            CR.Correlator(e, dict(make_settings(3, n), GPU={'general_n_phi': True}))
        cfg = _lib.MtipCorrelateCfg(8192, n, 8192, 8192, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0)
        assert not e.lib.mtip_correlate_create_ex(e.ctx, ctypes.byref(cfg), _lib.ptr(big), _lib.ptr(big), None, FLAG)
        msg = e.lib.mtip_last_error(e.ctx).decode()
        assert f'n_phi = {n} is not built' in msg and '2, 3 and 5' in msg and 'GB' not in msg, msg
        assert f'below: {"none" if below is None else below}, above: {"none" if above is None else above}' in msg, msg
    for flags in (2, 3, 0x80000000):
        cfg = _lib.MtipCorrelateCfg(8192, 64, 8192, 8192, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0)
        assert not e.lib.mtip_correlate_create_ex(e.ctx, ctypes.byref(cfg), _lib.ptr(big), _lib.ptr(big), None, flags)
        msg = e.lib.mtip_last_error(e.ctx).decode()
        assert 'flags' in msg and 'MTIP_CORRELATE_GENERAL_NPHI' in msg and 'GB' not in msg, msg
    # without the flag the new entry is the old one: the same refusal, the same message
    cfg = _lib.MtipCorrelateCfg(3, 48, 3, 3, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0)
    assert not e.lib.mtip_correlate_create_ex(e.ctx, ctypes.byref(cfg), _lib.ptr(sel), _lib.ptr(sel), None, 0)
    assert '16, 32, 64, 128, 256, 512, 1024' in e.lib.mtip_last_error(e.ctx).decode()
    with pytest.raises(NotImplementedError, match='16, 32, 64, 128, 256, 512, 1024'):
        CR.Correlator(e, make_settings(3, 24), general_n_phi=False)
    e.close()


def check_default_settings(lib_path):
    """the default settings (phi_range 1536, 'exact') with n_q cut down through qrange: the handle builds and accepts a pattern"""
    e = small_engine(lib_path)
    with pytest.raises(NotImplementedError, match='n_phi = 1536 is not built'):
        CR.Correlator(e, {'qrange': [0.125, 0.3125, 0.0625]})
    c = CR.Correlator(e, {'qrange': [0.125, 0.3125, 0.0625]}, general_n_phi=True)
    assert (c.n_q, c.n_phi, c.acc_shape) == (4, 1536, (4, 4, 1536))
    rng = np.random.default_rng(3)
    image = 100.0 + rng.random((1, 4, 1536))
    c.add(image, np.ones((4, 1536), np.uint8))
    part, res = c.partial(), c.result()
    c.close()
    e.close()
    assert np.all(part['count'] == 1) and part['is_good'].tolist() == [1]
    # mask of ones: M = 1536 everywhere, sum = D / 1536.  A smoke check against numpy's double-precision transform, NOT the acceptance
    # bound: the device and numpy each stay inside the suite's bound of the exact value, so they differ by at most twice it.  The
    # acceptance at this length is case n1536, held to the longdouble direct sum at once the bound.
    d = np.fft.irfft(np.conj(np.fft.rfft(image[0]))[:, None, :] * np.fft.rfft(image[0])[None, :, :], 1536) / 1536.0
    norm = np.sqrt((image[0] ** 2).sum(axis=1))
    bound = 4 * EPS * np.log2(1536) * norm[:, None, None] * norm[None, :, None] / 1536.0 + EPS * np.abs(d)
    assert np.all(np.abs(part['sum'] - d) <= 2 * bound)
    assert res['cross_correlation']['I1I1'].shape == (4, 4, 1536) and res['num_images_good'] == 1

"""Cases of the worker `simulate_ccd`: density -> B_l -> C(q1, q2, Delta) (csrc/k_simulate.h, Engine.deg2_to_cc, fxs/simulate_ccd.py),
shared by tests/test_emul_simulate.py (CPU emulator) and tests/test_gpu_simulate.py (MI355X).

Yardsticks:
  * G28 (tests/golden/simulate_ccd.npz): outputs of the reference's own functions at 16 shells x L = 8 and 5 shells x L = 7;
  * the numpy restatements below (each cites its reference lines), held to G28 by a CPU test;
  * a direct sum in extended precision on the operator's own double-precision inputs, with an a-priori rounding bound per element.

The bound of case 3.  Every output element is a sum of terms t_i; S = sum |t_i| is
    back_substitution / dimensions 2:  S = sum_n w_n sum_{l >= n} |B_l| |T_l^n(q1)| |T_l^n(q2)| / (2l + 1)   (w_0 = w_L = 1, else 2; |cos|, |sin| <= 1)
    lstsq:                             S = sum_l |B_l| / (4 pi)                                              (|P_l| <= 1)
A sum of k terms in any order errs by at most (k - 1) u S (u = eps / 2), each term carries a few roundings of its own (the products, the
rounded twiddle or recurrence coefficient), and the two nested sums have at most L + 1 terms each: (2L + 8) u S for the harmonics route;
for lstsq the recurrence adds an error of a few l u to P_l, again O(L) u S.  A fast Fourier transform replaces one factor L by log2 n_Delta,
hence the form  BOUND_C eps (L + log2 n_Delta) S.  BOUND_C = 8 covers (2L + 8) u <= 8 eps (L + log2 2L) for every L >= 1 with a factor
of more than three to spare ((L + 4) eps against 8 (L + log2 2L) eps), and the numpy restatement (pocketfft, scipy's eval_legendre, pairwise sums) has to stay below half of it
(checked in every case; its worst ratio is printed beside the device's)."""
import os

import numpy as np

import ccextract_cases as CC
from helpers import rel_l2
from xframe_amd.fxs import _lib, extract as X, hostsetup as hs, io as IO, simulate_ccd as SIM
from xframe_amd.fxs import settings as ST

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'simulate_ccd.npz')
WAVELENGTH = CC.WAVELENGTH
TOL_OP = 1e-12                    # whole-array operator tolerance
TOL_FT = 1e-10                    # operators behind a Fourier transform
BOUND_C = 8.0
EPS = np.finfo(float).eps
GOLDEN_SIZES = ((16, 8), (5, 7))  # (shells, L) of the operator arrays in G28
FLOW = {'grid': {'max_q': False, 'oversampling': 4, 'max_order': 6, 'n_phi': 0, 'n_theta': 0, 'n_radial_points': 12},
        'shapes': {'types': ['sphere', 'sphere'], 'centers': [(30.0, 1.0, 0.5), (25.0, 2.0, 3.0)], 'sizes': [40, 30],
                   'densities': [25, 50], 'random_orientation': [False, False]},
        'n_particles': 7}         # (read and never used upstream: number_of_particles stays 1)
DISK_SHAPES = {'types': ['sphere', 'sphere'], 'centers': [(3.0, 0.7, 1.1), (2.5, 2.2, 4.0)], 'sizes': [2.0, 1.5], 'densities': [1.5, -2.0],
               'random_orientation': [False, False]}


def small_engine(lib_path=None):
    return CC.small_engine(lib_path)


def seeded_bl(nq, L, seed, kind):
    """'real': symmetric positive semi-definite, falling with l (ccextract_cases.synthetic_bl, every order); 'cplx': complex, neither
    Hermitian nor symmetric"""
    if kind == 'real':
        return CC.synthetic_bl(nq, L, seed, stride=1).astype(complex)
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(L + 1, nq, nq)) + 1j * rng.normal(size=(L + 1, nq, nq))) * np.exp(-0.1 * np.arange(L + 1))[:, None, None]


def uniform_phis(n):
    return np.arange(n) * 2 * np.pi / n


def disk_grid():
    rs, thetas, phis = (np.arange(6) + 0.5) * 0.9, (np.arange(5) + 0.5) * np.pi / 5, np.arange(8) * 2 * np.pi / 8
    return np.stack(np.meshgrid(rs, thetas, phis, indexing='ij'), axis=-1)


# ---- numpy restatements ---------------------------------------------------------------------------------------------------------------
def r_back_substitution(bl, qs):
    """deg2_invariant_to_cc_3d, mode back_substitution (fxs_invariant_tools.py:979-988): ccextract_cases.cc_from_bl over every order"""
    return CC.cc_from_bl(bl, qs, 2 * (len(bl) - 1), stride=1)


def r_lstsq(bl, qs, phis):
    """deg2_invariant_to_cc_3d, mode lstsq (963-971, 76-97, 992-1001)"""
    from scipy.special import eval_legendre
    thetas = np.arccos(qs * WAVELENGTH / (4 * np.pi))
    low = phis[phis <= np.pi]
    orders = np.arange(len(bl))
    arg = np.cos(thetas)[:, None, None] * np.cos(thetas)[None, :, None] + np.sin(thetas)[:, None, None] * np.sin(thetas)[None, :, None] \
        * np.cos(low)[None, None, :]
    leg = np.moveaxis(1 / (4 * np.pi) * eval_legendre(orders[:, None, None, None], arg[None]), 0, -1)         # q, q', phi, l
    part = np.sum(leg * np.moveaxis(bl, 0, -1)[:, :, None, :], axis=-1)
    cc = np.zeros(bl.shape[1:] + (len(phis),), dtype=complex)
    cc[..., phis <= np.pi] = part
    cc[..., phis > np.pi] = part[..., 1:-1][..., ::-1]
    return cc


def r_cc_2d(bl):
    """deg2_invariant_to_cc_2d (934-939)"""
    size = 2 * (len(bl) - 1)
    return np.fft.irfft(np.moveaxis(bl, 0, -1) * size, size)


# ---- extended-precision direct sums and their bounds -------------------------------------------------------------------------------
def _synthesis_ld(cn, L):
    """sum_n w_n (Re C_n cos(2 pi n d / N) - Im C_n sin(..)) for d = 0 .. N - 1 in long double; cn (.., L + 1) long double pairs"""
    N = 2 * L
    k = (np.arange(L + 1)[:, None] * np.arange(N)[None, :]) % N
    ang = 2 * np.arccos(np.longdouble(-1)) * k.astype(np.longdouble) / N
    w = np.full(L + 1, 2.0, np.longdouble)
    w[0] = w[L] = 1
    cs, sn = np.cos(ang) * w[:, None], np.sin(ang) * w[:, None]
    sn[0] = sn[L] = 0                                                       # numpy's irfft drops Im C_0 and Im C_L
    return cn[0] @ cs - cn[1] @ sn


def direct_harmonics(bl, table_t=None):
    """(reference values, S) of the harmonics route on the double-precision inputs bl and table_t ((L+1)(L+2)/2, nq); table_t None:
    dimensions 2 (C_n = B_n)"""
    L, nq = len(bl) - 1, bl.shape[1]
    re, im, ab = (np.zeros((nq, nq, L + 1), np.longdouble) for _ in range(3))
    if table_t is None:
        re[:], im[:], ab[:] = np.moveaxis(bl.real, 0, -1), np.moveaxis(bl.imag, 0, -1), np.moveaxis(np.abs(bl), 0, -1)
    else:
        t = table_t.astype(np.longdouble)
        for l in range(L + 1):
            for n in range(l + 1):
                row = t[l * (l + 1) // 2 + n]
                w = row[:, None] * row[None, :] / np.longdouble(2 * l + 1)
                re[..., n] += bl[l].real * w
                im[..., n] += bl[l].imag * w
                ab[..., n] += np.abs(bl[l]) * np.abs(w)
    wn = np.full(L + 1, 2.0)
    wn[0] = wn[L] = 1
    return _synthesis_ld((re, im), L), (ab * wn).sum(-1).astype(float)


def direct_lstsq(bl, cst, cos_delta):
    """(reference values on the samples <= pi, S): x rounded as numpy rounds it (an input of the sum), P_l by the recurrence in long double"""
    L = len(bl) - 1
    x = (cst[0][:, None, None] * cst[0][None, :, None] + cst[1][:, None, None] * cst[1][None, :, None] * cos_delta[None, None, :])
    x = x.astype(np.longdouble)
    p0, p1 = np.ones_like(x), x.copy()
    re = bl[0].real[..., None] * p0 + bl[1].real[..., None] * p1
    im = bl[0].imag[..., None] * p0 + bl[1].imag[..., None] * p1
    for l in range(1, L):
        p0, p1 = p1, ((2 * l + 1) * x * p1 - l * p0) / np.longdouble(l + 1)
        re = re + bl[l + 1].real[..., None] * p1
        im = im + bl[l + 1].imag[..., None] * p1
    four_pi = 4 * np.arccos(np.longdouble(-1))
    return re / four_pi, im / four_pi, np.abs(bl).sum(0) / (4 * np.pi)


def _mirror(part, n_delta):
    out = np.zeros(part.shape[:-1] + (n_delta,), part.dtype)
    nh = part.shape[-1]
    out[..., :nh] = part
    out[..., nh:] = part[..., 1:-1][..., ::-1]
    return out


def _ratios(name, dev, rest, ref_re, ref_im, S, L, n_delta):
    """worst |value - reference| / bound over EVERY element, for the device and for the numpy restatement"""
    bound = BOUND_C * EPS * (L + np.log2(n_delta)) * S[..., None]
    assert (bound > 0).all()

    def worst(v):
        v = np.asarray(v)
        err = np.abs(v.real.astype(np.longdouble) - ref_re)
        if ref_im is not None:
            err = np.maximum(err, np.abs(v.imag.astype(np.longdouble) - ref_im))
        return float((err / bound).max())
    assert dev.shape == rest.shape == ref_re.shape, (dev.shape, rest.shape, ref_re.shape)
    rd, rr = worst(dev), worst(rest)
    print(f'{name}: worst |error| / bound  device {rd:.3f}  numpy restatement {rr:.3f}')
    assert rr <= 0.5, (name, 'the restatement itself is above half the bound', rr)
    assert np.isfinite(np.asarray(dev)).all() and rd <= 1.0, (name, rd)
    return rd, rr


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def load_golden():
    return np.load(GOLDEN)


def golden_operator_arrays(g):
    """(name, function of (engine or None) -> array, reference array): every operator array of G28; engine None: the restatement"""
    out = []
    for nq, L in GOLDEN_SIZES:
        qs = g[f'G28_qs_{nq}']
        phis = g[f'G28_phis_{nq}']
        grid = {'qs': qs, 'phis': phis}
        for kind in ('real', 'cplx'):
            bl = g[f'G28_bl_{kind}_{nq}']
            assert np.array_equal(bl, seeded_bl(nq, L, 2800 + nq, kind))
            out.append((f'back_substitution {kind} {nq} x L{L}', g[f'G28_cc_bs_{kind}_{nq}'],
                        lambda e, bl=bl, qs=qs, grid=grid: r_back_substitution(bl, qs) if e is None else
                        SIM.deg2_invariant_to_cc(e, bl, WAVELENGTH, grid, mode='back_substitution')))
            out.append((f'lstsq {kind} {nq} x L{L}', g[f'G28_cc_ls_{kind}_{nq}'],
                        lambda e, bl=bl, qs=qs, phis=phis, grid=grid: r_lstsq(bl, qs, phis) if e is None else
                        SIM.deg2_invariant_to_cc(e, bl, WAVELENGTH, grid, orders=np.arange(len(bl)), mode='lstsq')))
            out.append((f'2d {kind} {nq} x M{L}', g[f'G28_cc_2d_{kind}_{nq}'],
                        lambda e, bl=bl: r_cc_2d(bl) if e is None else SIM.deg2_invariant_to_cc_2d(e, bl)))
    return out


def check_restatement_golden(g):
    """case 1: the numpy restatements and the host-side tables against the reference's own outputs, <= 1e-15"""
    for name, ref, fn in golden_operator_arrays(g):
        got = fn(None)
        d = rel_l2(got, ref)
        print(f'restatement vs G28 {name}: {d:.2e}')
        assert got.shape == ref.shape and got.dtype == ref.dtype, (name, got.shape, got.dtype, ref.dtype)
        assert d <= 1e-15, (name, d)
    # the Legendre table: products of its rows are the reference's qq_matrix of the highest order (60-74)
    for nq, L in GOLDEN_SIZES:
        t = SIM.legendre_table_t(g[f'G28_qs_{nq}'], WAVELENGTH, L)
        rows = t[L * (L + 1) // 2:]
        qq = np.moveaxis(rows[:, None, :] * rows[:, :, None] / (2 * L + 1), 0, -1)
        d = rel_l2(qq, g[f'G28_qq_matrix_{nq}'])
        print(f'Legendre products vs G28 {nq} x L{L}: {d:.2e}')
        assert d <= 1e-15, d
    # shapes: two off-centre spheres (mathLibrary.py:137-167)
    dens = SIM.shape_density(disk_grid(), DISK_SHAPES)
    assert np.array_equal(dens, g['G28_disk_density']) and 0 < np.count_nonzero(dens) < dens.size
    # the grid of the flow (simulate_ccd.py:109-123) and its density
    opt = ST.resolve_simulate_ccd(FLOW)
    max_q, n, max_r = SIM.simulation_grid(opt)
    kappa = ST.reciprocity_coefficient(opt['fourier_transform'])
    rs, qs = hs.radial_grids(max_q, n, kappa, 'midpoint')
    assert np.abs(rs - g['G28_flow_rs']).max() <= 1e-15 * max_r and np.abs(qs - g['G28_flow_qs']).max() <= 1e-15 * max_q
    grid = g['G28_flow_grid']
    assert np.array_equal(SIM.shape_density(grid, opt['shapes']), g['G28_flow_density'])
    # the default settings are the reference's file
    d = ST.simulate_ccd_default_settings()
    assert d['grid'] == {'max_q': False, 'oversampling': 8, 'max_order': 63, 'n_phi': 0, 'n_theta': 0, 'n_radial_points': 256}
    assert d['cross_correlation'] == {'method': 'back_substitution', 'xray_wavelength': 1.23984} and d['n_particles'] == 1
    assert len(d['shapes']['centers']) == 6 and d['shapes']['densities'] == [25, 50, 25, 50, 25, 50]


def check_operator_golden(g, lib_path=None):
    """case 2: every operator array of G28 through the device, whole-array rel-L2 <= 1e-12; complex B_l: the dropped imaginary parts of
    C_0 and C_L (the real output of back_substitution) and the complex output of lstsq"""
    e = small_engine(lib_path)
    for name, ref, fn in golden_operator_arrays(g):
        got = np.asarray(fn(e))
        d = rel_l2(got, ref)
        print(f'operator vs G28 {name}: {d:.2e}')
        assert got.shape == ref.shape and got.dtype == ref.dtype, (name, got.shape, got.dtype, ref.dtype)
        assert d <= TOL_OP, (name, d)
    e.close()


HARMONIC_SHAPES = ((3, 1), (5, 7), (67, 8), (67, 7), (5, 63), (3, 128))                   # (n_q, L); 67 = one q2 tile of 64 and a tail
LSTSQ_SHAPES = ((3, 1, 16), (5, 7, 70), (67, 8, 258), (5, 63, 258), (3, 128, 70), (5, 8, 16))   # (n_q, L, n_delta)


def check_bound_harmonics(lib_path, nq, L, dimensions):
    """case 3, back_substitution (dimensions 3) and the 2-D inverse transform: every element within the bound of the module docstring"""
    bl = seeded_bl(nq, L, 31 * nq + L, 'cplx')
    qs = CC.radial_points(nq)
    table = SIM.legendre_table_t(qs, WAVELENGTH, L) if dimensions == 3 else None
    ref, S = direct_harmonics(bl, table)
    e = small_engine(lib_path)
    out = np.full((nq, nq, 2 * L), np.nan)
    blc, tc = _lib.as_c128(bl), None if table is None else _lib.as_f64(table)
    rc = e.lib.mtip_op_deg2_to_cc(e.ctx, nq, L, 2 * L, dimensions, 0, _lib.ptr(blc), _lib.ptr(tc), None, None, _lib.ptr(out))
    assert rc == 0, e.lib.mtip_last_error(e.ctx).decode()
    e.close()
    rest = r_back_substitution(bl, qs) if dimensions == 3 else r_cc_2d(bl)
    return _ratios(f'harmonics dim {dimensions} {nq} x L{L}', out, rest, ref, None, S, L, 2 * L)


def check_bound_lstsq(lib_path, nq, L, n_delta):
    """case 3, lstsq: every element (both halves of the mirror) within the bound"""
    bl = seeded_bl(nq, L, 37 * nq + L, 'cplx')
    qs, phis = CC.radial_points(nq), uniform_phis(n_delta)
    thetas = np.arccos(qs * WAVELENGTH / (4 * np.pi))
    nh = n_delta // 2 + 1
    assert (phis <= np.pi).sum() == nh
    cst, cd = np.stack([np.cos(thetas), np.sin(thetas)]), np.cos(phis[:nh])
    re, im, S = direct_lstsq(bl, cst, cd)
    e = small_engine(lib_path)
    out = SIM.deg2_invariant_to_cc(e, bl, WAVELENGTH, {'qs': qs, 'phis': phis}, mode='lstsq')
    e.close()
    return _ratios(f'lstsq {nq} x L{L} x {n_delta}', out, r_lstsq(bl, qs, phis), _mirror(re, n_delta), _mirror(im, n_delta), S, L, n_delta)


def _round_trip_errors(e, bl, qs, zero_odd, on_device=False):
    """(device error, host error) of B -> C -> B against B, whole-array rel-L2"""
    L = len(bl) - 1
    phis = uniform_phis(2 * L)
    meta = CC.metadata(qs, phis, L, zero_odd, {}, None)
    src = bl
    if on_device:
        import torch
        src = torch.from_numpy(_lib.as_c128(bl)).to(f'cuda:{e.device_index}')
    cc = SIM.deg2_invariant_to_cc(e, src, WAVELENGTH, meta['data_grid'])
    back, _ = X.cross_correlation_to_deg2_invariant(e, cc, 3, **meta)
    host, _ = CC.r_cc_to_deg2(r_back_substitution(bl, qs), 3, qs, phis, L, zero_odd, {}, None)
    return rel_l2(back, bl), rel_l2(host, bl)


def check_round_trip(lib_path, stride, on_device=False):
    """case 4: cross_correlation_to_deg2_invariant(deg2_invariant_to_cc(B)) against B at 16 x L8; the yardstick is the same round trip
    through the numpy restatements: the device may err 4 x as much (another summation order) plus 1e-15"""
    nq, L = 16, 8
    bl = CC.synthetic_bl(nq, L, 44, stride=stride).astype(complex)
    e = small_engine(lib_path)
    dev, host = _round_trip_errors(e, bl, CC.radial_points(nq), stride == 2, on_device)
    e.close()
    print(f'round trip 16 x L8 stride {stride}: device {dev:.2e}, numpy restatements {host:.2e}, ratio {dev / max(host, 1e-300):.2f}')
    assert dev <= 4 * host + 1e-15, (dev, host)
    return dev, host


def check_flow(g, lib_path=None):
    """case 5: simulate_ccd with two spheres at 12 x L6 against the flow arrays of G28 (B_l, cc <= 1e-10; scalars <= 1e-12); its cc_data
    through io.load_ccd and extract_from_cross_correlation gives back the B_l it was made from within the bound of case 4"""
    res = SIM.simulate_ccd(FLOW, lib_path=lib_path)
    cc_data = res.cc_data
    assert set(cc_data) == {'radial_points', 'angular_points', 'xray_wavelength', 'cross_correlation', 'average_intensity',
                            'deg_2_invariant', 'number_of_particles'}
    assert cc_data['number_of_particles'] == 1 and int(g['G28_flow_number_of_particles']) == 1            # n_particles = 7 is never used
    assert cc_data['xray_wavelength'] == float(g['G28_flow_wavelength'])
    assert np.array_equal(res.density, g['G28_flow_density']) and np.array_equal(res.grid, g['G28_flow_grid'])
    bl, cc = cc_data['deg_2_invariant']['I1I1'], cc_data['cross_correlation']['I1I1']
    L = 6
    for name, got, ref, tol in (('B_l', bl, g['G28_flow_bl'], TOL_FT), ('cc', cc, g['G28_flow_cc'], TOL_FT),
                                ('average_intensity', cc_data['average_intensity'], g['G28_flow_average_intensity'], TOL_FT),
                                ('radial_points', cc_data['radial_points'], g['G28_flow_qs'], 1e-15),
                                ('angular_points', cc_data['angular_points'], g['G28_flow_angular_points'], 0.0)):
        d = rel_l2(got, ref)
        print(f'flow {name}: {d:.2e}')
        assert np.shape(got) == ref.shape and d <= tol, (name, d)
    d = abs(res.integrated_intensity / float(g['G28_flow_integrated_intensity']) - 1)
    print(f'flow integrated_intensity: {d:.2e}')
    assert d <= 1e-12, d
    # the chain: load_ccd and extract take the dict as it is
    e = small_engine(lib_path)
    ccd = IO.load_ccd(cc_data, 'direct')
    data = X.extract_from_cross_correlation(e, ccd, CC.flow_settings(L, CC.MASK_CASES['none'], modify_cc={}, enforce_psd=False))
    back = data['b_coeff']['I1I1']
    qs, phis = cc_data['radial_points'], cc_data['angular_points']
    host, _ = CC.r_cc_to_deg2(CC.cc_from_bl(bl, qs, 2 * L, stride=1), 3, qs, phis, L, True, {}, None)
    e.close()
    dev_err, host_err = rel_l2(back, bl), rel_l2(host, bl)
    print(f'flow round trip through extract: device {dev_err:.2e}, numpy restatements {host_err:.2e}')
    assert dev_err <= 4 * host_err + 1e-15, (dev_err, host_err)
    for k in CC.RECONSTRUCT_KEYS:
        assert k in data, k


def check_raises(g, lib_path=None):
    """case 6: what is not built raises, sizes beyond the limits come back as an error code with a message and untouched outputs"""
    import pytest
    e = small_engine(lib_path)
    nq, L = GOLDEN_SIZES[1]
    bl, qs, phis = g[f'G28_bl_cplx_{nq}'], g[f'G28_qs_{nq}'], g[f'G28_phis_{nq}']
    grid = {'qs': qs, 'phis': phis}
    with pytest.raises(NotImplementedError, match=r'legendre.*1028-1031'):
        SIM.deg2_invariant_to_cc(e, bl, WAVELENGTH, grid, mode='legendre')
    with pytest.raises(ValueError, match='is unknown. Known modes are'):
        SIM.deg2_invariant_to_cc(e, bl, WAVELENGTH, grid, mode='Pl')
    for bad in (uniform_phis(2 * L + 1), uniform_phis(2 * L) + 0.01, np.linspace(0, 2 * np.pi, 2 * L)):   # grids without pi
        with pytest.raises(ValueError, match='mirror'):
            SIM.deg2_invariant_to_cc(e, bl, WAVELENGTH, {'qs': qs, 'phis': bad}, mode='lstsq')
    for fn in (lambda: SIM.deg2_invariant_to_cc(e, bl[:1], WAVELENGTH, grid), lambda: SIM.deg2_invariant_to_cc_2d(e, bl[:1]),
               lambda: SIM.deg2_invariant_to_cc(e, bl[:1], WAVELENGTH, grid, mode='lstsq')):
        with pytest.raises(ValueError, match='max_order = 0'):
            fn()
    with pytest.raises(NotImplementedError, match='orders'):
        SIM.deg2_invariant_to_cc(e, bl, WAVELENGTH, grid, orders=np.arange(0, L + 1, 2))
    # the entry point's limits: an error code and a message, never values
    out = np.full(64, np.nan, complex)
    small = _lib.as_c128(np.zeros((3, 2, 2)))
    tab = _lib.as_f64(np.zeros((6, 2)))
    args = lambda *a: e.lib.mtip_op_deg2_to_cc(e.ctx, *a, _lib.ptr(small), _lib.ptr(tab), _lib.ptr(tab), _lib.ptr(tab), _lib.ptr(out))
    for a, word in (((5000, 2, 4, 3, 0), 'n_q <= 4096'), ((2, 129, 258, 3, 0), 'max_order <= 128'), ((2, 0, 2, 3, 0), '1 <= max_order'),
                    ((2, 2, 5000, 3, 1), 'n_delta <= 4096'), ((2, 2, 6, 3, 0), '2 max_order'), ((2, 2, 6, 2, 0), '2 max_order'),
                    ((2, 2, 7, 3, 1), 'even n_delta'), ((2, 2, 4, 4, 0), 'dimensions'), ((2, 2, 4, 3, 2), 'mode'),
                    ((2, 2, 4, 2, 1), 'mode')):
        rc = args(*a)
        msg = e.lib.mtip_last_error(e.ctx).decode()
        assert rc == -1 and 'deg2_to_cc' in msg and word in msg, (a, rc, msg)
        assert np.isnan(out).all()
    rc = e.lib.mtip_op_deg2_to_cc(e.ctx, 2, 2, 4, 3, 0, _lib.ptr(small), None, None, None, _lib.ptr(out))
    assert rc == -1 and 'legendre_t' in e.lib.mtip_last_error(e.ctx).decode() and np.isnan(out).all()
    with pytest.raises(_lib.MtipError, match='max_order <= 128'):
        e.deg2_to_cc(np.zeros((130, 2, 2), complex), 'back_substitution', 2)
    # an output that does not fit the device: MTIP_ENOMEM and its size before anything is allocated or touched (4096^2 pairs x 4096
    # angles x 16 B = 1099.5 GB of complex128, more than any device holds)
    rc = args(4096, 2, 4096, 3, 1)
    msg = e.lib.mtip_last_error(e.ctx).decode()
    assert rc == -4 and np.isnan(out).all(), (rc, msg)
    with pytest.raises(MemoryError, match=r'4096 x 4096 pairs x 4096 angles needs 1099\.5\d\d GB \(complex128\)'):
        e._ck_memory(rc)
    e.close()
    # the worker
    opt = dict(FLOW)
    for key, val, word in (('types', ['sphere', 'cube'], 'cube'), ('types', ['tetrahedron', 'sphere'], 'tetrahedron'),
                           ('random_orientation', [False, True], 'random_orientation')):
        with pytest.raises(NotImplementedError, match=word):
            SIM.simulate_ccd({**opt, 'shapes': {**FLOW['shapes'], key: val}}, lib_path=lib_path)
        with pytest.raises(NotImplementedError, match=word):
            SIM.shape_density(disk_grid(), {**DISK_SHAPES, key: val})
    with pytest.raises(NotImplementedError, match='dimensions = 2'):
        SIM.simulate_ccd({**opt, 'dimensions': 2}, lib_path=lib_path)
    with pytest.raises(NotImplementedError, match='legendre'):
        SIM.simulate_ccd({**opt, 'cross_correlation': {'method': 'legendre'}}, lib_path=lib_path)


def check_overwrite_and_launches(lib_path):
    """emulator: an output pre-filled with NaN comes back fully overwritten, and one call launches one kernel"""
    import parity_cases as PC
    e = small_engine(lib_path)
    for nq, L in ((5, 3), (66, 4)):
        bl = _lib.as_c128(seeded_bl(nq, L, 5, 'cplx'))
        qs = CC.radial_points(nq)
        tab = _lib.as_f64(SIM.legendre_table_t(qs, WAVELENGTH, L))
        out = np.full((nq, nq, 2 * L), np.nan)
        PC.launched_kernels(e, ('k_',))
        rc = e.lib.mtip_op_deg2_to_cc(e.ctx, nq, L, 2 * L, 3, 0, _lib.ptr(bl), _lib.ptr(tab), None, None, _lib.ptr(out))
        assert rc == 0 and PC.launched_kernels(e, ('k_',)) == ('k_sim_harmonics_cc',)
        assert np.isfinite(out).all() and rel_l2(out, r_back_substitution(bl, qs)) <= TOL_OP
        n_delta = 2 * L + 2
        out = np.full((nq, nq, n_delta), np.nan, complex)
        th = np.arccos(qs * WAVELENGTH / (4 * np.pi))
        cst, cd = _lib.as_f64(np.stack([np.cos(th), np.sin(th)])), _lib.as_f64(np.cos(uniform_phis(n_delta)[:n_delta // 2 + 1]))
        rc = e.lib.mtip_op_deg2_to_cc(e.ctx, nq, L, n_delta, 3, 1, _lib.ptr(bl), None, _lib.ptr(cst), _lib.ptr(cd), _lib.ptr(out))
        assert rc == 0 and PC.launched_kernels(e, ('k_',)) == ('k_sim_legendre_cc',)
        assert np.isfinite(out).all() and rel_l2(out, r_lstsq(bl, qs, uniform_phis(n_delta))) <= TOL_OP
    e.close()

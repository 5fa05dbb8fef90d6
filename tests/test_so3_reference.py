"""The host code the SO(3) kernels and their oracle share (hostsetup.wigner_d / wigner_d_table / wigner_D_flat,
oracle/alignment.py wigner_d / rotate_coeff / correlation / mean_C_layout) against references that share no code with either
(tests/so3_reference.py): the explicit Wigner sum at 80 digits, rotated functions evaluated with scipy's spherical harmonics, and
the correlation from its definition.  No GPU, no emulator.  These pin the conventions to the published definitions the reference's
pysofft plugin quotes; whether pysofft's own conventions equal them needs pysofft."""
import numpy as np
import pytest

import so3_reference as SR
from oracle import alignment as OA
from xframe_amd.fxs import hostsetup as hs

TOL_WIGNER = 1e-13          # absolute, entries are <= 1: a tenth of the 1e-12 the operators this table feeds are held to
TOL_ROT = 1e-12             # of max|f|


def _betas(l):
    return hs.euler_grid(l + 1)[1]


def _check_entries(l, betas, entries):
    """entries: iterable of (beta index, m, n)"""
    d_hs, d_oa = hs.wigner_d(l, betas), OA.wigner_d(l, betas)
    worst = 0.0
    for b, m, n in entries:
        ex = SR.wigner_d_exact(l, m, n, betas[b])
        worst = max(worst, abs(d_hs[b, m + l, n + l] - ex), abs(d_oa[b, m + l, n + l] - ex))
    return worst


def test_wigner_exact_known_values():
    """the explicit sum itself at closed forms: d^1_10 = -sin(b) / sqrt 2, d^1_11 = (1 + cos b) / 2, d^2_00 = (3 cos^2 b - 1) / 2,
    d^l_mn(0) = delta_mn, d^l_mn(pi) = (-1)^(l-n) delta_m,-n"""
    b = 0.7
    assert abs(SR.wigner_d_exact(1, 1, 0, b) + np.sin(b) / np.sqrt(2)) < 1e-16
    assert abs(SR.wigner_d_exact(1, 1, 1, b) - (1 + np.cos(b)) / 2) < 2e-16
    assert abs(SR.wigner_d_exact(2, 0, 0, b) - (3 * np.cos(b) ** 2 - 1) / 2) < 2e-16
    for l in (1, 4):
        for m in range(-l, l + 1):
            for n in range(-l, l + 1):
                assert SR.wigner_d_exact(l, m, n, 0.0) == float(m == n)
                assert abs(SR.wigner_d_exact(l, m, n, np.pi) - (-1) ** (l - n) * float(m == -n)) < 1e-14 * (l + 1)


@pytest.mark.parametrize('l', range(7))
def test_wigner_d_every_entry_small_l(l):
    betas = hs.euler_grid(7)[1]
    worst = _check_entries(l, betas, [(b, m, n) for b in range(len(betas)) for m in range(-l, l + 1) for n in range(-l, l + 1)])
    print('l = %d: worst |d - exact| = %.2e' % (l, worst))
    assert worst <= TOL_WIGNER


@pytest.mark.parametrize('l', [16, 32, 48, 63])
def test_wigner_d_sampled_large_l(l):
    """>= 200 fixed-seed entries at the betas of bw = l + 1 and at 0, pi, 1e-8, always with the corners (m, n = +-l), the centre
    and the first and last beta"""
    betas = np.concatenate([_betas(l), [0.0, np.pi, 1e-8]])
    nbeta = len(betas)
    rng = np.random.default_rng(1000 + l)
    entries = {(b, m, n) for b in (0, nbeta - 4, nbeta - 3, nbeta - 2, nbeta - 1) for m, n in ((l, l), (l, -l), (-l, l), (-l, -l), (0, 0))}
    while len(entries) < 230:
        entries.add((int(rng.integers(nbeta)), int(rng.integers(-l, l + 1)), int(rng.integers(-l, l + 1))))
    worst = _check_entries(l, betas, sorted(entries))
    print('l = %d: worst |d - exact| over %d entries = %.2e' % (l, len(entries), worst))
    assert worst <= TOL_WIGNER


def test_wigner_sign_flip_is_seen():
    """the check can fail: the transposed matrix (m and n swapped, i.e. beta -> -beta) misses the exact sum by O(1)"""
    l, betas = 3, _betas(3)
    d = hs.wigner_d(l, betas).transpose(0, 2, 1)
    assert abs(d[2, 1 + l, 0 + l] - SR.wigner_d_exact(l, 1, 0, betas[2])) > 0.1


@pytest.mark.parametrize('L', [0, 1, 6, 10])
def test_wigner_table_layout(L):
    """wigner_d_table: slice l of row b is d^l(beta_b) row-major, at offset l (4 l^2 - 1) / 3 -- exactly; wigner_D_flat likewise"""
    tab = hs.wigner_d_table(L)
    be = OA.euler_grid(L + 1)[1]
    assert tab.shape == (2 * (L + 1), (L + 1) * (2 * L + 1) * (2 * L + 3) // 3)
    euler = (0.3, be[min(1, len(be) - 1)], 5.1)
    flat = hs.wigner_D_flat(L, euler)
    assert flat.shape == (tab.shape[1],)
    for l in range(L + 1):
        off = l * (4 * l * l - 1) // 3
        assert np.array_equal(tab[:, off:off + (2 * l + 1) ** 2], OA.wigner_d(l, be).reshape(len(be), -1)), l
        D = SR.wigner_D_ref(l, euler)
        assert np.abs(flat[off:off + (2 * l + 1) ** 2].reshape(2 * l + 1, 2 * l + 1) - D).max() < 1e-13, l
        assert np.abs(OA.wigner_D(l, euler) - D).max() < 1e-13, l


def _test_points(rng, n=40):
    p = rng.normal(size=(n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    return np.concatenate([p, [[0, 0, 1.0], [0, 0, -1.0]]])


def _flat_apply(c, L, euler):
    """hostsetup.wigner_D_flat applied by hand, as k_rotate_coeff reads it: out_lm = sum_n D[off_l + (m+l)(2l+1) + (n+l)] c_ln"""
    D = hs.wigner_D_flat(L, euler)
    out = np.empty_like(c)
    for l in range(L + 1):
        off, n = l * (4 * l * l - 1) // 3, 2 * l + 1
        out[:, l * l:(l + 1) ** 2] = c[:, l * l:(l + 1) ** 2] @ D[off:off + n * n].reshape(n, n).T
    return out


@pytest.mark.parametrize('L', [3, 10, 32])
def test_rotation_is_f_of_R_inverse(L):
    """rotate_coeff(c, R) evaluated at x equals f(R^-1 x), not f(R x): generic angles, grid angles, and the flipped
    (2 pi - alpha, beta, 2 pi - gamma) form find_rotation hands out"""
    rng = np.random.default_rng(40 + L)
    c = (rng.normal(size=(2, (L + 1) ** 2)) + 1j * rng.normal(size=(2, (L + 1) ** 2))) / (1 + np.arange((L + 1) ** 2)) ** 0.5
    pts = _test_points(rng)
    al, be, ga = OA.euler_grid(L + 1)
    cases = [(0.83, 1.91, 4.4), (5.9, 0.21, 0.05), (al[3], be[2], ga[5]), (2 * np.pi - al[3], be[L], 2 * np.pi - ga[2]),
             (2 * np.pi, be[0], 2 * np.pi)]
    worst = 0.0
    for euler in cases:
        R = SR.rotation_matrix(euler)
        want = SR.evaluate(c, L, pts @ R)                            # rows of pts @ R are R^-1 x
        wrong = SR.evaluate(c, L, pts @ R.T)                         # R x
        scale = np.abs(want).max()
        for name, rot in (('oracle', OA.rotate_coeff(c, euler, L)), ('flat', _flat_apply(c, L, euler)),
                          ('ref', SR.rotate_ref(c, euler, L).astype(complex))):
            got = SR.evaluate(rot, L, pts)
            err = np.abs(got - want).max() / scale
            worst = max(worst, err)
            assert err <= TOL_ROT, (name, euler, err)
            assert np.abs(got - wrong).max() / scale > 0.1, (name, euler)      # the two conventions are told apart
    print('L = %d: worst |rotated - f(R^-1 x)| / max|f| = %.2e' % (L, worst))


def _coeff(rng, N, L, decay=True):
    c = rng.normal(size=(N, (L + 1) ** 2)) + 1j * rng.normal(size=(N, (L + 1) ** 2))
    return c / (1 + np.arange((L + 1) ** 2)[None, :]) ** 0.5 if decay else c


def test_correlation_whole_array_and_definition():
    N, L, lo, hi = 8, 10, 2, 7
    rng = np.random.default_rng(5)
    ref, sig = _coeff(rng, N, L), _coeff(rng, N, L)
    C = OA.correlation(ref, sig, L, [lo, hi])
    Cr = SR.correlation_ref(ref, sig, L, lo, hi)
    scale = float(np.abs(Cr).max())
    err = float(np.abs(C - Cr).max()) / scale
    print('oracle correlation vs longdouble restatement: %.2e of max|C|' % err)
    assert C.shape == (2 * L + 2,) * 3 and err <= 1e-13
    # the definition: mean_r Re <ref_r, rotate_coeff(sig, R)_r> at 30 sampled grid rotations
    al, be, ga = OA.euler_grid(L + 1)
    worst = 0.0
    for _ in range(30):
        j, b, k = (int(x) for x in rng.integers(2 * L + 2, size=3))
        rot = SR.rotate_ref(sig, (al[j], be[b], ga[k]), L)
        want = float(np.mean(np.sum(ref[lo:hi].conj() * rot[lo:hi], axis=1).real))
        worst = max(worst, abs(C[j, b, k] - want) / scale, abs(float(Cr[j, b, k]) - want) / scale)
    print('correlation vs its definition at 30 rotations: %.2e of max|C|' % worst)
    assert worst <= 1e-13


def test_correlation_swapped_arguments_is_seen():
    """the check can fail: C(sig, ref) differs from C(ref, sig) by O(max|C|)"""
    rng = np.random.default_rng(6)
    ref, sig = _coeff(rng, 4, 5), _coeff(rng, 4, 5)
    C, Cs = OA.correlation(ref, sig, 5), SR.correlation_ref(sig, ref, 5, 0, 4)
    assert np.abs(C - Cs).max() > 0.1 * np.abs(C).max()


def test_argmax_reading_order():
    """mean_C_layout + argmax against the key formula written out: i_beta nb^2 + ((-j) mod nb) nb + ((-k) mod nb), first maximum"""
    rng = np.random.default_rng(7)
    nb = 8
    for trial in range(6):
        C = rng.normal(size=(nb, nb, nb))
        if trial >= 3:                                               # ties: the same maximum at several places
            idx = rng.integers(nb, size=(4, 3))
            C[idx[:, 0], idx[:, 1], idx[:, 2]] = 10.0
        if trial == 5:
            C[:] = 1.25                                              # all equal: key 0
        want = None
        for b in range(nb):                                          # by hand, in key order
            for ja in range(nb):
                for kg in range(nb):
                    v = C[(-ja) % nb, b, (-kg) % nb]
                    if want is None or v > want[0]:
                        want = (v, b * nb * nb + ja * nb + kg)
        assert int(np.argmax(OA.mean_C_layout(C))) == want[1], trial
        assert SR.argmax_key(C)[0] == want[1], trial
    assert SR.argmax_key(np.full((4, 4, 4), 2.0)) == (0, 0.0)


def test_stats_and_prtf_references_known_answers():
    """the longdouble restatements of the grid statistics and the PRTF on data whose answers are known in closed form"""
    N, nt, nph = 3, 4, 8
    ct, wt_g = np.polynomial.legendre.leggauss(nt)
    ct, wt = ct[::-1].copy(), wt_g[::-1] * np.pi / nt
    rs, wr = np.array([0.5, 1.5, 2.5]), np.array([1.0, 2.0, 3.0])
    g = np.full((N, nt, nph), 2.0 - 1.0j)
    val, mag = SR.stats_ref(g, wr, wt, rs, ct, ref=np.zeros_like(g))
    tot = wr.sum() * wt.sum() * nph
    assert np.allclose(np.asarray(val[[0, 4, 5, 6, 7, 8, 9, 10]], float), [2 * tot, 4 * tot, 4 * tot, 2, 2, 2 * g.size, -g.size, g.size])
    assert np.abs(np.asarray(val[1:4], float)).max() < 1e-14 * tot     # a constant has its centre of mass at the origin
    g2 = np.zeros((N, nt, nph), complex)
    g2[1, 0, 0], g2[1, 0, 1], g2[2, 3, 5] = 1j, -1j, -3.0
    val, _ = SR.stats_ref(g2, wr, wt, rs, ct)
    assert (float(val[6]), float(val[7]), float(val[8]), float(val[9]), float(val[10])) == (0.0, -3.0, 0.0, 1.0, 1.0)
    g2[0, 0, 0] = np.nan
    val, _ = SR.stats_ref(g2, wr, wt, rs, ct)
    assert np.isnan(float(val[6])) and np.isnan(float(val[7]))
    # PRTF: a1 = a2 = b gives 1; the three rules; the branch cut
    a = np.array([[1 + 1j, -2.0, 3j, 0.5]])
    m, s, _ = SR.prtf_ref(a, a, np.abs(a) ** 2, np.abs(a) ** 2)
    assert abs(complex(m[0]) - 1) < 1e-15 and float(s[0]) < 1e-15
    a1, a2 = np.array([[1.0, 0.0, -1.0, 1.0]], complex), np.array([[1.0, 1.0, 1.0, -1.0]], complex)
    I = np.array([[0.0, 0.0, 1.0, 1.0]])
    # 0 (b = 0, both a), 1 (b = 0, an a = 0), then a1 conj(a2) = -1 + 0i and -1 - 0i: numpy's complex division by b1 conj(b2)
    # (promoted to x + 0i) returns +0 for the imaginary part of both, so both square roots are +i -- the branch cut is never
    # approached from below
    m, _, _ = SR.prtf_ref(a1, a2, I, I)
    assert abs(complex(m[0]) - (0.25 + 0.5j)) < 1e-15

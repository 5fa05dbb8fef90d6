"""Independent references (TEST INFRASTRUCTURE) for the alignment and averaging kernels (csrc/k_align.hip, csrc/k_average.hip).

Nothing here imports the product's host code or ``oracle/alignment.py`` for a *value*, with two stated exceptions:

* ``wigner_small`` takes the small Wigner matrices from ``hostsetup.wigner_d`` (eigen-decomposition of J_y) and widens them to
  ``numpy.longdouble``.  That function is first held to ``wigner_d_exact`` (explicit sum, integer factorials, mpmath at 80 digits)
  by tests/test_so3_reference.py: every entry for l <= 6, fixed-seed samples with corners, centre and end betas up to l = 63,
  bound 1e-13 absolute.  ``rotate_ref`` and ``correlation_ref`` may be used as references only because of that test.
* ``prtf_ref`` takes the point rule from ``oracle.alignment.prtf_points``, which fixture G14 pins to the reference's own function; only
  the longdouble sums are added here.

Definitions (header of k_align.hip; soft_plugin.py:64-99 quotes them): ZYZ Euler angles, R = Rz(alpha) Ry(beta) Rz(gamma),
D^l_mn(R) = e^{-i m alpha} d^l_mn(beta) e^{-i n gamma}, d^l_mn(beta) = <l m| exp(-i beta J_y) |l n>, (R f)(x) = f(R^-1 x) has the
coefficients sum_n D^l_mn f_ln, and C(R) = mean_r Re <ref_r, R sig_r> on the grid alpha_j = gamma_j = 2 pi j / 2bw,
beta_k = pi (2k+1) / 4bw, bw = L + 1."""
from math import factorial

import numpy as np

try:  # scipy >= 1.15
    from scipy.special import sph_harm_y as _sph_harm_y

    def _ylm(l, m, theta, phi):
        return _sph_harm_y(l, m, theta, phi)
except ImportError:  # pragma: no cover
    from scipy.special import sph_harm as _sph_harm

    def _ylm(l, m, theta, phi):
        return _sph_harm(m, l, phi, theta)

LD = np.longdouble
CLD = np.clongdouble
PI_LD = 4 * np.arctan(LD(1))
MP_DIGITS = 80


# ---------------------------------------------------------------------------------------------- Wigner matrices, exact
def wigner_d_exact(l, m, n, beta):
    """d^l_mn(beta) = <l m| exp(-i beta J_y) |l n> from the explicit sum (Wigner 1931; Varshalovich 4.3.1 (2)):
    sum_s (-1)^(m-n+s) sqrt((l+m)! (l-m)! (l+n)! (l-n)!) / ((l+n-s)! s! (m-n+s)! (l-m-s)!) cos(b/2)^(2l+n-m-2s) sin(b/2)^(m-n+2s)
    with Python integers for the factorials and mpmath at MP_DIGITS digits (the terms reach 2^(2l) before they cancel:
    38 digits at l = 63).  `beta` is taken as the double it is.  Returns a float."""
    import mpmath as mp
    with mp.workdps(MP_DIGITS):
        half = mp.mpf(float(beta)) / 2
        c, s = mp.cos(half), mp.sin(half)
        root = mp.sqrt(mp.mpf(factorial(l + m) * factorial(l - m) * factorial(l + n) * factorial(l - n)))
        tot = mp.mpf(0)
        for k in range(max(0, n - m), min(l + n, l - m) + 1):
            den = factorial(l + n - k) * factorial(k) * factorial(m - n + k) * factorial(l - m - k)
            term = root / den * c ** (2 * l + n - m - 2 * k) * s ** (m - n + 2 * k)
            tot += -term if (m - n + k) % 2 else term
        return float(tot)


def wigner_small(l, betas):
    """(len(betas), 2l+1, 2l+1) longdouble d^l_mn(beta): hostsetup.wigner_d widened (see the module docstring: usable as a
    reference only because tests/test_so3_reference.py holds that function to wigner_d_exact)"""
    from xframe_amd.fxs import hostsetup as hs
    return hs.wigner_d(l, np.atleast_1d(np.asarray(betas, dtype=float))).astype(LD)


# ---------------------------------------------------------------------------------------------- rotations of functions
def rotation_matrix(euler):
    """R = Rz(alpha) Ry(beta) Rz(gamma), active, right-handed"""
    a, b, g = (float(x) for x in euler)

    def rz(t):
        return np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])

    def ry(t):
        return np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]])
    return rz(a) @ ry(b) @ rz(g)


def evaluate(coeff, L, points):
    """f(x) = sum_lm c_lm Y_lm(x) at unit vectors `points` (n, 3); coeff (..., (L+1)^2), index l(l+1)+m; orthonormal Y_lm with
    the Condon-Shortley phase (scipy's).  Returns (..., n)."""
    p = np.asarray(points, dtype=float)
    p = p / np.linalg.norm(p, axis=1, keepdims=True)
    theta, phi = np.arccos(np.clip(p[:, 2], -1, 1)), np.arctan2(p[:, 1], p[:, 0])
    Y = np.empty(((L + 1) ** 2, len(p)), complex)
    for l in range(L + 1):
        for m in range(-l, l + 1):
            Y[l * (l + 1) + m] = _ylm(l, m, theta, phi)
    return np.asarray(coeff) @ Y


def _cexp(x):
    """exp(i x) for a longdouble array"""
    out = np.empty(np.shape(x), CLD)
    out.real, out.imag = np.cos(x), np.sin(x)
    return out


def wigner_D_ref(l, euler):
    """D^l_mn = e^{-i m alpha} d^l_mn(beta) e^{-i n gamma}, clongdouble (2l+1, 2l+1)"""
    a, b, g = (LD(float(x)) for x in euler)
    m = np.arange(-l, l + 1).astype(LD)
    return _cexp(-m * a)[:, None] * wigner_small(l, [float(euler[1])])[0] * _cexp(-m * g)[None, :]


def rotate_ref(coeff, euler, L):
    """coefficients of (R f)(x) = f(R^-1 x): f_lm -> sum_n D^l_mn(R) f_ln per shell; coeff (Nq, (L+1)^2) -> clongdouble"""
    c = np.asarray(coeff).astype(CLD)
    out = np.empty(c.shape, CLD)
    for l in range(L + 1):
        out[:, l * l:(l + 1) ** 2] = c[:, l * l:(l + 1) ** 2] @ wigner_D_ref(l, euler).T
    return out


def correlation_ref(ref, sig, L, lo, hi):
    """C[j, b, k] = Re sum_l sum_mn T^l_mn d^l_mn(beta_b) e^{-i m alpha_j} e^{-i n gamma_k}, T^l_mn = mean over the shells
    lo <= r < hi of conj(ref_lm(r)) sig_ln(r): two matrix products in longdouble, twiddle angles 2 pi ((m j) mod 2bw) / 2bw reduced
    as integers.  Returns longdouble (2bw, 2bw, 2bw) indexed [alpha, beta, gamma]."""
    bw = L + 1
    nb, M = 2 * bw, 2 * L + 1
    ref, sig = np.asarray(ref)[lo:hi].astype(CLD), np.asarray(sig)[lo:hi].astype(CLD)
    betas = np.pi * (2 * np.arange(nb) + 1) / (4 * bw)               # the doubles the host table is built at
    S = np.zeros((nb, M, M), CLD)
    for l in range(L + 1):
        T = ref[:, l * l:(l + 1) ** 2].conj().T @ sig[:, l * l:(l + 1) ** 2] / LD(hi - lo)
        S[:, L - l:L + l + 1, L - l:L + l + 1] += T[None] * wigner_small(l, betas)
    mj = (np.arange(-L, L + 1)[None, :] * np.arange(nb)[:, None]) % nb           # (j, m)
    E = _cexp(-2 * PI_LD * mj.astype(LD) / nb)
    C = np.empty((nb, nb, nb), LD)
    for b in range(nb):
        C[:, b, :] = (E @ (S[b] @ E.T)).real
    return C


def argmax_key(C):
    """arg-max of C[alpha j, beta b, gamma k] in the reading order of average.py:936-940, written out: the key of an element is
    b nb^2 + ((-j) mod nb) nb + ((-k) mod nb); the largest value wins, among equal values the smallest key.  Returns
    (key, gap) with gap = (largest - second largest value) / max|C|."""
    nb = C.shape[0]
    j, b, k = np.meshgrid(np.arange(nb), np.arange(nb), np.arange(nb), indexing='ij')
    key = (b * nb * nb + ((-j) % nb) * nb + ((-k) % nb)).ravel()
    v = np.asarray(C).ravel()
    order = np.lexsort((key, -v))
    scale = np.max(np.abs(v))
    gap = (v[order[0]] - v[order[1]]) / scale if scale > 0 else 0.0
    return int(key[order[0]]), float(gap)


# ---------------------------------------------------------------------------------------------- grid arithmetic of the averaging
def grid_points_ld(cos_theta, n_phi):
    """sin theta, cos theta (n_theta,), cos phi, sin phi (n_phi,) in longdouble for the doubles cos_theta, phi_p = 2 pi p / n_phi"""
    ct = np.asarray(cos_theta).astype(LD)
    st = np.sqrt(np.maximum(LD(0), 1 - ct * ct))
    phi = 2 * PI_LD * np.arange(n_phi).astype(LD) / n_phi
    return st, ct, np.cos(phi), np.sin(phi)


def stats_ref(g, wr, wt, rs, cos_theta, ref=None):
    """the 11 statistics of k_av_stats for one grid g (Nq, n_theta, n_phi), complex: (values (11,) longdouble, sum of the
    magnitudes of the terms (11,) longdouble; 0 for the extrema and the count).
      [0] sum w Re, [1..3] sum w Re (x, y, z): the moments of the centre of mass (misk.py:295-312), w = wr[q] wt[t]
      [4] sum w Re^2, [5] sum w (Re ref - Re)^2: the normed integrals (mathLibrary.py:1223-1237)
      [6] max Re, [7] min Re (average.py:721-727), numpy's: a NaN is returned
      [8] + i [9] sum and [10] count of the entries that numpy calls > 0 (average.py:424-435: lexicographic on complex numbers)"""
    g = np.asarray(g)
    re, im = g.real.astype(LD), g.imag.astype(LD)
    st, ct, cp, sp = grid_points_ld(cos_theta, g.shape[2])
    w = (np.asarray(wr).astype(LD)[:, None] * np.asarray(wt).astype(LD)[None, :])[:, :, None]
    r = np.asarray(rs).astype(LD)[:, None, None]
    x, y, z = r * st[None, :, None] * cp[None, None, :], r * st[None, :, None] * sp[None, None, :], r * ct[None, :, None] * np.ones(g.shape[2], LD)
    terms = [w * re, w * re * x, w * re * y, w * re * z, w * re * re]
    if ref is not None:
        d = np.asarray(ref).real.astype(LD) - re
        terms.append(w * d * d)
    else:
        terms.append(np.zeros(g.shape, LD))
    pos = (g.real > 0) | ((g.real == 0) & (g.imag > 0))
    val, mag = np.zeros(11, LD), np.zeros(11, LD)
    for i, t in enumerate(terms):
        val[i], mag[i] = t.sum(), np.abs(t).sum()
    val[6], val[7] = np.max(g.real), np.min(g.real)
    val[8], val[9], val[10] = re[pos].sum(), im[pos].sum(), pos.sum()
    mag[8], mag[9] = np.abs(re[pos]).sum(), np.abs(im[pos]).sum()
    return val, mag


def phase_ref(g, center, sign, qs, cos_theta):
    """g exp(-i sign k . c), k = q (sin theta cos phi, sin theta sin phi, cos theta) (fxs_Projections.py:1436-1443), clongdouble"""
    g = np.asarray(g)
    st, ct, cp, sp = grid_points_ld(cos_theta, g.shape[2])
    cx, cy, cz = (LD(float(v)) for v in center)
    u = st[:, None] * (cp[None, :] * cx + sp[None, :] * cy) + ct[:, None] * cz
    kc = np.asarray(qs).astype(LD)[:, None, None] * u[None]
    return g.astype(CLD) * _cexp(-LD(float(sign)) * kc)


def combine_ref(op, A, scalars=None):
    """the five operations of k_av_combine on a stack A (n, ...) in clongdouble"""
    A = np.asarray(A).astype(CLD)
    if op == 'conj':
        return A.conj()
    if op == 'sum':
        return A.sum(axis=0)
    if op == 'abs2sum':
        return (A.real ** 2 + A.imag ** 2).sum(axis=0).astype(CLD)
    s = np.asarray(scalars).astype(CLD)
    if op == 'scale':
        return A * s.reshape((-1,) + (1,) * (A.ndim - 1))
    if op == 'affine':
        return (A - s[0]) * s[1]
    raise KeyError(op)


def prtf_ref(a1, a2, I1, I2):
    """resolution_metrics.py:62-78 per shell: (mean (Nq,) clongdouble, standard deviation (Nq,) longdouble, sum over the sphere of
    the magnitudes |nd| (Nq,) longdouble).  The point rule is oracle.alignment.prtf_points (pinned by G14)."""
    from oracle import alignment as OA
    nd = OA.prtf_points(np.asarray(a1), np.asarray(a2), np.sqrt(np.asarray(I1).real), np.sqrt(np.asarray(I2).real))
    nd = nd.reshape(nd.shape[0], -1).astype(CLD)
    n = nd.shape[1]
    mean = nd.sum(axis=1) / LD(n)
    dev = nd - mean[:, None]
    std = np.sqrt((dev.real ** 2 + dev.imag ** 2).sum(axis=1) / LD(n))
    mag = np.sqrt(nd.real ** 2 + nd.imag ** 2).sum(axis=1)
    return mean, std, mag

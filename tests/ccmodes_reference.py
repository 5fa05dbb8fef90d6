"""numpy restatement of the three back-substitution modes beside `back_substitution` (each function cites its reference lines):

    xframe/projects/fxs/projectLibrary/fxs_invariant_tools.py:519-576   ccd_to_deg2_invariant_3d_back_substitution_memory_hungry
                                                              646-694   ..._back_substitution_qqsym
                                                              710-761   ..._back_substitution_psd
                                                              374-422   cross_correlation_to_deg2_invariant (the bookkeeping around them)
    xframe/library/mathLibrary.py:872-892, 1499-1517                    nearest_positive_semidefinite_matrix, (psd_)back_substitution

tests/test_ccmodes_reference.py holds it to the reference's own outputs (G31, tests/golden/cc_backsub_modes.npz); the device tests of
tests/ccmodes_cases.py use it at the sizes the fixture cannot hold."""
import numpy as np

import ccextract_cases as CC
import ccmask_cases as MC
from xframe_amd.fxs import hostsetup as hs

MODES = ('back_substitution_memory_hungry', 'back_substitution_qqsym', 'back_substitution_psd')
CLIP_GUARD = 1e-10                    # an eigenvalue closer to zero than this (relative to |A|_F) may fall on either side of the clip


def nearest_psd(A, eigh=np.linalg.eigh):
    """mathLibrary.py:878-890 with limit = 0, one matrix or a stack"""
    B = (A + np.swapaxes(A, -1, -2).conj()) / 2
    w, v = eigh(B)
    w = np.where(w < 0, 0, w)
    return v * w[..., None, :] @ np.swapaxes(v, -1, -2).conj()


def shifted_eigh(B):
    """eigh through the shift the device takes: eigh(B + |B|_F 1) - |B|_F (eigenvalues to eps |B|_F absolute)"""
    B = np.asarray(B)
    s = np.linalg.norm(B, axis=(-2, -1))
    w, v = np.linalg.eigh(B + s[..., None, None] * np.eye(B.shape[-1]))
    return w - s[..., None], v


def clip_counts(A):
    """(eigenvalues below zero, eigenvalues within CLIP_GUARD |A|_F of zero) of the Hermitian part of one matrix"""
    B = (A + A.conj().T) / 2
    w = np.linalg.eigvalsh(B)
    scale = max(np.linalg.norm(A), 1e-300)
    return int((w < 0).sum()), int((np.abs(w) <= CLIP_GUARD * scale).sum())


def legendre_matrices(qs, l_max):
    """ccd_associated_legendre_matrices(thetas, l_max, l_max) (23-33): (q1, q2, m, l), zero for m > l"""
    x = np.cos(np.arccos(qs * CC.WAVELENGTH / (4 * np.pi)))
    l, m = np.meshgrid(np.arange(l_max + 1), np.arange(l_max + 1), indexing='ij')
    p = np.zeros((len(qs), l_max + 1, l_max + 1))                                 # (q, m, l)
    ok = m <= l
    p[:, m[ok], l[ok]] = hs.sph_plm(l[ok][None, :], m[ok][None, :], x[:, None])
    return p[None, :] * p[:, None] / (2 * np.arange(l_max + 1) + 1)[None, None, None, :]


def back_substitution(cn, ppm):
    """mathLibrary.py:1509-1517"""
    bl = np.zeros(cn.shape, dtype=complex)
    cn, pm = cn.copy(), ppm.copy()
    for i in np.arange(0, cn.shape[-1])[::-1]:
        bl[..., i] = cn[..., -1] / pm[..., -1, -1]
        cn = cn[..., :-1] - bl[..., i, None] * pm[..., :-1, -1]
        pm = pm[..., :-1, :-1]
    return bl


def psd_back_substitution(cn, ppm, eigh=np.linalg.eigh):
    """mathLibrary.py:1499-1507; also returns per step (clipped eigenvalues, eigenvalues inside the guard band, the most negative
    eigenvalue relative to |A_l|_F)"""
    bl = np.zeros(cn.shape, dtype=complex)
    cn, pm = cn.copy(), ppm.copy()
    steps = [None] * cn.shape[-1]
    for i in np.arange(0, cn.shape[-1])[::-1]:
        a = cn[..., -1] / pm[..., -1, -1]
        h = (a + a.conj().T) / 2
        steps[i] = clip_counts(a) + (float(np.linalg.eigvalsh(h).min() / max(np.linalg.norm(h), 1e-300)),)
        bl[..., i] = nearest_psd(a, eigh)
        cn = cn[..., :-1] - bl[..., i, None] * pm[..., :-1, -1]
        pm = pm[..., :-1, :-1]
    return bl, steps


def mode_3d(mode, cc, qs, orders, cc_mask, route='rfft', eigh=np.linalg.eigh):
    """the worker of `mode` (519-576 / 646-694 / 710-761) on modified data: (b (Nq, Nq, n_m), qq_mask, steps or None).  memory_hungry
    interpolates masked samples first (546-549)."""
    phis = np.arange(cc.shape[-1]) * 2 * np.pi / cc.shape[-1]
    l_max = int(orders.max())
    cc_mask = np.asarray(cc_mask, dtype=bool)
    if mode == 'back_substitution_memory_hungry' and not cc_mask.all():
        cc, cc_mask = MC.r_interpolate(cc, cc_mask, phis), np.ones_like(cc_mask)
    qq_mask = cc_mask.all(-1)
    stride = 1 if (orders % 2).any() else 2
    ppm = legendre_matrices(qs, l_max)
    harmonics = CC.r_harmonics(cc, l_max + 1, route)
    if mode == 'back_substitution_psd':
        ccn = np.moveaxis(np.array([nearest_psd(harmonics[..., o], eigh) for o in range(l_max + 1)]), 0, -1)
        ccn[~qq_mask] = 0
        b, steps = psd_back_substitution(ccn, ppm, eigh)
        return b[..., ::stride], qq_mask, steps
    ppm = ppm[:, :, ::stride, ::stride]
    ccn = np.zeros(ppm.shape[:3], dtype=complex)
    if mode == 'back_substitution_qqsym':
        ppm = (ppm + np.swapaxes(ppm, 0, 1)) / 2
        t = harmonics[..., ::stride]
        t = (t + np.swapaxes(t, 0, 1).conj()) / 2
        ccn[qq_mask, :] = t[qq_mask, :]
    else:
        ccn[qq_mask, :] = harmonics[qq_mask][..., ::stride]
    return back_substitution(ccn, ppm), qq_mask, None


def cc_to_deg2(mode, cc, qs, phis, max_order, zero_odd, modify_cc, avg, cc_mask=None, route='rfft', eigh=np.linalg.eigh):
    """cross_correlation_to_deg2_invariant (374-422) in three dimensions with `mode`: (b_coeff (max_order + 1, Nq, Nq), qq_mask, steps)"""
    cc_mask = np.ones(cc.shape, dtype=bool) if cc_mask is None else cc_mask
    cc, cc_mask = MC.r_modify_masked(cc, cc_mask, phis, avg, modify_cc)
    orders = np.arange(max_order + 1)
    keep = ~(orders % 2).astype(bool) if zero_odd else np.ones(len(orders), dtype=bool)        # 396-399
    b = np.zeros(cc.shape[:2] + (max_order + 1,), dtype=complex)                               # 417
    part, qq_mask, steps = mode_3d(mode, cc, qs, orders[keep], cc_mask, route, eigh)
    b[..., keep] = part                                                                        # 418
    return np.moveaxis(b, -1, 0), qq_mask, steps                                               # 419

"""Cases for the Legendre synthesis shared by k_sht_chain and k_sht_inv_wide (xframe_amd/csrc/k_sht_legendre.h): the records in
LDS padded to l = L + 1, the uniform trip count of a wave's two orders, the start values of all items of a wave requested at
kernel entry.  Shared by tests/test_gpu_chain_latency.py (MI355X) and tests/test_emul_chain_latency.py (CPU emulator of the same
sources); judged with the oracle and the suite's own tolerances (parity_cases).

Shapes: the smallest at which this code takes another path -- both parities of L (an even L leaves the last order without a
partner in its wave) on every grid width the chained kernel is instantiated for (n_phi = 16, 32, 64, 128: the default grid of
L = 3..5, 6..10, 11..21, 22..42), 2 or 3 shells, 2 restarts.  L = 3 has two items for eight waves: six waves get none."""
import numpy as np

import parity_cases as PC
from helpers import rel_l2
from xframe_amd.fxs.engine import Engine

# (N shells, L): all of them chain (n_phi <= 128 and a shell fits one CU)
TRANSFORM_CASES = [(2, 3), (3, 4), (2, 5), (2, 9), (2, 10), (3, 15), (2, 16), (2, 31), (3, 32), (2, 33)]
# unit coefficients, both parities each: n_phi = 32 (6, 7); n_phi = 64 with accumulation groups of 128 (19, 20); n_phi = 128 with
# tables in registers and 2 (l, m) pairs per thread (27, 28), 3 pairs (32, 33), groups of 512 and run-time tables (38, 39)
UNIT_L = [6, 7, 19, 20, 27, 28, 32, 33, 38, 39]


def check_transforms(N, L, lib_path):
    PC.check_transforms(N, L, lib_path, seed=100 + N + L, expect_chain=True)


def check_wide_two_chunks(lib_path):
    """k_sht_inv_wide with 64 theta pairs per workgroup: two chunks of 32, cos(theta) read from LDS per item, the start-value
    queue indexed by (order pair, chunk); n_phi = 256 has no chained kernel"""
    PC.check_transforms(2, 9, lib_path, seed=77, expect_chain=False, n_theta=128, n_phi=256, n_batch=2)


def unit_points(L):
    """(l, m) with l in {|m|, |m| + 1, L - 1, L} for every m = -L..L: the first two steps of the recurrence (start values), the
    last double step and the closing single step of either lane of a wave"""
    pts = []
    for m in range(-L, L + 1):
        for l in sorted({abs(m), abs(m) + 1, L - 1, L}):
            if abs(m) <= l <= L:
                pts.append((l, m))
    return pts


def check_unit_coefficients(L, lib_path):
    """one shell per point with the single coefficient c_lm = 1: a dropped or doubled last step, or a start value handed to the
    wrong item, changes a whole shell, so every shell is judged on its own (TOL_SHT each, not diluted over the batch)"""
    pts = unit_points(L)
    N = len(pts)
    e, fp = PC.transforms_engine(N, L, lib_path, n_batch=1)
    sht = fp.sht
    co = np.zeros((1, N, e.nlm), complex)
    for s, (l, m) in enumerate(pts):
        co[0, s, l * (l + 1) + m] = 1.0
    ref_g = sht.inverse_d(co)
    ref_c = sht.forward_d(ref_g)
    e.profile(True)
    gi, ci = e.sht_inverse_forward(co, 0)
    assert e.profile_get('sht_chain')[1] > 0
    e.profile(False)
    gw = e.sht_inverse(co)                                   # k_sht_inv_wide
    worst = 0.0
    for s, (l, m) in enumerate(pts):
        for got, ref in ((gi[0, s], ref_g[0, s]), (ci[0, s], ref_c[0, s]), (gw[0, s], ref_g[0, s])):
            d = rel_l2(got, ref)
            worst = max(worst, d)
            assert d < PC.TOL_SHT, (L, l, m, d)
    print('unit coefficients L = %d: %d shells, worst rel-L2 %.2e' % (L, N, worst))
    e.close()


def check_fused_steps_ft_stab(lib_path, N=4, L=32):
    """2 HIO + 2 ER steps with ft_stab at the benchmark's angular size with few shells: the fused step (the three chained kernels)
    against the reference-order step (separate transforms, k_sht_inv_wide with the coefficient difference) from the same state,
    at the bounds parity_cases.check_full_size_properties uses for fused against reference order"""
    import xframe_amd.fxs.hostsetup as hs
    import bigl_loop_cases as BL
    # the problem of chain_diet_cases.steps_problem for this N x L (bigl_loop_cases.problem: particle, support and guess reach out to
    # between shells 2 and 3, upper value bound inside the density's range): with the 250 A particle of the BASELINE configs one
    # shell lies inside the support and the error sums of the three chained kernels are exactly zero in every step
    data, opt = BL.problem(N, L, 0, 0, big_l=False)
    radius = opt['particle_radius']
    out = {}
    for fused in (False, True):
        e = Engine(opt, data, n_batch=2, lib_path=lib_path, fused=fused)
        rho0 = hs.bump_density(e.rs, e.shape, radius, 0.3, 2, np.random.default_rng(1000),
                               e.rsetup.integrated_intensity, e.int_wr, e.int_wt)
        for b in range(2):
            e.set_density(b, rho0)
        e.init_state()
        err_h, _ = e.run('HIO', True, np.full(2, 0.45))
        err_e, _ = e.run('ER', True, np.full(2, 0.45))
        out[fused] = (np.concatenate([err_h, err_e]), e.density(0), e.reciprocal_density(0))
        e.close()
    errs_a, rho_a, F_a = out[False]
    errs_b, rho_b, F_b = out[True]
    print('fused vs reference order, %d x L%d: density %.2e, F %.2e, first-step error ratio - 1 %.2e'
          % (N, L, rel_l2(rho_b, rho_a), rel_l2(F_b, F_a), np.abs(errs_b[0] / errs_a[0] - 1).max()))
    print('error histories, reference order: %s fused: %s' % (errs_a[:, 0], errs_b[:, 0]))
    assert np.isfinite(errs_a).all() and np.isfinite(errs_b).all()
    assert (errs_a > 0).all() and (errs_b > 0).all(), (errs_a, errs_b)                      # not zeros against zeros
    assert rel_l2(rho_b, rho_a) < 1e-7 and rel_l2(F_b, F_a) < 1e-7
    assert np.allclose(errs_b[0], errs_a[0], rtol=PC.TOL_STEP)

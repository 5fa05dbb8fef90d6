"""Cases for the leaner L = 32 instantiation of k_sht_chain (geometry at compile time, no EXEC regions around the panel stores, the
Legendre table in 16-byte loads from d_PTw), shared by tests/test_emul_chain_diet.py (CPU emulator of the same sources) and
tests/test_gpu_chain_diet.py (MI355X).  Nothing of the arithmetic was meant to move, so the results are compared BIT FOR BIT
with those of the commit in front of the change, as tests/golden/chain_bits.npz holds them (recorded from that commit's build by
tests/golden/make_golden_chain_bits.py, once on the emulator, once on the MI355X: hardware division and square root need not
round like the host's).

Shapes -- the smallest that reach each path:
- l32:    3 shells x L 32 on the 64 x 128 grid, 2 restarts: SHT_CHAIN_L32; shell 0 and shells > 0 (add-back), two slot tables.
- regtab: 3 shells x L 31 on the same grid, 1 restart: SHT_CHAIN_REGTAB (run-time geometry, table rows in registers).
- rt:     2 shells x L 9 (24 x 32 grid), 2 restarts: SHT_CHAIN_RT.
The last two must not have moved either.

What is compared: (a) grid and coefficients of Engine.sht_inverse_forward for the store link (prologue 0) and the |.|^2 link
(prologue 1) on seeded coefficients; (b, l32 only) 2 HIO + 2 ER fused steps with ft_stab from seeded densities -- all three
chained kernels and the error sums -- : the error history, the density and the reciprocal density F of both restarts.  Every
array is compared in full through the SHA-256 of its bytes; the file also stores the arrays themselves, so that a difference can
be located -- the error histories in full, the coefficients of restart 0 in full, the grids as a seeded sample of SAMPLE points
(the file has to stay small; the digests cover every element)."""
import hashlib
import os

import numpy as np

import parity_cases as PC
from helpers import golden_settings, OracleTransforms
from oracle.fourier import FourierPair
from oracle.sht import SHT
from xframe_amd.fxs import _lib
from xframe_amd.fxs import synthetic as S
from xframe_amd.fxs.engine import Engine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'chain_bits.npz')
# name: (N, L, n_theta, n_phi, restarts)
CASES = {'l32': (3, 32, 64, 128, 2), 'regtab': (3, 31, 64, 128, 1), 'rt': (2, 9, 0, 0, 2)}
SEED = 2718
SAMPLE = 512
STEPS_CASE = 'l32'
CHAIN_DBG_SLOTS = 18


def digest(a):
    return np.array(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def sample(a, seed):
    """a seeded sample of SAMPLE elements of a grid array (the same elements whoever calls)"""
    flat = np.ascontiguousarray(a).reshape(-1)
    idx = np.random.default_rng(seed).choice(flat.size, size=min(SAMPLE, flat.size), replace=False)
    return flat[np.sort(idx)]


def stamps_written(e):
    """True if the chained launches since mtip_debug_chain_timing(ctx, None) wrote phase stamps: only the L = 32 instantiation does"""
    out = np.zeros((3, e.B * e.N, CHAIN_DBG_SLOTS), np.int64)
    e._ck(e.lib.mtip_debug_chain_timing(e.ctx, _lib.ptr(out)))
    return bool((out[:, :, CHAIN_DBG_SLOTS - 1] != 0).any())


def transform_results(name, lib_path, check_l32=True):
    """(a): {key: array} of the two links on seeded coefficients"""
    N, L, nt, nphi, B = CASES[name]
    e, _ = PC.transforms_engine(N, L, lib_path, n_batch=B, n_theta=nt, n_phi=nphi)
    try:
        assert not nt or (e.n_theta, e.n_phi) == (nt, nphi)
        co = PC.cplx(np.random.default_rng(SEED + L), (B, N, e.nlm))
        out = {}
        e.profile(True)
        for pro in (0, 1):
            grid, coeff = e.sht_inverse_forward(co, pro)
            out['%s_coeff%d' % (name, pro)] = coeff
            out['%s_grid%d' % (name, pro)] = grid
        assert e.profile_get('sht_chain')[1] == 2, 'the chained kernel did not run'
        e.profile(False)
        if check_l32:
            # which instantiation: the phase stamps exist for SHT_CHAIN_L32 alone (the results above are those of the plain one)
            e._ck(e.lib.mtip_debug_chain_timing(e.ctx, None))
            e.sht_inverse_forward(co, 0)
            assert stamps_written(e) == (name == 'l32'), name
        return out
    finally:
        e.close()


def steps_problem():
    """(invariants, settings, particle radius) of the l32 shape.  Three shells are too few nodes for the cubic regridding of the
    invariants, so the problem takes the data grid itself with linear regridding (then the identity), and a particle, support and
    guess that reach out to between shells 2 and 3 with an upper value bound inside the density's range -- with the 250 A particle
    of the BASELINE configs one shell lies inside the support and the real-space error sums, which this is about, are exactly zero
    (tests/bigl_loop_cases.py has the reasoning and the figures)"""
    import xframe_amd.fxs.hostsetup as hs
    N, L, nt, nphi, _ = CASES[STEPS_CASE]
    fpd = FourierPair(SHT(L, nt, nphi), N, S.data_cutoff(N), 2.0)
    q_d = S.midpoint_points(S.data_cutoff(N), N)
    max_q = float(S.data_cutoff(N))
    rs, _ = hs.radial_grids(max_q, N, 2.0, 'midpoint')
    radius = float((rs[1] + rs[2]) / 2)
    tr = OracleTransforms(fpd)
    F = tr.ft(S.ball_density(tr.rs, tr.thetas, tr.phis, particle_radius=radius))
    data = S.invariants_from_intensity_coefficients(tr.forward_l(F * F.conj()), q_d, L, tr)
    opt = golden_settings(N, L, {
        'grid': {'n_theta': nt, 'n_phi': nphi, 'max_q': max_q}, 'particle_radius': radius, 'density_guess': {'radius': radius},
        'projections': {'reciprocal': {'regrid': {'interpolation': 'linear'}},
                        'real': {'projections': {'support': {'initial_support': {'max_radius': radius}},
                                                 'value_threshold': {'threshold': [0, 0.3]}}}}})
    return data, opt, radius


def steps_results(lib_path):
    """(b): 2 HIO + 2 ER fused steps with ft_stab at the l32 shape from seeded densities (one per restart)"""
    import xframe_amd.fxs.hostsetup as hs
    N, L, nt, nphi, B = CASES[STEPS_CASE]
    data, opt, radius = steps_problem()
    e = Engine(opt, data, n_batch=B, lib_path=lib_path, fused=True)
    try:
        assert (e.n_theta, e.n_phi) == (nt, nphi)
        for b in range(B):
            e.set_density(b, hs.bump_density(e.rs, e.shape, radius, 0.3, 2, np.random.default_rng(SEED + b),
                                             e.rsetup.integrated_intensity, e.int_wr, e.int_wt))
        e.init_state()
        e.profile(True)
        err_h, _ = e.run('HIO', True, np.full(2, 0.45))
        err_e, _ = e.run('ER', True, np.full(2, 0.45))
        for fam in ('sht_chain', 'sht_chain_modulus', 'sht_chain_real'):
            assert e.profile_get(fam)[1] > 0, fam
        e.profile(False)
        out = {'steps_errors': np.concatenate([err_h, err_e])}
        assert np.isfinite(out['steps_errors']).all() and (out['steps_errors'] > 0).all(), out['steps_errors']
        for b in range(B):
            out['steps_density%d' % b] = e.density(b)
            out['steps_F%d' % b] = e.reciprocal_density(b)
        return out
    finally:
        e.close()


def stored(key, a, i):
    """what the golden file keeps of array `a`, the i-th of its run, next to its digest"""
    if 'grid' in key or 'density' in key or '_F' in key:
        return sample(a, SEED + i)
    return a[0] if 'coeff' in key else a


def record(results, kind, held):
    """into the dict `held` (the contents of the golden file): digest of every array, the array or its sample"""
    for i, key in enumerate(sorted(results)):
        a = results[key]
        held['%s_%s_sha256' % (kind, key)] = digest(a)
        held['%s_%s' % (kind, key)] = stored(key, a, i)
    return held


def check(results, kind):
    """`results` against what tests/golden/chain_bits.npz holds under kind_* ('emul' or 'gpu')"""
    g = np.load(GOLDEN)
    parent = str(g['parent_commit'])
    bad = []
    for i, key in enumerate(sorted(results)):
        a = results[key]
        assert np.isfinite(a.view(np.float64)).all(), key
        gold = g['%s_%s' % (kind, key)]
        got = stored(key, a, i)
        if not np.array_equal(got, gold):
            d = np.abs(got - gold)
            bad.append('%s: %d of %d stored elements differ from commit %s, by at most %.3g' % (key, int((d > 0).sum()), d.size,
                                                                                              parent, float(d.max())))
        elif str(digest(a)) != str(g['%s_%s_sha256' % (kind, key)]):
            bad.append('%s: the stored elements agree with commit %s, the digest of the whole array does not' % (key, parent))
    assert not bad, '\n'.join(bad)
    print('%s: %d arrays bit-identical to commit %s (%s)' % (kind, len(results), parent, ', '.join(sorted(results))))


def check_fallback(lib_path):
    """L = 32 on a grid the L = 32 instantiation is not compiled for (n_theta = 66): the plan and the launcher must take a kernel
    with run-time geometry -- no phase stamps -- and the transforms must be right"""
    e, _ = PC.transforms_engine(2, 32, lib_path, n_batch=2, n_theta=66, n_phi=128)
    try:
        e._ck(e.lib.mtip_debug_chain_timing(e.ctx, None))
        e.profile(True)
        e.sht_inverse_forward(PC.cplx(np.random.default_rng(SEED), (2, 2, e.nlm)), 0)
        assert e.profile_get('sht_chain')[1] == 1
        e.profile(False)
        assert not stamps_written(e), 'the L = 32 instantiation ran on a 66 x 128 grid'
    finally:
        e.close()
    PC.check_transforms(2, 32, lib_path, seed=SEED, expect_chain=True, n_theta=66, n_phi=128)


def run_guarded(lib_path):
    """main of the child process of test_emul_chain_diet.test_no_access_past_buffer_ends: (a) at the l32 shape with
    MTIP_EMUL_GUARD=1, every device buffer followed by an inaccessible page -- a read past d_PTw or a store past the transpose
    buffers ends the process"""
    assert os.environ.get('MTIP_EMUL_GUARD') == '1'
    check(transform_results('l32', lib_path), 'emul')
    print('CHAIN_DIET_GUARDED_OK')

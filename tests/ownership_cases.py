"""Cases of tests/test_emul_ownership.py: every handle of the library (mtip_ctx, mtip2d_ctx, mtip_correlate, mtip_resample) is driven
through its allocating paths on the CPU emulator and destroyed; the emulator's count of live device allocations
(mtip_emul_live_allocations, tests/emul/emul_runtime.cpp) must then be back where it was before the handle was made.  The handles own
their device memory through DevBuf members (csrc/mtip_internal.h): a buffer that is not a DevBuf, or one that is overwritten without
being released, shows here as a count that does not return.  The sizes are the smallest the handles accept; nothing is compared with
a reference here (the parity tests do that).  Run in a child process: the engines of other tests are not collected in the middle."""
import ctypes
import gc
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def live(lib_path):
    from xframe_amd.fxs import _lib
    fn = _lib.load(lib_path).mtip_emul_live_allocations
    fn.restype = ctypes.c_longlong
    gc.collect()
    return int(fn())


def made(lib_path):
    from xframe_amd.fxs import _lib
    fn = _lib.load(lib_path).mtip_emul_total_allocations
    fn.restype = ctypes.c_longlong
    return int(fn())


def engine_case(lib_path):
    """12 shells x L4, two restarts: projection data set twice, II_error / ccd_diff / fqc_error, the reciprocal l2 metric and deg2, both
    debug timers, the histories grown once, an alignment and an averaging operator.
    The histories hold 4096 steps.  A step of this size takes 0.13 s on the emulator, 4097 of them nine minutes, so the growth is asked
    for without running them: a group run of 4097 steps whose second member has no state is refused before anything is enqueued
    (mtip_run_group_async: every check comes before the first launch), after the first member's prelude has grown its histories for
    the steps asked for -- all five of them, with the rows of the steps done so far copied over.  The steps after it write into the
    grown arrays, and the rows from before it are read back unchanged."""
    import torch
    from helpers import OracleTransforms, golden_settings
    from oracle.fourier import FourierPair
    from oracle.sht import SHT
    from xframe_amd.fxs import _lib, synthetic as S
    from xframe_amd.fxs.engine import METHOD_ID, Engine
    N, L, B = 12, 4, 2
    data, rho = S.make_invariants(OracleTransforms(FourierPair(SHT(L), N, S.data_cutoff(N), 2.0)), N, L)
    data['xray_wavelength'] = 1.23984
    calc = ['II_error', 'ccd_diff', 'fqc_error', 'l2_projection_diff', 'deg2_invariant_l2_diff']
    opt = golden_settings(N, L, {'main_loop': {'error': {'methods': {'reciprocal': {'calculate': calc, 'ccd_diff': {'C_order': 2}}}}}})
    e = Engine(opt, data, n_batch=B, lib_path=lib_path)
    assert e.reciprocal_l2 and e.deg2_enabled and len(e.invariant_metrics) == 3
    e._ck(e.lib.mtip_debug_polar_timing(e.ctx, None))
    e._ck(e.lib.mtip_debug_chain_timing(e.ctx, None))
    for b in range(B):
        e.set_density(b, rho)
    e.init_state()
    e.run('HIO', True, np.full(3, 0.5))                                 # builds the order list, the tile lists and the real projection's tables
    e._setup_projections(data)                                          # ... which the second upload of the projection data drops
    before, _ = e.fetch_errors(0, 3)
    blocks = live(lib_path)
    stateless = Engine(opt, data, n_batch=B, lib_path=lib_path)        # never initialised: the group run below stops at it
    betas = np.full(4097, 0.5)
    group = (ctypes.c_void_p * 2)(e.ctx, stateless.ctx)
    made_before = made(lib_path)
    assert e.lib.mtip_run_group_async(group, 2, METHOD_ID['ER'], 1, len(betas), _lib.ptr(betas)) != 0
    assert b'mtip_init_state' in e.lib.mtip_last_error(stateless.ctx)
    assert made(lib_path) - made_before == 5                            # the growth happened: error, main, deg2, l2 and invariant histories
    stateless.close()
    assert live(lib_path) == blocks                                     # ... replaced: none added, none lost
    err, deg2 = e.run('ER', True, np.full(2, 0.5))
    assert np.isfinite(err).all() and np.isfinite(deg2).all()
    assert np.array_equal(e.fetch_errors(0, 3)[0], before)
    rng = np.random.default_rng(0)
    coeff = rng.normal(size=(B, N, e.nlm)) + 1j * rng.normal(size=(B, N, e.nlm))
    assert np.isfinite(e.so3_correlation(coeff[0], coeff)).all()
    stack = torch.from_numpy(rng.normal(size=(3,) + e.shape) + 0j)
    assert e.t_grid_stats(stack).shape == (3, 12)
    e.close()


def mtip2d_case(lib_path):
    """the resident 2-D loop at the size of fixture G20 (12 shells, M = 6) with deg2_invariant_l2_diff, then the per-order tables a
    second time (projection, metric tables, state)"""
    import parity_cases as PC
    from xframe_amd.fxs.reconstruct2d import MTIP2D
    g = np.load(os.path.join(HERE, 'golden', 'mtip2d_N12_M6.npz'))
    gv = np.load(os.path.join(HERE, 'golden', 'mtip2d_variants_N12_M6.npz'))
    data, o, _ = PC.mtip2d_variant_problem(g, gv, 'recip_deg2')
    m = MTIP2D(o, data, n_restarts=2, initial_densities=[g['rho0'], g['rho0']], lib_path=lib_path, resident=True)
    assert len(m.phasing_loop()) == 2
    e, rs_ = m.engine, m.rsetup
    e.set_projection(rs_.projection_matrices, rs_.used_orders, rs_.radial_mask, rs_.number_of_particles)
    e.set_reciprocal_metrics(m._deg2_ref, m._deg2_norm)
    e.init_state()
    e.run('HIO', True, np.full(3, 0.5))
    m.close()


def correlate_case(lib_path):
    """4 rings x 16 angles: a handle with the shared mask's table, then one with the average_sigma filter's work array"""
    import ccextract_cases as CC
    import correlate_cases as CO
    from xframe_amd.fxs import correlate as CR
    n_q, n_phi, P = 4, 16, 3
    images, masks = CO.make_patterns(n_q, n_phi, P, 5)
    e = CC.small_engine(lib_path)
    c = CR.Correlator(e, CO.make_settings(n_q, n_phi), shared_mask=True)
    assert c.shared_mask
    c.add(images * masks[0], masks[0])
    c.finalize()
    c.close()
    c = CR.Correlator(e, CO.make_settings(n_q, n_phi, filter=2.0))
    c.add(images[:1], masks[:1]).add(images[1:], masks[1:])
    assert c.num_patterns == P
    c.close()
    e.close()


def resample_case(lib_path):
    """8 x 8 frames, order 3: the static mask's arrays, then the per-pattern ones on the same handle, then add_detector (the
    correlator's own resampler and the patterns between the two stages)"""
    import ccextract_cases as CC
    import resample_cases as RC
    from xframe_amd.fxs import correlate as CR
    H, W, n_q, n_phi, P = 8, 8, 4, 16, 3
    images, masks, binary, background = RC.make_frames(H, W, P, 11, np.float64)
    settings = RC.detector_settings(H, W, n_q, n_phi, interpolation_order=3, use_binary_mask=True, subtract_background=True)
    e = CC.small_engine(lib_path)
    rs = CR.Resampler(e, settings, binary_mask=binary, background=background)
    rs.run(images)
    rs.run(images)                                                      # (the static mask is set up once)
    rs.run(images, masks)
    rs.close()
    c = CR.Correlator(e, settings, binary_mask=binary, background=background)
    c.add_detector(images[:1]).add_detector(images[1:], masks[1:])
    assert c.num_patterns == P
    c.close()
    e.close()


CASES = (engine_case, mtip2d_case, correlate_case, resample_case)


def run_all(lib_path):
    np.seterr(all='ignore')
    import ccextract_cases as CC
    start = live(lib_path)
    e = CC.small_engine(lib_path)
    assert live(lib_path) > start                                       # (the counter counts)
    e.close()
    assert live(lib_path) == start
    for case in CASES:
        case(lib_path)
        after = live(lib_path)
        print('OWNERSHIP %s live=%d' % (case.__name__, after), flush=True)
        assert after == start, (case.__name__, 'device allocations left behind', after - start)

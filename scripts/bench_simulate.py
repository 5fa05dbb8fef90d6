"""GPU: B_l -> C(q1, q2, Delta) (Engine.deg2_to_cc, csrc/k_simulate.h) and the worker flow simulate_ccd around it, at 256 x L63 (the
reference's default), 128 x L32 and 512 x L128 (the tutorial's size: the operator here, the flow with --tutorial).
Per size, after a warm-up, five windows each (median, min .. max):
  (a) the kernel (event bracket of the family `deg2_cc`) with B_l and the output in HBM, for back_substitution and for lstsq on the
      worker's angular grid, beside the time the output write alone (and output + B_l read) takes at 8 TB/s: the floor;
      and the whole call on a device tensor (table set-up, upload and synchronise included);
  (b) the call with host arrays (copies in and out included);
  (c) the numpy restatement of the route on this host, as context, and the device against it;
  (d) the flow simulate_ccd(settings) from the shapes to cc_data (engine set-up included), where the engine takes the size.
  (e) --tutorial: the flow at the settings of the reference's settings/simulate_ccd/tutorial.yaml (512 shells, max_order 128, max_q
      0.322416, its six spheres = the default shapes, back_substitution), run twice (13 GB of device memory, host arrays of 1 GB),
      the first with the one-off Hankel weights, the second with them cached; beside it the host's Legendre table of the back half.
usage: python scripts/bench_simulate.py [--once NQ L MODE | --tutorial]     (--once: one call on a device tensor, for a profiler run)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
np.seterr(all='ignore')
import torch                                        # noqa: E402
from xframe_amd.fxs import simulate_ccd as SIM      # noqa: E402
from xframe_amd.fxs.engine import Engine            # noqa: E402

WAVELENGTH = 1.23984
HBM_PEAK = 8e12


def problem(nq, L, seed=0):
    rng = np.random.default_rng(seed)
    qs = (np.arange(nq) + 0.5) * (0.9 / nq)
    bl = (rng.standard_normal((L + 1, nq, nq)) + 1j * rng.standard_normal((L + 1, nq, nq))) * np.exp(-0.05 * np.arange(L + 1))[:, None, None]
    return qs, bl, np.arange(2 * L) * np.pi / L


def stats(v):
    v = np.sort(np.asarray(v))
    return '%.3f ms (min %.3f .. max %.3f)' % (1e3 * np.median(v), 1e3 * v[0], 1e3 * v[-1])


def windows(e, fn, reps):
    """five windows of `reps` calls: (kernel seconds per call, wall seconds per call)"""
    for _ in range(3):
        fn()
    kern, call = [], []
    for _ in range(5):
        e.profile(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        call.append((time.perf_counter() - t0) / reps)
        ms, n = e.profile_get('deg2_cc')
        assert n == reps, n
        kern.append(1e-3 * ms / n)
        e.profile(False)
    return kern, call


TUTORIAL = {'grid': {'max_q': 0.322416, 'n_radial_points': 512, 'max_order': 128},
            'cross_correlation': {'method': 'back_substitution', 'xray_wavelength': WAVELENGTH}}


def tutorial_flow():
    for i in range(2):
        t0 = time.perf_counter()
        res = SIM.simulate_ccd(TUTORIAL)
        t1 = time.perf_counter()
        cc = res.cc_data['cross_correlation']['I1I1']
        print('  (e) simulate_ccd at the tutorial\'s settings, run %d: %.1f s; grid %s, B_l %s, cc %s, integrated intensity %.6e'
              % (i + 1, t1 - t0, res.density.shape, res.cc_data['deg_2_invariant']['I1I1'].shape, cc.shape, res.integrated_intensity))
        assert np.isfinite(cc).all()
    t0 = time.perf_counter()
    SIM.legendre_table_t(res.cc_data['radial_points'], WAVELENGTH, 128)
    print('      of which the Legendre table of the back half, on the host in every run: %.1f s (the Hankel weights are computed in the '
          'first run and kept by hostsetup for the second)' % (time.perf_counter() - t0))


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bench_simulate needs a GPU: a timing without one measures nothing')
    if len(sys.argv) > 1 and sys.argv[1] == '--tutorial':
        return tutorial_flow()
    e = Engine({'grid': {'n_radial_points': 8, 'max_order': 2}}, None, n_batch=1, max_q=1.0)
    if len(sys.argv) > 1 and sys.argv[1] == '--once':
        nq, L, mode = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
        qs, bl, phis = problem(nq, L)
        d = torch.from_numpy(bl).cuda()
        SIM.deg2_invariant_to_cc(e, d, WAVELENGTH, {'qs': qs, 'phis': phis}, mode=mode)
        torch.cuda.synchronize()
        print('one call at %d x L%d, %s' % (nq, L, mode))
        e.close()
        return
    import simulate_cases as SC
    for nq, L, flow, rest_lsq in ((256, 63, True, True), (128, 32, True, True), (512, 128, False, False)):
        qs, bl, phis = problem(nq, L)
        grid = {'qs': qs, 'phis': phis}
        d = torch.from_numpy(bl).cuda()
        bl_bytes = 16.0 * (L + 1) * nq * nq
        print('%d x L%d x %d angles (B_l %.1f MB)' % (nq, L, 2 * L, bl_bytes / 1e6))
        for mode, item in (('back_substitution', 8.0), ('lstsq', 16.0)):
            out_bytes = item * nq * nq * 2 * L
            kern, call = windows(e, lambda: SIM.deg2_invariant_to_cc(e, d, WAVELENGTH, grid, mode=mode), 10)
            k = float(np.median(kern))
            print('  %s: output %.1f MB; write floor at 8 TB/s %.3f ms, with the read of B_l %.3f ms' %
                  (mode, out_bytes / 1e6, 1e3 * out_bytes / HBM_PEAK, 1e3 * (out_bytes + bl_bytes) / HBM_PEAK))
            print('    (a) kernel, operands in HBM          : %s = %.1f x the write floor' % (stats(kern), k * HBM_PEAK / out_bytes))
            print('        call on a device tensor          : %s' % stats(call))
            host = []
            SIM.deg2_invariant_to_cc(e, bl, WAVELENGTH, grid, mode=mode)
            for _ in range(5):
                t0 = time.perf_counter()
                cc = SIM.deg2_invariant_to_cc(e, bl, WAVELENGTH, grid, mode=mode)
                host.append(time.perf_counter() - t0)
            print('    (b) call with host arrays, copies in : %s' % stats(host))
            if mode == 'back_substitution' or rest_lsq:
                t0 = time.perf_counter()
                ref = SC.r_back_substitution(bl, qs) if mode == 'back_substitution' else SC.r_lstsq(bl, qs, phis)
                t1 = time.perf_counter()
                print('    (c) numpy restatement on this host   : %.0f ms; device vs it, whole-array rel-L2 %.1e' %
                      (1e3 * (t1 - t0), np.linalg.norm(cc - ref) / np.linalg.norm(ref)))
                del ref
            del cc
        del d
        if flow:
            opt = {'grid': {'n_radial_points': nq, 'max_order': L}}
            SIM.simulate_ccd(opt)
            t = []
            for _ in range(5):
                t0 = time.perf_counter()
                res = SIM.simulate_ccd(opt)
                t.append(time.perf_counter() - t0)
            print('  (d) simulate_ccd, shapes -> cc_data (default shapes, grid %s): %s' % (res.density.shape, stats(t)))
    e.close()


if __name__ == '__main__':
    main()

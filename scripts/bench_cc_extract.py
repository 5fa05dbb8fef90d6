"""GPU: cross-correlation -> B_l (Engine.cc_to_deg2, csrc/k_extract.hip) at 512 x L68 x 1024 and 256 x L32 x 512.
Per size, five windows each (median, min .. max):
  (a) the kernel (event bracket of the family `cc_deg2`) with the input already in HBM, against the algorithmic bytes
      8 Nq^2 n_delta as a fraction of 8 TB/s; and the whole call on a device tensor (table upload and synchronise included);
  (b) the call with a host array in (copy to the device and B_l back included);
  (c) the numpy restatement of the route on this host, as context.
usage: python scripts/bench_cc_extract.py [--lib PATH] [--once NQ L ND | --wide]
       --once: one call on a device tensor, for a profiler run:
       rocprofv3 --kernel-trace --stats -- python ..., and rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE runs of their own; per launch
       of k_cc_deg2 divide 2 x FETCH_SIZE KiB (gfx950 tallies 128-byte reads at 64) by 8 Nq^2 n_delta and WRITE_SIZE KiB by
       16 (L + 1) Nq^2
       --wide: the kernel beyond 64 extracted orders (mtip_op_cc_to_deg2_wide, k_cc_deg2<HM>) at 512 shells x 256 angles, the size of
       simulate_ccd's tutorial output: 64 orders through the narrow entry (HM = 1), 65 (HM = 2) and 129 (HM = 3) through the wide
       one, the time per extracted order, and the split contraction / back-substitution from the dimensions = 2 run of the same
       data; the 512 x L68 x 1024 row of (a) through the narrow entry for comparison with other builds
       --lib PATH: another build of libmtip_hip.so (from a build without the wide entry --wide times the narrow rows only)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
np.seterr(all='ignore')
import torch                                        # noqa: E402
from xframe_amd.fxs import extract as X             # noqa: E402
from xframe_amd.fxs.engine import Engine            # noqa: E402

WAVELENGTH = 1.23984
HBM_PEAK = 8e12


def problem(nq, L, nd, seed=0, stride=2):
    rng = np.random.default_rng(seed)
    qs = (np.arange(nq) + 0.5) * (0.9 / nq)
    cc = rng.standard_normal((nq, nq, nd)) * np.exp(-np.arange(nd) / nd)[None, None, :]
    return qs, cc, X.legendre_table(qs, WAVELENGTH, L, stride)


def stats(v):
    v = np.sort(np.asarray(v))
    return '%.3f ms (min %.3f .. max %.3f)' % (1e3 * np.median(v), 1e3 * v[0], 1e3 * v[-1])


def kernel_windows(e, call, reps=20, windows=5):
    """seconds per launch of the family `cc_deg2`, one figure per window of `reps` calls"""
    for _ in range(3):
        call()
    kern = []
    for _ in range(windows):
        e.profile(True)
        torch.cuda.synchronize()
        for _ in range(reps):
            call()
        torch.cuda.synchronize()
        ms, n = e.profile_get('cc_deg2')
        assert n == reps, n
        kern.append(1e-3 * ms / n)
        e.profile(False)
    return kern


def wide_table(e, have_wide):
    """the rows of --wide; without the wide entry (another build) only the narrow rows"""
    nq, nd = 512, 256
    rows = [('L = 126, stride 2', 126, 2, False, 1)]
    if have_wide:
        rows += [('L = 128, stride 2', 128, 2, True, 2), ('L = 128, stride 1', 128, 1, True, 3)]
    print('%d shells x %d angles (input %.1f MB); kernel k_cc_deg2<HM>, input in HBM, five windows of 20 launches' % (nq, nd, 8e-6 * nq * nq * nd))
    for name, L, stride, wide, hm in rows:
        qs, cc, leg = problem(nq, L, nd, stride=stride)
        d = torch.from_numpy(cc).cuda()
        kw = {'wide': True} if wide else {}
        full = kernel_windows(e, lambda: e.cc_to_deg2(d, L, stride, 3, legendre=leg, **kw))
        flat = kernel_windows(e, lambda: e.cc_to_deg2(d, L, stride, 2, **kw))
        n_m = L // stride + 1
        k3, k2 = float(np.median(full)), float(np.median(flat))
        print('  %s, %s entry, %3d orders, HM = %d: %s = %.2f us per order; dimensions 2 (contraction) %s, back-substitution %.3f ms' %
              (name, 'wide' if wide else 'narrow', n_m, hm, stats(full), 1e6 * k3 / n_m, stats(flat), 1e3 * (k3 - k2)))
        del d
    nq, L, nd = 512, 68, 1024
    qs, cc, leg = problem(nq, L, nd)
    d = torch.from_numpy(cc).cuda()
    kern = kernel_windows(e, lambda: e.cc_to_deg2(d, L, 2, 3, legendre=leg))
    print('%d x L%d x %d, narrow entry, HM = 1: %s' % (nq, L, nd, stats(kern)))


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bench_cc_extract needs a GPU: a timing without one measures nothing')
    args = sys.argv[1:]
    lib_path = None
    if '--lib' in args:
        i = args.index('--lib')
        lib_path = args[i + 1]
        del args[i:i + 2]
    e = Engine({'grid': {'n_radial_points': 8, 'max_order': 2}}, None, n_batch=1, max_q=1.0, lib_path=lib_path)
    if args and args[0] == '--wide':
        wide_table(e, hasattr(e.lib, 'mtip_op_cc_to_deg2_wide'))
        e.close()
        return
    if args and args[0] == '--once':
        nq, L, nd = (int(x) for x in args[1:4])
        qs, cc, leg = problem(nq, L, nd)
        d = torch.from_numpy(cc).cuda()
        e.cc_to_deg2(d, L, 2, 3, legendre=leg)
        torch.cuda.synchronize()
        print('one call at %d x L%d x %d: input %.1f MB, B_l %.1f MB' % (nq, L, nd, 8e-6 * nq * nq * nd, 16e-6 * (L + 1) * nq * nq))
        e.close()
        return
    for nq, L, nd in ((512, 68, 1024), (256, 32, 512)):
        qs, cc, leg = problem(nq, L, nd)
        d = torch.from_numpy(cc).cuda()
        bytes_in = 8.0 * nq * nq * nd
        reps = 20
        for _ in range(3):
            e.cc_to_deg2(d, L, 2, 3, legendre=leg)
        kern, call = [], []
        for _ in range(5):
            e.profile(True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                e.cc_to_deg2(d, L, 2, 3, legendre=leg)
            torch.cuda.synchronize()
            call.append((time.perf_counter() - t0) / reps)
            ms, n = e.profile_get('cc_deg2')
            assert n == reps, n
            kern.append(1e-3 * ms / n)
            e.profile(False)
        k = float(np.median(kern))
        print('%d x L%d x %d (input %.1f MB, B_l %.1f MB)' % (nq, L, nd, bytes_in / 1e6, 16e-6 * (L + 1) * nq * nq))
        print('  (a) kernel k_cc_deg2, input in HBM : %s -> %.2f TB/s of algorithmic bytes = %.1f %% of 8 TB/s' %
              (stats(kern), bytes_in / k / 1e12, 100 * bytes_in / k / HBM_PEAK))
        print('      call on a device tensor        : %s' % stats(call))
        host = []
        e.cc_to_deg2(cc, L, 2, 3, legendre=leg)
        for _ in range(5):
            t0 = time.perf_counter()
            b = e.cc_to_deg2(cc, L, 2, 3, legendre=leg)
            host.append(time.perf_counter() - t0)
        print('  (b) call with a host array, copies in: %s' % stats(host))
        import ccextract_cases as CC
        phis = np.arange(nd) * 2 * np.pi / nd
        t0 = time.perf_counter()
        ref, _ = CC.r_cc_to_deg2(cc, 3, qs, phis, L, True, {}, None)
        t1 = time.perf_counter()
        print('  (c) numpy restatement on this host   : %.0f ms; device vs it, whole-array rel-L2 %.1e' %
              (1e3 * (t1 - t0), np.linalg.norm(b - ref) / np.linalg.norm(ref)))
        del d
    e.close()


if __name__ == '__main__':
    main()

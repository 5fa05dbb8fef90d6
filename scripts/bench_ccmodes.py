"""GPU: the back-substitution mode psd (Engine.cm_backsub, Engine.nearest_psd, csrc/k_extract_psd.h) at 128 shells x L = 32 and
L = 64 with 256 angles, odd orders assumed zero, inputs already in HBM.  Warm, median of five (min .. max):
  (a) back_substitution_psd from C(q1, q2, Delta) on the device: the harmonics (k_cc_deg2, dimensions 2) and the elimination, host
      clock around the two calls (each ends in a stream synchronise), and the event brackets `cc_deg2` and `cm_backsub`;
  (b) the plain elimination with the Hermitian mean (qqsym) on the same harmonics, for scale;
  (c) Engine.nearest_psd for 33 matrices of 128 x 128 (event bracket `nearest_psd`);
  (d) for context: the numpy restatement of the psd mode on this host.
The split of (a) by kernel comes from a run under rocprofv3 --kernel-trace --stats of its own (--once: one warm-up and one call).
usage: python scripts/bench_ccmodes.py [--once] [--orders 32 64]"""
import argparse
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


def stats(v):
    v = np.sort(np.asarray(v))
    return '%.3f ms (min %.3f .. max %.3f)' % (1e3 * np.median(v), 1e3 * v[0], 1e3 * v[-1])


def wall(call, windows=5):
    call()
    out = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def bracket(e, names, call, windows=5):
    call()
    out = {n: [] for n in names}
    for _ in range(windows):
        e.profile(True)
        call()
        torch.cuda.synchronize()
        for n in names:
            ms, count = e.profile_get(n)
            out[n].append(1e-3 * ms / max(count, 1))
        e.profile(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--once', action='store_true', help='one warm-up and one psd call per size, nothing else (for a kernel trace)')
    ap.add_argument('--orders', type=int, nargs='+', default=[32, 64])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ccmodes needs a GPU: a timing without one measures nothing')
    import ccmodes_cases as QC
    import ccmodes_reference as R
    nq, nd = 128, 256
    e = Engine({'grid': {'n_radial_points': 8, 'max_order': 2}}, None, n_batch=1, max_q=1.0)
    for L in args.orders:
        qs, phis, cc, avg = QC.modes_cc(nq, L, nd, 31, 2)
        d_cc = torch.from_numpy(cc).cuda()
        leg1, leg2 = X.legendre_table(qs, WAVELENGTH, L, 1), X.legendre_table(qs, WAVELENGTH, L, 2)
        wide = X._wants_wide_entry(L, 1)

        def psd():
            cm = e.cc_to_deg2(d_cc, L, order_stride=1, dimensions=2, wide=wide)
            return e.cm_backsub(cm, leg1, order_stride=2, mode='psd')
        if args.once:
            psd()
            psd()
            continue
        b, info = psd()
        print('%d x L%d x %d, zero odd orders: eigenvalues clipped per step, min %d max %d' % (nq, L, nd, info.min(), info.max()))
        print('  (a) back_substitution_psd, harmonics + elimination : %s' % stats(wall(psd)))
        t = bracket(e, ('cc_deg2', 'cm_backsub'), psd)
        print('      bracket cc_deg2 (k_cc_deg2, dimensions 2)       : %s' % stats(t['cc_deg2']))
        print('      bracket cm_backsub (%d steps)                   : %s' % (L + 1, stats(t['cm_backsub'])))
        cm = e.cc_to_deg2(d_cc, L, order_stride=1, dimensions=2, wide=wide)
        t = bracket(e, ('cm_backsub',), lambda: e.cm_backsub(cm, leg2, order_stride=2, mode='plain', hermitian_mean=True))
        print('  (b) cm_backsub plain + Hermitian mean (qqsym)       : %s' % stats(t['cm_backsub']))
        if L <= 32:
            t0 = time.perf_counter()
            ref, _, _ = R.cc_to_deg2(R.MODES[2], cc, qs, phis, L, True, {}, avg)
            dt = time.perf_counter() - t0
            err = np.linalg.norm(b.cpu().numpy() - ref) / np.linalg.norm(ref)
            print('  (d) numpy restatement on this host                  : %.1f ms; device vs it %.2e' % (1e3 * dt, err))
    if not args.once:
        rng = np.random.default_rng(3)
        stack = rng.normal(size=(33, 128, 128)) + 1j * rng.normal(size=(33, 128, 128))
        d_stack = torch.from_numpy(stack).cuda()
        t = bracket(e, ('nearest_psd',), lambda: e.nearest_psd(d_stack))
        print('  (c) nearest_psd, 33 matrices of 128 x 128           : %s' % stats(t['nearest_psd']))
    e.close()


if __name__ == '__main__':
    main()

"""GPU: the conditioning operators of `extract` (Engine.cc_lowpass_q / cc_harmonic_filter / cc_binned_mean, csrc/k_extract_cond.h) at
256 x 256 x 1536 (what `correlate` delivers by default, 805 MB) and at 64 x 64 x 1536, inputs already in HBM, and the second kernel of
Engine.cc_lstsq_deg2_minnorm.  Per operator: the median of five windows of event-bracketed kernel time (min .. max), the bytes the
algorithm has to move (computed here from the shapes) over that time as a share of the achievable HBM rate, and the time of the
reference's own numpy / scipy call on this host (fxs_invariant_tools.py:248-263, 308-332), once.
  (a) k_cc_lowpass x 2 (bracket `cc_lowpass`): reads and writes the array once per axis
  (b) k_cc_harmonic_filter (bracket `cc_harmonic`): max_order 128 with and without zero_odd (129 / 65 kept harmonics), and
      k_cc_half_shift (zero_odd alone)
  (c) k_cc_binned_mean (bracket `cc_binned_mean`): max_order 69 -> 138 bins, a quarter of the samples masked
  (d) k_cc_lstsq<NT, true> (bracket `cc_lstsq_minnorm`) at 64 x 64 x 1536: 256 pairs with three samples fewer than orders, 33 and 64
      orders: time per deficient pair, beside numpy.linalg.lstsq per pair on this host and the worst deviation from it
usage: python scripts/bench_cccond.py [--small-only | --minnorm-only]"""
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
HBM_ACHIEVABLE = 6.3e12                             # bytes / s: what a streaming copy reaches on the MI355X (8.0e12 on the data sheet)


def stats(v):
    v = np.sort(np.asarray(v))
    return '%.3f ms (min %.3f .. max %.3f)' % (1e3 * np.median(v), 1e3 * v[0], 1e3 * v[-1])


def kernel_time(e, name, call, reps=3, windows=5):
    call()
    out = []
    for _ in range(windows):
        e.profile(True)
        for _ in range(reps):
            call()
        torch.cuda.synchronize()
        ms, n = e.profile_get(name)
        assert n == reps, (name, n)
        out.append(1e-3 * ms / n)
        e.profile(False)
    return out


def report(label, times, nbytes, host_seconds):
    t = float(np.median(times))
    print('  %-46s: %s; %.2f GB moved -> %.2f TB/s = %.0f %% of the achievable HBM rate; reference on this host %.2f s'
          % (label, stats(times), nbytes / 1e9, nbytes / t / 1e12, 100 * nbytes / t / HBM_ACHIEVABLE, host_seconds), flush=True)


def host_time(call):
    t0 = time.perf_counter()
    call()
    return time.perf_counter() - t0


def r_harmonic(cc, max_order, zero_odd):
    n = cc.shape[-1]
    c = np.fft.rfft(cc) / n
    if max_order is not None:
        c[..., max_order + 1:] = 0
    if zero_odd:
        c[..., 1::2] = 0
    return np.fft.irfft(c * n, n)


def r_binned(cc, mask, phis, max_order):
    step = np.pi / max_order
    ids = (phis + step / 2) // step
    n_roll = int(np.sum(ids == 2 * max_order))
    ids[ids == 2 * max_order] = 0
    ccr, mr, idr = np.roll(cc, n_roll, axis=-1), np.roll(mask, n_roll, axis=-1), np.roll(ids, n_roll)
    ccr[~mr] = 0.0
    split = np.where(np.roll(idr, 1) != idr)[0]
    new, cnt = np.add.reduceat(ccr, split, axis=-1), np.add.reduceat(mr, split, axis=-1)
    nz = cnt != 0
    new[nz] /= cnt[nz]
    return new, nz


def conditioning(e, nq, nd):
    from scipy.signal import butter, sosfilt
    rng = np.random.default_rng(nq)
    cc = rng.standard_normal((nq, nq, nd)) + 5.0
    mask = rng.random((nq, nq, nd)) > 0.25
    phis = np.arange(nd) * 2 * np.pi / nd
    n = cc.size
    print('%d x %d x %d float64 (%.0f MB)' % (nq, nq, nd, 8 * n / 1e6), flush=True)
    d_cc, d_mask = torch.from_numpy(cc).cuda(), torch.from_numpy(mask).cuda()
    sos = butter(1, 0.2 * nq, 'lp', fs=nq, output='sos')
    t = kernel_time(e, 'cc_lowpass', lambda: e.cc_lowpass_q(d_cc, sos))
    h = host_time(lambda: sosfilt(sos, sosfilt(sos, cc, axis=0), axis=1))
    report('(a) k_cc_lowpass, both axes', t, 4 * 8 * n, h)
    for label, mo, zo in (('(b) k_cc_harmonic_filter, 129 harmonics', 128, False), ('    k_cc_harmonic_filter, 65 even harmonics', 128, True),
                          ('    k_cc_half_shift (zero_odd alone)', None, True)):
        t = kernel_time(e, 'cc_harmonic', lambda: e.cc_harmonic_filter(d_cc, max_order=mo, zero_odd=zo))
        h = host_time(lambda: r_harmonic(cc, mo, zo))
        report(label, t, 2 * 8 * n, h)
    mo = 69
    bin_start, n_roll, _ = X.binned_mean_tables(phis, mo)
    t = kernel_time(e, 'cc_binned_mean', lambda: e.cc_binned_mean(d_cc, d_mask, bin_start, n_roll))
    h = host_time(lambda: r_binned(cc, mask, phis, mo))
    report('(c) k_cc_binned_mean, 138 bins', t, 9 * n + 9 * nq * nq * 2 * mo, h)
    # the results the timed calls produced, against the host's, so that the times belong to right answers
    out = e.cc_harmonic_filter(d_cc[:2, :2].contiguous(), max_order=128, zero_odd=True).cpu().numpy()
    ref = r_harmonic(cc[:2, :2], 128, True)
    print('      harmonic filter vs numpy on 4 pairs: %.1e of the largest value' % (np.abs(out - ref).max() / np.abs(ref).max()), flush=True)
    del d_cc, d_mask
    torch.cuda.empty_cache()


def minimum_norm(e, nq=64, nd=1536, n_short=256):
    import ccextract_cases as CC
    import ccmask_cases as MC
    for L, stride in ((64, 2), (63, 1)):
        orders = np.arange(0, L + 1, stride)
        n = len(orders)
        qs, phis, cc, _, _ = CC.synthetic_cc(nq, L, nd, 27, stride, noise=1e-3)
        thetas = np.arccos(qs * WAVELENGTH / (4 * np.pi))
        mask = np.ones((nq, nq, nd), dtype=bool)
        rng = np.random.default_rng(n)
        short = [(int(p) // nq, int(p) % nq) for p in rng.permutation(nq * nq)[:n_short]]
        # n - 3 evenly spaced angles within [0, pi] (even orders: [0, pi / 2], P_l(x) = P_l(-x)): distinct rows of F and singular
        # values far from LAPACK's cut, so that numpy's answer is defined (tests/cccond_cases.py: check_gap)
        span = nd // 2 if stride == 1 else nd // 4
        keep = np.arange(n - 3) * (span // (n - 3))
        for i, j in short:
            mask[i, j] = False
            mask[i, j, keep] = True
        d_cc, d_mask = torch.from_numpy(cc).cuda(), torch.from_numpy(mask).cuda()
        t = kernel_time(e, 'cc_lstsq_minnorm', lambda: e.cc_lstsq_deg2_minnorm(d_cc, d_mask, orders, thetas, phis))
        t1 = kernel_time(e, 'cc_lstsq', lambda: e.cc_lstsq_deg2_minnorm(d_cc, d_mask, orders, thetas, phis))
        b, _, _, rank = (x.cpu().numpy() for x in e.cc_lstsq_deg2_minnorm(d_cc, d_mask, orders, thetas, phis))
        t0 = time.perf_counter()
        ref = [np.linalg.lstsq(MC.legendre_matrix(qs, phis, orders, i, j)[mask[i, j]], cc[i, j, mask[i, j]], rcond=None) for i, j in short[:32]]
        dt = (time.perf_counter() - t0) / 32
        err = max(np.linalg.norm(b[orders, i, j].real - r[0]) / np.linalg.norm(r[0]) for (i, j), r in zip(short, ref))
        same = all(rank[i, j] == r[2] for (i, j), r in zip(short, ref))
        gap = min(min(s / (np.finfo(float).eps * max(n, n - 3) * r[3][0]) for s in r[3]) for r in ref)
        print('  (d) k_cc_lstsq<NT, true>, %2d orders, %d pairs of %d x %d x %d with %d samples: %s = %.1f us per deficient pair (first kernel, '
              'all %d pairs: %s); numpy per pair on this host %.0f us; device vs numpy worst of 32 pairs %.1e, ranks equal: %s; smallest singular '
              'value %.0f x numpy\'s cut'
              % (n, n_short, nq, nq, nd, n - 3, stats(t), 1e6 * np.median(t) / n_short, nq * nq, stats(t1), 1e6 * dt, err, same, gap), flush=True)


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bench_cccond needs a GPU: a timing without one measures nothing')
    e = Engine({'grid': {'n_radial_points': 8, 'max_order': 2}}, None, n_batch=1, max_q=1.0)
    if '--minnorm-only' not in sys.argv:
        conditioning(e, 64, 1536)
        if '--small-only' not in sys.argv:
            conditioning(e, 256, 1536)
    minimum_norm(e)
    e.close()


if __name__ == '__main__':
    main()

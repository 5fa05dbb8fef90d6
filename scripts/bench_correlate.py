"""GPU: patterns -> C(q1, q2, Delta) (fxs.correlate.Correlator, csrc/k_correlate.h) at the reference's tutorial shape (256 rings,
n_phi = 1024, every pair of rings) and at a small one (64 rings, n_phi = 256), with a shared mask and with per-pattern masks.
Per shape and mask mode, batch sizes 1, 8 and 32: ms per pattern of Correlator.add on device tensors (host clock around calls that end
in a synchronise; five windows after a warm-up: median, min .. max), and inside the same windows the event brackets of the kernel
families corr_ring (k_corr_stats + k_corr_ring) and corr_pair (k_corr_pair).  Derived, with the counts stated where they are printed:
the achieved FFT rate of k_corr_pair against the fp64 vector peak, and the accumulator bytes per pattern against HBM.
The numpy restatement of the route (tests/correlate_cases.r_correlate) on this host with 1 and with 8 processes, as context.
usage: python scripts/bench_correlate.py [--small] [--n-phi N [--rings R]] [--any-n-phi] [--filter KIND] [--batch B]
  --small       the small shape only
  --filter KIND the radial pixel filter: none (default), average_sigma (k_corr_stats) or median_mad (k_corr_stats_mad,
                csrc/k_ringfilter.h; Correlator(..., median_mad=True)), each at 3 sigmas / MADs.  With a filter 4 % of the samples are
                outliers, the masks are per pattern (a filter makes them so) and the statistics kernel's own event bracket (family
                corr_stats, one launch per chunk of 32 patterns) is printed per launch.
  --batch B     that batch size only
  --n-phi N     one shape only: R rings (default 256) x N angles.  A length the radix-2 kernels do not take (1536, the default settings'
                length, 1920, 2000, 2048 ..) goes through a handle made with general_n_phi=True (k_corr_pair_g, csrc/k_correlate_mr.h);
                the operation count 5 m log2 m is kept for it as the convention the rates are stated in.
  --any-n-phi   the handles are made with any_n_phi=True: every even N in 16 .. 2048; a length with a prime factor above 5 (1256, 2042 ..)
                runs the chirp-z kernels (k_corr_pair_b, csrc/k_correlate_bs.h), every other length the kernels it runs without the
                switch.  The FFT rate is still stated in 5 m log2 m per transform, not in the convolution's own operations."""
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
np.seterr(all='ignore')

HBM_PEAK = 8e12
FP64_VECTOR_PEAK = 78e12
BATCHES = (1, 8, 32)


FILTERS = ('none', 'average_sigma', 'median_mad')


def settings_for(n_q, n_phi, filt='none'):
    import correlate_cases as CO
    s = CO.make_settings(n_q, n_phi, q_step=2.0 ** -10, q_min=2.0 ** -10)
    if filt != 'none':
        s['intensity_radial_pixel_filter'] = [True, [filt, 3]]
    return s


def patterns(n_q, n_phi, P, seed=0, outliers=False):
    rng = np.random.default_rng(seed)
    masks = (rng.random((P, n_q, n_phi)) < 0.85).astype(np.uint8)
    images = (200.0 * (1.0 + 0.4 * rng.random((P, n_q, n_phi)))) * masks
    if outliers:
        images[rng.random(images.shape) < 0.04] *= 2.5
    return images, masks


def pair_flops(n_q1, n_q2, n_phi, shared):
    """per pattern: (2 or 1) inverse real transforms per pair, each one complex FFT of m = n_phi / 2 points (5 m log2 m) plus the
    spectrum product and the even / odd fold (24 m)"""
    m = n_phi // 2
    return n_q1 * n_q2 * (1 if shared else 2) * (5.0 * m * np.log2(m) + 24.0 * m)


def stats(v):
    v = np.sort(np.asarray(v))
    return '%8.3f ms (min %.3f .. max %.3f)' % (np.median(v), v[0], v[-1])


def _cpu_worker(args):
    n_q, n_phi, P, seed = args
    import correlate_cases as CO
    prm = CO.params(settings_for(n_q, n_phi))
    images, masks = patterns(n_q, n_phi, P, seed)
    t0 = time.perf_counter()
    CO.r_correlate(images, masks, prm)
    return time.perf_counter() - t0


def cpu_context(n_q, n_phi, P):
    t1 = _cpu_worker((n_q, n_phi, P, 1))
    t0 = time.perf_counter()
    with mp.get_context('spawn').Pool(8) as pool:
        pool.map(_cpu_worker, [(n_q, n_phi, P, 10 + i) for i in range(8)])
    t8 = time.perf_counter() - t0
    print('  numpy restatement on this host: 1 process %.1f ms per pattern; 8 processes (%d patterns each, pool start included) '
          '%.1f ms per pattern' % (1e3 * t1 / P, P, 1e3 * t8 / (8 * P)))


def main():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_correlate needs a GPU: a timing without one measures nothing')
    from xframe_amd.fxs import correlate as CR
    from xframe_amd.fxs.engine import Engine
    e = Engine({'grid': {'n_radial_points': 8, 'max_order': 2}}, None, n_batch=1, max_q=1.0)
    shapes = ((64, 256),) if '--small' in sys.argv else ((256, 1024), (64, 256))
    filt = sys.argv[sys.argv.index('--filter') + 1] if '--filter' in sys.argv else 'none'
    if filt not in FILTERS:
        raise SystemExit('--filter takes one of ' + ', '.join(FILTERS))
    batches = (int(sys.argv[sys.argv.index('--batch') + 1]),) if '--batch' in sys.argv else BATCHES
    any_n_phi = '--any-n-phi' in sys.argv
    if '--n-phi' in sys.argv:
        rings = int(sys.argv[sys.argv.index('--rings') + 1]) if '--rings' in sys.argv else 256
        shapes = ((rings, int(sys.argv[sys.argv.index('--n-phi') + 1])),)
    for n_q, n_phi in shapes:
        settings = settings_for(n_q, n_phi, filt)
        general = n_phi not in CR.SUPPORTED_N_PHI and not any_n_phi
        route = ' (any_n_phi)' if any_n_phi else ' (general_n_phi: mixed-radix kernels)' if general else ''
        images, masks = patterns(n_q, n_phi, max(batches), outliers=filt != 'none')
        d_img = torch.from_numpy(images).cuda()
        d_mask = torch.from_numpy(masks).cuda()
        n_acc = n_q * n_q * n_phi
        print('%d rings x %d angles%s, %d x %d pairs: accumulator %.1f MB (sum f64 + count int32), shared-mask table %.1f MB' %
              (n_q, n_phi, route, n_q, n_q, 12e-6 * n_acc, 8e-6 * n_acc))
        if filt != 'none':
            print('  intensity_radial_pixel_filter: %s, 3' % filt)
        for shared in ((True, False) if filt == 'none' else (False,)):
            per_pattern = {}
            for B in batches:
                c = CR.Correlator(e, settings, shared_mask=shared, general_n_phi=general, any_n_phi=any_n_phi, median_mad=filt == 'median_mad')
                m = d_mask[0] if shared else d_mask[:B]
                t0 = time.perf_counter()
                c.add(d_img[:B], m)                                    # warm-up (code objects, the shared mask's table)
                c.add(d_img[:B], m)
                torch.cuda.synchronize()
                one = (time.perf_counter() - t0) / 2
                reps = int(min(64, max(2, round(0.4 / max(one, 1e-4)))))
                wall, ring, pair, stat = [], [], [], []
                for _ in range(5):
                    e.profile(True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        c.add(d_img[:B], m)
                    torch.cuda.synchronize()
                    wall.append(1e3 * (time.perf_counter() - t0) / (reps * B))
                    r_ms, _ = e.profile_get('corr_ring')
                    p_ms, n = e.profile_get('corr_pair')
                    assert n == reps, (n, reps)
                    ring.append(r_ms / (reps * B))
                    pair.append(p_ms / (reps * B))
                    s_ms, s_n = e.profile_get('corr_stats')
                    stat.append(s_ms / max(s_n, 1))
                    e.profile(False)
                c.close()
                per_pattern[B] = float(np.median(wall))
                k = 1e-3 * float(np.median(pair))
                fl = pair_flops(n_q, n_q, n_phi, shared)
                acc_bytes = (24.0 + (8.0 if shared else 0.0)) * n_acc / B
                print('  %s mask, batch %2d (%2d calls per window): add %s per pattern' % ('shared     ' if shared else 'per-pattern', B, reps,
                                                                                         stats(wall)))
                print('      k_corr_pair %s | k_corr_stats + k_corr_ring %s per pattern' % (stats(pair), stats(ring)))
                if filt != 'none':
                    print('      %s alone: %s per launch of %d patterns x %d rings' %
                          ('k_corr_stats_mad' if filt == 'median_mad' else 'k_corr_stats', stats(stat), min(B, 32), n_q))
                print('      k_corr_pair: %.2f GFLOP of FFT per pattern -> %.2f TFLOP/s = %.1f %% of the fp64 vector peak (78 TFLOP/s); '
                      'accumulator traffic %.1f MB per pattern = %.3f ms at 8 TB/s (%.1f %% of the kernel time)' %
                      (1e-9 * fl, 1e-12 * fl / k, 100 * fl / k / FP64_VECTOR_PEAK, 1e-6 * acc_bytes, 1e3 * acc_bytes / HBM_PEAK,
                       100 * acc_bytes / HBM_PEAK / k))
            if batches == BATCHES:
                print('  %s mask: ms per pattern at batch 1 / 8 / 32 = %.3f / %.3f / %.3f  (batch 32 below batch 1: %s)' %
                      ('shared' if shared else 'per-pattern', per_pattern[1], per_pattern[8], per_pattern[32],
                       per_pattern[32] < per_pattern[1]))
        del d_img, d_mask
        if '--n-phi' not in sys.argv and filt == 'none' and batches == BATCHES:   # (else the device figures alone are asked for)
            cpu_context(n_q, n_phi, 1 if n_q >= 256 else 8)
    e.close()


if __name__ == '__main__':
    main()

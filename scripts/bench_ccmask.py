"""GPU: `extract` on masked cross-correlation data (Engine.cc_prepare_masked / cc_lstsq_deg2, csrc/k_extract_lsq.h) at
128 shells x L = 32 x 512 angles with a pixel_flat mask.  Five windows each (median, min .. max), inputs already in HBM:
  (a) kernel k_cc_prepare (event bracket `cc_prepare`): the three modify_cc switches, and the same plus interpolate_masked;
  (b) kernel k_cc_lstsq (event bracket `cc_lstsq`) with 17 orders (even) and 33 orders (all);
  (c) the unmasked kernel k_cc_deg2 at the same size, for scale;
  (d) the reference route's numpy loop (np.linalg.lstsq per pair on scipy's Legendre matrix) on this host: timed on a sample of pairs
      and scaled to all Nq^2, beside the device's error against it on those pairs.
usage: python scripts/bench_ccmask.py"""
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


def kernel_time(e, name, call, reps=5, windows=5):
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


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bench_ccmask needs a GPU: a timing without one measures nothing')
    import ccextract_cases as CC
    import ccmask_cases as MC
    nq, L, nd = 128, 32, 512
    e = Engine({'grid': {'n_radial_points': 8, 'max_order': 2}}, None, n_batch=1, max_q=1.0)
    qs, phis, cc, avg, _ = CC.synthetic_cc(nq, L, nd, 27, 2, noise=1e-3)
    grid = MC.grid_of(qs, phis)
    # r_pixel = 2 pi / pixel_size = 0.03: the pairs within four shells of the diagonal lose the angles around 0 (and pi)
    setting = {'type': 'pixel_flat', 'pixel_flat': {'pixel_size': 2 * np.pi / 0.03, 'mask_at_pi': True}}
    mask = X.cross_correlation_mask(grid, {'cc_mask': setting, 'xray_wavelength': WAVELENGTH})
    nv = mask.sum(-1)
    print('%d x L%d x %d, pixel_flat mask: %.2f %% of the samples masked, valid per pair %d .. %d, pairs without a sample %d'
          % (nq, L, nd, 100 * (~mask).mean(), nv.min(), nv.max(), (nv == 0).sum()))
    d_cc, d_mask = torch.from_numpy(cc).cuda(), torch.from_numpy(mask).cuda()
    bad = (phis < np.pi / 2) | (phis >= 3 * np.pi / 2)
    t = kernel_time(e, 'cc_prepare', lambda: e.cc_prepare_masked(d_cc, d_mask, average_intensity=avg, bad_angles=bad, q1q2_symmetric=True))
    print('  (a) k_cc_prepare, three switches            : %s' % stats(t))
    inner = torch.from_numpy(MC.periodic_mask(nq, nd, 1 / 16) | (np.arange(nd) % 64 == 0)[None, None, :] | (np.arange(nd) == nd - 1)).cuda()
    t = kernel_time(e, 'cc_prepare', lambda: e.cc_prepare_masked(d_cc, inner, average_intensity=avg, bad_angles=bad, q1q2_symmetric=True,
                                                                  interpolate_phis=phis))
    print('      k_cc_prepare, the same + interpolation  : %s' % stats(t))
    thetas = grid['thetas']
    results = {}
    for name, orders in (('17 orders (even)', np.arange(0, L + 1, 2)), ('33 orders (all)', np.arange(L + 1))):
        t = kernel_time(e, 'cc_lstsq', lambda: e.cc_lstsq_deg2(d_cc, d_mask, orders, thetas, phis), reps=3)
        b, n_valid, rc = (x.cpu().numpy() for x in e.cc_lstsq_deg2(d_cc, d_mask, orders, thetas, phis))
        results[name] = (orders, b)
        ok = n_valid > 0
        print('  (b) k_cc_lstsq, %-18s          : %s; reciprocal condition estimate %.1e .. %.1e' % (name, stats(t), rc[ok].min(), rc[ok].max()))
    leg = X.legendre_table(qs, WAVELENGTH, L, 2)
    t = kernel_time(e, 'cc_deg2', lambda: e.cc_to_deg2(d_cc, L, 2, 3, legendre=leg))
    print('  (c) k_cc_deg2 (unmasked back substitution)  : %s' % stats(t))
    rng = np.random.default_rng(1)
    pairs = [(int(i), int(j)) for i, j in rng.integers(0, nq, size=(48, 2))] + [(5, 5), (6, 7), (40, 41)]
    pairs = [p for p in pairs if mask[p].any()]
    for name, (orders, b) in results.items():
        t0 = time.perf_counter()
        ref = [np.linalg.lstsq(MC.legendre_matrix(qs, phis, orders, i, j)[mask[i, j]], cc[i, j, mask[i, j]], rcond=None)[0] for i, j in pairs]
        dt = (time.perf_counter() - t0) / len(pairs)
        err = max(np.linalg.norm(b[orders, i, j].real - r) / np.linalg.norm(r) for (i, j), r in zip(pairs, ref))
        print('  (d) numpy loop, %-18s          : %.3f ms per pair on %d pairs -> %.1f s for all %d pairs; device vs it, worst pair %.1e'
              % (name, 1e3 * dt, len(pairs), dt * nq * nq, nq * nq, err))
    e.close()


if __name__ == '__main__':
    main()

"""GPU: forward and inverse SHT beyond L = 63 (csrc/k_sht_big.h) against the generic kernels (MTIP_SHT_TIER=0) on the same build.
Per case (shells, L, restarts), after a warm-up of two calls, five windows of `reps` calls each; the figure is the median over the
windows of the event-bracketed family time per call (`sht_fwd` / `sht_inv`: both launches of a direction, operands in HBM; the copies
of the host arrays lie outside the brackets).  Beside each time: the algorithmic bytes of the direction's two launches (grid, spectra
written and read back, coefficients; the Legendre table once) and the share of the 8 TB/s HBM peak they amount to.
usage: python scripts/bench_sht_bigl.py [--lib libmtip_hip.so] [--cases N,L,B ...] [--no-tier0]
       python scripts/bench_sht_bigl.py --once N,L,B      (three calls of each direction, for a kernel trace)
--lib: another build of the library, e.g. the previous commit's at 256,63,1 (the largest band limit it runs on the 128 x 256 grid)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
np.seterr(all='ignore')
import torch                                        # noqa: E402
from xframe_amd.fxs import hostsetup as hs          # noqa: E402
from xframe_amd.fxs.engine import Engine            # noqa: E402

HBM_PEAK = 8e12
# the Hankel weights are not used here and take half a minute of host time at 512 x L128
hs.hankel_raw_weights = lambda L, N, kappa, mode: np.zeros((L + 1, N - 1 if hs.hankel_skips_first_shell(mode) else N, N))


def launch_bytes(e):
    """algorithmic bytes of (FFT stage, Legendre stage) of one direction: the same for both directions"""
    Q = e.B * e.N
    grid = 16.0 * Q * e.n_theta * e.n_phi
    spectra = 16.0 * Q * e.n_theta * (2 * e.L + 1)
    coeff = 16.0 * Q * e.nlm
    table = 8.0 * (e.L + 1) * (e.L + 2) / 2 * (e.n_theta / 2)
    return grid + spectra, spectra + coeff + table


def engine(N, L, B, lib, tier):
    if tier is None:
        os.environ.pop('MTIP_SHT_TIER', None)
    else:
        os.environ['MTIP_SHT_TIER'] = str(tier)          # read by the plan when the angular grid is set
    return Engine({'grid': {'n_radial_points': N, 'max_order': L}}, None, n_batch=B, lib_path=lib, max_q=1.0)


def measure(e, g, co, reps):
    out = {}
    for fam, fn in (('sht_fwd', lambda: e.sht_forward(g)), ('sht_inv', lambda: e.sht_inverse(co))):
        for _ in range(2):
            fn()
        w = []
        for _ in range(5):
            e.profile(True)
            for _ in range(reps):
                fn()
            ms, n = e.profile_get(fam)
            assert n == reps, (fam, n)
            w.append(ms / n)
            e.profile(False)
        out[fam] = np.sort(w)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None)
    ap.add_argument('--cases', nargs='+', default=['256,64,1', '512,128,1'])
    ap.add_argument('--no-tier0', action='store_true')
    ap.add_argument('--once', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sht_bigl needs a GPU: a timing without one measures nothing')
    rng = np.random.default_rng(0)
    if a.once:
        N, L, B = map(int, a.once.split(','))
        e = engine(N, L, B, a.lib, None)
        g = rng.standard_normal((B,) + e.shape) + 0j
        co = rng.standard_normal((B, N, e.nlm)) + 0j
        for _ in range(3):
            e.sht_forward(g)
            e.sht_inverse(co)
        e.close()
        return
    for case in a.cases:
        N, L, B = map(int, case.split(','))
        res = {}
        for name, tier in (('planned kernels', None),) + (() if a.no_tier0 else (('MTIP_SHT_TIER=0', 0),)):
            e = engine(N, L, B, a.lib, tier)
            g = rng.standard_normal((B,) + e.shape) + 1j * rng.standard_normal((B,) + e.shape)
            co = rng.standard_normal((B, N, e.nlm)) + 1j * rng.standard_normal((B, N, e.nlm))
            fb, lb = launch_bytes(e)
            if not res:
                print('%d shells x L%d, %d restart(s), angular grid %d x %d: FFT stage %.1f MB, Legendre stage %.1f MB per direction'
                      % (N, L, B, e.n_theta, e.n_phi, fb / 1e6, lb / 1e6))
            res[name] = measure(e, g, co, 3 if e.shape[0] * e.shape[1] * e.shape[2] > 2 ** 25 else 10)
            for fam, w in res[name].items():
                med = float(np.median(w))
                print('  %-16s %s: %.3f ms (min %.3f .. max %.3f) = %.2f TB/s of algorithmic bytes = %.0f %% of the HBM peak'
                      % (name, fam, med, w[0], w[-1], (fb + lb) / (med * 1e-3) / 1e12, 100 * (fb + lb) / (med * 1e-3) / HBM_PEAK))
            e.close()
            del g, co
        if len(res) == 2:
            for fam in ('sht_fwd', 'sht_inv'):
                print('  %s: tier 0 / planned = %.2f' % (fam, np.median(res['MTIP_SHT_TIER=0'][fam]) / np.median(res['planned kernels'][fam])))


if __name__ == '__main__':
    main()

"""Study: the resident 2-D loop (mtip2d_run, fused step kernels) against the operator-level 2-D loop (one mtip2d_op_step call per
step, host arrays in and out), in one process on one GPU.

    python scripts/bench_2d_resident.py [--n-radial 128] [--max-order 64] [--restarts 8] [--steps 200] [--windows 5] [--long-run 0]

Rows: HIO with / without ft_stab, ER with ft_stab, shrink-wrap.  Every row is timed in `windows` windows of `steps` steps for both
paths (the same context, the same densities and supports); the table gives the median time per step, the spread (max - min over
the windows) and the ratio of the medians.  A row counts as faster when the medians differ by more than both spreads.
`--long-run K` instead runs ONE resident HIO block of K steps and exits (for a kernel / memory-copy trace of the loop alone).
The data are synthetic (smooth projection vectors on the midpoint grid): the timings do not depend on the values."""
import argparse
import gc
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xframe_amd.fxs import settings as ST                       # noqa: E402
from xframe_amd.fxs import synthetic as S                       # noqa: E402
from xframe_amd.fxs.reconstruct2d import MTIP2D                 # noqa: E402


def problem(N, M, B):
    max_q = S.data_cutoff(N)
    q = S.midpoint_points(max_q, N)
    orders = np.arange(M + 1)
    pm = np.exp(-((q[None, :] / max_q - 0.1 * (orders[:, None] % 7)) ** 2) * 8.0) / (1.0 + orders[:, None]) * np.exp(1j * 0.3 * orders[:, None])
    pm[0] = np.abs(pm[0]) * 4
    data = {'dimensions': 2, 'xray_wavelength': 1.23984, 'average_intensity': np.abs(pm[0]), 'data_radial_points': q, 'max_order': M,
            'data_projection_matrices': pm}
    opt = ST.deep_update(ST.default_settings(), S.config_overrides(1))
    opt = ST.deep_update(opt, {'dimensions': 2, 'grid': {'n_radial_points': N, 'max_order': M, 'max_q': float(max_q)},
                               'projections': {'reciprocal': {'used_order_ids': orders}}})
    return MTIP2D(opt, data, n_restarts=B, seeds=list(range(B)), resident=True)


def windows(fn, n):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        k = fn()
        out.append((time.perf_counter() - t0) / k * 1e3)
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n-radial', type=int, default=128)
    ap.add_argument('--max-order', type=int, default=64)
    ap.add_argument('--restarts', type=int, default=8)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--long-run', type=int, default=0)
    a = ap.parse_args()
    m = problem(a.n_radial, a.max_order, a.restarts)
    e = m.engine
    rhos = [m._initial_density(b) for b in range(a.restarts)]

    def reset():
        for b, r in enumerate(rhos):
            e.set_density(b, r)
        e.set_initial_support(m.initial_support)
        e.set_reciprocal_metrics()
        e.set_main_error('mean', ['real'])
        e.init_state()
        e.synchronize()

    reset()
    gc.disable()                                                  # (no collector pauses inside a window, either path)
    betas = np.full(a.steps, 0.5)
    if a.long_run:
        e.run('HIO', True, np.full(16, 0.5))                     # warm-up
        e.synchronize()
        t0 = time.perf_counter()
        e.run('HIO', True, np.full(a.long_run, 0.5), fetch=False)
        e.synchronize()
        dt = time.perf_counter() - t0
        print(f'resident HIO ft_stab=1, {a.long_run} steps in one run: {dt / a.long_run * 1e3:.4f} ms per step')
        m.close()
        return
    print('# python scripts/bench_2d_resident.py ' + ' '.join(sys.argv[1:]))
    print(f'# {a.n_radial} shells x M = {a.max_order} (n_phi = {e.n_phi}), {a.restarts} restarts, {a.windows} windows of {a.steps} steps; ms per step '
          '(per call for the shrink-wrap): median [spread = max - min]')
    rho_h, sup_h = e.density(), e.support()
    rows = []
    for method, ft in (('HIO', True), ('HIO', False), ('ER', True)):
        def resident():
            e.run(method, ft, betas, fetch=False)
            e.synchronize()
            return a.steps

        def operators():
            r = rho_h
            for _ in range(a.steps):
                r = e.step(method, ft, 0.5, r, sup_h)[1]
            return a.steps
        reset()
        resident()                                                # warm-up window
        tr = windows(resident, a.windows)
        operators()
        to = windows(operators, a.windows)
        rows.append((f'{method} ft_stab={int(ft)}', to, tr))
    reset()
    sigma = m.default_sigma

    def sw_resident():
        for _ in range(a.steps):
            e.shrinkwrap_state(sigma, 0.06, np.inf)
        return a.steps

    def sw_operators():
        for _ in range(a.steps):
            e.shrinkwrap(rho_h, sigma, 0.06)
        return a.steps
    sw_resident()
    tr = windows(sw_resident, a.windows)
    sw_operators()
    to = windows(sw_operators, a.windows)
    rows.append(('shrink-wrap', to, tr))
    ok = True
    for name, to, tr in rows:
        mo, mr = np.median(to), np.median(tr)
        so, sr = to.max() - to.min(), tr.max() - tr.min()
        faster = mo - mr > max(so, sr)
        ok &= bool(faster)
        print(f'{name:16s} operator-level {mo:8.4f} [{so:.4f}]   resident {mr:8.4f} [{sr:.4f}]   ratio {mo / mr:6.2f}   '
              f'{1e3 / mr * 1:9.0f} steps/s resident   {"faster" if faster else "NOT faster by more than the spread"}')
        print('#   windows operator-level ' + ' '.join(f'{v:.4f}' for v in to) + ' | resident ' + ' '.join(f'{v:.4f}' for v in tr))
    print('# resident faster on every row by more than the spread:', ok)
    m.close()


if __name__ == '__main__':
    main()

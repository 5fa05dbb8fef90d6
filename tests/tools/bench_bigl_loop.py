"""Timing of the phasing loop beyond L = 63 (GPU.big_l_loop) on the GPU: ms per step and the mtip_profile families at the tutorial's
128 x L64 with 1 and 8 restarts and at 6 x L64 for scale (a study script: its problems are those of tests/bigl_loop_cases.py).
    python tests/tools/bench_bigl_loop.py [steps] > profiles/bigl_loop_timing.txt"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', '..'))
sys.path.insert(0, os.path.join(HERE, '..'))
np.seterr(all='ignore')
import bigl_loop_cases as BL                                                  # noqa: E402
from xframe_amd.fxs import hostsetup as hs                                    # noqa: E402
from xframe_amd.fxs.engine import Engine                                      # noqa: E402

FAMILIES = ('sht_fwd', 'sht_inv', 'sht_inv_modulus', 'hankel', 'proj', 'polar')
steps = int(sys.argv[1]) if len(sys.argv) > 1 else 20


def route(e):
    """the projection route plan_projection takes for this engine's active orders (the same arithmetic, restated)"""
    if e.projection_slots() > 0:
        return 'real arithmetic, one kernel (k_rproj)'
    act = [l for l in range(e.L + 1) if np.abs(e.rsetup.projection_matrices.get(l, np.zeros(1))).max() > 0]
    kmax = max(min(2 * l + 1, e.N) for l in act)
    nmax = max(2 * l + 1 for l in act)
    lds = (kmax * (nmax | 1) + kmax * (kmax | 1)) * 16
    where = 'LDS (k_polar_jacobi_lds)' if lds <= 158 * 1024 and nmax <= 128 else 'global memory (k_polar_jacobi, cold start every call)'
    return f'complex kernels, polar factors in {where}: largest active order {kmax} columns x {nmax} rows, {lds / 1024:.0f} KiB'


print(f'phasing loop with GPU.big_l_loop, fused step, ft_stab, HIO; {steps} timed steps after 3 warm-up steps; wall clock around steps that end in')
print('a synchronise; families from mtip_profile (event pairs) in a second run of the same steps: "proj" includes "polar", the rest of the')
print('step (real-space update, coefficient difference, error sums) is in no family')
for shape, n_used in (((128, 64, 0, 0, 1), 64), ((128, 64, 0, 0, 8), 64), ((6, 64, 66, 256, 2), None)):
    N, L, nt, nphi, B = shape
    data, opt = BL.problem(N, L, nt, nphi, n_used)
    e = Engine(opt, data, n_batch=B)
    for b in range(B):
        e.set_density(b, hs.bump_density(e.rs, e.shape, opt['particle_radius'], 0.3, 2, np.random.default_rng(1000 + b),
                                         e.rsetup.integrated_intensity, e.int_wr, e.int_wt))
    e.init_state()
    betas = np.full(steps, 0.45)
    e.run('HIO', True, betas[:3], fetch=False)
    e.synchronize()
    t = time.perf_counter()
    e.run('HIO', True, betas, fetch=False)
    e.synchronize()
    ms = (time.perf_counter() - t) / steps * 1e3
    e.profile(True)
    e.run('HIO', True, betas, fetch=False)
    e.synchronize()
    fam = {f: e.profile_get(f) for f in FAMILIES}
    e.profile(False)
    err = e.fetch_errors(0, 3 + 2 * steps)[0]
    print(f'\n---- {N} shells x L{L}, grid {e.n_theta} x {e.n_phi}, {B} restart{"s" if B > 1 else ""}, used_order_ids arange({n_used or L + 1}), odd orders zero')
    print(f'step: {ms:9.3f} ms ({ms / B:.3f} ms per restart); last real error of restart 0: {err[-1, 0]:.4e} (finite: {bool(np.isfinite(err).all())})')
    print(f'projection route: {route(e)}')
    print('  family             launches/step   ms/step   share of the step')
    for f in FAMILIES:
        t_ms, n = fam[f]
        print(f'  {f:18s} {n / steps:10.1f} {t_ms / steps:12.3f} {t_ms / steps / ms:10.1%}')
    print(f'  the polar-factor kernel takes {fam["polar"][0] / steps / ms:.1%} of the step')
    e.close()

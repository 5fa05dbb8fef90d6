"""GPU: detector frames -> polar patterns (fxs.correlate.Resampler, Correlator.add_detector; csrc/k_resample.h) at the reference's
tutorial shape: 512 x 512 frames to 256 rings x 1024 angles, interpolation orders 2 and 3, float32 frames.
Per order, with intensity_pixel_threshold on (a mask per pattern) and off (the static mask), frames from the host and resident on
the device, batch sizes 1, 8 and 32: ms per pattern of Resampler.run (host clock around calls that end in a synchronise; three
windows after a warm-up: median, min .. max) and, for resident frames, the event brackets of the kernel families rs_filter
(k_rs_cols + k_rs_rows) and rs_gather inside the same windows.  Then Correlator.add_detector against Correlator.add of polar data of
the same shape in the same run, and scipy.ndimage.map_coordinates on the same frames on this host with 1 and with 8 processes.
Derived, with the counts stated where they are printed: the frame and coefficient bytes per pattern against HBM.
usage: python scripts/bench_resample.py            the timings
       python scripts/bench_resample.py --trace    a short fixed workload without timers, to run under rocprofv3 --kernel-trace --stats"""
import multiprocessing as mp
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
np.seterr(all='ignore')

HBM_PEAK = 8e12
BATCHES = (1, 8, 32)
H = W = 512
N_Q, N_PHI = 256, 1024
THRESHOLD = [4.0, 1e4]


def settings_for(order, threshold):
    """the worker's defaults (512 x 512 frames, 200 um pixels at 620 mm) with 256 rings x 1024 angles, every pair of rings"""
    edge = H / 2 * 0.2
    q_max = 4 * np.pi * np.sin(np.arctan(edge / 620.0) / 2) / 1.23984
    return {'qrange': [0.0, q_max, q_max / (N_Q - 1) * (1 - 1e-12)], 'qrange_xcca': [[0.0, q_max, 1], [0.0, q_max, 1]],
            'phi_range': (0.0, 2 * np.pi, N_PHI, 'exact'), 'interpolation_order': order,
            'intensity_pixel_threshold': [bool(threshold)] + THRESHOLD}


def frames(P, seed=0):
    """photon-count-like frames: a radial fall-off around the origin; 3 % of the pixels lie below the lower threshold, in 8 x 8 blocks
    on a 16-pixel lattice (isolated dead pixels in unlucky constellations make the mask's spline overshoot past 1.5, which raises)"""
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(H) - 255.2, np.arange(W) - 255.5, indexing='ij')
    env = 40.0 + 400.0 * np.exp(-np.hypot(ii, jj) / 90.0)
    out = env[None] * (1.0 + 0.4 * rng.random((P, H, W)))
    dead = np.zeros((P, H // 16, 16, W // 16, 16), bool)
    dead[:, :, 4:12, :, 4:12] = (rng.random((P, H // 16, W // 16)) < 0.12)[:, :, None, :, None]
    out[dead.reshape(P, H, W)] = 1.0
    return out.astype(np.float32)


def bytes_per_pattern(static):
    """what the kernels move per pattern, from the shapes: the first pass of k_rs_cols reads the frame twice (start sum, recursion:
    4 B, + 1 B of mask where one is given), every recursion pass reads or writes 8 B per coefficient (cols: 1 write + 1 read +
    1 write, rows: 3 reads + 2 writes), per array (image, and the mask unless it is static); the gather reads (order + 1)^2
    coefficients per point and array (mostly from cache) and writes 9 B per point"""
    arrays = 1 if static else 2
    filt = arrays * H * W * (2 * 4 + 8 * 8)
    gather = N_Q * N_PHI * (16 + 9)
    return filt + gather


def stats(v):
    v = np.sort(np.asarray(v))
    return '%8.3f ms (min %.3f .. max %.3f)' % (np.median(v), v[0], v[-1])


def timed(call, sync, B, windows=3, target=0.25):
    call()
    call()
    sync()
    t0 = time.perf_counter()
    call()
    sync()
    one = time.perf_counter() - t0
    reps = int(min(64, max(2, round(target / max(one, 1e-4)))))
    wall = []
    for _ in range(windows):
        sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        sync()
        wall.append(1e3 * (time.perf_counter() - t0) / (reps * B))
    return wall, reps


def _scipy_worker(args):
    order, n, seed = args
    from scipy import ndimage
    from xframe_amd.fxs import correlate as CR
    geo = CR.polar_geometry(settings_for(order, False))
    xy = [geo['cart_x'].ravel(), geo['cart_y'].ravel()]
    img = frames(n, seed).astype(np.float64)
    mask = np.ones((H, W), np.int64)
    t0 = time.perf_counter()
    for p in range(n):
        ndimage.map_coordinates(img[p], xy, order=order, mode='constant', cval=0, prefilter=True)
        ndimage.map_coordinates(mask, xy, order=order, mode='constant', cval=0, prefilter=True)
    return time.perf_counter() - t0


def scipy_context(order, n=4):
    t1 = _scipy_worker((order, n, 1))
    t0 = time.perf_counter()
    with mp.get_context('spawn').Pool(8) as pool:
        pool.map(_scipy_worker, [(order, n, 10 + i) for i in range(8)])
    t8 = time.perf_counter() - t0
    print('  scipy.ndimage.map_coordinates on this host, order %d, image and mask: 1 process %.1f ms per pattern; 8 processes '
          '(%d patterns each, pool start included) %.1f ms per pattern' % (order, 1e3 * t1 / n, n, 1e3 * t8 / (8 * n)))


def trace_workload(e, CR, torch):
    for order in (2, 3):
        for thr in (False, True):
            rs = CR.Resampler(e, settings_for(order, thr))
            for B in (1, 32):
                d = torch.from_numpy(frames(B)).cuda()
                for _ in range(3):
                    rs.run(d)
            rs.close()
    torch.cuda.synchronize()


def main():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_resample needs a GPU: a timing without one measures nothing')
    from xframe_amd.fxs import correlate as CR
    from xframe_amd.fxs.engine import Engine
    e = Engine({'grid': {'n_radial_points': 8, 'max_order': 2}}, None, n_batch=1, max_q=1.0)
    if '--trace' in sys.argv:
        trace_workload(e, CR, torch)
        e.close()
        return
    sync = torch.cuda.synchronize
    host = frames(max(BATCHES))
    dev = torch.from_numpy(host).cuda()
    geo = CR.polar_geometry(settings_for(2, False))
    assert (geo['n_q'], geo['n_phi']) == (N_Q, N_PHI)
    outside = np.mean((geo['cart_x'] < 0) | (geo['cart_x'] > H - 1) | (geo['cart_y'] < 0) | (geo['cart_y'] > W - 1))
    print('%d x %d float32 frames -> %d rings x %d angles (%.1f %% of the points outside the frame)' % (H, W, N_Q, N_PHI, 100 * outside))
    for order in (2, 3):
        for thr in (False, True):
            rs = CR.Resampler(e, settings_for(order, thr))
            nbytes = bytes_per_pattern(not thr)
            print(' order %d, threshold %s (%s): %.1f MB moved per pattern = %.4f ms at 8 TB/s' %
                  (order, 'on ' if thr else 'off', 'a mask per pattern' if thr else 'static mask', 1e-6 * nbytes, 1e3 * nbytes / HBM_PEAK))
            for B in BATCHES:
                wall_h, reps_h = timed(lambda: rs.run(host[:B]), sync, B)
                e.profile(True)
                wall_d, reps_d = timed(lambda: rs.run(dev[:B]), sync, B)
                f_ms, n_f = e.profile_get('rs_filter')
                g_ms, n_g = e.profile_get('rs_gather')
                e.profile(False)
                print('  batch %2d: run, frames on the device %s per pattern | from the host %s' % (B, stats(wall_d), stats(wall_h)))
                print('            rs_filter %.4f ms, rs_gather %.4f ms per pattern (event brackets, mean of %d calls)' % (f_ms / (n_g * B), g_ms / (n_g * B), n_g))
            rs.close()
    # ---- add_detector against add of polar data of the same shape
    for thr, shared in ((False, True), (True, False)):
        settings = settings_for(2, thr)
        rs = CR.Resampler(e, settings)
        pol_i, pol_m = rs.run(dev)
        rs.close()
        for B in BATCHES:
            c = CR.Correlator(e, settings, shared_mask=shared)
            wall_a, _ = timed(lambda: c.add(pol_i[:B], pol_m[0] if shared else pol_m[:B]), sync, B)
            c.close()
            c = CR.Correlator(e, settings, shared_mask=shared)
            wall_d, _ = timed(lambda: c.add_detector(dev[:B]), sync, B)
            c.close()
            print(' order 2, threshold %s, %s correlate handle, batch %2d: add_detector %s per pattern | add of polar data %s' %
                  ('on ' if thr else 'off', 'shared-mask ' if shared else 'per-pattern', B, stats(wall_d), stats(wall_a)))
    del dev
    for order in (2, 3):
        scipy_context(order)
    e.close()


if __name__ == '__main__':
    main()

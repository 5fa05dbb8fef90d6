"""Cases of the alignment and averaging operators (csrc/k_align.hip: k_so3_T/S/P/C, k_so3_argmax, k_so3_build_D, k_rotate_coeff;
csrc/k_average.hip: k_av_stats, k_av_stats_finish, k_av_phase, k_av_combine, k_av_prtf) against the longdouble references of
tests/so3_reference.py, shared by tests/test_emul_align.py (CPU emulator, toy sizes) and tests/test_gpu_align.py (MI355X, the sizes
the README quotes numbers for).

Inputs: complex, no symmetry, fixed seeds, different for every item of a batch, one item of a batch all zero, ref != sig.
Tolerances (the project's bound for operators is 1e-12, README):
  * correlation, rotation, phase ramp, combine: max|got - ref| <= 1e-12 max|ref| per batch item, an all-zero item exactly zero;
  * sums of grid_stats, PRTF means: |got - ref| <= 1e-12 sum|terms|, the sum of magnitudes taken in longdouble (the sums cancel: a
    bound relative to the result would measure the data); extrema and the count exact; PRTF standard deviation 1e-10 relative,
    floor 1e-12;
  * arg-max: equal to the reference's, and the case ASSERTS on the reference alone that its two largest values differ by more than
    1e-9 of max|C| (1000 x the value tolerance).
Every case prints its worst measured ratio (figure / bound) on a line starting with 'ALIGN'."""
import ctypes

import numpy as np

import so3_reference as SR
from xframe_amd.fxs import _lib, hostsetup as hs, synthetic as S
from xframe_amd.fxs.engine import Engine

TOL = 1e-12
TOL_STD_REL, TOL_STD_FLOOR = 1e-10, 1e-12
GAP_MIN = 1e-9


def make_engine(N, L, B, lib_path, n_theta=0, n_phi=0):
    max_q = float(np.max(S.midpoint_points(S.data_cutoff(N), N)))
    return Engine({'grid': {'n_radial_points': N, 'max_order': L, 'n_theta': n_theta, 'n_phi': n_phi}}, None, n_batch=B,
                  lib_path=lib_path, max_q=max_q)


def report(case, **figures):
    print('ALIGN %-44s %s' % (case, '  '.join('%s=%.3g' % kv for kv in figures.items())), flush=True)


def coefficients(seed, B, N, L, spectrum):
    """(ref (N, nlm), sig (B, N, nlm), kinds): 'decay' is the spectrum of scripts/bench_average.py, 'flat' plain normal numbers.
    kinds[b]: 'random'; 'zero' (the last item of a batch of two or more); 'l0' (item 1 of a batch of three or more: only l = 0)"""
    rng = np.random.default_rng(seed)
    nlm = (L + 1) ** 2

    def one():
        c = rng.normal(size=(N, nlm)) + 1j * rng.normal(size=(N, nlm))
        if spectrum == 'decay':
            c = c * np.exp(-(np.arange(N)[:, None] / (0.35 * N)) ** 2) / (1 + np.arange(nlm)[None, :]) ** 0.5
        return c
    ref = one()
    sig = np.stack([one() for _ in range(B)])
    kinds = ['random'] * B
    if B >= 2:
        sig[B - 1] = 0
        kinds[B - 1] = 'zero'
    if B >= 3 and L > 0:
        sig[1, :, 1:] = 0
        kinds[1] = 'l0'
    return ref, sig, kinds


def _tensor(e, x):
    import torch
    return torch.from_numpy(np.array(x)).to(e.torch_device())          # (a copy: under the emulation device memory is host memory)


def _rel_max(got, ref):
    """max|got - ref| / max|ref| with the difference taken in longdouble; 0 / 0 = 0"""
    scale = float(np.max(np.abs(ref)))
    diff = float(np.max(np.abs(np.asarray(got).astype(ref.dtype) - ref)))
    return diff / scale if scale > 0 else diff


# ---------------------------------------------------------------------------------------------- SO(3) correlation and its arg-max
def check_correlation(lib_path, N, L, B, shells=None, spectrum='decay', n_theta=0, n_phi=0, seed=0):
    """so3_correlation, the C of t_find_rotation(keep_metric=True), arg and vmax against correlation_ref, whole array"""
    e = make_engine(N, L, B, lib_path, n_theta, n_phi)
    lo, hi = (0, N) if shells is None else shells
    nb = 2 * (L + 1)
    ref, sig, kinds = coefficients(1000 * L + 10 * N + B + seed, B, N, L, spectrum)
    rng = np.random.default_rng(seed + 5)
    # a rotation first: it stages its angles in the SO(3) scratch buffers the correlation then has to overwrite completely
    e.t_rotate_grid(_tensor(e, sig), rng.integers(nb, size=B), rng.uniform(0, 6, B), rng.uniform(0, 6, B))
    C1 = e.so3_correlation(ref, sig, [lo, hi])
    arg, vmax, C2 = e.t_find_rotation(_tensor(e, ref), _tensor(e, sig), [lo, hi], keep_metric=True)
    C2 = C2.cpu().numpy()
    C3 = e.so3_correlation(ref, sig, [lo, hi])
    e.close()
    assert C1.shape == (B, nb, nb, nb)
    assert np.array_equal(C1, C2) and np.array_equal(C1, C3), 'the correlation differs between two calls on the same input'
    worst, min_gap = 0.0, np.inf
    for b in range(B):
        Cr = SR.correlation_ref(ref, sig[b], L, lo, hi)
        key = int(arg[b, 0]) * nb * nb + int(arg[b, 1]) * nb + int(arg[b, 2])
        at = (b, (-int(arg[b, 1])) % nb, int(arg[b, 0]), (-int(arg[b, 2])) % nb)
        assert vmax[b] == C1[at], (b, vmax[b], C1[at])                # the maximum is the device's own value at its index, bit for bit
        want, gap = SR.argmax_key(Cr)
        if kinds[b] == 'zero':
            assert not Cr.any() and not C1[b].any() and key == 0, (b, key)
            continue
        err = _rel_max(C1[b], Cr)
        worst = max(worst, err)
        assert err <= TOL, (b, kinds[b], err)
        if kinds[b] == 'l0':                                          # exactly constant: numpy's arg-max of an all-equal array is 0
            assert Cr.max() == Cr.min() and C1[b].max() == C1[b].min() and key == 0, (b, key)
            continue
        min_gap = min(min_gap, gap)
        assert gap > GAP_MIN, 'seed without a clear maximum: the reference gap is %.3g of max|C| (item %d)' % (gap, b)
        assert key == want, (b, key, want)
    report('correlation N%d L%d B%d [%d,%d) %s' % (N, L, B, lo, hi, spectrum), err_over_tol=worst / TOL, min_gap=min_gap)
    return worst


# ---------------------------------------------------------------------------------------------- rotation of coefficients
def _grid_rotation_calls(L, B, rng, cover_all):
    """(beta_index, alpha, gamma) per call of t_rotate_grid: alpha, gamma from {0, 2 pi, 2 pi - alpha_j, a grid value, non-grid
    values}; with cover_all every beta index 0 .. 2bw-1 appears at least once over the calls"""
    nb = 2 * (L + 1)
    al = hs.euler_grid(L + 1)[0]
    special = [0.0, 2 * np.pi, 2 * np.pi - al[1 % nb], 2 * np.pi - al[nb - 1], al[nb // 2], 0.7390851332151607, 5.1]
    betas = list(range(nb)) if cover_all else [0, nb - 1] + [int(x) for x in rng.integers(nb, size=max(B, 4))]
    while len(betas) % B:
        betas.append(int(rng.integers(nb)))
    calls, s = [], 0
    for i in range(0, len(betas), B):
        a = [special[(s + 2 * j) % len(special)] for j in range(B)]
        g = [special[(s + 2 * j + 3) % len(special)] for j in range(B)]
        s += 1
        calls.append((np.array(betas[i:i + B]), np.array(a), np.array(g)))
    return calls


def check_rotation(lib_path, N, L, B, spectrum='decay', n_theta=0, n_phi=0, evaluate=False, seed=0):
    """rotate_coefficients (D from the host) and t_rotate_grid (D built by k_so3_build_D) against rotate_ref"""
    e = make_engine(N, L, B, lib_path, n_theta, n_phi)
    _, c, kinds = coefficients(2000 * L + 10 * N + B + seed, B, N, L, spectrum)
    rng = np.random.default_rng(seed + 9)
    eulers = np.stack([rng.uniform(0, 2 * np.pi, B), rng.uniform(0.05, np.pi - 0.05, B), rng.uniform(0, 2 * np.pi, B)], axis=1)
    got = e.rotate_coefficients(c, eulers)
    calls = _grid_rotation_calls(L, B, rng, cover_all=L <= 10)
    ct = _tensor(e, c)
    got_grid = [e.t_rotate_grid(ct, bi, a, g).cpu().numpy() for bi, a, g in calls]
    e.close()
    worst = 0.0
    for b in range(B):
        ref = SR.rotate_ref(c[b], eulers[b], L)
        if kinds[b] == 'zero':
            assert not got[b].any(), b
        err = _rel_max(got[b], ref)
        worst = max(worst, err)
        assert err <= TOL, ('rotate_coefficients', b, err)
    worst_eval = 0.0
    if evaluate:                                                      # the device output as a function on the sphere
        pts = np.random.default_rng(seed + 10).normal(size=(20, 3))
        pts /= np.linalg.norm(pts, axis=1, keepdims=True)
        rows = [0, N // 2, N - 1]
        for b in range(B):
            want = SR.evaluate(c[b][rows], L, pts @ SR.rotation_matrix(eulers[b]))       # f(R^-1 x)
            have = SR.evaluate(got[b][rows], L, pts)
            scale = np.abs(want).max()
            if scale > 0:
                worst_eval = max(worst_eval, np.abs(have - want).max() / scale)
        assert worst_eval <= TOL, worst_eval
    beta_grid = hs.euler_grid(L + 1)[1]
    worst_grid, seen = 0.0, set()
    for (bi, a, g), out in zip(calls, got_grid):
        for b in range(B):
            seen.add(int(bi[b]))
            ref = SR.rotate_ref(c[b], (a[b], beta_grid[bi[b]], g[b]), L)
            if kinds[b] == 'zero':
                assert not out[b].any(), b
            err = _rel_max(out[b], ref)
            worst_grid = max(worst_grid, err)
            assert err <= TOL, ('t_rotate_grid', b, int(bi[b]), a[b], g[b], err)
    if L <= 10:
        assert seen == set(range(2 * L + 2))
    report('rotation N%d L%d B%d %s' % (N, L, B, spectrum), host_D=worst / TOL, device_D=worst_grid / TOL, evaluated=worst_eval / TOL)
    return max(worst, worst_grid)


# ---------------------------------------------------------------------------------------------- grid data with the edges planted
def edge_grid(rng, shape, kind):
    """a complex grid whose values hit the branches of k_av_stats:
      'mixed'  random; real part exactly 0 with positive, negative and zero imaginary part; the maximum at the first point and the
               minimum at the last
      'nopos'  no entry that numpy calls > 0 (real parts <= 0, those that are 0 with imaginary part <= 0): count 0, max <= 0; the
               maximum (a zero) at the last point, the minimum at the first
      'zero'   all zero"""
    if kind == 'zero':
        return np.zeros(shape, complex)
    g = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    flat = g.reshape(-1)
    n = flat.size
    idx = rng.choice(np.arange(1, n - 1), size=min(9, n - 2), replace=False)
    if kind == 'mixed':
        flat[idx[0::3]] = 1j * np.abs(flat[idx[0::3]].imag)
        flat[idx[1::3]] = -1j * np.abs(flat[idx[1::3]].imag)
        flat[idx[2::3]] = 0
        flat[0] = 7.5 + 0.25j
        flat[n - 1] = -8.5 - 0.5j
    else:
        flat.real = -np.abs(flat.real) - 1e-3
        flat[idx[0::3]] = -1j * np.abs(flat[idx[0::3]].imag)
        flat[idx[1::3]] = 0
        flat[0] = -9.5 + 2j
        flat[n - 1] = 0 - 1j
        flat[idx[2::3]] = -1e-300 + 3j
    return g


def grid_stack(seed, n, shape):
    rng = np.random.default_rng(seed)
    kinds = (['mixed', 'nopos'] * n)[:n]
    if n >= 3:
        kinds[n - 1] = 'zero'
    return np.stack([edge_grid(rng, shape, k) * (1.0 + 0.5 * i) for i, k in enumerate(kinds)]), kinds


def check_grid_stats(lib_path, N, L, n, seed=0):
    """t_grid_stats, all 11 slots, with and without ref, against stats_ref"""
    e = make_engine(N, L, 1, lib_path)
    X, kinds = grid_stack(300 + N + n + seed, n, e.shape)
    R = np.random.default_rng(seed + 1).normal(size=e.shape) + 0j
    Xt = _tensor(e, X)
    got_ref, got_no = e.t_grid_stats(Xt, _tensor(e, R)), e.t_grid_stats(Xt)
    cos_theta, rs, wr, wt = e.cos_theta, e.rs, e.int_wr, e.int_wt
    e.close()
    worst = 0.0
    for i in range(n):
        for got, ref in ((got_ref[i], R), (got_no[i], None)):
            val, mag = SR.stats_ref(X[i], wr, wt, rs, cos_theta, ref)
            for k in (6, 7, 10):
                assert got[k] == float(val[k]), (i, kinds[i], k, got[k], float(val[k]))
            for k in (0, 1, 2, 3, 4, 5, 8, 9):
                diff = abs(float(np.longdouble(got[k]) - val[k]))
                assert diff <= TOL * float(mag[k]), (i, kinds[i], k, got[k], float(val[k]), diff / float(mag[k]) if mag[k] else np.inf)
                if mag[k] > 0:
                    worst = max(worst, diff / float(mag[k]))
            if kinds[i] == 'nopos':
                assert got[10] == 0 and got[6] <= 0
    report('grid_stats %dx%s n%d' % (N, 'x'.join(map(str, e.shape[1:])), n), err_over_tol=worst / TOL)
    return worst


def check_grid_stats_nan(lib_path, N=6, L=4):
    """a NaN in a grid: numpy's max / min return it (average.py:721-727 then normalises everything to NaN), and so do slots 6 and 7;
    numpy's `> 0` is false for it, so the sum and the count of the positive entries stay finite; the other grid is untouched"""
    e = make_engine(N, L, 1, lib_path)
    X, _ = grid_stack(77, 2, e.shape)
    X[1] = X[0][::-1].copy()
    clean = e.t_grid_stats(_tensor(e, X))
    X[1, N // 2, 1, 2] = np.nan + 1j
    got = e.t_grid_stats(_tensor(e, X))
    val, _ = SR.stats_ref(X[1], e.int_wr, e.int_wt, e.rs, e.cos_theta)
    e.close()
    assert np.array_equal(got[0], clean[0])
    assert np.isnan(float(val[6])) and np.isnan(float(val[7]))        # the reference's behaviour is numpy's
    assert np.isnan(got[1, 6]) and np.isnan(got[1, 7]), got[1]
    assert np.isnan(got[1, :5]).all()
    assert np.isfinite(got[1, 8:11]).all() and got[1, 10] == float(val[10])


def check_phase_ramp(lib_path, N, L, n, seed=0):
    """t_phase_ramp, both signs, centre zero (item 0 of a stack of two or more) and centres up to half the largest radius -- the particle radius of the densities the
    averaging is run on (they are cut off at 0.5 r_max, scripts/bench_average.py) -- against phase_ref"""
    e = make_engine(N, L, 1, lib_path)
    rng = np.random.default_rng(500 + N + n + seed)
    X = rng.normal(size=(n,) + e.shape) + 1j * rng.normal(size=(n,) + e.shape)
    centers = rng.normal(size=(n, 3))
    centers *= (0.5 * e.r_max * np.linspace(1.0, 0.3, n) / np.linalg.norm(centers, axis=1))[:, None]
    if n >= 2:
        centers[0] = 0
    if n >= 3:
        X[n - 1] = 0
    got = {sign: e.t_phase_ramp(_tensor(e, X), centers, sign).cpu().numpy() for sign in (1.0, -1.0)}
    qs, cos_theta = e.qs, e.cos_theta
    e.close()
    worst = 0.0
    for sign in (1.0, -1.0):
        for i in range(n):
            ref = SR.phase_ref(X[i], centers[i], sign, qs, cos_theta)
            if i == n - 1 and n >= 3:
                assert not got[sign][i].any()
            err = _rel_max(got[sign][i], ref)
            worst = max(worst, err)
            assert err <= TOL, (sign, i, err)
    if n >= 2:
        assert np.array_equal(got[1.0][0], X[0]) and np.array_equal(got[-1.0][0], X[0])  # centre zero: the identity, exactly
    report('phase_ramp %dx%s n%d' % (N, 'x'.join(map(str, e.shape[1:])), n), err_over_tol=worst / TOL,
           largest_phase=float(np.max(qs) * np.linalg.norm(centers, axis=1).max()))
    return worst


def check_combine(lib_path, N, L, n, seed=0):
    """t_combine, the five operations, and conj / scale / affine in place (dst == a) through the C ABI, against longdouble"""
    e = make_engine(N, L, 1, lib_path)
    rng = np.random.default_rng(700 + N + n + seed)
    A = rng.normal(size=(n,) + e.shape) + 1j * rng.normal(size=(n,) + e.shape)
    A *= (1.0 + np.arange(n))[:, None, None, None]
    if n >= 2:
        A[n // 2] = 0
    scalars = {'conj': None, 'sum': None, 'abs2sum': None, 'scale': rng.normal(size=n) + 1j * rng.normal(size=n),
               'affine': np.array([0.3 - 1.1j, -0.7 + 0.2j])}
    code = {'conj': 0, 'scale': 1, 'sum': 2, 'abs2sum': 3, 'affine': 4}
    worst = 0.0
    for op in ('conj', 'scale', 'sum', 'abs2sum', 'affine'):
        ref = SR.combine_ref(op, A, scalars[op])
        outs = [e.t_combine(op, _tensor(e, A), scalars[op]).cpu().numpy()]
        if op in ('conj', 'scale', 'affine'):
            At = _tensor(e, A)
            sc = None if scalars[op] is None else np.ascontiguousarray(scalars[op], dtype=np.complex128)
            p = ctypes.c_void_p(At.data_ptr())
            e._ck(e.lib.mtip_op_grid_combine(e.ctx, code[op], p, p, n, _lib.ptr(sc) if sc is not None else None))
            outs.append(At.cpu().numpy())
        for out in outs:
            assert out.shape == ref.shape, (op, out.shape)
            items = [(out, ref)] if op in ('sum', 'abs2sum') else list(zip(out, ref))
            for i, (o, r) in enumerate(items):
                if op not in ('sum', 'abs2sum', 'affine') and n >= 2 and i == n // 2:
                    assert not o.any(), (op, i)
                err = _rel_max(o, r)
                worst = max(worst, err)
                assert err <= TOL, (op, i, err)
            if op == 'conj':
                assert np.array_equal(out, A.conj())
    e.close()
    report('combine %dx%s n%d' % (N, 'x'.join(map(str, e.shape[1:])), n), err_over_tol=worst / TOL)
    return worst


def prtf_inputs(seed, shape):
    """a1, a2 complex, I1, I2 >= 0 with the three rules of resolution_metrics.py:62-78 and the branch cut of the square root
    planted: shell 0 has a1 = a2 and I = |a|^2 (PRTF 1, deviation 0), shell 1 has I1 = I2 = 0 throughout; elsewhere single points
    with I1 or I2 zero and amplitudes zero / non-zero, and ratios a1 conj(a2) on the negative real axis whose imaginary part is
    +0.0 and -0.0.  (Only axis-aligned amplitudes: their products are exact zeros with a definite sign whatever the compiler
    contracts; numpy's own complex division returns +0 for both, so every such point is +i.)"""
    rng = np.random.default_rng(seed)
    N = shape[0]
    a1 = rng.normal(size=shape) + 1j * rng.normal(size=shape)
    a2 = a1 * (1 + 0.3 * rng.normal(size=shape)) + 0.2 * (rng.normal(size=shape) + 1j * rng.normal(size=shape))
    I1 = np.abs(a1) ** 2 * rng.uniform(0.8, 1.5, size=shape)
    I2 = np.abs(a2) ** 2 * rng.uniform(0.8, 1.5, size=shape)
    a2[0] = a1[0]
    I1[0] = I2[0] = a1[0].real ** 2 + a1[0].imag ** 2
    if N > 1:
        I1[1] = I2[1] = 0
        a1[1, 0, :2] = 0
    q = N - 1
    pz, nz = 0.0, -0.0
    planted = [  # (a1, a2, I1, I2)
        (1 + 2j, 2 - 1j, 0.0, 1.0), (1 + 2j, 2 - 1j, 1.0, 0.0), (0j, 2 - 1j, 0.0, 1.0), (1 + 2j, 0j, 0.0, 0.0), (0j, 0j, 0.0, 0.0),
        (0j, 0j, 1.0, 2.0), (complex(-2, pz), complex(3, pz), 1.0, 4.0), (complex(2, pz), complex(-3, pz), 1.0, 4.0),
        (complex(-2, nz), complex(3, pz), 1.0, 4.0), (complex(2, nz), complex(-3, nz), 1.0, 4.0), (complex(-2, pz), complex(3, nz), 2.0, 2.0),
        (complex(pz, 2), complex(pz, -3), 1.0, 4.0), (complex(nz, -2), complex(pz, 3), 1.0, 4.0), (complex(nz, 2), complex(nz, -3), 1.0, 1.0),
        (complex(2, nz), complex(3, pz), 1.0, 4.0)]
    for i, (x1, x2, i1, i2) in enumerate(planted):
        t, p = divmod(i, shape[2])
        a1[q, t, p], a2[q, t, p], I1[q, t, p], I2[q, t, p] = x1, x2, i1, i2
    return a1, a2, I1.astype(complex), I2.astype(complex)


def check_prtf(lib_path, N, L, seed=0):
    """t_prtf against prtf_ref: general inputs with the rules and the branch cut planted, and the single-input form"""
    e = make_engine(N, L, 1, lib_path)
    a1, a2, I1, I2 = prtf_inputs(900 + N + seed, e.shape)
    worst_mean, worst_std = 0.0, 0.0
    for x1, x2, j1, j2 in ((a1, a2, I1, I2), (a1, a1, I1, I1)):
        p, sd = e.t_prtf(_tensor(e, x1), _tensor(e, x2), _tensor(e, j1), _tensor(e, j2))
        mean, std, mag = SR.prtf_ref(x1, x2, j1, j2)
        npts = e.shape[1] * e.shape[2]
        for q in range(N):
            diff = float(np.abs(p[q].astype(SR.CLD) - mean[q]))
            bound = TOL * float(mag[q]) / npts
            assert diff <= bound, ('mean', q, p[q], complex(mean[q]), diff, bound)
            if bound > 0:
                worst_mean = max(worst_mean, diff / bound)
            dsd = abs(float(np.longdouble(sd[q]) - std[q]))
            bound_sd = max(TOL_STD_REL * float(std[q]), TOL_STD_FLOOR)
            assert dsd <= bound_sd, ('std', q, sd[q], float(std[q]))
            worst_std = max(worst_std, dsd / bound_sd)
    e.close()
    assert abs(complex(mean[0]) - 1) < 1e-15                          # (single input form: shell 0 is exactly on the positive real axis)
    report('prtf %dx%s' % (N, 'x'.join(map(str, e.shape[1:]))), mean_over_tol=worst_mean, std_over_tol=worst_std)
    return worst_mean, worst_std

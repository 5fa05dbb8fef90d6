"""Cases of the 2-D averaging (xframe_amd.fxs.average.average_reconstructions_2d, the mtip2d_avg_* / mtip2d_op_grid_* operators of
csrc/k_average2d.h), shared by the CPU emulator suite (tests/test_emul_average2d.py, lib_path = the emulation build) and the MI355X
suite (tests/test_gpu_average2d.py, lib_path = None).  The yardstick is tests/average2d_reference.py: the operators in longdouble
within the project's operator bound (1e-12, stated on the sum of the magnitudes of the summed terms), the flow in double precision
on the transforms of oracle/polar2d.py within the project's flow bound (1e-10 relative L2)."""
import numpy as np

import average2d_reference as AR
from helpers import rel_l2
from oracle import polar2d as OP
from xframe_amd.fxs.average import average_reconstructions_2d
from xframe_amd.fxs.polar2d import Engine2D

TOL = 1e-12                      # operators (README)
TOL_FLOW = 1e-10                 # flows, relative L2
MARGIN = 1e-6                    # |diff - diff_inv| / max(diff, diff_inv) of every member of a flow case: rounding cannot flip a decision
MAX_Q = 2.0
LD, CLD = AR.LD, AR.CLD

SHAPES_CPU = [(12, 6), (8, 64)]
SHAPES_GPU = SHAPES_CPU + [(128, 64)]
STACKS = [1, 2, 5]               # on an engine with n_batch = 2: a full chunk, a tail, more than one trip


def make_engine(N, M, B, lib_path):
    return Engine2D(N, M, MAX_Q, n_batch=B, lib_path=lib_path)


def report(case, **figures):
    print('AVG2D %-44s %s' % (case, '  '.join('%s=%.3g' % kv for kv in figures.items())), flush=True)


def _tensor(e, x):
    import torch
    return torch.from_numpy(np.array(x)).to(e.torch_device())          # (a copy: under the emulation device memory is host memory)


def _np(x):
    return x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)


def cplx(rng, shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def _rel_max(got, ref):
    scale = float(np.max(np.abs(ref)))
    diff = float(np.max(np.abs(np.asarray(got).astype(ref.dtype) - ref)))
    return diff / scale if scale > 0 else diff


def edge_stack(seed, n, shape):
    """stacks whose grids take every branch of the statistics: 'mixed' (zeros in Re with Im of both signs among normal numbers),
    'nopos' (no entry > 0 in numpy's order), 'zero'"""
    rng = np.random.default_rng(seed)
    kinds = (['mixed', 'nopos', 'mixed', 'zero', 'mixed'] * n)[:n]
    out = []
    for i, k in enumerate(kinds):
        g = cplx(rng, shape) * (1.0 + 0.5 * i)
        if k == 'mixed':
            g.real[rng.random(shape) < 0.2] = 0.0
        elif k == 'nopos':
            g = -np.abs(g.real) - 1j * np.abs(g.imag)
            g.real[rng.random(shape) < 0.2] = 0.0
        else:
            g[:] = 0
        out.append(g)
    return np.stack(out), kinds


# ------------------------------------------------------------------------------------------------------------------ 1. operators
def check_transform_chunks(lib_path, N, M, n, seed=0):
    """t_fourier_transform / t_harmonic of a stack of n on n_batch = 2 against the batched operators on full batches, bit for bit"""
    e = make_engine(N, M, 2, lib_path)
    X = cplx(np.random.default_rng(40 + n + seed), (n,) + e.shape)
    for name, fn in (('ft', e.fourier_transform), ('harmonic', e.harmonic)):
        t_fn = e.t_fourier_transform if name == 'ft' else e.t_harmonic
        for inverse in (False, True):
            got = _np(t_fn(_tensor(e, X), inverse))
            got_np = t_fn(X, inverse)
            for i in range(n):
                ref = fn(X[i], inverse)[0]
                assert np.array_equal(got[i], ref) and np.array_equal(got_np[i], ref), (name, inverse, i)
    e.close()


def check_grid_stats(lib_path, N, M, n, seed=0):
    e = make_engine(N, M, 2, lib_path)
    X, kinds = edge_stack(300 + N + n + seed, n, e.shape)
    got = e.t_grid_stats(_tensor(e, X))
    single = np.stack([e.t_grid_stats(_tensor(e, X[i:i + 1]))[0] for i in range(n)])
    assert np.array_equal(got, single, equal_nan=True)              # a grid's statistics do not depend on the stack
    assert np.array_equal(got, e.t_grid_stats(X), equal_nan=True)   # host pointers
    rs = e.rs
    e.close()
    worst = 0.0
    for i in range(n):
        val, mag = AR.stats_ref(X[i], rs)
        for k in (3, 6, 7, 8):
            assert got[i, k] == float(val[k]), (i, kinds[i], k, got[i, k], float(val[k]))
        for k in (0, 1, 2, 4, 5):
            diff = abs(float(LD(got[i, k]) - val[k]))
            assert diff <= TOL * float(mag[k]), (i, kinds[i], k, got[i, k], float(val[k]))
            if mag[k] > 0:
                worst = max(worst, diff / float(mag[k]))
        if kinds[i] in ('nopos', 'zero'):
            assert got[i, 6] == 0 and got[i, 3] == -np.inf
    report('grid_stats %dxM%d n%d' % (N, M, n), err_over_tol=worst / TOL)


def check_phase_ramp(lib_path, N, M, n, seed=0):
    e = make_engine(N, M, 2, lib_path)
    rng = np.random.default_rng(500 + N + n + seed)
    X = cplx(rng, (n,) + e.shape)
    centers = rng.normal(size=(n, 2))
    centers *= (0.5 * e.r_max * np.linspace(1.0, 0.3, n) / np.linalg.norm(centers, axis=1))[:, None]
    if n >= 2:
        centers[0] = 0
    got = {sign: _np(e.t_phase_ramp(_tensor(e, X), centers, sign)) for sign in (1.0, -1.0)}
    host = X.copy()
    assert e.t_phase_ramp(host, centers, 1.0) is host and np.array_equal(host, got[1.0])       # in place, host pointers too
    qs = e.qs
    e.close()
    worst = 0.0
    for sign in (1.0, -1.0):
        for i in range(n):
            err = _rel_max(got[sign][i], AR.phase_ref(X[i], centers[i], sign, qs))
            worst = max(worst, err)
            assert err <= TOL, (sign, i, err)
    if n >= 2:
        assert np.array_equal(got[1.0][0], X[0]) and np.array_equal(got[-1.0][0], X[0])        # centre zero: the identity, exactly
    report('phase_ramp %dxM%d n%d' % (N, M, n), err_over_tol=worst / TOL, largest_phase=float(np.max(qs) * np.linalg.norm(centers, axis=1).max()))


def check_inversion_metric(lib_path, N, M, n, seed=0):
    e = make_engine(N, M, 2, lib_path)
    rng = np.random.default_rng(600 + N + n + seed)
    F, ref = cplx(rng, (n,) + e.shape), cplx(rng, e.shape)
    F[n - 1] = ref.conj()                                            # the reference's point inverse: diff_inv = 0 exactly
    got = e.t_inversion_metric(_tensor(e, F), _tensor(e, ref))
    single = np.stack([e.t_inversion_metric(_tensor(e, F[i:i + 1]), _tensor(e, ref))[0] for i in range(n)])
    assert np.array_equal(got, single)
    qs = e.qs
    e.close()
    worst = 0.0
    for i in range(n):
        d0, d1, mag = AR.inversion_metric_ref(F[i], ref, qs)
        for g, v in ((got[i, 0], d0), (got[i, 1], d1)):
            diff = abs(float(LD(g) - v))
            assert diff <= TOL * float(mag), (i, g, float(v))
            worst = max(worst, diff / float(mag))
    assert got[n - 1, 1] == 0.0 and got[n - 1, 0] > 0
    report('inversion_metric %dxM%d n%d' % (N, M, n), err_over_tol=worst / TOL)


def check_combine(lib_path, N, M, n, seed=0):
    e = make_engine(N, M, 2, lib_path)
    rng = np.random.default_rng(700 + N + n + seed)
    A = cplx(rng, (n,) + e.shape) * (1.0 + np.arange(n))[:, None, None]
    if n >= 2:
        A[n // 2] = 0
    div = cplx(rng, n)
    div[0] = 1.7                                                     # a real divisor (normalisation mode 'max')
    scalars = {'conj': None, 'div': div, 'mean': [n], 'abs2mean': [n], 'affine': [-0.4, 2.5]}
    worst = 0.0
    for op, sc in scalars.items():
        got = _np(e.t_combine(op, _tensor(e, A), sc))
        assert np.array_equal(got, e.t_combine(op, A, sc))           # host pointers
        ref = AR.combine_ref(op, A, sc)
        assert got.shape == ref.shape
        if op == 'conj':
            assert np.array_equal(got, A.conj())
            continue
        err = _rel_max(got, ref)
        worst = max(worst, err)
        assert err <= TOL, (op, err)
    e.close()
    report('combine %dxM%d n%d' % (N, M, n), err_over_tol=worst / TOL)


def curve_inputs(seed, shape):
    """(a_d, a_ft, I_d, I_ft) that take every rule of PRTF (resolution_metrics.py:66-69) and the zero denominator of _fsc: shell 1 has
    b1 == 0 everywhere (with a != 0: points become 0), shell 2 has b2 == 0 and a_d == 0 on half of it (points stay 1), shell 3 has
    a_d == 0 (FSC denominator 0 -> 1), scattered zeros of either intensity elsewhere"""
    rng = np.random.default_rng(seed)
    a_d, a_ft = cplx(rng, shape), cplx(rng, shape)
    I_d, I_ft = np.abs(cplx(rng, shape)) ** 2, np.abs(cplx(rng, shape)) ** 2
    I_d[rng.random(shape) < 0.1] = 0
    I_ft[rng.random(shape) < 0.1] = 0
    I_d[1] = 0
    I_ft[2] = 0
    a_d[2, ::2] = 0
    a_d[3] = 0
    return a_d, a_ft, I_d + 0j, I_ft + 0j


def check_curves(lib_path, N, M, seed=0):
    e = make_engine(N, M, 2, lib_path)
    a_d, a_ft, I_d, I_ft = curve_inputs(900 + N + seed, e.shape)
    mean, std, fsc = e.t_curves(*[_tensor(e, x) for x in (a_d, a_ft, I_d, I_ft)])
    mean_h, std_h, fsc_h = e.t_curves(a_d, a_ft, I_d, I_ft)
    assert np.array_equal(mean, mean_h) and np.array_equal(std, std_h) and np.array_equal(fsc, fsc_h)
    e.close()
    n_phi = e.n_phi
    worst = 0.0
    variants = ((a_d, a_ft, I_d, I_ft), (a_d, a_d, I_d, I_d), (a_ft, a_ft, I_ft, I_ft), (a_d, a_d, I_ft, I_ft))
    for k, args in enumerate(variants):
        rmean, rstd, mag = AR.prtf_ref(*args)
        nd = AR.prtf_points(args[0], args[1], np.sqrt(args[2].real), np.sqrt(args[3].real))
        for q in range(N):
            diff = float(np.abs(mean[k, q].astype(CLD) - rmean[q]))
            bound = TOL * float(mag[q]) / n_phi
            assert diff <= bound, ('mean', k, q, mean[k, q], complex(rmean[q]))
            dsd = abs(float(LD(std[k, q]) - rstd[q]))
            bound_sd = TOL * float(np.max(np.abs(nd[q])))             # |d std| <~ eps max|nd| (Cauchy-Schwarz on the deviations)
            assert dsd <= bound_sd, ('std', k, q, std[k, q], float(rstd[q]))
            worst = max(worst, diff / bound if bound > 0 else 0.0, dsd / bound_sd if bound_sd > 0 else 0.0)
    assert mean[0, 1] == 0 and std[0, 1] == 0                         # b1 == 0 with a1, a2 != 0: every point 0
    rfsc, mag = AR.fsc_ref(a_d, a_ft)
    for q in range(N):
        assert abs(float(LD(fsc[q]) - rfsc[q])) <= TOL * float(mag[q]), ('fsc', q, fsc[q], float(rfsc[q]))
    assert fsc[3] == 1.0
    report('curves %dxM%d' % (N, M), err_over_tol=worst)


def fqcb_inputs(seed, N, n1, n2):
    rng = np.random.default_rng(seed)
    t1, t2 = cplx(rng, (N, n1)), cplx(rng, (N, n2))
    t1[N // 2] = 0                                                   # row and column of B_n vanish: denominator 0, bb = 1
    t2 = t2 + 0.5 * t1[:, :n2] if n2 <= n1 else t2
    stack = cplx(rng, (n2, N, N))                                    # a B_n stack that is not Hermitian: the symmetrisation matters
    return t1, t2, stack


def check_fqcb(lib_path, N, M, seed=0):
    """t_fqcb for tables and stacks, odd and even o_stop, all four (skip_odd_orders, include_zero_order), against fqcb_2d in
    longdouble (absolute bound: |bb| <= 1 and, by Cauchy-Schwarz, the summed terms of its numerator are below its denominator);
    t_deg2_from_table against deg2_from_table"""
    e = make_engine(N, M, 2, lib_path)
    worst = 0.0
    for n1, n2 in ((M + 1, M + 1), (M + 1, M), (5, 7)):
        t1, t2, stack = fqcb_inputs(1100 + N + n1 + seed, N, n1, n2)
        wide = np.concatenate([t1, cplx(np.random.default_rng(1), (N, 3))], axis=1)      # ld > n: only the first n1 columns are read
        B1, B2 = AR.deg2_from_table(t1.astype(CLD)), AR.deg2_from_table(t2.astype(CLD))
        got_B = _np(e.t_deg2_from_table(_tensor(e, wide), n1))
        assert _rel_max(got_B, B1) <= TOL and got_B.shape == (n1, N, N)
        for skip in (False, True):
            for zero in (False, True):
                for a, b, ra, rb in (((_tensor(e, wide), n1), _tensor(e, t2), B1, B2), (t1, _tensor(e, stack), B1, stack.astype(CLD)),
                                     (stack, t1, stack.astype(CLD), B1)):
                    mean, std = e.t_fqcb(a, b, skip_odd_orders=skip, include_zero_order=zero)
                    rmean, rstd = AR.fqcb_2d(ra, rb, skip_odd_orders=skip, include_zero_order=zero)
                    dm, ds = float(np.max(np.abs(mean.astype(LD) - rmean))), float(np.max(np.abs(std.astype(LD) - rstd)))
                    assert dm <= TOL and ds <= TOL, (n1, n2, skip, zero, dm, ds)
                    worst = max(worst, dm, ds)
                    assert mean[N // 2] == 1.0 and std[N // 2] == 0.0 or ra is not B1 and rb is not B1
    e.close()
    report('fqcb %dxM%d' % (N, M), err_over_tol=worst / TOL)


# ----------------------------------------------------------------------------------------------------------------------- 2. flow
def flow_problem(seed, N, M, n, ref_pos):
    """a seeded stack of n reconstructions: perturbed copies of one asymmetric complex density (so that Im F is large), the members at
    odd positions replaced by the point inverse (IFT(conj(FT rho)), conj(F)) of their copy; errors with the least at `ref_pos`;
    projection matrices of two 'files' (M + 1 and M orders are both exercised by the callers)"""
    fp = OP.PolarFourierPair(N, M, MAX_Q)
    rng = np.random.default_rng(seed)
    r, p = np.meshgrid(fp.rs, fp.phis, indexing='ij')
    rmax = r.max()
    x, y = r * np.cos(p), r * np.sin(p)

    def blob(cx, cy, w):
        return np.exp(-((x - cx * rmax) ** 2 + (y - cy * rmax) ** 2) / (w * rmax) ** 2)
    base = (blob(0.15, -0.1, 0.2) + 0.6 * blob(-0.25, 0.2, 0.12)) * (1 + 0.3j) - 0.05 * blob(0, 0, 0.45)
    recs = []
    for i in range(n):
        # the members differ by smooth features, as reconstructions do: white noise on the polar grid is outside what the discrete
        # transform pair resolves, and IFT(FT(.)) amplifies the rounding of either implementation on it
        c = 0.3 * rng.normal(size=(3, 2))
        rho = base * (1.0 + 0.2 * i) + sum(0.1 * (1 + 0.5j * k) * blob(c[k, 0], c[k, 1], 0.15) for k in range(3))
        F = fp.ft(rho) * (1 + 0.05 * blob(c[0, 0], c[0, 1], 0.5))
        if i % 2 == 1:
            rho, F = fp.ift(fp.ft(rho).conj()), F.conj()
        recs.append([rho, F])
    errors = 1.0 + rng.random(n)
    errors[ref_pos] = 0.5
    files = [np.arange(0, n // 2), np.arange(n // 2, n)] if n >= 4 else [np.arange(n)]
    pms = [[cplx(rng, (N,)) for _ in range(M + 1)] for _ in files]
    return fp, recs, errors, files, pms


def _flow_ref(fp, N, M, recs, errors, opt, pms, files):
    fl = AR.Flow2D(fp.rs, fp.qs, fp.n_phi, fp.ft, fp.ift, OP.harmonic_forward)
    return AR.run_2d_ref(fl, recs, errors, opt, pms, files)


def _compare(got, ref, path=''):
    worst = 0.0
    if isinstance(ref, dict):
        assert set(ref) <= set(got), (path, sorted(set(ref) - set(got)))
        for k in ref:
            worst = max(worst, _compare(got[k], ref[k], path + '/' + k))
        return worst
    if isinstance(ref, (list, bool, int)):
        assert got == ref, (path, got, ref)
        return 0.0
    g, r = _np(got), np.asarray(ref)
    assert g.shape == r.shape, (path, g.shape, r.shape)
    if path.startswith('/inversion_metric'):
        assert g[2] == r[2] and np.allclose(g[:2], r[:2], rtol=TOL, atol=0), (path, g, r)
        return 0.0
    err = rel_l2(g, r) if r.size > 1 else float(np.abs(g - r).ravel()[0] / np.abs(r).ravel()[0])
    assert err < TOL_FLOW, (path, err)
    return float(err)


FLOW_OPTIONS = {
    'max': {},
    'mean': {'normalize_reconstructions': {'use': True, 'mode': 'mean'}},
    'no_norm_no_center': {'normalize_reconstructions': {'use': False}, 'center_reconstructions': False},
    'pointinvert_reference': {'pointinvert_reference': True},
    'cut': {'selection': {'n_reconstructions': 3}},
}
FLOW_STACKS = [(2, 0), (5, 2), (9, 8)]          # (n, position of the reference): first, middle, last


def flow_opt(name, metrics=('PRTF', 'pseudo_FSC', 'FQCB')):
    o = {'center_reconstructions': True, 'normalize_reconstructions': {'use': True, 'mode': 'max'}, 'pointinvert_reference': False,
         'selection': {'n_reconstructions': 100}, 'resolution_metrics': {m: True for m in metrics}}
    o.update(FLOW_OPTIONS[name])
    return o


def check_flow(lib_path, n, ref_pos, name, N=12, M=6, n_batch=2, seed=0):
    fp, recs, errors, files, pms = flow_problem(2000 + 10 * n + seed, N, M, n, ref_pos)
    opt = flow_opt(name)
    ref = _flow_ref(fp, N, M, recs, errors, opt, pms, files)
    # the decisions of the restatement are far from a tie, so rounding cannot flip one
    for k, m in ref['inversion_metric'].items():
        assert abs(m[0] - m[1]) / max(m[0], m[1]) > MARGIN, (k, m)
    flags = ref['point_inverted']
    assert ref['reference_arg'] == ref_pos
    if n >= 5:
        assert sum(flags) >= 2 and not all(flags)
    e = make_engine(N, M, n_batch, lib_path)
    got = average_reconstructions_2d(e, recs, errors, opt, pms, files)
    dev = average_reconstructions_2d(e, [[_tensor(e, r[0]), _tensor(e, r[1])] for r in recs], errors, dict(opt, keep_on_device=True), pms, files)
    e.close()
    worst = _compare(got, ref)
    assert got['n_averaged'] == len(ref['aligned'])
    import torch
    assert all(torch.is_tensor(v['real_density']) for v in dev['aligned'].values())
    assert np.array_equal(_np(dev['aligned']['0']['reciprocal_density']), got['aligned']['0']['reciprocal_density'])
    assert np.array_equal(dev['average']['real_density'], got['average']['real_density'])
    # the averaged reciprocal density that is saved is the one the centring shifted in place (average.py:246)
    assert np.array_equal(got['average']['reciprocal_density'], got['centered_average']['reciprocal_density'])
    report('flow n%d ref%d %s' % (n, ref_pos, name), worst_rel_l2=worst, n_inverted=sum(flags))
    return got


def check_split_invariance(lib_path, N=12, M=6, n=5):
    """the same stack through engines with n_batch 1, 2 and 5: bit-equal results"""
    fp, recs, errors, files, pms = flow_problem(3000, N, M, n, 2)
    opt = flow_opt('max')
    outs = []
    for B in (1, 2, 5):
        e = make_engine(N, M, B, lib_path)
        outs.append(average_reconstructions_2d(e, recs, errors, opt, pms, files))
        e.close()

    def same(a, b, path=''):
        if isinstance(a, dict):
            assert set(a) == set(b)
            for k in a:
                same(a[k], b[k], path + '/' + k)
        elif isinstance(a, np.ndarray):
            assert np.array_equal(a, b, equal_nan=True), path
        elif isinstance(a, list) and a and isinstance(a[0], (list, np.ndarray)):
            for x, y in zip(a, b):
                same(x, y, path)
        else:
            assert a == b, path
    same(outs[0], outs[1])
    same(outs[0], outs[2])


# --------------------------------------------------------------------------------------------------------------------- 6. raises
def check_raises(lib_path, N=12, M=6):
    import pytest
    fp, recs, errors, files, pms = flow_problem(4000, N, M, 3, 0)
    e = make_engine(N, M, 2, lib_path)
    with pytest.raises(NotImplementedError, match='154-161'):
        average_reconstructions_2d(e, recs, errors, dict(flow_opt('max', ('PRTF',)), use_masks=True))
    with pytest.raises(ValueError, match='projection_matrices'):
        average_reconstructions_2d(e, recs, errors, flow_opt('max'))
    with pytest.raises(ValueError):
        average_reconstructions_2d(e, recs[:1], errors[:1], flow_opt('max', ('PRTF',)))
    neg = [[-np.abs(r[0].real) + 0j, r[1]] for r in recs]          # no entry > 0: numpy's max of an empty selection raises (average.py:171)
    with pytest.raises(ValueError, match='zero-size'):
        average_reconstructions_2d(e, neg, errors, dict(flow_opt('max', ('PRTF',)), center_reconstructions=False))
    out = average_reconstructions_2d(e, neg, errors, dict(flow_opt('mean', ('PRTF',)), center_reconstructions=False))
    assert np.isnan(out['input_meta']['scaling_factors']).all()      # (178: the mean of an empty selection is nan, as upstream)
    e.close()


def check_bit_limit():
    from xframe_amd.fxs.average import fsc_bit_limit
    for shape in ((12, 13, 2), (128, 129, 2)):
        assert fsc_bit_limit(0.5, shape) == AR.fsc_bit_limit(0.5, np.zeros(shape))


# ------------------------------------------------------------------------------------------------------------- 7. emulator only
GUARDED = [(12, 6), (8, 64)]


def run_guarded(lib_path):
    """every new kernel at the shapes whose rows end at the ends of the buffers (run in a child process with MTIP_EMUL_GUARD=1: every
    device allocation is followed by an inaccessible page)"""
    for N, M in GUARDED:
        for n in (1, 5):
            check_grid_stats(lib_path, N, M, n)
            check_phase_ramp(lib_path, N, M, n)
            check_inversion_metric(lib_path, N, M, n)
            check_combine(lib_path, N, M, n)
        check_curves(lib_path, N, M)
        check_fqcb(lib_path, N, M)
    check_flow(lib_path, 5, 2, 'max')
    check_fsc_3d(lib_path)
    print('AVG2D_GUARDED_DONE', flush=True)


def flow_launches(n, n_inverted, n_batch, fqcb=True, curves=True):
    """kernel launches of average_reconstructions_2d with centring, normalisation and the given metrics: a transform
    of a stack of m grids is 3 launches per chunk of n_batch (harmonic, Hankel, harmonic), a harmonic transform one"""
    def chunks(m):
        return -(-m // n_batch)

    def ft(m):
        return 3 * chunks(m)
    total = 3 + 2 * ft(n)                          # centre: statistics, FT, ramp, IFT, ramp
    total += 3                                     # normalise: statistics, two divisions
    total += 1                                     # inversion metric
    total += (2 + 2 * ft(n_inverted)) if n_inverted else 0
    total += 4 + ft(n)                             # four means, FT of the aligned densities
    total += 3 + 2 * ft(1)                         # centre the average
    total += (ft(1) if (curves or fqcb) else 0) + (1 if curves else 0)
    total += (2 + chunks(2) + 5 + 3) if fqcb else 0    # two |.|^2, harmonic transform of the pair, five FQCB, three B_n arrays
    total += 4                                     # two normalised densities: statistics and the affine map each
    return total


def check_launch_count(lib_path, N=12, M=6):
    import parity_cases as PC
    fp, recs, errors, files, pms = flow_problem(2000 + 50, N, M, 5, 2)
    e = make_engine(N, M, 2, lib_path)
    PC.launched_kernels(e, prefixes=('k',))
    out = average_reconstructions_2d(e, recs, errors, flow_opt('max'), pms, files)
    log = PC.launched_kernels(e, prefixes=('k',))
    e.close()
    assert log is not None
    want = flow_launches(5, sum(out['point_inverted']), 2)
    assert sum(out['point_inverted']) == 2 and want == 74
    assert len(log) == want, (len(log), want, log)


# -------------------------------------------------------------------------------------------------------------- 4. extract in 2-D
def extract_problem(nq, L, n_delta, seed, negative_order=None):
    """synthetic 2-D cross-correlation from seeded rank-one B_n = v_n v_n^+ on the even orders (dimensions = 2: C_n = B_n,
    fxs_invariant_tools.py:813-839; the generator of tests/ccextract_cases.py for this dimension); `negative_order`: that order gets
    a negative definite matrix, whose leading eigenvalue is negative when the constraints are off"""
    import ccextract_cases as CC
    rng = np.random.default_rng(seed)
    qs = CC.radial_points(nq)
    env = np.exp(-qs / qs.max())
    bl = np.zeros((L + 1, nq, nq), complex)
    for n in range(0, L + 1, 2):
        v = (rng.normal(size=nq) + (1j * rng.normal(size=nq) if n else 0)) * env * np.exp(-0.3 * n)
        bl[n] = v[:, None] * v[None, :].conj()
        if n == negative_order:                                      # negative definite: the LEADING eigenvalue is negative too
            bl[n] = -(bl[n] + 0.05 * np.trace(bl[n]).real / nq * np.eye(nq))
    ccn = np.zeros((nq, nq, n_delta // 2 + 1), complex)
    ccn[..., :L + 1] = np.moveaxis(bl, 0, -1)
    cc = np.fft.irfft(ccn * n_delta, n_delta, axis=-1)
    avg = np.sqrt(np.abs(np.diagonal(bl[0]).real)) * (1 + 0.1 * rng.random(nq))
    return qs, np.arange(n_delta) * 2 * np.pi / n_delta, cc, avg, bl


def extract_2d(lib_path, qs, phis, cc, avg, L, lim, enforce_psd, modify_cc, method='back_substitution'):
    import ccextract_cases as CC
    from xframe_amd.fxs import extract as X, io as IO
    e = CC.small_engine(lib_path)
    ccd = IO.load_ccd({'cross_correlation': {'I1I1': cc.copy()}, 'radial_points': qs, 'angular_points': phis, 'average_intensity': avg,
                       'xray_wavelength': CC.WAVELENGTH})
    s = CC.flow_settings(L, lim, modify_cc=modify_cc, enforce_psd=enforce_psd, dimensions=2)
    s['cross_correlation']['datasets']['I1I1']['bl_extraction_method'] = method
    data = X.extract_from_cross_correlation(e, ccd, s)
    e.close()
    return data


def check_extract_2d(lib_path, nq=12, L=6, n_delta=32):
    """extract_from_cross_correlation with dimensions = 2 against the restatement: b_coeff <= 1e-12 (relative L2), the projection
    vectors through V V^+ (an eigenvector is free in its phase), keys and shapes, the zeroing branch of a negative leading eigenvalue"""
    import ccextract_cases as CC
    from xframe_amd.fxs import extract as X
    line = {'min': {'type': 'line', 'line': [[0.0, 0.1], [6.0, 0.25]]}, 'max': {'type': 'none'}}
    for name, lim, psd, mod, neg in (('plain', CC.MASK_CASES['none'], False, {}, None),
                                     ('psd_avg', CC.MASK_CASES['none'], True, CC.FLOW_MODIFY, None),
                                     ('line', line, True, CC.FLOW_MODIFY, None),
                                     ('negative', CC.MASK_CASES['none'], False, {}, 4)):
        qs, phis, cc, avg, bl = extract_problem(nq, L, n_delta, 77, neg)
        # the method is the 2-D Fourier series whatever bl_extraction_method says (extract.py:129-130)
        data = extract_2d(lib_path, qs, phis, cc, avg, L, lim, psd, mod, method='legendre' if name == 'plain' else 'back_substitution')
        b0, qmask = CC.r_cc_to_deg2(cc, 2, qs, phis, L, True, mod, avg)
        mask, ids = X.calc_deg_2_invariant_masks({'bl_q_limits': lim}, b0.shape, qmask, qs, L)
        rb, rv, rint = AR.extract_2d_ref(b0, ids, avg, qs, psd, bool(mod.get('subtract_average_intensity', False)))
        got_b = data['deg_2_invariant']['I1I1']
        err = rel_l2(got_b, rb)
        assert err <= TOL, (name, err)
        pms = data['data_projection_matrices']
        assert isinstance(pms, np.ndarray) and pms.shape == (L + 1, nq) and pms.dtype == complex
        scale = np.linalg.norm(rb)
        worst = 0.0
        for o in range(L + 1):
            vv, rr = pms[o][:, None] * pms[o][None, :].conj(), rv[o][:, None] * rv[o][None, :].conj()
            worst = max(worst, np.linalg.norm(vv - rr) / scale)
        assert worst <= TOL_FLOW, (name, worst)
        if name == 'plain':
            assert rel_l2(got_b, bl) <= 1e-11                     # (the synthetic B_n themselves, through the irfft / Fourier series pair)
        if neg is not None:
            assert not pms[neg].any() and not rv[neg].any() and pms[2].any()
        if name == 'line':
            lo = ids[:, 0, 0]
            assert lo.max() > 0 and all(not pms[o][:lo[o]].any() for o in range(L + 1))
        for k in CC.RECONSTRUCT_KEYS:
            assert k in data, k
        assert data['dimensions'] == 2 and data['max_order'] == L and data['data_low_resolution_intensity_coefficients'] is False
        assert np.isclose(data['integrated_intensity'], rint, rtol=1e-13)
        assert np.array_equal(data['deg_2_invariant_masks']['I1I1'], mask) and np.array_equal(data['deg_2_invariant_q_id_limits']['I1I1'], ids)
        assert data['data_projection_matrix_error_estimates']['I1I1'].shape == got_b.shape
        report('extract 2-D ' + name, b_rel_l2=err, vv_rel=worst)


def check_extract_2d_masked_raises(lib_path):
    import pytest
    import ccextract_cases as CC
    qs, phis, cc, avg, _ = extract_problem(8, 4, 16, 5)
    with pytest.raises(NotImplementedError, match='dimensions = 2'):
        extract_2d(lib_path, qs, phis, cc, avg, 4, CC.MASK_CASES['none'], False, {'interpolate_masked': True})


# ------------------------------------------------------------------------------------------------------------------- 5. the chain
def check_chain(lib_path, g):
    """cc -> extract (2-D) -> MTIP2D, a short schedule, 3 restarts -> average_reconstructions_2d with all three metrics, at the 2-D
    fixture's size (12 shells x M = 6): it runs, every returned array is finite, FQCB_bl_target is V V^+ of the extracted vectors"""
    import parity_cases as PC
    from xframe_amd.fxs.reconstruct2d import MTIP2D
    data0, o = PC.mtip2d_problem(g)
    pm0 = np.asarray(data0['data_projection_matrices'], dtype=complex)
    n_ord, nq = pm0.shape
    L = n_ord - 1
    n_delta = 4 * L + 8
    bl = pm0[:, :, None] * pm0[:, None, :].conj()
    bl[1::2] = 0
    bl[0] = bl[0].real
    ccn = np.zeros((nq, nq, n_delta // 2 + 1), complex)
    ccn[..., :L + 1] = np.moveaxis(bl, 0, -1)
    cc = np.fft.irfft(ccn * n_delta, n_delta, axis=-1)
    qs = np.asarray(data0['data_radial_points'], dtype=float)
    avg = np.asarray(getattr(data0['average_intensity'], 'data', data0['average_intensity']), dtype=float)
    import ccextract_cases as CC
    data = extract_2d(lib_path, qs, np.arange(n_delta) * 2 * np.pi / n_delta, cc, avg, L, CC.MASK_CASES['none'], False, {})
    main = o['main_loop']['sub_loops']['main']
    main['methods']['HIO']['iterations'] = 3
    main['methods']['ER']['iterations'] = 2
    main['iterations'] = 1
    rng = np.random.default_rng(9)
    rho0 = np.asarray(g['rho0'])
    m = MTIP2D(o, data, n_restarts=3, initial_densities=[rho0 * (1 + 0.2 * rng.random(rho0.shape)) for _ in range(3)], lib_path=lib_path,
               resident=True)
    res = m.phasing_loop()
    e = m.engine
    recs = [[r['real_density'], r['reciprocal_density']] for r in res]
    errors = [float(r['final_error']) for r in res]
    pms = [list(data['data_projection_matrices'])]
    out = average_reconstructions_2d(e, recs, errors, flow_opt('max'), pms, [np.arange(3)])
    m.close()

    def finite(x, path=''):
        if isinstance(x, dict):
            for k, v in x.items():
                finite(v, path + '/' + k)
        elif isinstance(x, np.ndarray) and x.dtype.kind in 'fc':
            assert np.isfinite(x).all(), path
    finite(out)
    assert {'PRTF', 'pseudo_FSC', 'FSC_0.5bit_limit', 'FQCB_from_density', 'FQCB_bl_target'} <= set(out['resolution_metrics'])
    v = np.asarray(data['data_projection_matrices']) / out['input_meta']['average_scaling_factors_per_file'][0] ** 2
    target = v[:, :, None] * v[:, None, :].conj()
    assert rel_l2(out['resolution_metrics']['FQCB_bl_target'], target) <= TOL
    assert out['n_averaged'] == 3 and len(out['inversion_metric']) == 2


# --------------------------------------------------------------------------------------------------------- 6. the 3-D pseudo FSC
def check_fsc_3d(lib_path, N=16, L=4):
    """mtip_op_fsc against _fsc in longdouble at 16 x L4 (a shell with a vanishing denominator included); average_reconstructions
    with resolution_metrics.pseudo_FSC adds the two keys of average.py:569-573 and changes nothing else, bit for bit; FQCB (`pass`
    upstream, 567-568) adds no key"""
    import align_cases as ALC
    from xframe_amd.fxs import average as AV
    e = ALC.make_engine(N, L, 2, lib_path)
    rng = np.random.default_rng(61)
    a1, a2 = cplx(rng, e.shape), cplx(rng, e.shape)
    a2 += 0.7 * a1
    a1[3] = 0
    got = e.t_fsc(ALC._tensor(e, a1), ALC._tensor(e, a2))
    ref, mag = AR.fsc_ref(a1.reshape(N, -1), a2.reshape(N, -1))
    for q in range(N):
        assert abs(float(LD(got[q]) - ref[q])) <= TOL * float(mag[q]), (q, got[q], float(ref[q]))
    assert got[3] == 1.0
    r = e.rs[:, None, None] / e.rs.max()
    recs = []
    for i in range(3):
        d = (np.exp(-(r / 0.4) ** 2) * (1 + 0.2 * rng.random(e.shape)) * (1 + 0.3 * i)).astype(complex)
        F = np.stack([d] * 2)
        recs.append((d, e.t_fourier_transform(ALC._tensor(e, F))[0].cpu().numpy()))
    errs = [0.3, 0.1, 0.2]
    opt = {'alignment_error_limit': 10.0, 'find_rotation': {'r_limit_ids': [0, N]}, 'keep_rotation_metrics': False}
    plain = AV.average_reconstructions(e, recs, errs, opt)
    both = AV.average_reconstructions(e, recs, errs, dict(opt, resolution_metrics={'PRTF': True, 'pseudo_FSC': True, 'FQCB': True}))
    assert set(both['resolution_metrics']) == set(plain['resolution_metrics']) | {'pseudo_FSC', 'FSC_0.5bit_limit'}
    for k, v in plain['resolution_metrics'].items():
        assert np.array_equal(v, both['resolution_metrics'][k], equal_nan=True), k
    for grp in ('average', 'centered_average'):
        for k, v in plain[grp].items():
            assert np.array_equal(v, both[grp][k], equal_nan=True), (grp, k)
    avg = both['average']
    a_d = e.t_fourier_transform(ALC._tensor(e, np.stack([avg['real_density']] * 2)))[0].cpu().numpy()
    ref, mag = AR.fsc_ref(a_d.reshape(N, -1), avg['reciprocal_density'].reshape(N, -1))
    assert np.max(np.abs(both['resolution_metrics']['pseudo_FSC'].astype(LD) - ref) / mag) <= TOL
    assert both['resolution_metrics']['FSC_0.5bit_limit'] == AR.fsc_bit_limit(0.5, np.zeros(e.shape + (3,)))
    e.close()

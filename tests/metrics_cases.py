"""Cases of the reciprocal-metric kernels (csrc/k_metrics.hip: k_metric_II, k_metric_ccd, k_metric_fold, k_metric_fqc,
k_metric_fqc_fold) at operator level, shared by tests/test_emul_metrics.py (CPU emulator) and tests/test_gpu_metrics.py (MI355X).

Inputs: the recipe of fixture G19 (tests/golden/make_golden.py, main_metrics) at any (N, L, B), seeded: qs = (arange(N) + 0.5) 0.012,
wavelength 1.23984, C_order 2, I_ref[l] complex normal (N, 2l+1) handed to hostsetup.invariant_metric_tables as the "projection
matrices", radial mask rng.random((L+1, N)) > 0.2 with mask[1] = True (so every (q, q') keeps at least one order >= 1: without it
fqc is 0 / 0 where all orders are masked), restart b = I_ref + s_b noise_b with s_b spread over [0.3, 1.0].

Two references, both on the host:
  (a) the oracle's fqc_error_routine / II_error_routine / ccd_diff_routine (oracle/metrics.py), which fixture G19 pins to the
      reference's own functions at 1e-13: catches a wrong table or convention;
  (b) a longdouble contraction of the very tables handed to the device with B_l = I_l I_l^+ (tables_reference, written from the
      header comments of k_metrics.hip): isolates the kernels' arithmetic and is the rounding yardstick.
Every case ASSERTS on the references alone, before it compares anything, that fqc_error is finite everywhere and that no (q, q') has
prod = average * reference_average <= 0 (the kernel's `fqc = 1` branch and a zero norm stay out of these inputs); no comparison here
uses equal_nan.

Bounds (the project's bound for operators is 1e-12, README):
  * II_error (1 - a ratio of order 1, close to 0 on these inputs) and fqc_error, per entry: |got - ref| <= 1e-12, against (a) and (b);
  * ccd_diff: |got - ref| <= 1e-12 |ref| against (b), rtol 1e-9 against (a) (the bound of the G19 check).
The references' own distance, (a) in fp64 against (b), is at most 3e-16 (II, fqc) and 6e-16 relative (ccd) at every shape.
Every case prints its figures on a line starting with 'METRICS'."""
import functools

import numpy as np

from oracle import metrics as M
from xframe_amd.fxs import _lib, hostsetup as hs
from xframe_amd.fxs.engine import Engine

TOL_OP = 1e-12
RTOL_CCD_ORACLE = 1e-9
WAVELENGTH, C_ORDER, Q_STEP = 1.23984, 2, 0.012
NAMES = ('II_error', 'ccd_diff', 'fqc_error')
FLAGS = {'II_error': 1, 'ccd_diff': 2, 'fqc_error': 4}
OWN_TABLES = {1: ('II_reference', 'qq'), 2: ('ccd_weights', 'ccd_reference', 'ccd_norm'),
              4: ('fqc_P', 'fqc_reference_average', 'fqc_reference_weights')}
LD, CLD = np.longdouble, np.clongdouble


def report(case, **figures):
    print('METRICS %-30s %s' % (case, '  '.join('%s=%.3g' % kv for kv in figures.items())), flush=True)


# ---------------------------------------------------------------------------------------------- the engine with the metrics armed
def metrics_engine(N, L, B, lib_path=None):
    """an engine of the grid alone (no data, no projection set-up): the metrics are armed by hand with arm_metrics"""
    return Engine({'grid': {'n_radial_points': N, 'max_order': L}}, None, n_batch=B, lib_path=lib_path, max_q=1.0)


def arm_metrics(e, t, which=7):
    """mtip_set_invariant_metrics on a live context with the tables t of hostsetup.invariant_metric_tables (what
    Engine._setup_projections does when it has data); a second call replaces the tables of the first"""
    def pp(key, conv):
        return _lib.ptr(conv(t[key])) if key in t else None
    e._im_keep = t                                                    # (the arrays must outlive the call)
    e._ck(e.lib.mtip_set_invariant_metrics(e.ctx, which, _lib.ptr(_lib.as_u8(t['zero_mask'])), pp('II_reference', _lib.as_c128),
                                           pp('qq', _lib.as_f64), pp('ccd_weights', _lib.as_f64), pp('ccd_reference', _lib.as_c128),
                                           float(t.get('ccd_norm', 0.0)), pp('fqc_P', _lib.as_f64), pp('fqc_reference_average', _lib.as_f64),
                                           pp('fqc_reference_weights', _lib.as_f64)))
    e.invariant_metrics = [n for n in NAMES if which & FLAGS[n]]


# ---------------------------------------------------------------------------------------------- inputs and references
def _cplx(rng, shape):
    return rng.normal(size=shape) + 1j * rng.normal(size=shape)


def tables_reference(t, restarts):
    """reference (b): the three metrics of every restart (a list of [I_0 .. I_L]) from the tables handed to the device, in longdouble,
    with B_l = I_l I_l^+.  Returns II (B,), ccd (B,), fqc (B, N) as longdouble and prod (B, N, N) = average * reference_average."""
    m = 1 - t['zero_mask'].astype(LD)                                                         # (L+1, N, N): 0 outside the invariant mask
    Bm = np.array([[a.astype(CLD) @ a.astype(CLD).conj().T for a in Ims] for Ims in restarts]) * m      # (B, L+1, N, N)
    nB, N = Bm.shape[0], Bm.shape[2]
    cur, ref, qq = Bm[:, 1:].sum(axis=1), t['II_reference'].astype(CLD), t['qq'].astype(LD)
    s = (1, 2)
    II = 1 - (np.sum(cur * ref * qq, axis=s) / np.sqrt(np.sum(cur * cur * qq, axis=s) * np.sum(ref * ref * qq))).real
    d = np.sum(Bm * t['ccd_weights'].astype(LD), axis=1) - t['ccd_reference'].astype(CLD)
    ccd = np.sum(d.real ** 2 + d.imag ** 2, axis=s) / LD(t['ccd_norm'])
    cr = np.zeros((nB,) + t['fqc_P'].shape[1:], LD)                                           # c_j(q, q') = sum_{l >= 1} B_l P_l[..., j]
    ci = np.zeros_like(cr)                                                                    # (real and imaginary part apart: P is real)
    for l in range(1, Bm.shape[1]):
        Pl = t['fqc_P'][l].astype(LD)
        for b in range(nB):
            cr[b] += Bm[b, l].real[..., None] * Pl
            ci[b] += Bm[b, l].imag[..., None] * Pl
    avg = cr[..., 0] ** 2 - ci[..., 0] ** 2 + 2 * np.sum(cr[..., 1:] ** 2 + ci[..., 1:] ** 2, axis=-1)
    ctrl = np.sum(Bm[:, 1:] * t['fqc_reference_weights'][1:].astype(LD), axis=1).real
    prod = avg * t['fqc_reference_average'].astype(LD)
    fq = np.where(prod >= 0, ctrl / np.sqrt(np.abs(prod)), LD(1))
    fqc = np.array([[1 - np.sum(fq[b, q, :q + 1]) / LD(q + 1) for q in range(N)] for b in range(nB)])
    return II, ccd, fqc, prod


class Problem:
    """seeded inputs at (N, L, B), the device tables, and both references of every restart"""

    def __init__(self, N, L, B, seed):
        rng = np.random.default_rng(seed)
        self.N, self.L, self.B, self.seed = N, L, B, seed
        self.qs = (np.arange(N) + 0.5) * Q_STEP
        Iref = [_cplx(rng, (N, 2 * l + 1)) for l in range(L + 1)]
        self.mask = rng.random((L + 1, N)) > 0.2
        self.mask[1] = True
        self.tables = hs.invariant_metric_tables(list(NAMES), self.qs, Iref, self.mask, WAVELENGTH, C_ORDER)
        scales = np.linspace(0.3, 1.0, B) if B > 1 else np.array([0.3])
        self.Ims = [[a + s * _cplx(rng, a.shape) for a in Iref] for s in scales]
        self.Ilm = np.stack([np.concatenate(ims, axis=1) for ims in self.Ims])                # (B, N, (L+1)^2)
        ref = np.array([a @ a.conj().T for a in Iref])
        used = {l: l for l in range(L + 1)}
        inv = self.mask[:, :, None] * self.mask[:, None, :]
        fq = M.fqc_error_routine(self.qs, ref, used, inv, WAVELENGTH)
        ii = M.II_error_routine(self.qs, ref, used, inv)
        cc = M.ccd_diff_routine(self.qs, ref, used, 2.0, inv, C_ORDER, WAVELENGTH)
        self.oracle = {'II_error': np.array([complex(ii(ims)).real for ims in self.Ims]),
                       'ccd_diff': np.array([complex(cc(ims)).real for ims in self.Ims]),
                       'fqc_error': np.array([fq(ims) for ims in self.Ims])}
        del fq, ii, cc
        II, ccd, fqc, prod = tables_reference(self.tables, self.Ims)
        self.exact = {'II_error': II, 'ccd_diff': ccd, 'fqc_error': fqc}
        self.min_prod = float(np.min(np.min(prod, axis=(1, 2)) / np.max(prod, axis=(1, 2))))
        for v in list(self.oracle.values()) + list(self.exact.values()):
            v.setflags(write=False)

    def assert_condition(self):
        """the inputs leave no room to hide behind NaN: asserted on the references alone"""
        for ref in (self.oracle, self.exact):
            for k in NAMES:
                assert np.isfinite(ref[k]).all(), (k, 'non-finite reference value', self.N, self.L, self.B)
        assert self.min_prod > 0, ('a (q, q\') with prod <= 0', self.min_prod)

    def yardstick(self):
        """(a) in fp64 against (b): absolute for II and fqc, relative for ccd"""
        o, x = self.oracle, self.exact
        return {'II_error': float(np.max(np.abs(o['II_error'] - x['II_error']))),
                'ccd_diff': float(np.max(np.abs(o['ccd_diff'] - x['ccd_diff']) / np.abs(x['ccd_diff']))),
                'fqc_error': float(np.max(np.abs(o['fqc_error'] - x['fqc_error'])))}


@functools.lru_cache(maxsize=3)
def problem(N, L, B, seed=1919):
    return Problem(N, L, B, seed)


def compare(p, got, names=NAMES, label=''):
    """the device's values `got` against both references of the problem p, every enabled metric; returns the worst figures"""
    p.assert_condition()
    fig = {}
    for k in names:
        g = np.asarray(got[k]).astype(LD)
        assert g.shape == p.exact[k].shape, (k, g.shape)
        assert np.isfinite(got[k]).all(), (k, 'non-finite device value')
        d_or, d_ex = np.abs(g - p.oracle[k]), np.abs(g - p.exact[k])
        if k == 'ccd_diff':
            d_or, d_ex = d_or / np.abs(p.oracle[k]), d_ex / np.abs(p.exact[k])
        fig[k] = float(np.max(d_ex))
        fig[k + '_vs_oracle'] = float(np.max(d_or))
    yard = p.yardstick()
    report('N%d L%d B%d %s' % (p.N, p.L, p.B, label), **{k.split('_')[0]: fig[k] for k in names},
           **{k.split('_')[0] + '_oracle': fig[k + '_vs_oracle'] for k in names}, **{k.split('_')[0] + '_yard': yard[k] for k in names},
           min_prod=p.min_prod)
    for k in names:
        assert yard[k] <= TOL_OP, ('the two references disagree', k, yard[k])
        assert fig[k] <= TOL_OP, (k, 'against the longdouble tables', fig[k])
        assert fig[k + '_vs_oracle'] <= (RTOL_CCD_ORACLE if k == 'ccd_diff' else TOL_OP), (k, 'against the oracle', fig[k + '_vs_oracle'])
    return fig


# ---------------------------------------------------------------------------------------------- the cases
def check_metrics(lib_path, N, L, B, seed=1919):
    """the three metrics of B restarts at (N, L) against both references; evaluated twice, the second bit-equal to the first"""
    p = problem(N, L, B, seed)
    p.assert_condition()
    e = metrics_engine(N, L, B, lib_path)
    arm_metrics(e, p.tables, 7)
    got = e.invariant_metrics_of(p.Ilm)
    again = e.invariant_metrics_of(p.Ilm)
    e.close()
    for k in NAMES:
        assert np.array_equal(got[k], again[k]), (k, 'differs between two calls on the same input')
    return compare(p, got)


def check_flag_subsets(lib_path, N=24, L=10, B=3):
    """which = 1, 2, 4, 5 return, for the enabled metrics, the bits of which = 7 (the same kernels, the same fold order); a subset
    armed with only its own tables (the others null) does too, and the metrics that are off are not returned"""
    p = problem(N, L, B)
    p.assert_condition()
    e = metrics_engine(N, L, B, lib_path)
    arm_metrics(e, p.tables, 7)
    full = e.invariant_metrics_of(p.Ilm)
    compare(p, full, label='which=7')
    for which in (1, 2, 4, 5):
        names = [n for n in NAMES if which & FLAGS[n]]
        own = {k: p.tables[k] for f, keys in OWN_TABLES.items() if which & f for k in keys}
        own['zero_mask'] = p.tables['zero_mask']
        for t in (p.tables, own):
            arm_metrics(e, t, which)
            got = e.invariant_metrics_of(p.Ilm)
            assert sorted(got) == sorted(names), (which, sorted(got))
            for k in names:
                assert np.array_equal(got[k], full[k]), (which, k, 'not the bits of which = 7')
    e.close()


def check_rearm(lib_path, N=24, L=10, B=3):
    """mtip_set_invariant_metrics a second time on the live context with the tables of another seed: the results follow the new
    tables (both references of the new problem), and back again they are the bits of the first round"""
    p1, p2 = problem(N, L, B), problem(N, L, B, 2020)
    assert not np.array_equal(p1.tables['zero_mask'], p2.tables['zero_mask'])
    e = metrics_engine(N, L, B, lib_path)
    arm_metrics(e, p1.tables, 7)
    first = e.invariant_metrics_of(p1.Ilm)
    compare(p1, first, label='first tables')
    arm_metrics(e, p2.tables, 7)
    compare(p2, e.invariant_metrics_of(p2.Ilm), label='re-armed')
    stale = e.invariant_metrics_of(p1.Ilm)                             # the first coefficients against the second tables: other values
    assert np.max(np.abs(stale['fqc_error'] - first['fqc_error'])) > 1e-3 and abs(stale['II_error'][0] - first['II_error'][0]) > 1e-3
    arm_metrics(e, p1.tables, 7)
    back = e.invariant_metrics_of(p1.Ilm)
    e.close()
    for k in NAMES:
        assert np.array_equal(back[k], first[k]), k

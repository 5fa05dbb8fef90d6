#!/usr/bin/env python3
"""tests/golden/cc_extract.npz (G24): the reference's route cross-correlation -> B_l -> V_l on seeded data.

Run:  python tests/golden/make_golden_cc.py         (build container only: needs the reference checkout make_golden.py names)

Outputs of the reference's OWN functions at 16 shells x L = 8 x 64 angles (and one array with 63 angles):
  * cross_correlation_to_deg2_invariant (fxs_invariant_tools.py:374-422) for every entry of ccextract_cases.VARIANTS: dim 3 with
    mode back_substitution (578-645), odd orders assumed zero and not, each modify_cc switch alone and all together; dim 2 (813-839);
  * InvariantExtractor.calc_deg_2_invariant_masks / apply_invariant_constraints (extract.py:332-430) on a stand-in `self` that holds
    exactly the attributes they read, for ccextract_cases.MASK_CASES;
  * the chain of extract_bl_from_cc + extract() after them (extract.py:160-167 B_0 replacement, 441-444 projection matrices and error
    estimate, 518 integrated intensity).
pygsl is absent: the slot `mathLibrary.gsl` gets the same kind of double as G19 (make_golden.main_metrics), built on
oracle/metrics.py's legendre_sphPlm_array and extended here by legendre_sphPlm_array_single_l (gsl_plugin.py:60-69) -- so the
back-substitution is the reference's code and the Legendre VALUES are not pinned.  The worker processes of
Multiprocessing.comm_module.request_mp_evaluation are replaced by a serial loop over the same arguments.
Only inputs and outputs (data) are written; no reference source is copied."""
import functools
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..'))

import make_golden as MG                                              # noqa: E402  (bootstrap, ShAdapter; puts the repository on sys.path)


def gsl_double():
    from oracle import metrics as OMx

    class GslDouble:
        @staticmethod
        def legendre_sphPlm_array(l_max, m_max, xs, return_orders=False, sorted_by_l=False):
            assert not sorted_by_l
            v, ls, ms = OMx.legendre_sphPlm_array(l_max, m_max, xs)
            return (np.squeeze(v), ls, ms) if return_orders else np.squeeze(v)

        @staticmethod
        def legendre_sphPlm_array_single_m(l_max, m, xs, return_orders=False):
            v, ls, ms = OMx.legendre_sphPlm_array_single_m(l_max, m, xs)
            return (np.squeeze(v), ls, ms) if return_orders else np.squeeze(v)

        @staticmethod
        def legendre_sphPlm_array_single_l(l, l_max, xs, return_orders=False):
            v, ls, ms = OMx.legendre_sphPlm_array(l, l, xs)          # ordered by m: the rows with l' = l are m = 0 .. l
            keep = ls == l
            v, ls, ms = v[keep], ls[keep], ms[keep]
            assert np.array_equal(ms, np.arange(l + 1))
            return (np.squeeze(v), ls, ms) if return_orders else np.squeeze(v)
    return GslDouble


def main():
    mods = MG.bootstrap()
    ml = mods['xframe.library.mathLibrary']
    pl = mods['xframe.library.pythonLibrary']
    mp = mods['xframe.Multiprocessing']
    ml.shtns = MG.ShAdapter
    ml.gsl = gsl_double()

    class Serial:
        @staticmethod
        def request_mp_evaluation(func, input_arrays=(), const_inputs=(), **kw):
            return [func(*args, *const_inputs) for args in zip(*input_arrays)]
    mp.comm_module = Serial
    it = importlib.import_module('xframe.projects.fxs.projectLibrary.fxs_invariant_tools')
    ex = importlib.import_module('xframe.projects.fxs.extract')
    import ccextract_cases as CC

    nq, L, nd = 16, 8, 64
    out = {'G24_L': np.array(L), 'G24_wavelength': np.array(CC.WAVELENGTH)}
    qs, phis, cc, avg, bl = CC.synthetic_cc(nq, L, nd, 2424, stride=1, noise=0.02)
    _, phis_odd, cc_odd, _, _ = CC.synthetic_cc(nq, L, nd - 1, 2425, stride=1, noise=0.02)
    assert qs.max() * CC.WAVELENGTH / (4 * np.pi) <= 0.1
    # condition of the worst pair's triangular matrix (rows m, columns l; stride 1)
    worst = 0.0
    cols = [CC.legendre_products(qs, l, 1) for l in range(L + 1)]
    for i in range(nq):
        for j in range(nq):
            T = np.zeros((L + 1, L + 1))
            for l in range(L + 1):
                T[:l + 1, l] = cols[l][i, j]
            worst = max(worst, np.linalg.cond(T))
    print('max q lambda / 4 pi = %.4f, worst triangular condition number %.1f' % (qs.max() * CC.WAVELENGTH / (4 * np.pi), worst))
    out.update({'G24_qs': qs, 'G24_avg': avg, 'G24_cc': cc, 'G24_cc_odd': cc_odd, 'G24_bl_true': bl})
    arrays = {'cc': (cc, phis), 'cc_odd': (cc_odd, phis_odd)}
    for name, (key, dim, zero_odd, mod) in CC.VARIANTS.items():
        c, p = arrays[key]
        meta = CC.metadata(qs, p, L, zero_odd, mod, avg)
        b, m = it.cross_correlation_to_deg2_invariant(c.copy(), dim, **meta)
        out[f'G24_{name}_b'], out[f'G24_{name}_qq_mask'] = np.asarray(b), np.asarray(m)
        print(name, b.shape, b.dtype, 'odd orders max', np.abs(b[1::2]).max(), 'mask all', m.all())
    # masks and constraints on a stand-in self
    cls = ex.InvariantExtractor if hasattr(ex, 'InvariantExtractor') else [v for v in vars(ex).values() if isinstance(v, type) and
                                                                          hasattr(v, 'calc_deg_2_invariant_masks')][0]
    me = types.SimpleNamespace(data_radial_points=qs, max_order=L)
    me.calc_deg_2_invariant_line_mask = functools.partial(cls.calc_deg_2_invariant_line_mask, me)
    to_ns = pl.DictNamespace.dict_to_dictnamespace
    qq = np.ones((nq, nq), bool)
    for name, lim in CC.MASK_CASES.items():
        dopt = to_ns({'bl_q_limits': lim, 'bl_enforce_psd': True})
        mask, ids = cls.calc_deg_2_invariant_masks(me, dopt, (L + 1, nq, nq), qq)
        out[f'G24_mask_{name}'], out[f'G24_qid_{name}'] = np.asarray(mask), np.asarray(ids)
        print('mask', name, mask.sum(), ids[:, 0, :].tolist())
    trapz = getattr(np, 'trapezoid', None) or np.trapz
    if not hasattr(np, 'trapz'):
        np.trapz = trapz
    out['G24_integrated_intensity'] = np.array(trapz(avg * qs ** 2, x=qs, axis=0) * 4 * np.pi)       # extract.py:518
    for name in ('none', 'line1'):
        dopt = to_ns({'bl_q_limits': CC.MASK_CASES[name], 'bl_enforce_psd': True})
        b = out['G24_sub_b'].copy()                                   # FLOW_MODIFY: subtract_average_intensity alone
        ids = out[f'G24_qid_{name}'].copy()
        bc = cls.apply_invariant_constraints(me, dopt, b, ids)
        bc[0] = avg[:, None] * avg[None, :] * 4 * np.pi               # extract.py:160-167
        pms, _ = it.deg2_invariant_to_projection_matrices(3, bc, q_id_limits=ids, sort_mode=0)
        err = it.calc_projection_matrix_error_estimate(bc, pms)
        out[f'G24_flow_{name}_b'], out[f'G24_flow_{name}_err'] = np.asarray(bc), np.asarray(err)
        for l, p in enumerate(pms):
            out[f'G24_flow_{name}_pm{l}'] = np.asarray(p)
    path = os.path.join(HERE, 'cc_extract.npz')
    np.savez_compressed(path, **out)
    print('cc extract fixture:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""tests/golden/cc_masked.npz (G27): the reference's route for MASKED cross-correlation data on the inputs of G24.

Run:  python tests/golden/make_golden_ccmask.py     (build container only: needs the reference checkout make_golden.py names)

Outputs of the reference's OWN functions on G24_cc / G24_qs / G24_avg (16 shells, L = 8, 64 angles, noise 0.02; cc_extract.npz):
  * cross_correlation_mask (fxs_invariant_tools.py:221-232) for every entry of ccmask_cases.MASK_SETTINGS: none, pixel_custom,
    pixel_flat, pixel_arc, each with mask_at_pi on and off; the 'direct' mask of ccmask_cases.direct_mask is stored beside them;
  * modify_cross_correlation (235-289) on the direct mask for every entry of ccmask_cases.PREPARE_VARIANTS (each switch alone, all
    together); the variant 'interp' is interpolate (335-351) called directly;
  * bl_3d_least_squares_worker (485-517) with the flattened mesh of all (q1, q2) ids (the Serial stand-in of make_golden_cc.py zips
    its input arrays and would only visit the diagonal), even orders and all orders, for ccmask_cases.LSQ_MASKS;
  * ccd_to_deg2_invariant_3d_back_substitution (578-645) on the direct mask;
  * for ccmask_cases.FLOWS the chain of extract_bl_from_cc + extract() (extract.py:134-167, 332-430, 441-444) as make_golden_cc.py
    runs it, with cross_correlation_to_deg2_invariant (374-422) in front; its request_mp_evaluation gets a stand-in that hands the
    worker the mesh of its two input arrays in one call.
The bootstrap is make_golden.py's, the `gsl` double make_golden_cc.py's.  Only inputs and outputs (data) are written."""
import functools
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..'))

import make_golden as MG                                              # noqa: E402
import make_golden_cc as MGC                                          # noqa: E402


def main():
    mods = MG.bootstrap()
    ml = mods['xframe.library.mathLibrary']
    pl = mods['xframe.library.pythonLibrary']
    mp = mods['xframe.Multiprocessing']
    ml.shtns = MG.ShAdapter
    ml.gsl = MGC.gsl_double()

    class Mesh:
        @staticmethod
        def request_mp_evaluation(func, input_arrays=(), const_inputs=(), call_with_multiple_arguments=False, **kw):
            if not call_with_multiple_arguments:                          # make_golden_cc.py's serial loop over zipped arguments
                return [func(*args, *const_inputs) for args in zip(*input_arrays)]
            grids = np.meshgrid(*input_arrays, indexing='ij')
            r = np.asarray(func(*[x.ravel() for x in grids], *const_inputs))
            return r.reshape(grids[0].shape + r.shape[1:])
    mp.comm_module = Mesh
    it = importlib.import_module('xframe.projects.fxs.projectLibrary.fxs_invariant_tools')
    ex = importlib.import_module('xframe.projects.fxs.extract')
    import ccextract_cases as CC
    import ccmask_cases as MC

    cc, qs, avg, phis, L = MC.golden_inputs()
    nq, nd = len(qs), len(phis)
    grid = MC.grid_of(qs, phis)
    thetas = grid['thetas']
    out = {}
    # ---- masks
    for name, setting in MC.MASK_SETTINGS.items():
        m = np.asarray(it.cross_correlation_mask(MC.grid_of(qs, phis), {'cc_mask': setting, 'xray_wavelength': CC.WAVELENGTH}))
        out['G27_mask_' + name] = m
        nv = m.sum(-1)
        print('mask %-10s masked %5d of %d; valid per pair min %d max %d; pairs without a sample %d, fully valid %d'
              % (name, (~m).sum(), m.size, nv.min(), nv.max(), (nv == 0).sum(), (nv == nd).sum()))
    direct = MC.direct_mask(nq, nd)
    out['G27_mask_direct'] = direct
    # every mask used with back_substitution / interpolate_masked: samples 0 and n - 1 valid in every row with a valid sample; one
    # row fully masked
    some = direct.any(-1)
    assert direct[some][:, 0].all() and direct[some][:, -1].all() and (~some).sum() >= 1 and not direct.all()
    print('direct mask: masked %d of %d, rows without a sample %d' % ((~direct).sum(), direct.size, (~some).sum()))
    # every mask used with lstsq: n_valid = 0 or >= 2 n_orders (all orders: 9) in every pair; across them a pair without a sample
    # and a fully valid pair
    for name in MC.LSQ_MASKS + tuple(m for m, method in MC.FLOWS.values() if method == 'lstsq'):
        nv = out['G27_mask_' + name].sum(-1)
        assert ((nv == 0) | (nv >= 2 * (L + 1))).all(), (name, np.unique(nv))
        assert (nv == nd).any(), name
    assert (out['G27_mask_flat'].sum(-1) == 0).any()
    # ---- modify_cross_correlation on the direct mask
    for name, mod in MC.PREPARE_VARIANTS.items():
        v, m, p = it.modify_cross_correlation(cc.copy(), direct.copy(), phis.copy(), L, average_intensity=avg, **mod)
        if name == 'interp':
            vi = it.interpolate(cc.copy(), direct.copy(), phis.copy())
            assert np.array_equal(vi, v)
            v = vi
        assert np.array_equal(p, phis)
        out[f'G27_prep_{name}_cc'], out[f'G27_prep_{name}_mask'] = np.asarray(v), np.asarray(m, dtype=bool)
        print('prepare %-6s mask true %d of %d' % (name, np.asarray(m).sum(), m.size))
    # ---- least squares: the pure worker on the mesh of all pairs
    q1, q2 = (x.ravel() for x in np.meshgrid(np.arange(nq), np.arange(nq), indexing='ij'))
    for mname in MC.LSQ_MASKS:
        for oname, orders in (('even', np.arange(0, L + 1, 2)), ('all', np.arange(L + 1))):
            b = np.asarray(it.bl_3d_least_squares_worker(q1, q2, cc.copy(), phis, thetas, orders, out['G27_mask_' + mname]))
            assert np.abs(b.imag).max() == 0
            out[f'G27_lstsq_{mname}_{oname}'] = b.real.reshape(nq, nq, len(orders)).copy()
            conds = [np.linalg.cond(MC.legendre_matrix(qs, phis, orders, i, j)[out['G27_mask_' + mname][i, j]])
                     for i in range(nq) for j in range(nq) if out['G27_mask_' + mname][i, j].any()]
            print('lstsq %s %s: condition numbers %.1f .. %.1f' % (mname, oname, min(conds), max(conds)))
    # ---- back substitution on the direct mask (interpolates first)
    b, qq = it.ccd_to_deg2_invariant_3d_back_substitution(cc.copy(), CC.WAVELENGTH, MC.grid_of(qs, phis), np.arange(0, L + 1, 2), direct.copy())
    out['G27_backsub_direct_b'], out['G27_backsub_direct_qq_mask'] = np.asarray(b), np.asarray(qq, dtype=bool)
    print('back substitution on the direct mask: qq_mask all', np.asarray(qq).all())
    # ---- flows
    cls = ex.InvariantExtractor if hasattr(ex, 'InvariantExtractor') else [v for v in vars(ex).values() if isinstance(v, type) and
                                                                          hasattr(v, 'calc_deg_2_invariant_masks')][0]
    me = types.SimpleNamespace(data_radial_points=qs, max_order=L)
    me.calc_deg_2_invariant_line_mask = functools.partial(cls.calc_deg_2_invariant_line_mask, me)
    to_ns = pl.DictNamespace.dict_to_dictnamespace
    for flow, (mname, method) in MC.FLOWS.items():
        setting = MC.mask_settings(mname, out)
        meta = MC.metadata(qs, phis, L, True, dict(CC.FLOW_MODIFY), avg, setting, method)
        b, qq = it.cross_correlation_to_deg2_invariant(cc.copy(), 3, **meta)
        dopt = to_ns({'bl_q_limits': CC.MASK_CASES['none'], 'bl_enforce_psd': True})
        mask, ids = cls.calc_deg_2_invariant_masks(me, dopt, b.shape, qq)
        bc = cls.apply_invariant_constraints(me, dopt, np.array(b), np.array(ids))
        bc[0] = avg[:, None] * avg[None, :] * 4 * np.pi               # extract.py:160-167
        pms, _ = it.deg2_invariant_to_projection_matrices(3, bc, q_id_limits=np.array(ids), sort_mode=0)
        out[f'G27_flow_{flow}_b'], out[f'G27_flow_{flow}_mask'], out[f'G27_flow_{flow}_qid'] = np.asarray(bc), np.asarray(mask), np.asarray(ids)
        out[f'G27_flow_{flow}_qq_mask'] = np.asarray(qq, dtype=bool)
        for l, p in enumerate(pms):
            out[f'G27_flow_{flow}_pm{l}'] = np.asarray(p)
        print('flow %-16s qq_mask false %d; q_id_limits[0] %s; |V_l| %s' % (flow, (~np.asarray(qq, dtype=bool)).sum(), np.asarray(ids)[0].tolist(),
                                                                           ['%.1e' % np.linalg.norm(p) for p in pms]))
    path = os.path.join(HERE, 'cc_masked.npz')
    np.savez_compressed(path, **out)
    print('cc masked fixture:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

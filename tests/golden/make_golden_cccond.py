#!/usr/bin/env python3
"""tests/golden/cc_condition.npz (G30): the reference's conditioning of masked cross-correlation data.

Run:  python tests/golden/make_golden_cccond.py     (build container only: needs the reference checkout make_golden.py names)

Outputs of the reference's OWN functions on the seeded data of cccond_cases.golden_inputs (6 shells, max_order 8, 64 and 70 angles,
noise 0.02) under the mask cccond_cases.cond_mask:
  * modify_cross_correlation (fxs_invariant_tools.py:235-289) for every entry of cccond_cases.MODIFY_VARIANTS: low_pass_order_in_q,
    enforce_max_order, enforce_zero_odd_harmonics and apply_binned_mean each alone, and all stages together (values, mask, angles);
  * binned_mean (308-332) called alone;
  * cross_correlation_to_deg2_invariant (374-422) with apply_binned_mean + interpolate_masked in the modes lstsq and
    back_substitution;
  * for cccond_cases.FLOWS, at 70 angles on the reference's pixel_custom mask, the chain of extract_bl_from_cc + extract() as
    make_golden_ccmask.py runs it: lstsq after the binned mean on a copy of that mask which leaves the pair (1, 4) three bins for
    five orders (numpy.linalg.lstsq returns the truncated minimum-norm solution there), and back_substitution after binned mean +
    interpolation.
The bootstrap is make_golden.py's, the `gsl` double make_golden_cc.py's, the mesh stand-in for request_mp_evaluation
make_golden_ccmask.py's.  Only inputs and outputs (data) are written."""
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
            if not call_with_multiple_arguments:
                return [func(*args, *const_inputs) for args in zip(*input_arrays)]
            grids = np.meshgrid(*input_arrays, indexing='ij')
            r = np.asarray(func(*[x.ravel() for x in grids], *const_inputs))
            return r.reshape(grids[0].shape + r.shape[1:])
    mp.comm_module = Mesh
    it = importlib.import_module('xframe.projects.fxs.projectLibrary.fxs_invariant_tools')
    ex = importlib.import_module('xframe.projects.fxs.extract')
    import ccextract_cases as CC
    import ccmask_cases as MC
    import cccond_cases as DC

    out = {}
    L = DC.G_L
    for nd in DC.G_NDS:
        cc, qs, avg, phis, mask = DC.golden_inputs(nd)
        some = mask.any(-1)
        assert mask[0, 1].all() and (~some).sum() == 2 and mask[some][:, 0].all() and mask[some][:, -1].all()
        for name, mod in DC.MODIFY_VARIANTS.items():
            v, m, p = it.modify_cross_correlation(cc.copy(), mask.copy(), phis.copy(), L, average_intensity=avg, **mod)
            out[f'G30_{nd}_{name}_cc'], out[f'G30_{nd}_{name}_mask'] = np.asarray(v, dtype=float), np.asarray(m, dtype=bool)
            out[f'G30_{nd}_{name}_phis'] = np.asarray(p, dtype=float)
            print('modify %d %-8s -> %s, mask true %d of %d' % (nd, name, np.asarray(v).shape, np.asarray(m).sum(), np.asarray(m).size))
        v, m, p = it.binned_mean(mask.copy(), cc.copy(), L, phis.copy())
        assert np.array_equal(v, out[f'G30_{nd}_binned_cc']) and not np.asarray(m).all()
        assert not np.asarray(m)[2, 2].all() and np.asarray(m)[2, 2].any(), 'the pair (2, 2) is there for its empty bin'
        out[f'G30_{nd}_binned_mean_cc'], out[f'G30_{nd}_binned_mean_mask'] = np.asarray(v, dtype=float), np.asarray(m, dtype=bool)
        out[f'G30_{nd}_binned_mean_phis'] = np.asarray(p, dtype=float)
        for mode in DC.BL_MODES:
            c2, meta = DC.bl_metadata(nd, mode)
            b, qq = it.cross_correlation_to_deg2_invariant(c2.copy(), 3, **meta)
            out[f'G30_{nd}_bl_{mode}'], out[f'G30_{nd}_bl_{mode}_qq'] = np.asarray(b), np.asarray(qq, dtype=bool)
            print('B_l %d %-17s |B| %.3e, qq_mask false %d' % (nd, mode, np.linalg.norm(b), (~np.asarray(qq, dtype=bool)).sum()))
    # ---- flows
    nd = DC.FLOW_ND
    cc, qs, avg, phis, _ = DC.golden_inputs(nd)
    custom = np.asarray(it.cross_correlation_mask(MC.grid_of(qs, phis), {'cc_mask': DC.CUSTOM_MASK, 'xray_wavelength': CC.WAVELENGTH}))
    print('pixel_custom mask: masked %d of %d' % ((~custom).sum(), custom.size))
    assert not custom.all()
    cls = ex.InvariantExtractor if hasattr(ex, 'InvariantExtractor') else [v for v in vars(ex).values() if isinstance(v, type) and
                                                                          hasattr(v, 'calc_deg_2_invariant_masks')][0]
    me = types.SimpleNamespace(data_radial_points=qs, max_order=L)
    me.calc_deg_2_invariant_line_mask = functools.partial(cls.calc_deg_2_invariant_line_mask, me)
    to_ns = pl.DictNamespace.dict_to_dictnamespace
    for flow, (method, extra, starved) in DC.FLOWS.items():
        mask = DC.starved_mask(custom) if starved else custom.copy()
        out[f'G30_flow_{flow}_cc_mask'] = mask
        meta = MC.metadata(qs, phis, L, True, {**CC.FLOW_MODIFY, **extra}, avg, {'type': 'direct', 'direct': {'mask': mask.copy()}}, method)
        if starved:
            # the condition on the inputs of a rank-deficient case, on the problem the reference solves for the starved pair
            _, bm, bp = it.binned_mean(mask.copy(), cc.copy(), L, phis.copy())
            valid = np.asarray(bm)[DC.STARVED_PAIR]
            assert valid.sum() == 3, valid
            A = MC.legendre_matrix(qs, np.asarray(bp), np.arange(0, L + 1, 2), *DC.STARVED_PAIR)[valid]
            rank, gap = DC.check_gap(A, flow)
            print('starved pair: %d valid bins, rank %d, gap to the cut %.0f x' % (valid.sum(), rank, gap))
        b, qq = it.cross_correlation_to_deg2_invariant(cc.copy(), 3, **meta)
        dopt = to_ns({'bl_q_limits': CC.MASK_CASES['none'], 'bl_enforce_psd': True})
        mk, ids = cls.calc_deg_2_invariant_masks(me, dopt, b.shape, qq)
        bc = cls.apply_invariant_constraints(me, dopt, np.array(b), np.array(ids))
        bc[0] = avg[:, None] * avg[None, :] * 4 * np.pi               # extract.py:160-167
        pms, _ = it.deg2_invariant_to_projection_matrices(3, bc, q_id_limits=np.array(ids), sort_mode=0)
        out[f'G30_flow_{flow}_b'], out[f'G30_flow_{flow}_mask'], out[f'G30_flow_{flow}_qid'] = np.asarray(bc), np.asarray(mk), np.asarray(ids)
        out[f'G30_flow_{flow}_qq_mask'] = np.asarray(qq, dtype=bool)
        for l, p in enumerate(pms):
            out[f'G30_flow_{flow}_pm{l}'] = np.asarray(p)
        print('flow %-22s qq_mask false %d; |V_l| %s' % (flow, (~np.asarray(qq, dtype=bool)).sum(), ['%.1e' % np.linalg.norm(p) for p in pms]))
    path = os.path.join(HERE, 'cc_condition.npz')
    np.savez_compressed(path, **out)
    print('cc conditioning fixture:', len(out), 'arrays,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()

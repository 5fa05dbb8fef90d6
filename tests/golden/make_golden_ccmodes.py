#!/usr/bin/env python3
"""tests/golden/cc_backsub_modes.npz (G31): the reference's three back-substitution modes beside `back_substitution`.

Run:  python tests/golden/make_golden_ccmodes.py    (build container only: needs the reference checkout make_golden.py names)

Outputs of the reference's OWN functions on the seeded data of ccmodes_cases.golden_inputs (6 shells, 32 angles, noise 0.02 with a
part that is antisymmetric in Delta: the harmonics C_m are complex and indefinite):
  * cross_correlation_to_deg2_invariant (fxs_invariant_tools.py:374-422) with mode back_substitution_memory_hungry (519-576),
    back_substitution_qqsym (646-694) and back_substitution_psd (710-761) for every entry of ccmodes_cases.VARIANTS: max_order 8
    with the odd orders assumed zero and not, max_order 9 with zero odd orders, the 'direct' mask of ccmodes_cases.pair_mask (samples
    of two pairs removed), and that mask with every modify_cc switch of ccmask_cases -- which pins what modify_cross_correlation
    leaves at the masked positions, since qqsym and psd transform them as they are;
  * the reference's own distance between back_substitution and back_substitution_memory_hungry;
  * nearest_positive_semidefinite_matrix (mathLibrary.py:872-892) on a stack of four matrices;
  * for each mode the chain of extract_bl_from_cc + extract() behind it as make_golden_ccmask.py runs it (bl_q_limits none,
    bl_enforce_psd off, subtract_average_intensity) down to the projection matrices.
The bootstrap is make_golden.py's, the `gsl` double make_golden_cc.py's.  Only inputs and outputs (data) are written.
The last lines print the restatement's distance to these outputs (tests/ccmodes_reference.py; the CPU test bounds it by 1e-13) and
the distance between two eigh routes on this machine."""
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

    class Serial:
        @staticmethod
        def request_mp_evaluation(func, input_arrays=(), const_inputs=(), **kw):
            return [func(*args, *const_inputs) for args in zip(*input_arrays)]
    mp.comm_module = Serial
    it = importlib.import_module('xframe.projects.fxs.projectLibrary.fxs_invariant_tools')
    ex = importlib.import_module('xframe.projects.fxs.extract')
    import ccextract_cases as CC
    import ccmask_cases as MC
    import ccmodes_cases as QC
    import ccmodes_reference as R
    from helpers import rel_l2

    out = {}
    for mode in QC.MODES:
        for name in QC.VARIANTS:
            cc, qs, phis, L, zero_odd, mod, avg, mask = QC.variant_call(name, mode)
            mset = {'type': 'none'} if mask is None else {'type': 'direct', 'direct': {'mask': mask.copy()}}
            b, qq = it.cross_correlation_to_deg2_invariant(cc.copy(), 3, **MC.metadata(qs, phis, L, zero_odd, mod, avg, mset, mode))
            out[f'G31_{mode}_{name}_b'], out[f'G31_{mode}_{name}_qq_mask'] = np.asarray(b), np.asarray(qq, dtype=bool)
            print('%-32s %-10s %s |imag| / |b| %.2e, qq_mask false %d' % (mode, name, b.shape, np.linalg.norm(b.imag) / np.linalg.norm(b),
                                                                           (~np.asarray(qq, dtype=bool)).sum()))
    # the reference's own distance between the two implementations of the plain elimination
    for name in ('s2', 's1'):
        cc, qs, phis, L, zero_odd, mod, avg, _ = QC.variant_call(name, 'back_substitution')
        b, _ = it.cross_correlation_to_deg2_invariant(cc.copy(), 3, **MC.metadata(qs, phis, L, zero_odd, mod, avg, {'type': 'none'},
                                                                                   'back_substitution'))
        d = rel_l2(np.asarray(b), out[f'G31_back_substitution_memory_hungry_{name}_b'])
        out[f'G31_hungry_vs_back_substitution_{name}'] = np.array(d)
        print('back_substitution vs memory_hungry %s: %.2e' % (name, d))
    rng = np.random.default_rng(31)
    stack = np.array([QC.psd_matrix(kind, 6, seed=k) for k, kind in enumerate(('hermitian', 'general', 'psd', 'pairs'))])
    stack[1] += rng.normal(size=(6, 6))
    out['G31_psd_in'], out['G31_psd_out'] = stack, np.asarray(ml.nearest_positive_semidefinite_matrix(stack.copy()))
    # ---- flows
    cls = ex.InvariantExtractor if hasattr(ex, 'InvariantExtractor') else [v for v in vars(ex).values() if isinstance(v, type) and
                                                                          hasattr(v, 'calc_deg_2_invariant_masks')][0]
    qs, phis, cc, avg = QC.golden_inputs()
    L = 8
    me = types.SimpleNamespace(data_radial_points=qs, max_order=L)
    me.calc_deg_2_invariant_line_mask = functools.partial(cls.calc_deg_2_invariant_line_mask, me)
    to_ns = pl.DictNamespace.dict_to_dictnamespace
    for mode in QC.MODES:
        meta = MC.metadata(qs, phis, L, True, dict(CC.FLOW_MODIFY), avg, {'type': 'none'}, mode)
        b, qq = it.cross_correlation_to_deg2_invariant(cc.copy(), 3, **meta)
        dopt = to_ns({'bl_q_limits': CC.MASK_CASES['none'], 'bl_enforce_psd': False})
        mask, ids = cls.calc_deg_2_invariant_masks(me, dopt, b.shape, qq)
        bc = cls.apply_invariant_constraints(me, dopt, np.array(b), np.array(ids))
        bc[0] = avg[:, None] * avg[None, :] * 4 * np.pi               # extract.py:160-167
        pms, _ = it.deg2_invariant_to_projection_matrices(3, bc, q_id_limits=np.array(ids), sort_mode=0)
        out[f'G31_flow_{mode}_b'], out[f'G31_flow_{mode}_mask'] = np.asarray(bc), np.asarray(mask)
        for l, p in enumerate(pms):
            out[f'G31_flow_{mode}_pm{l}'] = np.asarray(p)
        print('flow %-32s |V_l| %s' % (mode, ['%.1e' % np.linalg.norm(p) for p in pms]))
    path = os.path.join(HERE, 'cc_backsub_modes.npz')
    np.savez_compressed(path, **out)
    print('cc back-substitution modes fixture:', len(out), 'arrays,', os.path.getsize(path), 'bytes')
    worst = QC.check_restatement_golden(np.load(path))
    print('restatement vs the reference, worst whole-array relative L2: %.2e (bound %.0e)' % (worst, QC.TOL_RESTATEMENT))
    # two eigh routes on this machine: numpy's default driver against the shifted call
    worst = 0.0
    for name in QC.VARIANTS:
        cc, qs, phis, L, zero_odd, mod, avg, mask = QC.variant_call(name, QC.MODES[2])
        a, _, _ = R.cc_to_deg2(QC.MODES[2], cc, qs, phis, L, zero_odd, mod, avg, mask)
        b, _, _ = R.cc_to_deg2(QC.MODES[2], cc, qs, phis, L, zero_odd, mod, avg, mask, eigh=R.shifted_eigh)
        worst = max(worst, rel_l2(b, a))
    print('psd mode, eigh against shifted eigh, worst whole-array relative L2: %.2e' % worst)


if __name__ == '__main__':
    main()

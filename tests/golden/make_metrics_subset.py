"""tests/golden/metrics_subset.npz (G32): the reference's `_generate_ccd_diff_3d`, `_generate_II_3d` and `_generate_fqc_3d`
(fxs_IO_methods.py:651-683, 587-627, 507-550) with used_orders = the orders 0 .. L - 1 of L + 1, as `generate_ccd_diff` hands them
over (641: the reference invariants of the used orders; reconstruct.py:471: the invariant mask of all orders), under the stubs of
make_golden.main_metrics (fixture G19).  Records which of the three run, the messages of those that raise, and the values of those
that run on two sets of seeded intensity coefficients.

Needs the reference tree (make_golden.REF); run from the repository root:  python tests/golden/make_metrics_subset.py"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), HERE]
import make_golden as MG  # noqa: E402


def _stubs():
    """the doubles main_metrics installs: the Legendre functions of pygsl from oracle/metrics.py, presenters that accept anything"""
    from oracle import metrics as OMx
    from oracle import mtip as OM
    from xframe_amd.fxs import synthetic as S
    mods = MG.bootstrap()
    ml = mods['xframe.library.mathLibrary']
    ml.shtns = MG.ShAdapter

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
    ml.gsl = GslDouble

    class Anything:
        def __init__(self, *a, **k):
            pass

        def __getattr__(self, n):
            return Anything()

        def __call__(self, *a, **k):
            return Anything()

    class AnyModule(types.ModuleType):
        def __getattr__(self, n):
            if n.startswith('__'):
                raise AttributeError(n)
            return Anything()
    for name in ('xframe.presenters', 'xframe.presenters.matplotlibPresenter', 'xframe.presenters.openCVPresenter'):
        sys.modules[name] = AnyModule(name)
    pl = mods['xframe.library.pythonLibrary']
    mods['xframe.settings'].project = pl.DictNamespace.dict_to_dictnamespace(OM.deep_update(OM.default_settings(), S.config_overrides(1)))
    return importlib.import_module('xframe.projects.fxs.projectLibrary.fxs_IO_methods')


def main():
    io = _stubs()
    rng = np.random.default_rng(2222)
    N, L = 10, 5
    qs = (np.arange(N) + 0.5) * 0.012
    wavelength = 1.23984
    Iref = [MG.cplx(rng, (N, 2 * l + 1)) for l in range(L + 1)]
    used = {l: l for l in range(L)}                                  # used_order_ids = arange(L) of L + 1 orders
    ref = np.array([a @ a.T.conj() for a in Iref[:L]])               # fxs_IO_methods.py:641
    rm = rng.random((L + 1, N)) > 0.2
    inv_mask = rm[:, :, None] * rm[:, None, :]
    n_particles = np.array([2.0])
    sets = {'I': [a + 0.3 * MG.cplx(rng, a.shape) for a in Iref], 'J': [a + 1.0 * MG.cplx(rng, a.shape) for a in Iref]}
    out = {'G32_N': np.array(N), 'G32_L': np.array(L), 'G32_qs': qs, 'G32_wavelength': np.array(wavelength), 'G32_ref': ref,
           'G32_radial_mask': rm, 'G32_n_particles': n_particles, 'G32_C_order': np.array(2)}
    for tag, Ims in sets.items():
        for l in range(L + 1):
            out[f'G32_{tag}{l}'] = Ims[l]
    makers = {'ccd': lambda: io._generate_ccd_diff_3d(qs, ref.copy(), used, n_particles, inv_mask, 2, wavelength),
              'II': lambda: io._generate_II_3d(qs, ref.copy(), used, n_particles, inv_mask, wavelength),
              'fqc': lambda: io._generate_fqc_3d(qs, ref.copy(), used, n_particles, inv_mask, wavelength)}
    for name, make in makers.items():
        try:
            routine = make()
            values = {tag: np.asarray(routine(None, None, [a.copy() for a in Ims])) for tag, Ims in sets.items()}
        except Exception as ex:                                      # what upstream does with a subset is the recorded fact
            out[f'G32_{name}_runs'] = np.array(False)
            out[f'G32_{name}_raises'] = np.array('%s: %s' % (type(ex).__name__, ex))
            print(name, 'raises', type(ex).__name__, ex)
            continue
        out[f'G32_{name}_runs'] = np.array(True)
        for tag, v in values.items():
            out[f'G32_{name}_{tag}'] = v
        print(name, 'runs', values)
    np.savez_compressed(os.path.join(HERE, 'metrics_subset.npz'), **out)


if __name__ == '__main__':
    main()

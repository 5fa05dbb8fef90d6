"""Device engine: a thin Python object around one ``mtip_ctx`` (one GPU, one stream, ``n_batch`` restarts).

Does the reference's one-off host setup (``hostsetup``), uploads it through the C ABI and exposes the loop
primitives (`run`, `shrinkwrap`, getters) plus the single operators used by ``operators.py`` and the tests.
"""
import ctypes as C

import numpy as np

from . import _lib, hostsetup as hs
from .settings import reciprocity_coefficient, resolve

METHOD_ID = {'HIO': 0, 'ER': 1, 'HIO_non_FXS': 2, 'ER_non_FXS': 3}
LOOP_MAX_ORDER = 63                   # the phasing loop and the projection (MTIP_LOOP_L_MAX); the transforms alone reach 128


class Engine(_lib.TensorOperands):
    def __init__(self, settings=None, data=None, n_batch=1, device=0, fused=True, lib_path=None,
                 n_radial=None, l_max=None, max_q=None, big_l_loop=None):
        """settings: resolved (or override) settings dict; data: invariants dict (may be None for a
        transforms-only engine, then ``max_q`` must be given).  A transforms-only engine takes max_order <= 128 (the transforms, B_l
        and the context-independent operators); with ``data`` the limit is that of the phasing loop, max_order <= 63.
        big_l_loop (None: the setting ``GPU.big_l_loop``, default False) opts in to the phasing loop and the projection up to
        max_order 128 (MTIP_CFG_LOOP_BIG_L: DESIGN section 6 lists what stays refused); below 64 it changes nothing."""
        self.lib = _lib.load(lib_path)
        self.device_index = int(device)
        opt = resolve(settings)
        self.opt = opt
        g = opt['grid']
        self.N = int(n_radial if n_radial is not None else g['n_radial_points'])
        self.L = int(l_max if l_max is not None else g['max_order'])
        self.big_l_loop = bool(opt.get('GPU', {}).get('big_l_loop', False) if big_l_loop is None else big_l_loop)
        if data is not None and self.L > LOOP_MAX_ORDER and not self.big_l_loop:
            raise NotImplementedError('max_order = %d with invariants: the phasing loop and the projection are built for max_order <= %d; '
                                      'beyond it (up to 128) an engine without data runs the transforms only (DESIGN section 6)'
                                      % (self.L, LOOP_MAX_ORDER))
        self.kappa = float(reciprocity_coefficient(opt['fourier_transform']))
        self.mode = opt['fourier_transform']['type']
        if max_q is None:
            max_q = g['max_q']
            if not isinstance(max_q, float):                        # reconstruct.py:258-261
                if data is None:
                    raise ValueError('max_q is needed when no invariants are given')
                max_q = float(np.max(data['data_radial_points']))
        self.max_q = float(max_q)
        self.n_theta, self.n_phi = hs.angular_grid_size(self.L, g.get('n_theta', 0), g.get('n_phi', 0))
        self.B = int(n_batch)
        self.shape = (self.N, self.n_theta, self.n_phi)
        self.nlm = (self.L + 1) ** 2
        self.fused = bool(fused)
        if self.lib.mtip_device_count() <= 0:
            raise _lib.MtipError('no HIP device visible: the MTIP engine needs an MI355X (no CPU fallback)')
        cfg = _lib.MtipCfg(self.N, self.L, self.n_theta, self.n_phi, self.B, 1 if hs.hankel_skips_first_shell(self.mode) else 0,
                           1 if fused else 0, _lib.MTIP_CFG_LOOP_BIG_L if self.big_l_loop else 0)
        self.ctx = self.lib.mtip_create(C.byref(cfg), int(device))
        self.group = None                                            # EngineGroup this engine steps with (side-by-side restart groups)
        if not self.ctx:
            raise _lib.MtipError('mtip_create: ' + self.lib.mtip_last_error(None).decode())
        # ---- transforms
        self.cos_theta, self.gauss_w, self.theta, self.phi = hs.gauss_grid(self.n_theta, self.n_phi)
        self._ck(self.lib.mtip_set_angular_grid(self.ctx, _lib.ptr(self.cos_theta), _lib.ptr(self.gauss_w)))
        self.rs, self.qs = hs.radial_grids(self.max_q, self.N, self.kappa, self.mode)
        self._ck(self.lib.mtip_set_radial_grid(self.ctx, _lib.ptr(self.rs), _lib.ptr(self.qs)))
        self.r_max = float(np.max(self.rs))                          # reconstruct.py:329
        self.raw_weights = hs.hankel_raw_weights(self.L, self.N, self.kappa, self.mode)
        fs, ivs = hs.hankel_scales(self.r_max, self.N, self.kappa, self.mode)
        self._ck(self.lib.mtip_set_hankel_weights(self.ctx, _lib.ptr(self.raw_weights), fs, ivs))
        self.int_wr, self.int_wt = hs.integrator_weights(self.rs, self.n_theta)
        self.default_sigma = np.pi / np.max(self.qs)                 # fxs_Projections.py:189-193
        self.rsetup = None
        if data is not None:
            self._setup_projections(data)

    # ------------------------------------------------------------------ setup
    def _ck(self, rc):
        if rc != 0:
            raise _lib.MtipError(f'libmtip_hip error {rc}: ' + self.lib.mtip_last_error(self.ctx).decode())

    def _setup_projections(self, data):
        opt = self.opt
        self.xray_wavelength = data.get('xray_wavelength', None)
        ropt = opt['projections']['reciprocal']
        rs_ = hs.reciprocal_setup(self.qs, data, self.L, ropt)      # (shared by the engines of one worker: read only)
        self.rsetup = rs_
        used_ids = set(rs_.used_orders.values())
        for l in range(self.L + 1):
            if l in used_ids:
                V = _lib.as_c128(rs_.projection_matrices[l])
                mask = _lib.as_u8(rs_.radial_mask[l])
                self._ck(self.lib.mtip_set_projection_matrix(self.ctx, l, _lib.ptr(V), V.shape[1], _lib.ptr(mask), 1))
            else:
                self._ck(self.lib.mtip_set_projection_matrix(self.ctx, l, None, 1, None, 0))
        self._ck(self.lib.mtip_set_number_of_particles(self.ctx, rs_.number_of_particles))
        self._ck(self.lib.mtip_set_so_freedom(self.ctx, int(rs_.so_order)))
        popt = opt['projections']['real']['projections']
        considered = opt['projections']['real']['HIO'].get('considered_projections', ['all'])
        flags, lo, hi, thr, hio = hs.real_constraint_flags(popt, considered)
        self._ck(self.lib.mtip_set_real_constraints(self.ctx, flags, lo, hi, thr, hio))
        auto = None
        if popt['support']['initial_support']['type'] == 'auto_correlation':
            auto = self.autocorrelation_guess()
        self.initial_support = hs.initial_support(self.rs, self.shape, popt, opt['particle_radius'], auto)
        s0 = _lib.as_u8(self.initial_support)
        self._ck(self.lib.mtip_set_initial_support(self.ctx, _lib.ptr(s0)))
        em = opt['main_loop']['error']['methods']
        inside = em['real'].get('l2_projection_diff', {}).get('inside_initial_support', False)
        gen = opt.get('general', {})
        wr, wt, use_mask = hs.error_weights(self.rs, self.n_theta, self.shape, inside, gen.get('cache_aware', True),
                                            gen.get('L2_cache', 512))
        self._ck(self.lib.mtip_set_error_weights(self.ctx, _lib.ptr(_lib.as_f64(wr)), _lib.ptr(_lib.as_f64(wt)), int(use_mask)))
        # metrics that are not on the accelerated path must not be dropped silently (fxs_IO_methods.py:690-703 lists them)
        for cat, known in (('real', ('l2_projection_diff',)), ('reciprocal', ('deg2_invariant_l2_diff', 'II_error', 'ccd_diff', 'fqc_error', 'l2_projection_diff',
                                                                                      'deg2_ranked_invariant_l2_diff'))):
            for name in em.get(cat, {}).get('calculate', []) or []:
                if name not in known:
                    if (cat, name) == ('real', 'support_size'):
                        raise NotImplementedError("real metric 'support_size' raises upstream as well (fxs_IO_methods.py:687 is handed the "
                                                  "projection's output list: AttributeError on .real)")
                    raise NotImplementedError('main_loop.error.methods.%s.calculate: %r is not built (DESIGN section 6); built: %s'
                                              % (cat, name, ', '.join(known)))
        rec_calc = list(em['reciprocal']['calculate'])
        # deg2_ranked_invariant_l2_diff (fxs_IO_methods.py:330-366): the entry of deg2_invariant_l2_diff of the best ranked even order
        # (fxs_invariant_tools.py:1467-1486) or of the order the option names -- a column of the same per-step history
        self.deg2_ranked_id = None
        if 'deg2_ranked_invariant_l2_diff' in rec_calc:
            order = em['reciprocal'].get('deg2_ranked_invariant_l2_diff', {}).get('order', False)
            if isinstance(order, (int, np.integer)) and not isinstance(order, (bool, np.bool_)):
                self.deg2_ranked_id = int(self.rsetup.used_orders[int(order)])
            else:
                orders = np.array(list(self.rsetup.used_orders.keys())).astype(int)
                self.deg2_ranked_id = int(hs.rank_projection_matrices_3d(self.rsetup.projection_matrices, orders, self.qs)[0])
        self.deg2_listed = 'deg2_invariant_l2_diff' in rec_calc
        self.deg2_enabled = self.deg2_listed or self.deg2_ranked_id is not None
        self._ck(self.lib.mtip_set_deg2_metric(self.ctx, int(self.deg2_enabled)))
        # reciprocal l2_projection_diff (fxs_IO_methods.py:301-310): the real metric's integrator without a support mask, i.e. with shell
        # N - 2 zeroed (the cache-aware branch integrates over the real grid, the plain one over the proportional reciprocal grid)
        self.reciprocal_l2 = 'l2_projection_diff' in rec_calc
        if self.reciprocal_l2:
            wr2, wt2, _ = hs.error_weights(self.rs, self.n_theta, self.shape, False)
            self._ck(self.lib.mtip_set_reciprocal_l2_metric(self.ctx, _lib.ptr(_lib.as_f64(wr2)), _lib.ptr(_lib.as_f64(wt2))))
        # II_error / ccd_diff / fqc_error (fxs_IO_methods.py:587-627, 651-683, 507-550): per step on the device from B_l
        self.invariant_metrics = [n for n in ('II_error', 'ccd_diff', 'fqc_error') if n in em['reciprocal']['calculate']]
        if self.invariant_metrics:
            used_ids = sorted(self.rsetup.used_orders.values())
            subset = used_ids != list(range(self.L + 1))
            if subset:
                # ccd_diff indexes B_l, its weights and the mask by the used orders and runs upstream (fxs_IO_methods.py:653-677); the
                # other two mask B_l of ALL orders with arrays shaped by the used ones (594-597, 612; 514-516)
                refused = [n for n in self.invariant_metrics if n != 'ccd_diff']
                if refused:
                    raise NotImplementedError('%s with a subset of the orders: upstream raises in its first evaluation (IndexError: boolean '
                                              'index did not match indexed array along axis 0, fxs_IO_methods.py:612 / 535)' % ' / '.join(refused))
                if 0 not in self.rsetup.used_orders:
                    raise NotImplementedError('ccd_diff without order 0 among the used orders: upstream raises (KeyError: 0, zero_id = '
                                              'used_orders[0], fxs_IO_methods.py:654)')
            if self.xray_wavelength is None:
                raise KeyError("II_error / ccd_diff / fqc_error need data['xray_wavelength'] (fxs_IO_methods.py:511, 590, 657)")
            pms = [self.rsetup.projection_matrices.get(l, np.zeros((self.N, min(self.N, 2 * l + 1)), complex)) for l in range(self.L + 1)]
            t = hs.invariant_metric_tables(self.invariant_metrics, self.qs, pms, self.rsetup.radial_mask, float(self.xray_wavelength),
                                           em['reciprocal'].get('ccd_diff', {}).get('C_order', None), used_ids if subset else None)
            flags = sum(f for f, n in ((1, 'II_error'), (2, 'ccd_diff'), (4, 'fqc_error')) if n in self.invariant_metrics)

            def pp(key, conv):
                return _lib.ptr(conv(t[key])) if key in t else None
            self._im_keep = t                                         # (the arrays must outlive the call)
            self._ck(self.lib.mtip_set_invariant_metrics(
                self.ctx, flags, _lib.ptr(_lib.as_u8(t['zero_mask'])), pp('II_reference', _lib.as_c128), pp('qq', _lib.as_f64),
                pp('ccd_weights', _lib.as_f64), pp('ccd_reference', _lib.as_c128), float(t.get('ccd_norm', 0.0)), pp('fqc_P', _lib.as_f64),
                pp('fqc_reference_average', _lib.as_f64), pp('fqc_reference_weights', _lib.as_f64)))
        # generate_main_error_routine, fxs_IO_methods.py:746-765
        main = em.get('main', {'metrics': {'real': ['l2_projection_diff'], 'reciprocal': []}, 'type': 'mean'})
        real_m, rec_m = list(main['metrics'].get('real', [])), list(main['metrics'].get('reciprocal', []))
        types = {'mean': 0, 'min': 1, 'max': 2, 'prod': 3}
        if main.get('type', 'mean') not in types:
            raise ValueError('main error type %r (mean / min / max / prod)' % (main.get('type'),))
        codes = {('real', 'l2_projection_diff'): 0, ('reciprocal', 'deg2_invariant_l2_diff'): 1, ('reciprocal', 'l2_projection_diff'): 2,
                 ('reciprocal', 'II_error'): 3, ('reciprocal', 'ccd_diff'): 4, ('reciprocal', 'deg2_ranked_invariant_l2_diff'): 5}
        named = [('real', n) for n in real_m] + [('reciprocal', n) for n in rec_m]        # the reference's order (753-757)
        for name in rec_m:                                           # (the real metric is recorded whether it is listed or not)
            if name not in rec_calc:
                raise KeyError("main error uses %r but main_loop.error.methods.reciprocal.calculate does not list it" % (name,))
        if ('reciprocal', 'fqc_error') in named:
            raise NotImplementedError('main error over fqc_error: one value per shell, NaN throughout in three dimensions upstream '
                                      '(0 / 0 at shell 0, fxs_IO_methods.py:507-550); not built as a main metric (DESIGN section 6)')
        vector = ('reciprocal', 'deg2_invariant_l2_diff') in named
        if vector and len(named) > 1:
            raise NotImplementedError('main error over deg2_invariant_l2_diff (one value per order) AND %r: the '
                                      'reference itself raises there (np.array of an inhomogeneous list, fxs_IO_methods.py:760)'
                                      % ([n for n in named if n != ('reciprocal', 'deg2_invariant_l2_diff')],))
        unknown = [n for n in named if n not in codes]
        if unknown or not named or len(named) > 8:
            raise NotImplementedError('main error metrics %r / %r: one to eight of %s' % (real_m, rec_m, ', '.join('%s %s' % k for k in codes)))
        self.main_items = [codes[n] for n in named]
        # item 5 reads a column of the per-order history, which has a column for every order: the one of the ranked used order
        column = int(tuple(self.rsetup.used_orders.values())[self.deg2_ranked_id]) if 5 in self.main_items else 0
        items = np.ascontiguousarray(self.main_items, dtype=np.int32)
        self._ck(self.lib.mtip_set_main_error_ex(self.ctx, types[main.get('type', 'mean')], len(items), _lib.ptr(items), column))

    def autocorrelation_guess(self):
        """reconstruct.py:400-420: ift(icht(V_l padded)).real"""
        c = np.zeros((self.B, self.N, self.nlm), complex)
        for l, p in enumerate(self.rsetup.full_projection_matrices):
            c[:, :, l * l:l * l + p.shape[1]] = p[None]
        return self.fourier_transform(self.sht_inverse(c), inverse=True)[0].real

    def close(self):
        if getattr(self, 'group', None) is not None:
            self.group.leave(self)
        if getattr(self, 'ctx', None):
            self.lib.mtip_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ batch helpers
    def _bgrid(self, a):
        a = _lib.as_c128(a)
        if a.shape == self.shape:
            a = np.broadcast_to(a, (self.B,) + self.shape)
        assert a.shape == (self.B,) + self.shape, (a.shape, self.shape)
        return np.ascontiguousarray(a)

    def _bcoef(self, a):
        a = _lib.as_c128(a)
        if a.shape == (self.N, self.nlm):
            a = np.broadcast_to(a, (self.B, self.N, self.nlm))
        assert a.shape == (self.B, self.N, self.nlm), a.shape
        return np.ascontiguousarray(a)

    # ------------------------------------------------------------------ single operators (host arrays)
    def sht_forward(self, grid, prologue=0):
        g = self._bgrid(grid)
        out = np.empty((self.B, self.N, self.nlm), complex)
        self._ck(self.lib.mtip_op_sht_forward(self.ctx, _lib.ptr(g), _lib.ptr(out), prologue))
        return out

    def sht_inverse(self, coeff):
        c = self._bcoef(coeff)
        out = np.empty((self.B,) + self.shape, complex)
        self._ck(self.lib.mtip_op_sht_inverse(self.ctx, _lib.ptr(c), _lib.ptr(out)))
        return out

    def sht_inverse_forward(self, coeff, prologue=0):
        """grid = iSHT(coeff) and SHT(grid) (prologue 0) / SHT(|grid|^2) (prologue 1) in one kernel per shell."""
        c = self._bcoef(coeff)
        grid = np.empty((self.B,) + self.shape, complex)
        out = np.empty((self.B, self.N, self.nlm), complex)
        self._ck(self.lib.mtip_op_sht_inverse_forward(self.ctx, _lib.ptr(c), _lib.ptr(grid), _lib.ptr(out), prologue))
        return grid, out

    def hankel(self, coeff, inverse=False):
        c = self._bcoef(coeff)
        out = np.empty_like(c)
        self._ck(self.lib.mtip_op_hankel(self.ctx, _lib.ptr(c), _lib.ptr(out), int(inverse)))
        return out

    def hankel_difference(self, coeff, coeff_sub, inverse=False, sub_mask=None):
        """H(coeff - coeff_sub) above output shell 0 and H(coeff) on it, for the restarts sub_mask (B flags, None: all) selects;
        H(coeff) for the others: the launch of the one-pass ft_stab step"""
        c, s = self._bcoef(coeff), self._bcoef(coeff_sub)
        out = np.empty_like(c)
        m = None if sub_mask is None else _lib.as_u8(np.asarray(sub_mask).reshape(self.B) != 0)
        self._ck(self.lib.mtip_op_hankel_difference(self.ctx, _lib.ptr(c), _lib.ptr(s), _lib.ptr(out), int(inverse), _lib.ptr(m)))
        return out

    def fourier_transform(self, grid, inverse=False):
        g = self._bgrid(grid)
        out = np.empty_like(g)
        self._ck(self.lib.mtip_op_fourier_transform(self.ctx, _lib.ptr(g), _lib.ptr(out), int(inverse)))
        return out

    def project_coefficients(self, Ilm, real_intensity=False):
        """approximate_unknowns + mtip_projection.  real_intensity: the coefficients are those of a real grid (as in the
        phasing loop, SHT of |F|^2); only their m >= 0 half is read and real projection matrices take the real-arithmetic kernel."""
        c = self._bcoef(Ilm)
        out = np.empty_like(c)
        fn = self.lib.mtip_op_project_real_intensity if real_intensity else self.lib.mtip_op_project_coefficients
        self._ck(fn(self.ctx, _lib.ptr(c), _lib.ptr(out)))
        return out

    def apply_unknowns(self, Ilm, unknowns):
        """mtip_projection(Ilm, unknowns) (fxs_Projections.py:832-849): `unknowns` = per restart a sequence over l of
        (k_l, 2l+1) arrays, or one such sequence for all restarts."""
        c = self._bcoef(Ilm)
        if len(unknowns) == self.L + 1 and np.ndim(unknowns[0]) == 2:
            unknowns = [unknowns] * self.B
        flat = np.stack([np.concatenate([_lib.as_c128(u).reshape(-1) for u in per]) for per in unknowns])
        flat = np.ascontiguousarray(flat)
        out = np.empty_like(c)
        self._ck(self.lib.mtip_op_apply_unknowns(self.ctx, _lib.ptr(c), _lib.ptr(flat), _lib.ptr(out)))
        return out

    def modulus_replacement(self, F, I_new):
        f, i = self._bgrid(F), self._bgrid(I_new)
        out = np.empty_like(f)
        self._ck(self.lib.mtip_op_modulus_replacement(self.ctx, _lib.ptr(f), _lib.ptr(i), _lib.ptr(out)))
        return out

    def real_space_update(self, w, rho_prev, method, beta):
        w_, p_ = self._bgrid(w), self._bgrid(rho_prev)
        out = np.empty_like(w_)
        err = np.empty(self.B)
        self._ck(self.lib.mtip_op_real_space_update(self.ctx, _lib.ptr(w_), _lib.ptr(p_), METHOD_ID[method], float(beta),
                                                    _lib.ptr(out), _lib.ptr(err)))
        return out, err

    def deg2_invariants(self, Ilm):
        c = self._bcoef(Ilm)
        out = np.empty((self.B, self.L + 1, self.N, self.N), complex)
        self._ck(self.lib.mtip_op_deg2_invariants(self.ctx, _lib.ptr(c), _lib.ptr(out)))
        return out

    def apply_matrix(self, matrix, vects):
        m, v = _lib.as_f64(matrix), _lib.as_f64(vects)
        squeeze = v.ndim == 1
        if squeeze:
            v = np.ascontiguousarray(v[:, None])
        out = np.empty((m.shape[0], v.shape[1]))
        self._ck(self.lib.mtip_op_apply_matrix(self.ctx, _lib.ptr(m), _lib.ptr(v), _lib.ptr(out), m.shape[0], m.shape[1], v.shape[1]))
        return out[:, 0] if squeeze else out

    # ------------------------------------------------------------------ extract: B_l -> V_l (fxs_invariant_tools.py:1079-1207)
    def hermitian_eig(self, mats):
        """eigen-decomposition of a stack of Hermitian matrices (K, n, n) on the device: eigenvalues (K, n) in descending order,
        eigenvectors (K, n, n) with eigenvector i in [:, :, i] (numpy.linalg.eigh's layout, reversed order)"""
        m = _lib.as_c128(mats)
        K, n = m.shape[0], m.shape[1]
        if n <= 288 and not np.any(m.imag):
            # real symmetric (B_l of a real intensity): LDS-resident solver up to 128, column blocks over workgroups up to 288
            sym = np.ascontiguousarray((m.real + np.swapaxes(m.real, -1, -2)) / 2)
            vals = np.empty((K, n))
            vecs = np.empty((K, n, n))
            self._ck(self.lib.mtip_op_symmetric_eig(self.ctx, n, K, _lib.ptr(sym), _lib.ptr(vals), _lib.ptr(vecs)))
            order = np.argsort(vals, axis=1)[:, ::-1]
            vals = np.take_along_axis(vals, order, axis=1)
            vecs = np.take_along_axis(vecs, order[:, :, None], axis=1)          # rows = eigenvectors
            return vals, np.ascontiguousarray(np.swapaxes(vecs, -1, -2)).astype(complex)
        herm = np.ascontiguousarray((m + np.conj(np.swapaxes(m, -1, -2))) / 2)
        # the kernel rotates the columns of its column-major work matrix: hand it B^T = conj(B), whose eigenvectors are the
        # conjugates of B's
        vals = np.empty((K, n))
        vecs = np.empty((K, n, n), complex)
        self._ck(self.lib.mtip_op_hermitian_eig(self.ctx, n, K, _lib.ptr(np.ascontiguousarray(np.swapaxes(herm, -1, -2))),
                                                _lib.ptr(vals), _lib.ptr(vecs)))
        order = np.argsort(vals, axis=1)[:, ::-1]
        vals = np.take_along_axis(vals, order, axis=1)
        vecs = np.take_along_axis(vecs, order[:, :, None], axis=1)          # rows = eigenvectors
        return vals, np.ascontiguousarray(np.swapaxes(vecs, -1, -2))

    def extract_projection_matrices(self, Bl, orders=None):
        """deg2_invariant_to_projection_matrices_3d (fxs_invariant_tools.py:1171-1207) for B_l (L+1, Nq, Nq): V_l = the top
        min(2l+1, Nq) eigenvectors scaled by sqrt(eigenvalue), negative eigenvalues clipped.  Returns (list of V_l, list of
        eigenvalues)."""
        Bl = _lib.as_c128(Bl)
        orders = range(Bl.shape[0]) if orders is None else orders
        vals, vecs = self.hermitian_eig(Bl)
        pms, evs = [], []
        for i, l in enumerate(orders):
            k = min(Bl.shape[1], 2 * l + 1)
            w, v = vals[i, :k].copy(), vecs[i][:, :k].copy()
            neg = w < 0
            w[neg] = 0
            v[:, neg] = 0
            pms.append((v * np.sqrt(w)[None, :]).astype(complex))
            evs.append(w)
        return pms, evs

    # ------------------------------------------------------------------ extract: cross-correlation -> B_l (fxs_invariant_tools.py:578-645, 813-839)
    def cc_to_deg2(self, cc, max_order, order_stride=2, dimensions=3, legendre=None, average_intensity=None, bad_angles=None,
                   q1q2_symmetric=False, wide=False):
        """mtip_op_cc_to_deg2 (at most 64 extracted orders), with wide=True mtip_op_cc_to_deg2_wide (max_order <= 128, at most 129
        extracted orders; the same kernel and the same bits up to 64): cc (Nq, Nq, n_delta) float64, a numpy array or a torch tensor
        on this engine's device (then B_l comes back as a tensor on it).  Returns B_l (max_order + 1, Nq, Nq) complex128, the orders that are not multiples of
        order_stride as zeros.  legendre: (Nq, n_m (n_m + 1) / 2) table for dimensions 3 (``extract.legendre_table``);
        average_intensity (Nq): subtract_average_intensity; bad_angles (n_delta) bool: pi_periodicity."""
        on_device = not isinstance(cc, np.ndarray) and hasattr(cc, 'data_ptr')
        if on_device:
            import torch
            if cc.dtype != torch.float64 or not cc.is_cuda:
                raise TypeError('cc_to_deg2: a tensor must be float64 on the GPU (the reference takes .real of the data)')
            cc = cc.contiguous()
        else:
            cc = np.asarray(cc)
            cc = _lib.as_f64(cc.real if np.iscomplexobj(cc) else cc)
        if cc.ndim != 3 or cc.shape[0] != cc.shape[1]:
            raise ValueError('cc_to_deg2: cc must have shape (Nq, Nq, n_delta), got %r' % (tuple(cc.shape),))
        nq, nd = int(cc.shape[0]), int(cc.shape[2])
        flags = 0
        avg = bad = leg = None
        if average_intensity is not None:
            avg = _lib.as_f64(average_intensity)
            assert avg.shape == (nq,), avg.shape
            flags |= 1
        if bad_angles is not None:
            bad = _lib.as_u8(np.asarray(bad_angles, dtype=bool))
            assert bad.shape == (nd,), bad.shape
            flags |= 2
        if q1q2_symmetric:
            flags |= 4
        if legendre is not None:
            leg = _lib.as_f64(legendre)
            n_m = int(max_order) // int(order_stride) + 1
            assert leg.shape == (nq, n_m * (n_m + 1) // 2), leg.shape
        shape = (int(max_order) + 1, nq, nq)
        if on_device:
            out = torch.empty(shape, dtype=torch.complex128, device=cc.device)
            p_in, p_out = self._tp(cc), self._tp(out)
        else:
            out = np.empty(shape, complex)
            p_in, p_out = _lib.ptr(cc), _lib.ptr(out)
        entry = self.lib.mtip_op_cc_to_deg2_wide if wide else self.lib.mtip_op_cc_to_deg2
        self._ck(entry(self.ctx, nq, nd, int(max_order), int(order_stride), int(dimensions), flags, p_in, _lib.ptr(avg), _lib.ptr(bad),
                       _lib.ptr(leg), p_out))
        return out

    # ------------------------------------------------------------------ extract: the other back-substitution modes (fxs_invariant_tools.py:519-576, 646-761)
    def _c128_stack(self, name, a):
        """a complex128 stack (K, n, n): a numpy array, or a tensor on this engine's device"""
        on_device = not isinstance(a, np.ndarray) and hasattr(a, 'data_ptr')
        if on_device:
            import torch
            if a.dtype != torch.complex128 or not a.is_cuda:
                raise TypeError('%s: a tensor must be complex128 on the GPU' % name)
            a = a.contiguous()
        else:
            a = _lib.as_c128(a)
        if a.ndim != 3 or a.shape[1] != a.shape[2]:
            raise ValueError('%s: expected a stack of square matrices (K, n, n), got %r' % (name, tuple(a.shape)))
        return on_device, a

    def nearest_psd(self, mats):
        """mtip_op_nearest_psd: nearest_positive_semidefinite_matrix (mathLibrary.py:872-892, limit 0) of one matrix or a stack
        (K, n, n), a numpy array or a complex128 tensor on this engine's device (then the matrices come back as a tensor on it).
        Only the Hermitian part counts.  Returns (out, n_clipped (K) int32 numpy: eigenvalues set to zero)."""
        single = len(mats.shape) == 2
        on_device, a = self._c128_stack('nearest_psd', mats[None] if single else mats)
        K, n = int(a.shape[0]), int(a.shape[1])
        clipped = np.empty(K, np.int32)
        # the limits first: the call then writes nothing
        if on_device:
            import torch
            out = torch.empty_like(a)
            p_in, p_out = self._tp(a), self._tp(out)
        else:
            out = np.empty(a.shape if 1 <= n <= 1024 else (1,), complex)
            p_in, p_out = _lib.ptr(a), _lib.ptr(out)
        self._ck(self.lib.mtip_op_nearest_psd(self.ctx, n, K, p_in, p_out, _lib.ptr(clipped)))
        return (out[0] if single else out), clipped

    def cm_backsub(self, cm, legendre, order_stride=2, mode='plain', hermitian_mean=False, qq_mask=None):
        """mtip_op_cm_backsub: back-substitution on harmonic coefficients cm (max_order + 1, Nq, Nq) complex128 (``cc_to_deg2`` with
        dimensions=2, order_stride=1), a numpy array or a tensor on this engine's device (then B_l comes back as a tensor on it).
        mode 'plain': mathLibrary.py:1509-1517 on the harmonics m = 0, order_stride, ..; legendre the table of
        ``extract.legendre_table`` at order_stride; hermitian_mean: C_m = (C_m + C_m^+) / 2 first (back_substitution_qqsym).
        mode 'psd': back_substitution_psd (fxs_invariant_tools.py:755-760); legendre the table at stride 1.  qq_mask (Nq, Nq) bool:
        pairs to keep.  Returns (B_l (max_order + 1, Nq, Nq), info (max_order + 1) int32 numpy: eigenvalues clipped per step; None
        for 'plain')."""
        if mode not in ('plain', 'psd'):
            raise ValueError('cm_backsub: mode %r (plain, psd)' % (mode,))
        if hermitian_mean and mode != 'plain':
            raise ValueError('cm_backsub: hermitian_mean belongs to mode plain')
        on_device, cm = self._c128_stack('cm_backsub', cm)
        L, nq = int(cm.shape[0]) - 1, int(cm.shape[1])
        stride = int(order_stride)
        n_m = L + 1 if mode == 'psd' else L // max(stride, 1) + 1
        leg = _lib.as_f64(legendre)
        assert leg.shape == (nq, n_m * (n_m + 1) // 2), leg.shape
        mask = None
        if qq_mask is not None:
            mask = _lib.as_u8(np.asarray(qq_mask, dtype=bool))
            assert mask.shape == (nq, nq), mask.shape
        info = np.empty(L + 1, np.int32) if mode == 'psd' else None
        if on_device:
            import torch
            out = torch.empty_like(cm)
            p_in, p_out = self._tp(cm), self._tp(out)
        else:
            out = np.empty(cm.shape, complex)
            p_in, p_out = _lib.ptr(cm), _lib.ptr(out)
        self._ck_memory(self.lib.mtip_op_cm_backsub(self.ctx, nq, L, stride, 1 if mode == 'psd' else 0, 1 if hermitian_mean else 0, p_in,
                                                    _lib.ptr(leg), _lib.ptr(mask), p_out, _lib.ptr(info)))
        return out, info

    # ------------------------------------------------------------------ simulate_ccd: B_l -> cross-correlation (fxs_invariant_tools.py:934-1001)
    def deg2_to_cc(self, bl, mode='back_substitution', dimensions=3, legendre_t=None, cos_sin_theta=None, cos_delta=None):
        """mtip_op_deg2_to_cc: bl (max_order + 1, Nq, Nq) complex128, a numpy array or a torch tensor on this engine's device (then
        the cross-correlation comes back as a tensor on it).  mode 'back_substitution': (Nq, Nq, 2 max_order) float64; dimensions 3
        needs legendre_t ((max_order + 1)(max_order + 2) / 2, Nq) (``simulate_ccd.legendre_table_t``), dimensions 2 is the plain
        inverse harmonic transform.  mode 'lstsq': (Nq, Nq, 2 len(cos_delta) - 2) complex128 from cos_sin_theta (2, Nq) and
        cos_delta: cos of the samples Delta <= pi.  An output that does not fit the device raises MemoryError with its size."""
        if mode not in ('back_substitution', 'lstsq'):
            raise ValueError('deg2_to_cc: mode %r (back_substitution, lstsq)' % (mode,))
        on_device = not isinstance(bl, np.ndarray) and hasattr(bl, 'data_ptr')
        if on_device:
            import torch
            if bl.dtype != torch.complex128 or not bl.is_cuda:
                raise TypeError('deg2_to_cc: a tensor must be complex128 on the GPU')
            bl = bl.contiguous()
        else:
            bl = _lib.as_c128(bl)
        if bl.ndim != 3 or bl.shape[1] != bl.shape[2]:
            raise ValueError('deg2_to_cc: bl must have shape (max_order + 1, Nq, Nq), got %r' % (tuple(bl.shape),))
        L, nq = int(bl.shape[0]) - 1, int(bl.shape[1])
        lsq = mode == 'lstsq'
        leg = cst = cd = None
        if lsq:
            cst, cd = _lib.as_f64(cos_sin_theta), _lib.as_f64(cos_delta)
            assert cst.shape == (2, nq) and cd.ndim == 1, (cst.shape, cd.shape)
            nd = 2 * len(cd) - 2
        else:
            nd = 2 * L
            if dimensions == 3:
                leg = _lib.as_f64(legendre_t)
                assert leg.shape == ((L + 1) * (L + 2) // 2, nq), leg.shape
        # the limits first: the call then writes nothing, and no output of a refused size is allocated here
        fits = 1 <= L <= 128 and nq <= 4096 and 2 <= nd <= 4096
        shape = (nq, nq, nd) if fits else (1,)
        if on_device:
            out = torch.empty(shape, dtype=torch.complex128 if lsq else torch.float64, device=bl.device)
            p_in, p_out = self._tp(bl), self._tp(out)
        else:
            out = np.empty(shape, complex if lsq else float)
            p_in, p_out = _lib.ptr(bl), _lib.ptr(out)
        rc = self.lib.mtip_op_deg2_to_cc(self.ctx, nq, L, nd, int(dimensions), 1 if lsq else 0, p_in, _lib.ptr(leg), _lib.ptr(cst),
                                         _lib.ptr(cd), p_out)
        self._ck_memory(rc)
        return out

    def _ck_memory(self, rc):
        """MTIP_ENOMEM with sizes in the message is a MemoryError (as ``correlate.Correlator`` reports its accumulator)"""
        if rc == -4:
            msg = self.lib.mtip_last_error(self.ctx).decode()
            if 'GB' in msg:
                raise MemoryError(msg)
        self._ck(rc)

    # ------------------------------------------------------------------ extract on masked data (fxs_invariant_tools.py:235-289, 335-351, 452-517)
    def _cc_pair(self, name, cc, cc_mask):
        """cc float64 and cc_mask bool / uint8 (Nq, Nq, n_delta): both numpy arrays, or both tensors on this engine's device"""
        on_device = not isinstance(cc, np.ndarray) and hasattr(cc, 'data_ptr')
        if on_device:
            import torch
            if cc.dtype != torch.float64 or not cc.is_cuda or not hasattr(cc_mask, 'data_ptr') or not cc_mask.is_cuda:
                raise TypeError('%s: tensors must be float64 data and a bool / uint8 mask, both on the GPU' % name)
            cc = cc.contiguous()
            cc_mask = cc_mask.contiguous().view(torch.uint8) if cc_mask.dtype == torch.bool else cc_mask.contiguous()
            if cc_mask.dtype != torch.uint8:
                raise TypeError('%s: the mask tensor must be bool or uint8' % name)
        else:
            cc = np.asarray(cc)
            cc = _lib.as_f64(cc.real if np.iscomplexobj(cc) else cc)
            cc_mask = _lib.as_u8(np.asarray(cc_mask, dtype=bool))
        if cc.ndim != 3 or cc.shape[0] != cc.shape[1] or tuple(cc_mask.shape) != tuple(cc.shape):
            raise ValueError('%s: cc and cc_mask must both have shape (Nq, Nq, n_delta), got %r and %r'
                             % (name, tuple(cc.shape), tuple(cc_mask.shape)))
        return on_device, cc, cc_mask

    def cc_prepare_masked(self, cc, cc_mask, average_intensity=None, bad_angles=None, q1q2_symmetric=False, interpolate_phis=None):
        """mtip_op_cc_prepare_masked: modify_cross_correlation with a mask.  cc (Nq, Nq, n_delta) float64 and cc_mask (same shape,
        True = keep) as numpy arrays, or as tensors on this engine's device (then the results stay on it).  average_intensity
        (Nq): subtract_average_intensity; bad_angles (n_delta) bool: pi_periodicity; interpolate_phis (n_delta): interpolate_masked
        on these abscissae.  Returns (cc', mask' (bool), status) with status = (rows that cannot be interpolated, first such
        pair q1 Nq + q2): the caller must raise when status[0] != 0."""
        on_device, cc, cc_mask = self._cc_pair('cc_prepare_masked', cc, cc_mask)
        nq, nd = int(cc.shape[0]), int(cc.shape[2])
        flags = 0
        avg = bad = phis = None
        if average_intensity is not None:
            avg = _lib.as_f64(average_intensity)
            assert avg.shape == (nq,), avg.shape
            flags |= 1
        if bad_angles is not None:
            bad = _lib.as_u8(np.asarray(bad_angles, dtype=bool))
            assert bad.shape == (nd,), bad.shape
            flags |= 2
        if q1q2_symmetric:
            flags |= 4
        if interpolate_phis is not None:
            phis = _lib.as_f64(interpolate_phis)
            assert phis.shape == (nd,), phis.shape
            flags |= 8
        status = np.zeros(2, np.int32)
        if on_device:
            import torch
            out, mout = torch.empty_like(cc), torch.empty_like(cc_mask)
            ptrs = (self._tp(cc), self._tp(cc_mask), self._tp(out), self._tp(mout))
        else:
            out, mout = np.empty_like(cc), np.empty_like(cc_mask)
            ptrs = (_lib.ptr(cc), _lib.ptr(cc_mask), _lib.ptr(out), _lib.ptr(mout))
        self._ck(self.lib.mtip_op_cc_prepare_masked(self.ctx, nq, nd, flags, ptrs[0], ptrs[1], _lib.ptr(avg), _lib.ptr(bad), _lib.ptr(phis),
                                                    ptrs[2], ptrs[3], _lib.ptr(status)))
        mout = mout.view(torch.bool) if on_device else mout.view(bool)
        return out, mout, (int(status[0]), int(status[1]))

    def cc_lstsq_deg2(self, cc, cc_mask, orders, thetas, phis):
        """mtip_op_cc_lstsq_deg2: per pair the least-squares fit of cc[q1, q2, valid] to sum_k B_k P_orders[k](x(Delta)) / 4 pi,
        x = cos t1 cos t2 + sin t1 sin t2 cos Delta.  orders: strictly increasing ints (at most 64); thetas (Nq):
        ewald_sphere_theta_pi of the shells; phis (n_delta).  Their cosines and sines are taken here with numpy, as the reference
        takes them (fxs_invariant_tools.py:95).  Returns (B (max(orders) + 1, Nq, Nq)
        complex128 with the orders that are not listed as zeros, n_valid (Nq, Nq) int32, rcond (Nq, Nq)), numpy arrays or tensors as
        the input is.  Rank deficiency is not solved: see ``extract.masked_cross_correlation_to_deg2_invariant``."""
        on_device, cc, cc_mask = self._cc_pair('cc_lstsq_deg2', cc, cc_mask)
        nq, nd = int(cc.shape[0]), int(cc.shape[2])
        orders = np.ascontiguousarray(orders, dtype=np.int32)
        thetas, phis = np.asarray(thetas, dtype=float), np.asarray(phis, dtype=float)
        if orders.ndim != 1 or orders.size < 1 or thetas.shape != (nq,) or phis.shape != (nd,):
            raise ValueError('cc_lstsq_deg2: orders (n_orders >= 1), thetas (Nq) and phis (n_delta) do not fit cc %r' % (tuple(cc.shape),))
        cth, phis = _lib.as_f64(np.stack([np.cos(thetas), np.sin(thetas)])), _lib.as_f64(np.cos(phis))
        shape = (int(max(orders.max(), 0)) + 1, nq, nq)
        if on_device:
            import torch
            out = torch.empty(shape, dtype=torch.complex128, device=cc.device)
            nv = torch.empty((nq, nq), dtype=torch.int32, device=cc.device)
            rc = torch.empty((nq, nq), dtype=torch.float64, device=cc.device)
            ptrs = tuple(self._tp(t) for t in (cc, cc_mask, out, nv, rc))
        else:
            out, nv, rc = np.empty(shape, complex), np.empty((nq, nq), np.int32), np.empty((nq, nq))
            ptrs = tuple(_lib.ptr(t) for t in (cc, cc_mask, out, nv, rc))
        self._ck(self.lib.mtip_op_cc_lstsq_deg2(self.ctx, nq, nd, int(orders.size), _lib.ptr(orders), ptrs[0], ptrs[1], _lib.ptr(cth),
                                                _lib.ptr(phis), ptrs[2], ptrs[3], ptrs[4]))
        return out, nv, rc

    def cc_lstsq_deg2_minnorm(self, cc, cc_mask, orders, thetas, phis):
        """mtip_op_cc_lstsq_deg2_minnorm: ``cc_lstsq_deg2`` with LAPACK's truncated minimum-norm solution (numpy.linalg.lstsq,
        rcond=None) for the pairs that are rank deficient -- 0 < n_valid < n_orders, or rcond < 1e-12; every other pair keeps the
        bits of ``cc_lstsq_deg2``.  Same arguments; returns (B, n_valid, rcond, rank (Nq, Nq) int32: n_orders for a pair solved
        at full rank, the number of singular values kept for a deficient one, 0 for a pair without a valid sample)."""
        on_device, cc, cc_mask = self._cc_pair('cc_lstsq_deg2_minnorm', cc, cc_mask)
        nq, nd = int(cc.shape[0]), int(cc.shape[2])
        orders = np.ascontiguousarray(orders, dtype=np.int32)
        thetas, phis = np.asarray(thetas, dtype=float), np.asarray(phis, dtype=float)
        if orders.ndim != 1 or orders.size < 1 or thetas.shape != (nq,) or phis.shape != (nd,):
            raise ValueError('cc_lstsq_deg2_minnorm: orders (n_orders >= 1), thetas (Nq) and phis (n_delta) do not fit cc %r'
                             % (tuple(cc.shape),))
        cth, phis = _lib.as_f64(np.stack([np.cos(thetas), np.sin(thetas)])), _lib.as_f64(np.cos(phis))
        shape = (int(max(orders.max(), 0)) + 1, nq, nq)
        if on_device:
            import torch
            out = torch.empty(shape, dtype=torch.complex128, device=cc.device)
            nv = torch.empty((nq, nq), dtype=torch.int32, device=cc.device)
            rc = torch.empty((nq, nq), dtype=torch.float64, device=cc.device)
            rank = torch.empty((nq, nq), dtype=torch.int32, device=cc.device)
            ptrs = tuple(self._tp(t) for t in (cc, cc_mask, out, nv, rc, rank))
        else:
            out, nv, rc, rank = np.empty(shape, complex), np.empty((nq, nq), np.int32), np.empty((nq, nq)), np.empty((nq, nq), np.int32)
            ptrs = tuple(_lib.ptr(t) for t in (cc, cc_mask, out, nv, rc, rank))
        self._ck(self.lib.mtip_op_cc_lstsq_deg2_minnorm(self.ctx, nq, nd, int(orders.size), _lib.ptr(orders), ptrs[0], ptrs[1],
                                                        _lib.ptr(cth), _lib.ptr(phis), ptrs[2], ptrs[3], ptrs[4], ptrs[5]))
        return out, nv, rc, rank

    # ------------------------------------------------------------------ extract: the rest of modify_cross_correlation (fxs_invariant_tools.py:248-263, 281-283, 308-332)
    def _cc_array(self, name, cc):
        """cc float64 (Nq, Nq, n_delta): a numpy array, or a tensor on this engine's device"""
        on_device = not isinstance(cc, np.ndarray) and hasattr(cc, 'data_ptr')
        if on_device:
            import torch
            if cc.dtype != torch.float64 or not cc.is_cuda:
                raise TypeError('%s: a tensor must be float64 on the GPU' % name)
            cc = cc.contiguous()
        else:
            cc = np.asarray(cc)
            cc = _lib.as_f64(cc.real if np.iscomplexobj(cc) else cc)
        if cc.ndim != 3 or cc.shape[0] != cc.shape[1]:
            raise ValueError('%s: cc must have shape (Nq, Nq, n_delta), got %r' % (name, tuple(cc.shape)))
        return on_device, cc

    def _cc_average(self, average_intensity, nq):
        if average_intensity is None:
            return None
        avg = _lib.as_f64(average_intensity)
        assert avg.shape == (nq,), avg.shape
        return avg

    def cc_lowpass_q(self, cc, sos, average_intensity=None):
        """mtip_op_cc_lowpass_q: scipy.signal.sosfilt(sos, ., axis=0) then axis=1 for one second-order section with zero initial
        state (low_pass_order_in_q).  cc (Nq, Nq, n_delta) float64, numpy or a tensor on this engine's device (the result then
        stays on it); sos: (1, 6) or (6,) with a0 = 1; average_intensity (Nq): I(q1) I(q2) is subtracted first."""
        on_device, cc = self._cc_array('cc_lowpass_q', cc)
        nq, nd = int(cc.shape[0]), int(cc.shape[2])
        sos = _lib.as_f64(sos).reshape(-1)
        if sos.shape != (6,):
            raise ValueError('cc_lowpass_q: one second-order section (six coefficients) is built, got %d numbers' % sos.size)
        avg = self._cc_average(average_intensity, nq)
        if on_device:
            import torch
            out = torch.empty_like(cc)
            p_in, p_out = self._tp(cc), self._tp(out)
        else:
            out = np.empty_like(cc)
            p_in, p_out = _lib.ptr(cc), _lib.ptr(out)
        self._ck(self.lib.mtip_op_cc_lowpass_q(self.ctx, nq, nd, _lib.ptr(sos), p_in, _lib.ptr(avg), p_out))
        return out

    def cc_harmonic_filter(self, cc, max_order=None, zero_odd=False, average_intensity=None):
        """mtip_op_cc_harmonic_filter: per pair irfft(Z rfft(row)), Z zeroing the harmonics above max_order (None: no cut) and, with
        zero_odd, the odd ones (enforce_max_order, enforce_zero_odd_harmonics).  cc and average_intensity as for
        ``cc_lowpass_q``."""
        on_device, cc = self._cc_array('cc_harmonic_filter', cc)
        nq, nd = int(cc.shape[0]), int(cc.shape[2])
        if max_order is None and not zero_odd:
            raise ValueError('cc_harmonic_filter: neither max_order nor zero_odd is set')
        if max_order is not None and int(max_order) < 0:
            raise ValueError('cc_harmonic_filter: max_order %r is negative' % (max_order,))
        avg = self._cc_average(average_intensity, nq)
        if on_device:
            import torch
            out = torch.empty_like(cc)
            p_in, p_out = self._tp(cc), self._tp(out)
        else:
            out = np.empty_like(cc)
            p_in, p_out = _lib.ptr(cc), _lib.ptr(out)
        self._ck(self.lib.mtip_op_cc_harmonic_filter(self.ctx, nq, nd, -1 if max_order is None else int(max_order), 1 if zero_odd else 0,
                                                     p_in, _lib.ptr(avg), p_out))
        return out

    def cc_binned_mean(self, cc, cc_mask, bin_start, n_roll, average_intensity=None):
        """mtip_op_cc_binned_mean: the masked mean over runs of the row rolled by n_roll (apply_binned_mean); bin_start
        (n_bins + 1) and n_roll as ``extract.binned_mean_tables`` forms them with the reference's expressions.  cc and cc_mask as
        for ``cc_prepare_masked``.  Returns (cc' (Nq, Nq, n_bins), mask' bool: False where a bin has no valid sample, its value
        then 0)."""
        on_device, cc, cc_mask = self._cc_pair('cc_binned_mean', cc, cc_mask)
        nq, nd = int(cc.shape[0]), int(cc.shape[2])
        bin_start = np.ascontiguousarray(bin_start, dtype=np.int32)
        if bin_start.ndim != 1 or bin_start.size < 2:
            raise ValueError('cc_binned_mean: bin_start must hold n_bins + 1 >= 2 offsets')
        n_bins = int(bin_start.size) - 1
        avg = self._cc_average(average_intensity, nq)
        fits = nq <= 4096 and nd <= 4096                                # (beyond the limits the call writes nothing: no large output)
        shape = (nq, nq, n_bins) if fits else (1,)
        if on_device:
            import torch
            out = torch.empty(shape, dtype=torch.float64, device=cc.device)
            mout = torch.empty(shape, dtype=torch.uint8, device=cc.device)
            ptrs = (self._tp(cc), self._tp(cc_mask), self._tp(out), self._tp(mout))
        else:
            out, mout = np.empty(shape), np.empty(shape, np.uint8)
            ptrs = (_lib.ptr(cc), _lib.ptr(cc_mask), _lib.ptr(out), _lib.ptr(mout))
        self._ck(self.lib.mtip_op_cc_binned_mean(self.ctx, nq, nd, n_bins, _lib.ptr(bin_start), int(n_roll), ptrs[0], ptrs[1],
                                                 _lib.ptr(avg), ptrs[2], ptrs[3]))
        mout = mout.view(torch.bool) if on_device else mout.view(bool)
        return out, mout

    # ------------------------------------------------------------------ rotational alignment (average.py:920-960)
    def _so3_setup(self):
        if not getattr(self, '_so3_ready', False):
            tab = np.ascontiguousarray(hs.wigner_d_table(self.L))
            self._ck(self.lib.mtip_set_so3_tables(self.ctx, self.L + 1, _lib.ptr(tab)))
            self._so3_ready = True

    def so3_correlation(self, ref_coeff, sig_coeff, r_limit_ids=None):
        """C[b, alpha, beta, gamma] = mean_r Re <ref_r, R sig_r> on the (2 bw)^3 Euler grid (soft.calc_mean_C)"""
        self._so3_setup()
        ref = np.ascontiguousarray(_lib.as_c128(ref_coeff).reshape(self.N, self.nlm))
        sig = self._bcoef(sig_coeff)
        lo, hi = (0, self.N) if r_limit_ids is None else (int(r_limit_ids[0]), int(r_limit_ids[1]))
        nb = 2 * (self.L + 1)
        out = np.empty((self.B, nb, nb, nb))
        self._ck(self.lib.mtip_op_so3_correlation(self.ctx, _lib.ptr(ref), _lib.ptr(sig), lo, hi, _lib.ptr(out)))
        return out

    def rotate_coefficients(self, coeff, eulers):
        """f_lm -> sum_n D^l_mn(euler_b) f_ln per restart (soft.rotate_coeff); eulers: (3,) or (B, 3)"""
        self._so3_setup()
        c = self._bcoef(coeff)
        eulers = np.broadcast_to(np.asarray(eulers, dtype=float), (self.B, 3))
        D = np.ascontiguousarray(np.stack([hs.wigner_D_flat(self.L, e) for e in eulers]))
        out = np.empty_like(c)
        self._ck(self.lib.mtip_op_rotate_coefficients(self.ctx, _lib.ptr(c), _lib.ptr(D), _lib.ptr(out)))
        return out

    # ------------------------------------------------------------------ the same operators on device-resident batches
    # torch tensors hold the memory (complex128, contiguous, leading dimension n_batch) on the context's device -- CPU tensors
    # under the emulation; the operators read and write them in place in HBM, nothing crosses PCIe.
    def t_fourier_transform(self, g, inverse=False):
        import torch
        assert tuple(g.shape) == (self.B,) + self.shape and g.dtype == torch.complex128
        out = torch.empty_like(g)
        self._ck(self.lib.mtip_op_fourier_transform(self.ctx, self._tp(g), self._tp(out), int(inverse)))
        return out

    def t_sht_forward(self, g):
        import torch
        assert tuple(g.shape) == (self.B,) + self.shape and g.dtype == torch.complex128
        out = torch.empty((self.B, self.N, self.nlm), dtype=torch.complex128, device=g.device)
        self._ck(self.lib.mtip_op_sht_forward(self.ctx, self._tp(g), self._tp(out), 0))
        return out

    def t_sht_inverse(self, c):
        import torch
        assert tuple(c.shape) == (self.B, self.N, self.nlm) and c.dtype == torch.complex128
        out = torch.empty((self.B,) + self.shape, dtype=torch.complex128, device=c.device)
        self._ck(self.lib.mtip_op_sht_inverse(self.ctx, self._tp(c), self._tp(out)))
        return out

    # ---- grid arithmetic of the averaging worker on device stacks (csrc/k_average.hip): torch owns the memory, nothing else
    def t_grid_stats(self, X, ref=None):
        """(n, 12) host array per grid of the stack X (n, Nq, n_theta, n_phi): integrals, moments, extrema (mtip_op_grid_stats)"""
        import torch
        assert X.dtype == torch.complex128 and tuple(X.shape[1:]) == self.shape and X.is_contiguous()
        out = np.zeros((X.shape[0], 12))
        wr, wt = _lib.as_f64(self.int_wr), _lib.as_f64(self.int_wt)
        self._ck(self.lib.mtip_op_grid_stats(self.ctx, self._tp(X), int(X.shape[0]), self._tp(ref) if ref is not None else None,
                                             _lib.ptr(wr), _lib.ptr(wt), _lib.ptr(out)))
        return out

    def t_phase_ramp(self, X, centers_cartesian, sign):
        """X[b] *= exp(-i sign k . c_b) in place (generate_shift_by_operator, fxs_Projections.py:1419-1444)"""
        import torch
        assert X.dtype == torch.complex128 and tuple(X.shape[1:]) == self.shape and X.is_contiguous()
        cc = np.ascontiguousarray(centers_cartesian, dtype=np.float64)
        assert cc.shape == (X.shape[0], 3)
        self._ck(self.lib.mtip_op_grid_phase_ramp(self.ctx, self._tp(X), int(X.shape[0]), _lib.ptr(cc), float(sign)))
        return X

    def t_combine(self, op, A, scalars=None):
        """mtip_op_grid_combine on a stack A (n, ...): 'conj', 'scale' (complex per grid), 'sum', 'abs2sum' (one grid out), 'affine'"""
        import torch
        code = {'conj': 0, 'scale': 1, 'sum': 2, 'abs2sum': 3, 'affine': 4}[op]
        assert A.dtype == torch.complex128 and tuple(A.shape[1:]) == self.shape and A.is_contiguous()
        out = torch.empty(self.shape if code in (2, 3) else tuple(A.shape), dtype=torch.complex128, device=A.device)
        sc = None if scalars is None else np.ascontiguousarray(scalars, dtype=np.complex128)
        self._ck(self.lib.mtip_op_grid_combine(self.ctx, code, self._tp(out), self._tp(A), int(A.shape[0]), _lib.ptr(sc) if sc is not None else None))
        return out

    def t_prtf(self, a1, a2, I1, I2):
        """resolution_metrics.py:62-78: per-shell mean (complex) and standard deviation of sqrt(a1 conj(a2) / sqrt(I1 I2))"""
        mean = np.zeros(self.N, complex)
        std = np.zeros(self.N)
        for x in (a1, a2, I1, I2):
            assert tuple(x.shape) == self.shape and x.is_contiguous()
        self._ck(self.lib.mtip_op_prtf(self.ctx, self._tp(a1), self._tp(a2), self._tp(I1), self._tp(I2), _lib.ptr(mean), _lib.ptr(std)))
        return mean, std

    def t_fsc(self, a1, a2):
        """resolution_metrics.py:23-33: per-shell Fourier shell correlation of two grids, (Nq,) on the host"""
        fsc = np.zeros(self.N)
        for x in (a1, a2):
            assert tuple(x.shape) == self.shape and x.is_contiguous()
        self._ck(self.lib.mtip_op_fsc(self.ctx, self._tp(a1), self._tp(a2), _lib.ptr(fsc)))
        return fsc

    def t_state(self, kind, batch, best=False):
        """a grid of the loop state -- 'density', 'reciprocal_density' (complex128) or 'support' (uint8), current or best pair -- as a
        tensor ON THE ENGINE'S DEVICE (device-to-device copy out of the slot arrays; the getters of the C ABI take a device
        destination as well as a host one).  What the end-of-run gather sends from (parallel.gather_results)."""
        import torch
        dev = self.torch_device()
        if kind == 'support':
            out = torch.empty(self.shape, dtype=torch.uint8, device=dev)
            self._ck(self.lib.mtip_get_support(self.ctx, int(batch), int(best), self._tp(out)))
            return out
        fn = {'density': self.lib.mtip_get_density, 'reciprocal_density': self.lib.mtip_get_reciprocal_density}[kind]
        out = torch.empty(self.shape, dtype=torch.complex128, device=dev)
        self._ck(fn(self.ctx, int(batch), int(best), self._tp(out)))
        return out

    def t_find_rotation(self, ref_coeff, sig_coeff, r_limit_ids=None, keep_metric=False):
        """find_rotation (average.py:920-947) for a batch: (arg-max in the reference's reading order as (i_beta, i_alpha, i_gamma)
        per restart, the maxima, the correlation (B, nb, nb, nb) [alpha, beta, gamma] on the device or None)"""
        import torch
        self._so3_setup()
        assert tuple(ref_coeff.shape) == (self.N, self.nlm) and tuple(sig_coeff.shape) == (self.B, self.N, self.nlm)
        lo, hi = (0, self.N) if r_limit_ids is None else (int(r_limit_ids[0]), int(r_limit_ids[1]))
        nb = 2 * (self.L + 1)
        arg = np.empty(self.B, np.int64)
        vmax = np.empty(self.B)
        Cm = torch.empty((self.B, nb, nb, nb), dtype=torch.float64, device=sig_coeff.device) if keep_metric else None
        self._ck(self.lib.mtip_op_so3_find_rotation(self.ctx, self._tp(ref_coeff), self._tp(sig_coeff), lo, hi, _lib.ptr(arg),
                                                    _lib.ptr(vmax), self._tp(Cm) if keep_metric else None))
        return np.stack(np.unravel_index(arg, (nb, nb, nb)), axis=1), vmax, Cm

    def t_rotate_grid(self, coeff, beta_index, alpha, gamma):
        """rotate (average.py:948-960) by Euler angles (alpha[b], beta sample beta_index[b], gamma[b])"""
        import torch
        self._so3_setup()
        assert tuple(coeff.shape) == (self.B, self.N, self.nlm) and coeff.dtype == torch.complex128
        bi = np.ascontiguousarray(beta_index, dtype=np.int32)
        al, ga = _lib.as_f64(alpha), _lib.as_f64(gamma)
        assert bi.shape == (self.B,) and al.shape == (self.B,) and ga.shape == (self.B,)
        out = torch.empty_like(coeff)
        self._ck(self.lib.mtip_op_rotate_coefficients_grid(self.ctx, self._tp(coeff), _lib.ptr(bi), _lib.ptr(al), _lib.ptr(ga), self._tp(out)))
        return out

    # ------------------------------------------------------------------ state and loop
    def set_density(self, batch, rho):
        r = _lib.as_c128(rho)
        assert r.shape == self.shape
        self._ck(self.lib.mtip_set_density(self.ctx, batch, _lib.ptr(r)))

    def init_state(self):
        self._ck(self.lib.mtip_init_state(self.ctx))

    def reset_support(self):
        """back to the initial support, enforced, for every restart (the state a fresh reconstruction starts from,
        fxs_Projections.py:34, 133-155)"""
        s0 = _lib.as_u8(self.initial_support)
        self._ck(self.lib.mtip_set_initial_support(self.ctx, _lib.ptr(s0)))

    def density(self, batch, best=False):
        out = np.empty(self.shape, complex)
        self._ck(self.lib.mtip_get_density(self.ctx, batch, int(best), _lib.ptr(out)))
        return out

    def reciprocal_density(self, batch, best=False):
        out = np.empty(self.shape, complex)
        self._ck(self.lib.mtip_get_reciprocal_density(self.ctx, batch, int(best), _lib.ptr(out)))
        return out

    def support(self, batch, best=False):
        out = np.empty(self.shape, np.uint8)
        self._ck(self.lib.mtip_get_support(self.ctx, batch, int(best), _lib.ptr(out)))
        return out.astype(bool)

    def set_support(self, batch, support, enforce_initial_support):
        s = _lib.as_u8(support)
        self._ck(self.lib.mtip_set_support(self.ctx, batch, _lib.ptr(s), int(bool(enforce_initial_support))))

    def unknowns(self, batch):
        out = []
        for l in range(self.L + 1):
            k = min(2 * l + 1, self.N)
            u = np.empty((k, 2 * l + 1), complex)
            self._ck(self.lib.mtip_get_unknowns(self.ctx, batch, l, _lib.ptr(u)))
            out.append(u)
        return tuple(out)

    def best_error(self):
        out = np.empty(self.B)
        n = C.c_int64(0)
        self._ck(self.lib.mtip_get_best_error(self.ctx, _lib.ptr(out), C.byref(n)))
        return out, int(n.value)

    def select_best(self, where=None):
        """reconstruct.py:945-949 for all restarts, or for those flagged in `where` (bool per restart)."""
        if where is None:
            self._ck(self.lib.mtip_select_best(self.ctx))
        else:
            w = np.ascontiguousarray(np.asarray(where, dtype=np.uint8))
            assert w.shape == (self.B,)
            self._ck(self.lib.mtip_select_best_where(self.ctx, _lib.ptr(w)))

    def set_ft_stab_mask(self, mask):
        """ft_stab per restart for the runs that follow (bool per restart), None = every restart (mtip_set_ft_stab_mask)"""
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask, dtype=bool).astype(np.uint8))
        assert m is None or m.shape == (self.B,)
        self._ck(self.lib.mtip_set_ft_stab_mask(self.ctx, _lib.ptr(m)))
        self._ft_mask_set = m is not None

    def run(self, method, ft_stab, betas, fetch=True):
        """n = len(betas) steps of `method`; ft_stab: bool, or a bool per restart (the reference links ft_stab to the shrink-wrap's
        enforce decision per reconstruction process: restarts of a batch may disagree)"""
        betas = _lib.as_f64(np.atleast_1d(betas))
        n = len(betas)
        ft_stab = _lib.ft_stab_flag(self, ft_stab)
        if self.group is not None:
            # side by side with other engines of this GPU: the group enqueues everybody's steps in turn order (EngineGroup); a
            # per-restart ft_stab mask is state of this engine's context, the call itself says ft_stab = 1
            best = np.empty(self.B)
            first = C.c_int64(0)
            if fetch:
                self._ck(self.lib.mtip_get_best_error(self.ctx, _lib.ptr(best), C.byref(first)))
            self.group.member_run(self, method, ft_stab, betas)
            if not fetch:
                return None, None
            return self.fetch_errors(first.value, n)
        if not fetch:
            self._ck(self.lib.mtip_run_async(self.ctx, METHOD_ID[method], int(bool(ft_stab)), n, _lib.ptr(betas)))
            return None, None
        err = np.empty((n, self.B))
        deg2 = np.empty((n, self.B, self.L + 1)) if self.deg2_enabled else None
        self._ck(self.lib.mtip_run(self.ctx, METHOD_ID[method], int(bool(ft_stab)), n, _lib.ptr(betas), _lib.ptr(err), _lib.ptr(deg2)))
        return err, deg2

    def fetch_errors(self, first, n):
        err = np.empty((n, self.B))
        deg2 = np.empty((n, self.B, self.L + 1)) if self.deg2_enabled else None
        self._ck(self.lib.mtip_fetch_errors(self.ctx, first, n, _lib.ptr(err), _lib.ptr(deg2)))
        return err, deg2

    def fetch_reciprocal_l2(self, first, n):
        """reciprocal l2_projection_diff of the steps [first, first + n): (n, B), or None when the metric is off"""
        if not self.reciprocal_l2:
            return None
        out = np.empty((n, self.B))
        self._ck(self.lib.mtip_fetch_reciprocal_l2_metric(self.ctx, first, n, _lib.ptr(out)))
        return out

    def fetch_invariant_metrics(self, first, n):
        """{'II_error': (n, B), 'ccd_diff': (n, B), 'fqc_error': (n, B, Nq)} for the enabled ones"""
        out = {}
        if not self.invariant_metrics:
            return out
        II = np.empty((n, self.B)) if 'II_error' in self.invariant_metrics else None
        ccd = np.empty((n, self.B)) if 'ccd_diff' in self.invariant_metrics else None
        fqc = np.empty((n, self.B, self.N)) if 'fqc_error' in self.invariant_metrics else None
        self._ck(self.lib.mtip_fetch_invariant_metrics(self.ctx, first, n, _lib.ptr(II), _lib.ptr(ccd), _lib.ptr(fqc)))
        for k, v in (('II_error', II), ('ccd_diff', ccd), ('fqc_error', fqc)):
            if v is not None:
                out[k] = v
        return out

    def invariant_metrics_of(self, Ilm):
        """the enabled metrics of given intensity coefficients: {'II_error': (B,), 'ccd_diff': (B,), 'fqc_error': (B, Nq)}"""
        c = self._bcoef(Ilm)
        II, ccd, fqc = np.empty(self.B), np.empty(self.B), np.empty((self.B, self.N))
        self._ck(self.lib.mtip_op_invariant_metrics(self.ctx, _lib.ptr(c), _lib.ptr(II), _lib.ptr(ccd), _lib.ptr(fqc)))
        return {k: v for k, v in (('II_error', II), ('ccd_diff', ccd), ('fqc_error', fqc)) if k in self.invariant_metrics}

    def fetch_main_errors(self, first, n):
        err = np.empty((n, self.B))
        self._ck(self.lib.mtip_fetch_main_errors(self.ctx, first, n, _lib.ptr(err)))
        return err

    def shrinkwrap(self, sigma, threshold, error_limit):
        enforced = np.empty(self.B, np.uint8)
        self._ck(self.lib.mtip_shrinkwrap(self.ctx, float(sigma), float(threshold), float(error_limit), _lib.ptr(enforced)))
        return enforced.astype(bool)

    def begin_sub_loop(self):
        """top of a sub-loop call (reconstruct.py:859, 866): stale `hist` and latest_intensity are reset"""
        self._ck(self.lib.mtip_begin_sub_loop(self.ctx))

    def refresh_reciprocal_density(self):
        """'SW_center' tail (reconstruct.py:891-894), literally: the last pair becomes (reciprocal, real) = (rho, FT(rho))."""
        self._ck(self.lib.mtip_refresh_reciprocal_density(self.ctx))

    def last_deg2_invariant(self, batch):
        out = np.empty((self.L + 1, self.N, self.N), complex)
        self._ck(self.lib.mtip_last_deg2_invariant(self.ctx, batch, _lib.ptr(out)))
        return out

    def synchronize(self):
        self._ck(self.lib.mtip_synchronize(self.ctx))

    # ------------------------------------------------------------------ profiling
    def profile(self, enable=True):
        self._ck(self.lib.mtip_profile(self.ctx, int(enable)))
        self._ck(self.lib.mtip_profile_reset(self.ctx))

    def profile_get(self, name):
        ms, n = C.c_double(0), C.c_int64(0)
        self._ck(self.lib.mtip_profile_get(self.ctx, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def debug_spin(self, microseconds):
        """enqueue a kernel that spins for `microseconds` on this engine's stream (asynchronous; see streams_side_by_side)"""
        self._ck(self.lib.mtip_debug_spin(self.ctx, float(microseconds)))

    def jacobi_sweeps(self):
        out = np.zeros((self.B, self.L + 1), np.int32)
        self._ck(self.lib.mtip_debug_jacobi_sweeps(self.ctx, _lib.ptr(out)))
        return out & 0xff

    def jacobi_active_columns(self):
        """columns of X_l the last polar-factor call still rotated in its final sweep (numerical rank estimate)"""
        out = np.zeros((self.B, self.L + 1), np.int32)
        self._ck(self.lib.mtip_debug_jacobi_sweeps(self.ctx, _lib.ptr(out)))
        return (out >> 8) & 0xffff

    def hankel_tiles(self):
        """(ct, n_tiles, n_row_blocks) of the Hankel kernel's launch plan: 16-column tiles per workgroup, grid x, grid y"""
        ct, nt, nr = C.c_int(0), C.c_int(0), C.c_int(0)
        self._ck(self.lib.mtip_debug_hankel_tiles(self.ctx, C.byref(ct), C.byref(nt), C.byref(nr)))
        return ct.value, nt.value, nr.value

    SHT_PLAN_FIELDS = ('fwd', 'inv', 'fwd_rp', 'fwd_th', 'fwd_maxi', 'inv_rp', 'inv_nsplit', 'inv_jl', 'real_update',
                       'chain', 'chain_gsz', 'chain_thg', 'chain_maxi')
    SHT_FWD_KINDS = ('generic', 'lds', 'reg', 'pair', 'big')
    SHT_INV_KINDS = ('generic', 'lds', 'reg', 'wide', 'big')
    SHT_CHAIN_KINDS = ('off', 'rt', 'regtab', 'l32')

    def sht_plan(self):
        """the SHT kernel choice of this context (ShtPlan, csrc/mtip_internal.h) as a dict: the kinds as names, real_update as a
        bool, the rest as ints; host only, nothing is launched"""
        out = np.zeros(len(self.SHT_PLAN_FIELDS), np.int32)
        self._ck(self.lib.mtip_debug_sht_plan(self.ctx, _lib.ptr(out)))
        p = {k: int(v) for k, v in zip(self.SHT_PLAN_FIELDS, out)}
        p['fwd'], p['inv'], p['chain'] = self.SHT_FWD_KINDS[p['fwd']], self.SHT_INV_KINDS[p['inv']], self.SHT_CHAIN_KINDS[p['chain']]
        p['real_update'] = bool(p['real_update'])
        return p

    def projection_slots(self):
        """workgroups per restart of the real projection kernel in the last call (0: general complex kernels)"""
        n = self.lib.mtip_debug_projection_slots(self.ctx)
        if n < 0:
            self._ck(n)
        return int(n)

    def jacobi_closing_step(self):
        """how the real-arithmetic projection closed its sweeps in the last call, per (restart, order): 0 = classic confirming sweep,
        1 = first-order, 2 = second-order polar step on the Gram matrix (k_projr.hip)"""
        out = np.zeros((self.B, self.L + 1), np.int32)
        self._ck(self.lib.mtip_debug_jacobi_sweeps(self.ctx, _lib.ptr(out)))
        return (out >> 24) & 3

    # ------------------------------------------------------------------ helpers shared with synthetic.py
    @property
    def thetas(self):
        return self.theta

    @property
    def phis(self):
        return self.phi

    def ft(self, grid):
        """transforms adapter for synthetic.make_invariants (batch element 0)."""
        return self.fourier_transform(grid)[0]

    def forward_l(self, grid):
        c = self.sht_forward(grid)[0]
        return [np.array(c[:, l * l:(l + 1) ** 2]) for l in range(self.L + 1)]


class EngineGroup:
    """Engines of one GPU that step side by side (the reference's `GPU.n_gpu_workers` restart groups, reconstruct.py:104), run
    through mtip_run_group_async: the same steps per engine, enqueued so that the engines take turns at the chip-filling
    transforms while the others' projections run beside them (mtip_api.hip).

    ``run(method, ft_stab, betas)`` is the direct form (one host thread drives all engines: bench.py).  A worker whose restart
    groups run the reference's loop each in their own host thread attaches the engines (``attach``): every ``Engine.run`` then
    meets the others here, and the last one to arrive enqueues for all that asked for the same steps (engines that asked for
    something else -- a data-dependent ft_stab decision, say -- are enqueued on their own).  A member that is done ``leave``s;
    nobody waits for a member that has left, and a wait that lasts longer than `patience` seconds stops waiting and enqueues alone."""

    def __init__(self, engines=(), patience=30.0):
        import threading
        self.engines = list(engines)
        self.cond = threading.Condition()
        self.members = []
        self.pending = {}
        self.generation = 0
        self.patience = patience
        self.calls = {'group': 0, 'single': 0}

    # -- direct form
    def run(self, method, ft_stab, betas):
        betas = _lib.as_f64(np.atleast_1d(betas))
        self._enqueue(self.engines, method, ft_stab, betas)

    def _enqueue(self, engines, method, ft_stab, betas):
        e0 = engines[0]
        if len(engines) == 1:
            e0._ck(e0.lib.mtip_run_async(e0.ctx, METHOD_ID[method], int(bool(ft_stab)), len(betas), _lib.ptr(betas)))
            self.calls['single'] += 1
            return
        import ctypes as C
        arr = (C.c_void_p * len(engines))(*[e.ctx for e in engines])
        rc = e0.lib.mtip_run_group_async(arr, len(engines), METHOD_ID[method], int(bool(ft_stab)), len(betas), _lib.ptr(betas))
        self.calls['group'] += 1
        if rc != 0:
            for e in engines:                       # the context that failed holds the message
                msg = e.lib.mtip_last_error(e.ctx).decode()
                if msg:
                    raise RuntimeError('mtip_run_group_async: %s' % msg)
            raise RuntimeError('mtip_run_group_async failed with code %d' % rc)

    # -- rendezvous form (one host thread per engine)
    def attach(self, engine):
        with self.cond:
            self.members.append(engine)
            engine.group = self

    def leave(self, engine):
        with self.cond:
            if engine in self.members:
                self.members.remove(engine)
            engine.group = None
            self.pending.pop(id(engine), None)
            self._flush_if_complete()

    def _flush_if_complete(self):
        if not self.pending or len(self.pending) < len(self.members):
            return
        self._flush()

    def _flush(self):
        todo = list(self.pending.values())
        self.pending.clear()
        self.generation += 1
        errors = []
        while todo:
            e, method, ft_stab, betas = todo[0]
            same = [t for t in todo if t[1] == method and t[2] == ft_stab and np.array_equal(t[3], betas)]
            todo = [t for t in todo if not any(t is u for u in same)]
            try:
                self._enqueue([t[0] for t in same], method, ft_stab, betas)
            except Exception as ex:                 # delivered to every waiting member: nobody is left hanging
                errors.append(ex)
        self.error = errors[0] if errors else None
        self.cond.notify_all()

    def member_run(self, engine, method, ft_stab, betas):
        import time
        with self.cond:
            self.pending[id(engine)] = (engine, method, bool(ft_stab), betas)
            gen = self.generation
            if len(self.pending) >= len(self.members):
                self._flush()
            else:
                deadline = time.monotonic() + self.patience
                while self.generation == gen:
                    left = deadline - time.monotonic()
                    if left <= 0:                    # the others are busy elsewhere: go alone
                        self.pending.pop(id(engine), None)
                        self._enqueue([engine], method, ft_stab, betas)
                        return
                    self.cond.wait(left)
            if getattr(self, 'error', None) is not None:
                raise self.error


def streams_side_by_side(engines, microseconds=2000.0, reps=3):
    """How many of the engines' streams execute at the same time: every engine gets `reps` spin kernels, the ratio of the
    serial time to the measured wall time is the number of chains that ran side by side.  HIP maps streams onto a pool of
    hardware queues (GPU_MAX_HW_QUEUES); two engines on one queue serialise, which no kernel timing shows directly."""
    import time
    for e in engines:
        e.debug_spin(10.0)
    for e in engines:
        e.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        for e in engines:
            e.debug_spin(microseconds)
    for e in engines:
        e.synchronize()
    wall = time.perf_counter() - t0
    return len(engines) * reps * microseconds * 1e-6 / wall

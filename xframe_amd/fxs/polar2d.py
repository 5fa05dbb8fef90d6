"""The 2-D (polar) variant of the hot path on the MI355X, operator level: the circular harmonic transforms
(``xframe/library/mathLibrary.py:469-496``), the polar Hankel pair with midpoint weights (``hankel_transforms.py:411-424, 300-362,
602-640``), the Fourier pair ``generate_ft`` builds from them (``fourier_transforms.py:49-88``) on the polar midpoint grid pair
(``ft_grid_pairs.py:282-291, 325-336``) and the 2-D reciprocal projection (``fxs_Projections.py:723-745, 803-826, 855-863``),
through the ``mtip2d_*`` entry points of ``include/mtip_hip.h`` (``csrc/k_polar2d.hip``); the radial rules besides midpoint (trapz,
gauss, Zernike: ``hankel_transforms.py:133-176, 335-375, 492-535``) are host weight tables for the same device contraction.  The 2-D
phasing loop on these operators is ``reconstruct2d.py``; ``Engine2D`` also carries the resident loop (``set_density`` ... ``run``, the 3-D
engine's names on ``mtip2d_run`` and friends: the state of a batch of restarts stays in HBM between the steps); no CPU fallback."""
import ctypes as C

import numpy as np
from scipy.special import jv

from . import _lib


def polar_mid_weights(orders, n_radial_points, reciprocity_coefficient):
    """calc_polar_mid_weights (hankel_transforms.py:411-424)"""
    N = n_radial_points
    ps = np.arange(N) + 0.5
    ks = np.arange(N) + 0.5
    ms = np.asarray(orders, dtype=float)
    return ps[None, :, None] * jv(ms[:, None, None], ks[None, None, :] * ps[None, :, None] * reciprocity_coefficient / N)


def assemble_weights_mid(weights, orders, r_max, reciprocity_coefficient):
    """assemble_weights_mid, 2-D branch (hankel_transforms.py:300-362)"""
    orders = np.asarray(orders)
    N = weights.shape[-1]
    q_max = reciprocity_coefficient * N / r_max
    all_orders = np.concatenate((orders, -orders[:0:-1]))
    w = np.concatenate((weights, (-1.0) ** orders[:0:-1, None, None] * weights[:0:-1]), axis=0)
    w = np.moveaxis(w, 0, 2)
    return (w * ((-1.j) ** all_orders[None, None, :] * (r_max / N) ** 2), w * ((1.j) ** all_orders[None, None, :] * (q_max / N) ** 2))


def polar_raw_weights(orders, n, kappa, mode='midpoint'):
    """raw polar Hankel weights [m, p, k] of a radial rule, as the reference's loader builds them for dimensions = 2: `midpoint`
    (hankel_transforms.py:411-424), `trapz` (335-347) and `Zernike` (133-176) sum over p = 1..N-1, `gauss` (492-507) over the
    Gauss-Legendre nodes.  Zernike: the loader passes the reciprocity coefficient on as `expansion_limit` (26, 52-62), so the expansion
    stops at max(kappa, M) and the Bessel arguments use pi (the same quirk as in 3-D, hostsetup._zernike_raw_weights)"""
    ms = np.asarray(orders, dtype=float)
    if mode == 'midpoint':
        return polar_mid_weights(orders, n, kappa)
    if mode == 'trapz':
        ps, ks = np.arange(1, n), np.arange(n)
        return ps[None, :, None] * jv(ms[:, None, None], ks[None, None, :] * ps[None, :, None] * kappa / n)
    if mode == 'gauss':
        from scipy.special import roots_legendre
        xi, wg = roots_legendre(n)
        node = xi + 1
        return node[None, :, None] * wg[None, :, None] * jv(ms[:, None, None], node[None, None, :] * node[None, :, None] * kappa * n / 4)
    if mode == 'Zernike':
        from scipy.special import eval_jacobi
        limit = max(kappa, ms.max())
        ps, ks = np.arange(1, n), np.arange(n)
        x = ps / n
        out = np.zeros((len(ms), n - 1, n))
        for i, m in enumerate(ms):
            terms = np.arange(m, limit + 1, 2)
            j = (terms - m) / 2
            radial = (x ** m)[None, :] * eval_jacobi(j[:, None], m, 0, (1 - 2 * x * x)[None, :])        # (-1)^j R^m_s(x), mathLibrary.py:805-819 with D = 2
            out[i, :, 1:] = np.einsum('s,sp,sk->pk', 2 * terms + 2, radial, jv((terms + 1)[:, None], (ks[1:] * np.pi)[None, :]))
            if m == 0:
                out[i, :, 0] = np.pi
        out[:, :, 1:] *= (ps[:, None] / ks[None, 1:])[None]
        out[:, :, 0] *= ps[None, :]
        return out
    raise NotImplementedError(f"2-D fourier_transform.type {mode!r}: 'midpoint', 'trapz', 'gauss', 'Zernike'")


def assemble_weights_2d(weights, orders, r_max, kappa, mode='midpoint'):
    """(forward, inverse) complex weights (p, k, all orders 0..M, -M..-1), N x N x (2M + 1): assemble_weights for dimensions = 2
    (midpoint 426-452, trapz 349-375, gauss 509-535, Zernike 270-300); the rules that leave out shell 0 of their input get a zero row
    for it, so that the device contraction is the same N x N sum for every rule"""
    orders = np.asarray(orders)
    n = weights.shape[-1]
    q_max = kappa * n / r_max
    signed = np.concatenate((orders, orders[:0:-1] if mode == 'Zernike' else -orders[:0:-1]))       # (Zernike's sign vector has no signs)
    fs, iv = {'gauss': ((r_max / 2) ** 2, (q_max / 2) ** 2),
              'Zernike': ((r_max / n) ** 2 / np.pi, (q_max / n) ** 2 / np.pi)}.get(mode, ((r_max / n) ** 2, (q_max / n) ** 2))
    w = np.concatenate((weights, (-1.0) ** orders[:0:-1, None, None] * weights[:0:-1]), axis=0)
    if w.shape[1] == n - 1:
        w = np.concatenate((np.zeros((w.shape[0], 1, n)), w), axis=1)
    w = np.moveaxis(w, 0, 2)
    return w * ((-1.j) ** signed[None, None, :] * fs), w * ((1.j) ** signed[None, None, :] * iv)


class Engine2D(_lib.TensorOperands):
    """transforms (and, after ``set_projection``, the reciprocal projection) of the 2-D variant for batches of ``n_batch`` grids"""

    def __init__(self, n_radial_points, max_order, max_q, reciprocity_coefficient=2.0, n_batch=1, device=0, lib_path=None, used_orders=None,
                 weights_r_max=None, mode='midpoint'):
        self.lib = _lib.load(lib_path)
        self.N, self.M, self.B = int(n_radial_points), int(max_order), int(n_batch)
        self.n_phi = 2 * self.M + 1                              # harmonic_transforms.py:44-47
        self.kappa = float(reciprocity_coefficient)
        self.q_max = float(max_q)
        self.r_max = self.kappa * self.N / self.q_max            # mathLibrary.py:1169-1176
        from .hostsetup import radial_grids
        self.mode = mode
        self.rs, self.qs = radial_grids(self.q_max, self.N, self.kappa, mode)      # the polar pairs use the spherical pairs' radial functions (ft_grid_pairs.py:312-349)
        self.phis = np.arange(self.n_phi) / self.n_phi * 2 * np.pi
        self.shape = (self.N, self.n_phi)
        if self.lib.mtip_device_count() <= 0:
            raise _lib.MtipError('no HIP device visible: the 2-D operators need an MI355X (no CPU fallback)')
        self.device_index = int(device)
        self.ctx = self.lib.mtip2d_create(self.N, self.n_phi, self.B, int(device))
        if not self.ctx:
            raise _lib.MtipError('mtip2d_create failed (sizes: n_phi odd, 3..2047; a visible device)')
        orders = np.arange(self.M + 1)
        # (the phasing loop hands generate_ft max(r_p) instead of the cutoff, reconstruct.py:329: `weights_r_max`)
        fw, iw = assemble_weights_2d(polar_raw_weights(orders, self.N, self.kappa, mode), orders,
                                     self.r_max if weights_r_max is None else float(weights_r_max), self.kappa, mode)
        all_abs = np.concatenate((orders, orders[:0:-1]))
        unused = ~np.isin(all_abs, orders if used_orders is None else np.asarray(used_orders))     # hankel_transforms.py:611-613
        self._ck(self.lib.mtip2d_set_hankel_weights(self.ctx, _lib.ptr(_lib.as_c128(fw)), _lib.ptr(_lib.as_c128(iw)), _lib.ptr(_lib.as_u8(unused))))
        self.n_used = 0

    def _ck(self, rc):
        if rc != 0:
            raise _lib.MtipError(f'libmtip_hip (2-D) error {rc}: ' + self.lib.mtip2d_last_error(self.ctx).decode())

    def close(self):
        if getattr(self, 'ctx', None):
            self.lib.mtip2d_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _grid(self, a, last=None):
        a = _lib.as_c128(a)
        shape = (self.N, self.n_phi if last is None else last)
        if a.shape == shape:
            a = np.broadcast_to(a, (self.B,) + shape)
        assert a.shape == (self.B,) + shape, (a.shape, shape)
        return np.ascontiguousarray(a)

    def harmonic(self, grid, inverse=False):
        g = self._grid(grid)
        out = np.empty_like(g)
        self._ck(self.lib.mtip2d_op_harmonic(self.ctx, _lib.ptr(g), _lib.ptr(out), int(inverse)))
        return out

    def real_harmonic_forward(self, grid):
        g = self._grid(grid)
        out = np.empty((self.B, self.N, self.M + 1), complex)
        self._ck(self.lib.mtip2d_op_real_harmonic_forward(self.ctx, _lib.ptr(g), _lib.ptr(out)))
        return out

    def real_harmonic_inverse(self, coeff):
        c = self._grid(coeff, self.M + 1)
        out = np.empty((self.B, self.N, self.n_phi))
        self._ck(self.lib.mtip2d_op_real_harmonic_inverse(self.ctx, _lib.ptr(c), _lib.ptr(out)))
        return out

    def hankel(self, coeff, inverse=False):
        c = self._grid(coeff)
        out = np.empty_like(c)
        self._ck(self.lib.mtip2d_op_hankel(self.ctx, _lib.ptr(c), _lib.ptr(out), int(inverse)))
        return out

    def fourier_transform(self, grid, inverse=False):
        g = self._grid(grid)
        out = np.empty_like(g)
        self._ck(self.lib.mtip2d_op_fourier_transform(self.ctx, _lib.ptr(g), _lib.ptr(out), int(inverse)))
        return out

    def set_projection(self, projection_vectors, used_orders, radial_mask, number_of_particles=1.0):
        """projection_vectors (n_used, Nq): one per used order; used_orders {order: id} (ascending ids, order 0 included);
        radial_mask (n_orders, Nq) indexed by id as upstream"""
        ids = np.ascontiguousarray(list(used_orders.values()), dtype=np.int32)
        pm = _lib.as_c128(projection_vectors)
        assert pm.shape == (len(ids), self.N)
        rm = _lib.as_u8(np.asarray(radial_mask, dtype=bool)[ids])
        self._ck(self.lib.mtip2d_set_projection(self.ctx, len(ids), _lib.ptr(ids), _lib.ptr(pm), _lib.ptr(rm), _lib.ptr(_lib.as_f64(self.qs)),
                                                float(number_of_particles)))
        self.n_used = len(ids)

    def set_so_freedom(self, position):
        """SO_freedom (dimensions == 2): the unknown at this position among the used orders is 1 in every projection; None: off"""
        self._ck(self.lib.mtip2d_set_so_freedom(self.ctx, -1 if position is None else int(position)))

    def project(self, I):
        """approximate_unknowns + mtip_projection + number-of-particles rule: (projected coefficients, unknowns)"""
        c = self._grid(I, self.M + 1)
        out = np.empty_like(c)
        unk = np.empty((self.B, self.n_used), complex)
        self._ck(self.lib.mtip2d_op_project(self.ctx, _lib.ptr(c), _lib.ptr(out), _lib.ptr(unk)))
        return out, unk

    # ---- operators of the phasing loop
    def set_real_constraints(self, flags, lo, hi, imag_thr, hio_flags):
        self._ck(self.lib.mtip2d_set_real_constraints(self.ctx, int(flags), float(lo), float(hi), float(imag_thr), int(hio_flags)))

    def set_error_weights(self, weights):
        w = _lib.as_f64(weights)
        assert w.shape == (self.N, self.n_phi)
        self._ck(self.lib.mtip2d_set_error_weights(self.ctx, _lib.ptr(w)))

    def step(self, method, ft_stab, beta, rho, support, fixed_intensity=None, want_inputs=False):
        """one HIO / ER (or HIO_non_FXS / ER_non_FXS: `fixed_intensity` (B, Nq, n_phi)) step for the batch:
        (F_new, rho_new, errors (B,), unknowns (B, n_used) or None); with want_inputs also (F = FT(rho), I_m of |F|^2 or None),
        the arguments of the reciprocal error metrics"""
        r = self._grid(rho)
        sup = np.ascontiguousarray(np.broadcast_to(np.asarray(support, dtype=np.uint8), (self.B,) + self.shape))
        F_new, rho_new = np.empty_like(r), np.empty_like(r)
        err = np.empty(self.B)
        mid = {'HIO': 0, 'ER': 1, 'HIO_non_FXS': 2, 'ER_non_FXS': 3}[method]
        fxs = mid < 2
        unk = np.empty((self.B, self.n_used), complex) if fxs else None
        fixed = None
        if not fxs:
            fixed = np.ascontiguousarray(np.broadcast_to(np.asarray(fixed_intensity, dtype=np.float64), (self.B,) + self.shape))
        F_in = np.empty_like(r) if want_inputs else None
        I_in = np.empty((self.B, self.N, self.M + 1), complex) if (want_inputs and fxs) else None
        self._ck(self.lib.mtip2d_op_step_ex(self.ctx, mid, int(bool(ft_stab)), float(beta), _lib.ptr(r), _lib.ptr(sup), _lib.ptr(fixed),
                                            _lib.ptr(F_new), _lib.ptr(rho_new), _lib.ptr(err), _lib.ptr(unk), _lib.ptr(F_in), _lib.ptr(I_in)))
        if want_inputs:
            return F_new, rho_new, err, unk, F_in, I_in
        return F_new, rho_new, err, unk

    def shrinkwrap(self, rho, sigma, threshold):
        r = self._grid(rho)
        mask = np.empty((self.B,) + self.shape, np.uint8)
        self._ck(self.lib.mtip2d_op_shrinkwrap(self.ctx, _lib.ptr(r), float(sigma), float(threshold), _lib.ptr(mask)))
        return mask.astype(bool)

    # ---- the resident loop (mtip2d_set_density ... mtip2d_run, csrc/k_polar2d.hip): the names of the 3-D engine
    METHOD_ID = {'HIO': 0, 'ER': 1, 'HIO_non_FXS': 2, 'ER_non_FXS': 3}
    MAIN_TYPE = {'mean': 0, 'min': 1, 'max': 2, 'prod': 3}
    MAIN_ITEM = {'real': 0, 'deg2_invariant_l2_diff': 1, 'l2_projection_diff': 2}

    def set_density(self, batch, rho):
        r = _lib.as_c128(rho)
        assert r.shape == self.shape
        self._ck(self.lib.mtip2d_set_density(self.ctx, int(batch), _lib.ptr(r)))

    def set_initial_support(self, support):
        s = _lib.as_u8(np.asarray(support, dtype=bool))
        assert s.shape == self.shape
        self._ck(self.lib.mtip2d_set_initial_support(self.ctx, _lib.ptr(s)))

    def set_support(self, batch, support):
        s = _lib.as_u8(np.asarray(support, dtype=bool))
        assert s.shape == self.shape
        self._ck(self.lib.mtip2d_set_support(self.ctx, int(batch), _lib.ptr(s)))

    def init_state(self):
        """the state starts from IFT(FT(guess)) of the densities given to `set_density` (reconstruct.py:962-963)"""
        self._ck(self.lib.mtip2d_init_state(self.ctx))
        self.n_steps = 0

    def set_ft_stab_mask(self, mask):
        """ft_stab per restart for the runs that follow (bool per restart), None = every restart"""
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask, dtype=bool).astype(np.uint8))
        assert m is None or m.shape == (self.B,)
        self._ck(self.lib.mtip2d_set_ft_stab_mask(self.ctx, _lib.ptr(m)))
        self._ft_mask_set = m is not None

    def set_reciprocal_metrics(self, deg2_reference=None, deg2_norms=None, l2_weights=None):
        """deg2_invariant_l2_diff with its reference table (n_used, Nq, Nq) and norms (n_used), and / or the reciprocal
        l2_projection_diff with its weights (Nq, n_phi); nothing given: both off"""
        which = (1 if deg2_reference is not None else 0) | (2 if l2_weights is not None else 0)
        ref = None if deg2_reference is None else _lib.as_c128(deg2_reference)
        nrm = None if deg2_reference is None else _lib.as_f64(deg2_norms)
        w = None if l2_weights is None else _lib.as_f64(l2_weights)
        assert ref is None or (ref.shape == (self.n_used, self.N, self.N) and nrm.shape == (self.n_used,))
        assert w is None or w.shape == self.shape
        self._ck(self.lib.mtip2d_set_reciprocal_metrics(self.ctx, which, _lib.ptr(ref), _lib.ptr(nrm), _lib.ptr(w)))
        self.metrics = which

    def set_main_error(self, kind, items):
        """main error = kind ('mean', 'min', 'max', 'prod') over `items`: 'real', 'deg2_invariant_l2_diff', 'l2_projection_diff'"""
        it = np.ascontiguousarray([self.MAIN_ITEM[i] for i in items], dtype=np.int32)
        self._ck(self.lib.mtip2d_set_main_error(self.ctx, self.MAIN_TYPE[kind], len(it), _lib.ptr(it)))

    def run(self, method, ft_stab, betas, fetch=True):
        """n = len(betas) steps of `method` in one call; ft_stab: bool, or a bool per restart (read inside the step).  With fetch the
        real errors (n, B) of these steps come back, else nothing crosses the host"""
        betas = _lib.as_f64(np.atleast_1d(betas))
        n = len(betas)
        ft_stab = _lib.ft_stab_flag(self, ft_stab)
        mid = self.METHOD_ID[method]
        if not fetch:
            self._ck(self.lib.mtip2d_run_async(self.ctx, mid, int(bool(ft_stab)), n, _lib.ptr(betas)))
            self.n_steps += n
            return None
        err = np.empty((n, self.B))
        self._ck(self.lib.mtip2d_run(self.ctx, mid, int(bool(ft_stab)), n, _lib.ptr(betas), _lib.ptr(err)))
        self.n_steps += n
        return err

    def fetch_errors(self, first, n):
        err = np.empty((n, self.B))
        self._ck(self.lib.mtip2d_fetch_errors(self.ctx, first, n, _lib.ptr(err)))
        return err

    def fetch_main_errors(self, first, n):
        err = np.empty((n, self.B))
        self._ck(self.lib.mtip2d_fetch_main_errors(self.ctx, first, n, _lib.ptr(err)))
        return err

    def fetch_reciprocal_metrics(self, first, n):
        """{name: (n, B, n_used) or (n, B)} of the enabled reciprocal metrics"""
        which = getattr(self, 'metrics', 0)
        deg2 = np.empty((n, self.B, self.n_used)) if which & 1 else None
        l2 = np.empty((n, self.B)) if which & 2 else None
        self._ck(self.lib.mtip2d_fetch_reciprocal_metrics(self.ctx, first, n, _lib.ptr(deg2), _lib.ptr(l2)))
        out = {}
        if deg2 is not None:
            out['deg2_invariant_l2_diff'] = deg2
        if l2 is not None:
            out['l2_projection_diff'] = l2
        return out

    def shrinkwrap_state(self, sigma, threshold, error_limit):
        """shrink-wrap of the resident density; the enforce decision (last main error > error_limit) per restart comes back"""
        enforced = np.empty(self.B, np.uint8)
        self._ck(self.lib.mtip2d_shrinkwrap(self.ctx, float(sigma), float(threshold), float(error_limit), _lib.ptr(enforced)))
        return enforced.astype(bool)

    def begin_sub_loop(self):
        self._ck(self.lib.mtip2d_begin_sub_loop(self.ctx))

    def refresh_reciprocal_density(self):
        """'SW_center' tail (reconstruct.py:891-894), literally: the last pair becomes (reciprocal, real) = (rho, FT(rho))"""
        self._ck(self.lib.mtip2d_refresh_reciprocal_density(self.ctx))

    def select_best(self, where=None):
        if where is None:
            self._ck(self.lib.mtip2d_select_best(self.ctx))
        else:
            w = np.ascontiguousarray(np.asarray(where, dtype=bool).astype(np.uint8))
            assert w.shape == (self.B,)
            self._ck(self.lib.mtip2d_select_best_where(self.ctx, _lib.ptr(w)))

    def _get(self, fn, best, dtype):
        out = np.empty((self.B,) + self.shape, dtype)
        for b in range(self.B):
            self._ck(fn(self.ctx, b, int(bool(best)), _lib.ptr(out[b])))
        return out

    def density(self, best=False):
        return self._get(self.lib.mtip2d_get_density, best, complex)

    def reciprocal_density(self, best=False):
        return self._get(self.lib.mtip2d_get_reciprocal_density, best, complex)

    def support(self, best=False):
        return self._get(self.lib.mtip2d_get_support, best, np.uint8).astype(bool)

    def unknowns(self):
        out = np.empty((self.B, self.n_used), complex)
        for b in range(self.B):
            self._ck(self.lib.mtip2d_get_unknowns(self.ctx, b, _lib.ptr(out[b])))
        return out

    def best_error(self):
        err = np.empty(self.B)
        n = C.c_int64(0)
        self._ck(self.lib.mtip2d_get_best_error(self.ctx, _lib.ptr(err), C.byref(n)))
        return err, int(n.value)

    def synchronize(self):
        self._ck(self.lib.mtip2d_synchronize(self.ctx))

    # ---- grid arithmetic of the averaging worker on stacks (csrc/k_average2d.h): torch tensors on the engine's device (they own
    #      the memory, nothing else) or numpy arrays; stacks (n, Nq, n_phi) complex128 of any length
    @classmethod
    def _p(cls, x):
        """void* of a numpy array or of a tensor (after torch's stream has finished writing it: _lib.TensorOperands)"""
        if x is None:
            return None
        return _lib.ptr(x) if isinstance(x, np.ndarray) else cls._tp(x)

    def _stack(self, X):
        """a stack as the kernels read it: contiguous complex128 (n, Nq, n_phi), numpy or torch"""
        if isinstance(X, np.ndarray):
            X = _lib.as_c128(X)
        else:
            import torch
            assert X.dtype == torch.complex128
            X = X.contiguous()
        assert X.ndim == 3 and tuple(X.shape[1:]) == self.shape, (tuple(X.shape), self.shape)
        return X

    @staticmethod
    def _like(X, shape):
        if isinstance(X, np.ndarray):
            return np.empty(shape, complex)
        import torch
        return torch.empty(shape, dtype=torch.complex128, device=X.device)

    def _avg_setup(self):
        if getattr(self, '_avg_ready', False):
            return

        def trapz_w(x):                                          # PolarIntegrator.integrate (mathLibrary.py:1254-1262) as weights
            w = np.zeros(len(x))
            d = np.diff(x)
            w[:-1] += d / 2
            w[1:] += d / 2
            return w
        rs, qs = _lib.as_f64(self.rs), _lib.as_f64(self.qs)
        self.int_wr, self.int_wq, self.int_wphi = _lib.as_f64(trapz_w(rs) * rs), _lib.as_f64(trapz_w(qs) * qs), _lib.as_f64(trapz_w(self.phis))
        self._ck(self.lib.mtip2d_avg_set_grid(self.ctx, _lib.ptr(rs), _lib.ptr(qs), _lib.ptr(self.int_wr), _lib.ptr(self.int_wq),
                                              _lib.ptr(self.int_wphi)))
        self._avg_ready = True

    def _chunked(self, fn, X, inverse):
        """a batched transform of the C ABI over a stack of any length, in chunks of n_batch (a short last chunk is filled up with its
        last grid); a grid's transform does not depend on its neighbours in the chunk"""
        X = self._stack(X)
        n, out = X.shape[0], self._like(X, tuple(X.shape))
        for i in range(0, n, self.B):
            m = min(self.B, n - i)
            if m == self.B:
                self._ck(fn(self.ctx, self._p(X[i:i + m]), self._p(out[i:i + m]), int(inverse)))
                continue
            buf, res = self._like(X, (self.B,) + self.shape), self._like(X, (self.B,) + self.shape)
            buf[:m] = X[i:i + m]
            buf[m:] = X[n - 1]
            self._ck(fn(self.ctx, self._p(buf), self._p(res), int(inverse)))
            out[i:i + m] = res[:m]
        return out

    def t_fourier_transform(self, X, inverse=False):
        """mtip2d_op_fourier_transform of a stack of any length"""
        return self._chunked(self.lib.mtip2d_op_fourier_transform, X, inverse)

    def t_harmonic(self, X, inverse=False):
        """mtip2d_op_harmonic (complex circular harmonic transform, orders 0..M, -M..-1) of a stack of any length"""
        return self._chunked(self.lib.mtip2d_op_harmonic, X, inverse)

    def t_grid_stats(self, X):
        """(n, 9) host array per grid (mtip2d_avg_grid_stats): integral and first moments of Re, and the statistics of the entries > 0"""
        self._avg_setup()
        X = self._stack(X)
        out = np.zeros((X.shape[0], 9))
        self._ck(self.lib.mtip2d_avg_grid_stats(self.ctx, self._p(X), int(X.shape[0]), _lib.ptr(out)))
        return out

    def t_inversion_metric(self, F, F_ref):
        """(n, 2) host array: integrals of |Im F - Im F_ref| and |Im F - Im conj(F_ref)| (average.py:216-217)"""
        self._avg_setup()
        F, F_ref = self._stack(F), self._stack(F_ref[None])
        out = np.zeros((F.shape[0], 2))
        self._ck(self.lib.mtip2d_avg_inversion_metric(self.ctx, self._p(F), int(F.shape[0]), self._p(F_ref), _lib.ptr(out)))
        return out

    def t_phase_ramp(self, X, centers_cartesian, sign):
        """X[b] *= exp(-i sign k . c_b) IN PLACE (generate_shift_by_operator, fxs_Projections.py:1426-1434); returns X"""
        self._avg_setup()
        assert self._stack(X) is X, 'phase ramp works in place: a contiguous complex128 stack'
        cc = _lib.as_f64(centers_cartesian)
        assert cc.shape == (X.shape[0], 2)
        self._ck(self.lib.mtip2d_op_grid_phase_ramp(self.ctx, self._p(X), int(X.shape[0]), _lib.ptr(cc), float(sign)))
        return X

    def t_combine(self, op, A, scalars=None):
        """mtip2d_op_grid_combine on a stack: 'conj', 'div' (complex divisor per grid) -> a stack; 'mean', 'abs2mean' (sum over the
        stack in its order, divided by scalars[0]) -> one grid; 'affine' ((a - s0) / s1, real scalars) -> a stack"""
        code = {'conj': 0, 'div': 1, 'mean': 2, 'abs2mean': 3, 'affine': 4}[op]
        A = self._stack(A)
        out = self._like(A, self.shape if code in (2, 3) else tuple(A.shape))
        sc = None if scalars is None else _lib.as_c128(np.atleast_1d(scalars))
        assert code == 0 or sc.shape == ((A.shape[0],) if code == 1 else ((2,) if code == 4 else (1,)))
        self._ck(self.lib.mtip2d_op_grid_combine(self.ctx, code, self._p(out), self._p(A), int(A.shape[0]), _lib.ptr(sc)))
        return out

    def t_curves(self, a_d, a_ft, I_d, I_ft):
        """mtip2d_avg_curves: (prtf_mean (4, Nq) complex, prtf_std (4, Nq), fsc (Nq)) on the host"""
        args = [self._stack(x[None]) for x in (a_d, a_ft, I_d, I_ft)]
        mean, std, fsc = np.zeros((4, self.N), complex), np.zeros((4, self.N)), np.zeros(self.N)
        self._ck(self.lib.mtip2d_avg_curves(self.ctx, *[self._p(x) for x in args], _lib.ptr(mean), _lib.ptr(std), _lib.ptr(fsc)))
        return mean, std, fsc

    def _fqcb_arg(self, x):
        """(array, kind, n_orders, ld) of an FQCB input: a coefficient table (Nq, ld) -- a tuple (table, n_orders) reads only its first
        n_orders columns -- or a B_n stack (n_orders, Nq, Nq)"""
        n = None
        if isinstance(x, tuple):
            x, n = x
        if isinstance(x, np.ndarray):
            x = _lib.as_c128(x)
        else:
            x = x.contiguous()
        if x.ndim == 2:
            assert x.shape[0] == self.N and (n is None or n <= x.shape[1])
            return x, 0, int(x.shape[1] if n is None else n), int(x.shape[1])
        assert x.ndim == 3 and tuple(x.shape[1:]) == (self.N, self.N) and n is None
        return x, 1, int(x.shape[0]), 0

    def t_fqcb(self, b1, b2, skip_odd_orders=False, include_zero_order=False):
        """FQCB_2D (resolution_metrics.py:146-187) on the device: (mean, std) over q' <= q, (Nq,) each, on the host"""
        x1, k1, n1, ld1 = self._fqcb_arg(b1)
        x2, k2, n2, ld2 = self._fqcb_arg(b2)
        o_start, o_step = (2, 2) if skip_odd_orders else (1, 1)
        if include_zero_order:
            o_start = 0
        mean, std = np.zeros(self.N), np.zeros(self.N)
        self._ck(self.lib.mtip2d_avg_fqcb(self.ctx, self._p(x1), k1, n1, ld1, self._p(x2), k2, n2, ld2, o_start, o_step, _lib.ptr(mean), _lib.ptr(std)))
        return mean, std

    def t_deg2_from_table(self, table, n_orders=None):
        """B_n(q, q') = I_n(q) conj(I_n(q')) (fxs_invariant_tools.py:906-914) of the first n_orders columns of a table (Nq, ld):
        (n_orders, Nq, Nq), where the table lives"""
        x, _, n, ld = self._fqcb_arg(table if n_orders is None else (table, n_orders))
        out = self._like(x, (n, self.N, self.N))
        self._ck(self.lib.mtip2d_op_deg2_from_table(self.ctx, self._p(x), n, ld, self._p(out)))
        return out

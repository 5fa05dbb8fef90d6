"""ctypes binding of libmtip_hip.so (include/mtip_hip.h).

There is deliberately NO CPU fallback: if the HIP library is missing or no MI355X is visible the
import of the engine fails loudly (the reference would silently drop to its numpy path,
``xframe/projects/fxs/reconstruct.py:96-107``; a silent fallback here would void every parity claim).
"""
import ctypes as C
import os

import numpy as np

# HIP maps streams onto 4 hardware queues by default (one is the null stream's): with up to 3 engines per GPU give every
# engine its own queue.  Only effective if set before the HIP runtime initialises; harmless otherwise.
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(os.path.dirname(_HERE), 'csrc', 'libmtip_hip.so')

c_double_p = C.POINTER(C.c_double)
c_u8_p = C.POINTER(C.c_uint8)
c_void = C.c_void_p


class MtipCfg(C.Structure):
    _fields_ = [('n_radial', C.c_int32), ('l_max', C.c_int32), ('n_theta', C.c_int32), ('n_phi', C.c_int32),
                ('n_batch', C.c_int32), ('hankel_trapz', C.c_int32), ('fused', C.c_int32), ('reserved', C.c_int32)]


MTIP_CORRELATE_GENERAL_NPHI = 1   # mtip_correlate_create_ex flags bit 0: every even 5-smooth n_phi in 16 .. 2048
MTIP_CORRELATE_ANY_NPHI = 4       # bit 2: every even n_phi in 16 .. 2048 (chirp-z transforms where n_phi has a prime factor above 5)
MTIP_CFG_LOOP_BIG_L = 1          # MtipCfg.reserved bit 0 (include/mtip_hip.h): the phasing loop and the projection beyond L = 63


class MtipCorrelateCfg(C.Structure):
    _fields_ = [('n_q', C.c_int32), ('n_phi', C.c_int32), ('n_q1', C.c_int32), ('n_q2', C.c_int32), ('filter_kind', C.c_int32),
                ('roi_lo', C.c_int32), ('roi_hi', C.c_int32), ('roi_filter', C.c_int32), ('roi_normalize', C.c_int32),
                ('shared_mask', C.c_int32), ('filter_k', C.c_double), ('roi_min', C.c_double), ('roi_max', C.c_double)]


class MtipResampleCfg(C.Structure):
    _fields_ = [('H', C.c_int32), ('W', C.c_int32), ('order', C.c_int32), ('threshold_on', C.c_int32), ('has_binary_mask', C.c_int32),
                ('has_background', C.c_int32), ('n_points', C.c_int64), ('threshold_lo', C.c_double), ('threshold_hi', C.c_double)]


class MtipError(RuntimeError):
    pass


_SIGNATURES = {
    'mtip_device_count': (C.c_int, []),
    'mtip_create': (c_void, [C.POINTER(MtipCfg), C.c_int]),
    'mtip_destroy': (None, [c_void]),
    'mtip_last_error': (C.c_char_p, [c_void]),
    'mtip_get_cfg': (C.c_int, [c_void, C.POINTER(MtipCfg)]),
    'mtip_synchronize': (C.c_int, [c_void]),
    'mtip_set_angular_grid': (C.c_int, [c_void, c_void, c_void]),
    'mtip_set_radial_grid': (C.c_int, [c_void, c_void, c_void]),
    'mtip_set_hankel_weights': (C.c_int, [c_void, c_void, C.c_double, C.c_double]),
    'mtip_set_projection_matrix': (C.c_int, [c_void, C.c_int, c_void, C.c_int, c_void, C.c_int]),
    'mtip_set_number_of_particles': (C.c_int, [c_void, C.c_double]),
    'mtip_set_so_freedom': (C.c_int, [c_void, C.c_int]),
    'mtip_set_invariant_metrics': (C.c_int, [c_void, C.c_uint32, c_void, c_void, c_void, c_void, c_void, C.c_double, c_void, c_void, c_void]),
    'mtip_fetch_invariant_metrics': (C.c_int, [c_void, C.c_int64, C.c_int64, c_void, c_void, c_void]),
    'mtip_set_reciprocal_l2_metric': (C.c_int, [c_void, c_void, c_void]),
    'mtip_fetch_reciprocal_l2_metric': (C.c_int, [c_void, C.c_int64, C.c_int64, c_void]),
    'mtip_op_invariant_metrics': (C.c_int, [c_void, c_void, c_void, c_void, c_void]),
    'mtip_set_deg2_metric': (C.c_int, [c_void, C.c_int]),
    'mtip_set_main_error': (C.c_int, [c_void, C.c_int, C.c_int]),
    'mtip_set_main_error_ex': (C.c_int, [c_void, C.c_int, C.c_int, c_void, C.c_int]),
    'mtip_set_real_constraints': (C.c_int, [c_void, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_uint32]),
    'mtip_set_initial_support': (C.c_int, [c_void, c_void]),
    'mtip_set_error_weights': (C.c_int, [c_void, c_void, c_void, C.c_int]),
    'mtip_set_density': (C.c_int, [c_void, C.c_int, c_void]),
    'mtip_init_state': (C.c_int, [c_void]),
    'mtip_get_density': (C.c_int, [c_void, C.c_int, C.c_int, c_void]),
    'mtip_get_reciprocal_density': (C.c_int, [c_void, C.c_int, C.c_int, c_void]),
    'mtip_get_support': (C.c_int, [c_void, C.c_int, C.c_int, c_void]),
    'mtip_set_support': (C.c_int, [c_void, C.c_int, c_void, C.c_int]),
    'mtip_get_unknowns': (C.c_int, [c_void, C.c_int, C.c_int, c_void]),
    'mtip_get_best_error': (C.c_int, [c_void, c_void, C.POINTER(C.c_int64)]),
    'mtip_select_best': (C.c_int, [c_void]),
    'mtip_select_best_where': (C.c_int, [c_void, c_void]),
    'mtip_run': (C.c_int, [c_void, C.c_int, C.c_int, C.c_int, c_void, c_void, c_void]),
    'mtip_run_async': (C.c_int, [c_void, C.c_int, C.c_int, C.c_int, c_void]),
    'mtip_set_ft_stab_mask': (C.c_int, [c_void, c_void]),
    'mtip_run_group_async': (C.c_int, [c_void, C.c_int, C.c_int, C.c_int, C.c_int, c_void]),
    'mtip_fetch_errors': (C.c_int, [c_void, C.c_int64, C.c_int64, c_void, c_void]),
    'mtip_fetch_main_errors': (C.c_int, [c_void, C.c_int64, C.c_int64, c_void]),
    'mtip_shrinkwrap': (C.c_int, [c_void, C.c_double, C.c_double, C.c_double, c_void]),
    'mtip_begin_sub_loop': (C.c_int, [c_void]),
    'mtip_refresh_reciprocal_density': (C.c_int, [c_void]),
    'mtip_last_deg2_invariant': (C.c_int, [c_void, C.c_int, c_void]),
    'mtip_op_sht_forward': (C.c_int, [c_void, c_void, c_void, C.c_int]),
    'mtip_op_sht_inverse': (C.c_int, [c_void, c_void, c_void]),
    'mtip_op_sht_inverse_forward': (C.c_int, [c_void, c_void, c_void, c_void, C.c_int]),
    'mtip_op_hankel': (C.c_int, [c_void, c_void, c_void, C.c_int]),
    'mtip_op_hankel_difference': (C.c_int, [c_void, c_void, c_void, c_void, C.c_int, c_void]),
    'mtip_op_fourier_transform': (C.c_int, [c_void, c_void, c_void, C.c_int]),
    'mtip_op_project_coefficients': (C.c_int, [c_void, c_void, c_void]),
    'mtip_op_project_real_intensity': (C.c_int, [c_void, c_void, c_void]),
    'mtip_op_apply_unknowns': (C.c_int, [c_void, c_void, c_void, c_void]),
    'mtip_op_modulus_replacement': (C.c_int, [c_void, c_void, c_void, c_void]),
    'mtip_op_real_space_update': (C.c_int, [c_void, c_void, c_void, C.c_int, C.c_double, c_void, c_void]),
    'mtip_op_deg2_invariants': (C.c_int, [c_void, c_void, c_void]),
    'mtip_op_apply_matrix': (C.c_int, [c_void, c_void, c_void, c_void, C.c_int, C.c_int, C.c_int]),
    'mtip_op_grid_stats': (C.c_int, [c_void, c_void, C.c_int, c_void, c_void, c_void, c_void]),
    'mtip_op_grid_phase_ramp': (C.c_int, [c_void, c_void, C.c_int, c_void, C.c_double]),
    'mtip_op_grid_combine': (C.c_int, [c_void, C.c_int, c_void, c_void, C.c_int, c_void]),
    'mtip_op_prtf': (C.c_int, [c_void, c_void, c_void, c_void, c_void, c_void, c_void]),
    'mtip_op_fsc': (C.c_int, [c_void, c_void, c_void, c_void]),
    'mtip_set_so3_tables': (C.c_int, [c_void, C.c_int, c_void]),
    'mtip_op_so3_correlation': (C.c_int, [c_void, c_void, c_void, C.c_int, C.c_int, c_void]),
    'mtip_op_rotate_coefficients': (C.c_int, [c_void, c_void, c_void, c_void]),
    'mtip2d_create': (c_void, [C.c_int, C.c_int, C.c_int, C.c_int]),
    'mtip2d_destroy': (None, [c_void]),
    'mtip2d_last_error': (C.c_char_p, [c_void]),
    'mtip2d_set_hankel_weights': (C.c_int, [c_void, c_void, c_void, c_void]),
    'mtip2d_set_projection': (C.c_int, [c_void, C.c_int, c_void, c_void, c_void, c_void, C.c_double]),
    'mtip2d_op_harmonic': (C.c_int, [c_void, c_void, c_void, C.c_int]),
    'mtip2d_op_real_harmonic_forward': (C.c_int, [c_void, c_void, c_void]),
    'mtip2d_op_real_harmonic_inverse': (C.c_int, [c_void, c_void, c_void]),
    'mtip2d_op_hankel': (C.c_int, [c_void, c_void, c_void, C.c_int]),
    'mtip2d_op_fourier_transform': (C.c_int, [c_void, c_void, c_void, C.c_int]),
    'mtip2d_op_project': (C.c_int, [c_void, c_void, c_void, c_void]),
    'mtip2d_set_real_constraints': (C.c_int, [c_void, C.c_uint32, C.c_double, C.c_double, C.c_double, C.c_uint32]),
    'mtip2d_set_error_weights': (C.c_int, [c_void, c_void]),
    'mtip2d_set_so_freedom': (C.c_int, [c_void, C.c_int]),
    'mtip2d_op_step': (C.c_int, [c_void, C.c_int, C.c_int, C.c_double, c_void, c_void, c_void, c_void, c_void, c_void]),
    'mtip2d_op_step_ex': (C.c_int, [c_void, C.c_int, C.c_int, C.c_double, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void]),
    'mtip2d_op_shrinkwrap': (C.c_int, [c_void, c_void, C.c_double, C.c_double, c_void]),
    'mtip2d_set_density': (C.c_int, [c_void, C.c_int, c_void]),
    'mtip2d_set_initial_support': (C.c_int, [c_void, c_void]),
    'mtip2d_set_support': (C.c_int, [c_void, C.c_int, c_void]),
    'mtip2d_init_state': (C.c_int, [c_void]),
    'mtip2d_set_ft_stab_mask': (C.c_int, [c_void, c_void]),
    'mtip2d_set_reciprocal_metrics': (C.c_int, [c_void, C.c_uint32, c_void, c_void, c_void]),
    'mtip2d_set_main_error': (C.c_int, [c_void, C.c_int, C.c_int, c_void]),
    'mtip2d_run': (C.c_int, [c_void, C.c_int, C.c_int, C.c_int, c_void, c_void]),
    'mtip2d_run_async': (C.c_int, [c_void, C.c_int, C.c_int, C.c_int, c_void]),
    'mtip2d_fetch_errors': (C.c_int, [c_void, C.c_int64, C.c_int64, c_void]),
    'mtip2d_fetch_main_errors': (C.c_int, [c_void, C.c_int64, C.c_int64, c_void]),
    'mtip2d_fetch_reciprocal_metrics': (C.c_int, [c_void, C.c_int64, C.c_int64, c_void, c_void]),
    'mtip2d_shrinkwrap': (C.c_int, [c_void, C.c_double, C.c_double, C.c_double, c_void]),
    'mtip2d_refresh_reciprocal_density': (C.c_int, [c_void]),
    'mtip2d_begin_sub_loop': (C.c_int, [c_void]),
    'mtip2d_select_best': (C.c_int, [c_void]),
    'mtip2d_select_best_where': (C.c_int, [c_void, c_void]),
    'mtip2d_get_density': (C.c_int, [c_void, C.c_int, C.c_int, c_void]),
    'mtip2d_get_reciprocal_density': (C.c_int, [c_void, C.c_int, C.c_int, c_void]),
    'mtip2d_get_support': (C.c_int, [c_void, C.c_int, C.c_int, c_void]),
    'mtip2d_get_unknowns': (C.c_int, [c_void, C.c_int, c_void]),
    'mtip2d_get_best_error': (C.c_int, [c_void, c_void, C.POINTER(C.c_int64)]),
    'mtip2d_synchronize': (C.c_int, [c_void]),
    'mtip2d_avg_set_grid': (C.c_int, [c_void, c_void, c_void, c_void, c_void, c_void]),
    'mtip2d_avg_grid_stats': (C.c_int, [c_void, c_void, C.c_int, c_void]),
    'mtip2d_avg_inversion_metric': (C.c_int, [c_void, c_void, C.c_int, c_void, c_void]),
    'mtip2d_op_grid_phase_ramp': (C.c_int, [c_void, c_void, C.c_int, c_void, C.c_double]),
    'mtip2d_op_grid_combine': (C.c_int, [c_void, C.c_int, c_void, c_void, C.c_int, c_void]),
    'mtip2d_avg_curves': (C.c_int, [c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void]),
    'mtip2d_avg_fqcb': (C.c_int, [c_void, c_void, C.c_int, C.c_int, C.c_int, c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_void, c_void]),
    'mtip2d_op_deg2_from_table': (C.c_int, [c_void, c_void, C.c_int, C.c_int, c_void]),
    'mtip_op_so3_find_rotation': (C.c_int, [c_void, c_void, c_void, C.c_int, C.c_int, c_void, c_void, c_void]),
    'mtip_op_rotate_coefficients_grid': (C.c_int, [c_void, c_void, c_void, c_void, c_void, c_void]),
    'mtip_op_hermitian_eig': (C.c_int, [c_void, C.c_int, C.c_int, c_void, c_void, c_void]),
    'mtip_op_symmetric_eig': (C.c_int, [c_void, C.c_int, C.c_int, c_void, c_void, c_void]),
    'mtip_op_cc_to_deg2': (C.c_int, [c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, c_void, c_void, c_void, c_void, c_void]),
    'mtip_op_cc_to_deg2_wide': (C.c_int, [c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, c_void, c_void, c_void, c_void, c_void]),
    'mtip_op_cc_prepare_masked': (C.c_int, [c_void, C.c_int, C.c_int, C.c_uint32, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void]),
    'mtip_op_cc_lstsq_deg2': (C.c_int, [c_void, C.c_int, C.c_int, C.c_int, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void]),
    'mtip_op_cc_lstsq_deg2_minnorm': (C.c_int, [c_void, C.c_int, C.c_int, C.c_int, c_void, c_void, c_void, c_void, c_void, c_void, c_void, c_void,
                                                 c_void]),
    'mtip_op_cc_lowpass_q': (C.c_int, [c_void, C.c_int, C.c_int, c_void, c_void, c_void, c_void]),
    'mtip_op_cc_harmonic_filter': (C.c_int, [c_void, C.c_int, C.c_int, C.c_int, C.c_int, c_void, c_void, c_void]),
    'mtip_op_cc_binned_mean': (C.c_int, [c_void, C.c_int, C.c_int, C.c_int, c_void, C.c_int, c_void, c_void, c_void, c_void, c_void]),
    'mtip_op_nearest_psd': (C.c_int, [c_void, C.c_int, C.c_int, c_void, c_void, c_void]),
    'mtip_op_cm_backsub': (C.c_int, [c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, c_void, c_void, c_void, c_void, c_void]),
    'mtip_op_deg2_to_cc': (C.c_int, [c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_void, c_void, c_void, c_void, c_void]),
    'mtip_correlate_create': (c_void, [c_void, C.POINTER(MtipCorrelateCfg), c_void, c_void, c_void]),
    'mtip_correlate_create_ex': (c_void, [c_void, C.POINTER(MtipCorrelateCfg), c_void, c_void, c_void, C.c_uint32]),
    'mtip_correlate_destroy': (None, [c_void]),
    'mtip_correlate_add': (C.c_int, [c_void, C.c_int, c_void, c_void]),
    'mtip_correlate_num_patterns': (C.c_int, [c_void]),
    'mtip_correlate_get_partial': (C.c_int, [c_void, c_void, c_void, c_void, c_void]),
    'mtip_correlate_merge': (C.c_int, [c_void, c_void, c_void, C.c_int, c_void, c_void]),
    'mtip_correlate_finalize': (C.c_int, [c_void, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_void, c_void]),
    'mtip_op_ring_median_mad': (C.c_int, [c_void, C.c_int, C.c_int, c_void, c_void, C.c_double, c_void, c_void, c_void]),
    'mtip_resample_create': (c_void, [c_void, C.POINTER(MtipResampleCfg), c_void, c_void, c_void, c_void]),
    'mtip_resample_destroy': (None, [c_void]),
    'mtip_resample_run': (C.c_int, [c_void, C.c_int, c_void, C.c_int, c_void, c_void, c_void, C.POINTER(C.c_int64)]),
    'mtip_correlate_add_detector': (C.c_int, [c_void, c_void, C.c_int, c_void, C.c_int, c_void, C.POINTER(C.c_int64)]),
    'mtip_profile': (C.c_int, [c_void, C.c_int]),
    'mtip_profile_get': (C.c_int, [c_void, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'mtip_profile_reset': (C.c_int, [c_void]),
    'mtip_debug_jacobi_sweeps': (C.c_int, [c_void, c_void]),
    'mtip_debug_projection_slots': (C.c_int, [c_void]),
    'mtip_debug_sht_plan': (C.c_int, [c_void, c_void]),
    'mtip_debug_hankel_tiles': (C.c_int, [c_void, c_void, c_void, c_void]),
    'mtip_debug_chain_timing': (C.c_int, [c_void, c_void]),
    'mtip_debug_check_jacobi_schedule': (C.c_int, [c_void, C.c_int]),
    'mtip_debug_polar_timing': (C.c_int, [c_void, c_void]),
    'mtip_debug_spin': (C.c_int, [c_void, C.c_double]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)
_libs = {}


def load(path=None):
    """Open the HIP library and declare every prototype of include/mtip_hip.h."""
    path = os.path.abspath(path or DEFAULT_LIB)
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise MtipError(f'{path} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                        '(hipcc --offload-arch=gfx950). There is no CPU fallback.')
    # One HIP runtime per process: the torch wheel bundles its own libamdhip64.so.7 (+ libhsa-runtime64) and /opt/rocm holds
    # another with the same soname.  Whichever is loaded first serves both; with this library first, torch's later import mixes
    # its bundled HSA runtime with /opt/rocm's HIP and finds "No HIP GPUs", and device memory of one runtime is unknown to the
    # other.  The averaging hands torch device tensors to the operators, so torch goes first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError = ABI mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    _libs[path] = lib
    return lib


def ptr(a):
    """void* of a C-contiguous numpy array (or None)."""
    if a is None:
        return None
    assert a.flags['C_CONTIGUOUS']
    return a.ctypes.data_as(c_void)


def as_c128(a):
    return np.ascontiguousarray(a, dtype=np.complex128)


def as_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def as_u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def ft_stab_flag(engine, ft_stab):
    """the `ft_stab` of an engine's `run` (a bool, or a bool per restart) as the flag of the C call: restarts that disagree go to the
    context as a mask (`engine.set_ft_stab_mask`) under the flag True; a mask left from an earlier run is cleared"""
    if isinstance(ft_stab, np.ndarray):
        flags = np.asarray(ft_stab, dtype=bool).reshape(engine.B)
        if flags.any() and not flags.all():
            engine.set_ft_stab_mask(flags)
            return True
        ft_stab = bool(flags.all())
    if getattr(engine, '_ft_mask_set', False):
        engine.set_ft_stab_mask(None)                                # a plain flag again: every restart
    return ft_stab


class TensorOperands:
    """What the engines share for operators that work in place on torch tensors (the averaging keeps its batch in HBM and hands
    ``tensor.data_ptr()`` across the ABI).  Needs ``self.lib`` and ``self.device_index``.

    Ordering rule: a context's stream is created non-blocking, so nothing orders it against the stream torch writes the tensors on
    (stack, cat, clone, index assignment ... right before an operator call).  Every operator call therefore first waits for torch's
    current stream of the tensor's device (``_tp``); in the other direction every ``mtip*_op_*`` / ``mtip2d_avg_*`` entry point
    returns after it has synchronised its own stream, so torch never reads a half-written result."""

    @property
    def emulated(self):
        return hasattr(self.lib, 'mtip_emulated')               # the CPU emulation of tests/emul: its device memory is host memory

    def torch_device(self):
        import torch
        return torch.device('cpu') if self.emulated else torch.device('cuda', self.device_index)

    @staticmethod
    def _tp(t):
        assert t.is_contiguous()
        if t.is_cuda:
            import torch
            torch.cuda.current_stream(t.device).synchronize()
        return C.c_void_p(t.data_ptr())

"""Resolved settings tree of the ``fxs reconstruct`` worker.

Key names are the reference's (``xframe/projects/fxs/settings/reconstruct/default_0.01.yaml:1-321``); the
reference's YAML defaults DSL (``_value`` / ``_if`` / ``command:`` eval, ``xframe/database/database.py:495-697``)
is not re-implemented: callers pass plain nested dicts that are merged over :func:`default_settings`.
"""
import copy

import numpy as np


class DictNamespace(dict):
    """dict with attribute access (``xframe/library/pythonLibrary.py:911-976`` look-alike)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v

    def dict(self):
        return to_plain(self)

    @classmethod
    def dict_to_dictnamespace(cls, d):
        return to_namespace(d)


def to_namespace(d):
    if isinstance(d, dict):
        return DictNamespace({k: to_namespace(v) for k, v in d.items()})
    return d


def to_plain(d):
    if isinstance(d, dict):
        return {k: to_plain(v) for k, v in d.items()}
    return d


def deep_update(base, upd):
    out = copy.deepcopy(base)
    for k, v in upd.items():
        if isinstance(v, dict) and isinstance(out.get(k), dict):
            out[k] = deep_update(out[k], v)
        else:
            out[k] = copy.deepcopy(v)
    return out


def default_settings():
    return {
        'dimensions': 3,
        'structure_name': 'default_structure',
        'particle_radius': 150,
        'grid': {'max_q': False, 'max_order': 63, 'n_phi': 0, 'n_theta': 0, 'n_radial_points': 128},
        'fourier_transform': {'type': 'midpoint', 'reciprocity_coefficient': 2.0,
                              'allow_weight_calculation': True, 'allow_weight_saving': True},
        'density_guess': {'type': 'bump', 'bump': {'slope': 0.3}, 'radius': 150,
                          'amplitude_function': 'random', 'random': {'SNR': 2}},
        'projections': {
            'real': {
                'projections': {
                    'apply': ['support', 'value_threshold', 'assert_real'],
                    'value_threshold': {'threshold': [0, False]},
                    'limit_imag': {'threshold': 2},
                    'support': {'initial_support': {'type': 'max_radius', 'max_radius': 150,
                                                    'auto_correlation': {'threshold': 0.01}},
                                'enforce_initial_support': {'apply': True, 'if_error_bigger_than': 6e-3}},
                },
                'shrink_wrap': {'sigmas': [[False, [False, False], False], [False, [False, False], False]],
                                'thresholds': [[0.08, [0, 0], 0], [0.08, [0, 0], 0]]},
                'HIO': {'beta': [[0.5, 0.4, -1 / 700, 1600], [0.01, 0.002, -1 / 200, 200]],
                        'considered_projections': ['all']},
            },
            'reciprocal': {
                'number_of_particles': {'initial': 1.0, 'estimate': False},
                'regrid': {'interpolation': 'cubic'},
                'used_order_ids': np.arange(64),
                'odd_orders_to_0': True,
                'use_averaged_intensity': True,
                'q_mask': {'type': 'none'},
                'SO_freedom': {'use': False},
            },
        },
        'output_density_modifiers': {'shift_to_center': False},
        'main_loop': {
            'error': {'methods': {
                'real': {'calculate': ['l2_projection_diff'],
                         'l2_projection_diff': {'inside_initial_support': True}},
                'reciprocal': {'calculate': [], 'deg2_invariant_l2_diff': {'order': 2}},
                'main': {'metrics': {'real': ['l2_projection_diff'], 'reciprocal': []}, 'type': 'mean'}}},
            'sub_loops': {
                'order': ['main', 'refinement'],
                'main': {'methods': {'HIO': {'iterations': 60, 'ft_stab': True},
                                     'ER': {'iterations': 40, 'ft_stab': True}, 'SW': 1},
                         'order': ['HIO', 'SW', 'ER'], 'iterations': 5,
                         'best_density_not_in_first_n_iterations': np.inf},
                'refinement': {'methods': {'ER': {'iterations': 100, 'ft_stab': True}, 'SW': 1},
                               'order': ['SW', 'ER'], 'iterations': 2,
                               'best_density_not_in_first_n_iterations': np.inf},
            },
        },
        # resident_2d (this project's key): dimensions == 2 on the resident engine (mtip2d_run) instead of one operator call per step
        # big_l_loop (this project's key): the 3-D phasing loop and the projection for 64 <= max_order <= 128 (Engine, MTIP_CFG_LOOP_BIG_L)
        'GPU': {'use': True, 'n_gpu_workers': 1, 'resident_2d': False, 'big_l_loop': False},
        'multi_process': {'use': True, 'n_parallel_reconstructions': 1},
        'profiling': {'enable': False, 'reconstruction_process_id': 1, 'gpu_worker_id': -1},
        # xframe/settings/general.py:25-27 (decides which variant of the real error metric the reference uses)
        'general': {'cache_aware': True, 'L2_cache': 512},
    }


def correlate_default_settings():
    """the keys of the ``fxs correlate`` worker that the device route reads, with the reference's defaults
    (``xframe/projects/fxs/settings/correlate/default_0.01.yaml``).  The Cartesian stage is part of it: intensity_pixel_threshold
    [on, lo, hi] masks pixels of the raw frame outside lo .. hi, use_binary_mask / subtract_background switch on the arrays handed to
    ``Resampler``, interpolation_order (0 .. 5) is the spline order of the polar resampling.  File lists and process splitting stay
    with the caller (``read_raw_images`` reads the frames).  GPU.general_n_phi (this project's key): ``Correlator`` takes every even
    n_phi in 16 .. 2048 with prime factors 2, 3, 5 -- the default's 1536 among them -- instead of the powers of two up to 1024.
    GPU.any_n_phi (this project's key): ``Correlator`` takes every even n_phi in 16 .. 2048, the ring pixel counts of phi_range's
    'max' and 'min' modes among them.  GPU.median_mad (this project's key): ``Correlator`` takes intensity_radial_pixel_filter
    [True, ['median_mad', k]]."""
    return {
        'GPU': {'general_n_phi': False, 'any_n_phi': False, 'median_mad': False},
        'intensity_pixel_threshold': [False, 4.0, 1e4],
        'use_binary_mask': False,
        'subtract_background': False,
        'interpolation_order': 2,
        'compute': ['is_good', 'waxs_aver', 'ccf_q1q2'],
        'intensity_radial_pixel_filter': [False, ['average_sigma', 3]],
        'ROI_normalization': [False, 0.3, 0.9],
        'ROI_mean_filter': [False, 1e2, 1e4],
        'polarization_correction': [False, 'h'],
        'solid_angle_correction': False,
        'qrange': False,
        'qrange_xcca': False,
        'phi_range': (0.0, 2 * np.pi, 1536, 'exact'),
        'fc_n_max': 15,
        'ccf_2p_symmetrize': False,
        'image_dimensions': [512, 512],
        'pixel_size': 200.0,
        'sample_distance': 620.0,
        'wavelength': 1.23984,
        'detector_origin': [255.2, 255.5],
    }


def resolve_correlate(overrides=None):
    o = correlate_default_settings()
    if overrides:
        o = deep_update(o, to_plain(overrides))
    return o


def simulate_ccd_default_settings():
    """the keys of the ``fxs simulate_ccd`` worker that the device route reads, with the reference's defaults
    (``xframe/projects/fxs/settings/simulate_ccd/default_0.01.yaml``; its `command:` entries evaluated).  n_particles is read by the
    reference (simulate_ccd.py:208) and never used; file names and the vtk switches stay with the caller."""
    return {
        'dimensions': 3,
        'structure_name': 'default',
        'grid': {'max_q': False, 'oversampling': 8, 'max_order': 63, 'n_phi': 0, 'n_theta': 0, 'n_radial_points': 256},
        'fourier_transform': {'type': 'midpoint', 'reciprocity_coefficient': 1, 'allow_weight_calculation': True,
                              'allow_weight_saving': True},
        'shapes': {'types': ['sphere'] * 6,
                   'centers': [(0, 0, 0)] + [(140.0, np.pi / 2, phi * 2 * np.pi / 5) for phi in range(5)],
                   'sizes': [70] * 6,
                   'densities': [25, 50, 25, 50, 25, 50],
                   'random_orientation': [False] * 6},
        'n_particles': 1,
        'cross_correlation': {'method': 'back_substitution', 'xray_wavelength': 1.23984},
        'GPU': {'use': True, 'n_gpu_workers': 1},
        'n_processes': True,
    }


def resolve_simulate_ccd(overrides=None):
    o = simulate_ccd_default_settings()
    if overrides:
        o = deep_update(o, to_plain(overrides))
    return o


def resolve(overrides=None):
    o = default_settings()
    if overrides:
        o = deep_update(o, to_plain(overrides))
    return o


def reciprocity_coefficient(ft_opt):
    """``misk.py:387-394`` / ``mathLibrary.py:1178-1182``."""
    pi_in_q = ft_opt.get('pi_in_q', None)
    if isinstance(pi_in_q, bool):
        return np.pi if pi_in_q else 1 / 2
    return ft_opt.get('reciprocity_coefficient', np.pi)

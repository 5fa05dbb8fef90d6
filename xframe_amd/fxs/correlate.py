"""``fxs correlate`` from detector frames on: frames -> polar patterns -> averaged two-point cross-correlation C(q1, q2, Delta).

Reference: ``xframe/projects/fxs/correlate.py`` (``process_image`` 377-452, accumulation 347-355, normalisation and result dict
249-295, ``_analyse_dependencies`` 478-484, ``_prepare_polar_representation`` 489-559, correction tables 565-591,
``_read_binary_2D_arr`` 606-620) and ``projectLibrary/cross_correlation.py`` (``ccf_analysis``).  The arithmetic runs in the kernels
of ``csrc/k_resample.h`` and ``csrc/k_correlate.h``; this file is settings bookkeeping, the host-side tables and the result dict.

The boundary is the detector frame: ``read_raw_images`` reads the files, ``Correlator.add_detector`` takes frames (P, H, W) and
optional initial masks through ``Resampler`` (``intensity_pixel_threshold``, binary mask, background, ``image *= mask`` and the
two ``map_coordinates`` calls of lines 382-398 on the ``cart_x`` / ``cart_y`` of :func:`polar_geometry`) into the accumulation
without the polar arrays leaving the device.  ``Correlator.add`` still takes what ``process_image`` holds at line 398: images
(P, n_q, n_phi) float and masks (P, n_q, n_phi) -- or one shared (n_q, n_phi) -- with values 0 / 1.

Deviations from the reference, all deliberate: a (q1, q2, Delta) element of a pattern counts where the mask's pair count
|M| >= 0.5 (the reference tests the rounded value M != 0; the two agree wherever the reference is deterministic), a pattern's own
``is_good`` flag decides whether it is accumulated (the reference indexes the flag array with the position inside a sub-batch, 347),
and ``use_binary_mask`` multiplies the mask by ``binary_mask != 0`` (line 385 multiplies an integer mask in place by a float array,
which numpy refuses: the option raises upstream).
"""
import ctypes as C
import math
import warnings

import numpy as np

from . import _lib
from .settings import resolve_correlate

SUPPORTED_N_PHI = (16, 32, 64, 128, 256, 512, 1024)
GENERAL_N_PHI_MIN, GENERAL_N_PHI_MAX = 16, 2048     # general_n_phi=True: even lengths in this range with prime factors 2, 3, 5 only
SUPPORTED_ORDERS = (0, 1, 2, 3, 4, 5)
FRAME_DIM_MIN, FRAME_DIM_MAX = 2, 4096
BAD_MASK = 'correlate: mask values other than 0 / 1'


def general_n_phi_ok(n):
    """n_phi a ``Correlator`` made with general_n_phi=True takes"""
    n = int(n)
    if n < GENERAL_N_PHI_MIN or n > GENERAL_N_PHI_MAX or n % 2:
        return False
    for p in (2, 3, 5):
        while n % p == 0:
            n //= p
    return n == 1


def any_n_phi_ok(n):
    """n_phi a ``Correlator`` made with any_n_phi=True takes: every even length in 16 .. 2048"""
    n = int(n)
    return GENERAL_N_PHI_MIN <= n <= GENERAL_N_PHI_MAX and n % 2 == 0


ANY_N_PHI_HINT = ' (any_n_phi=True takes this length: every even one in 16 .. 2048)'


def general_n_phi_near(n):
    """(below, above): the nearest lengths general_n_phi=True takes on either side of n (None: there is none), e.g. to pick the
    n_phi of phi_range where its 'max' / 'min' mode would give the ring's pixel count"""
    n = int(n)
    below = next((k for k in range(min(n - 1, GENERAL_N_PHI_MAX), GENERAL_N_PHI_MIN - 1, -1) if general_n_phi_ok(k)), None)
    above = next((k for k in range(max(n + 1, GENERAL_N_PHI_MIN), GENERAL_N_PHI_MAX + 1) if general_n_phi_ok(k)), None)
    return below, above


def analyse_dependencies(compute):
    """``_analyse_dependencies`` (correlate.py:478-484)"""
    compute = list(compute)
    if 'ccf_q1q2' in compute and 'xcca' not in compute:
        compute.append('xcca')
    if 'waxs_aver' in compute and 'waxs' not in compute:
        compute.append('waxs')
    return compute


def polar_geometry(settings):
    """``_prepare_polar_representation`` (correlate.py:489-559) and the default q ranges of ``ProjectWorker.__init__`` (77-90) on the
    host: everything the caller's resampling and the result dict need.  Returns a dict with qvals, theta, phi, n_q, n_phi, maxpix,
    cart_x, cart_y (n_q, n_phi), q1vals_pos, q2vals_pos, q1vals, q2vals."""
    opt = resolve_correlate(settings)
    wavelng, det_sam, pixelsize = float(opt['wavelength']), float(opt['sample_distance']), float(opt['pixel_size'])
    qrange, qrange_xcca = opt['qrange'], opt['qrange_xcca']
    if isinstance(qrange, bool) or isinstance(qrange_xcca, bool):                        # 77-90
        detector_edge = opt['image_dimensions'][0] / 2 * (pixelsize / 1000)
        scattering_angle = np.arctan(detector_edge / det_sam)
        q_max = 4 * np.pi * np.sin(scattering_angle / 2) / wavelng
        if isinstance(qrange, bool):
            qrange = [0, q_max, q_max / (opt['image_dimensions'][0] / 2 - 1)]
        if isinstance(qrange_xcca, bool):
            qrange_xcca = [[0, q_max, 1], [0, q_max, 1]]
    phirange = opt['phi_range']
    q_min, q_max, q_step = qrange[0], qrange[1], qrange[2]
    pixsz = pixelsize * 0.001
    n_q = int((q_max - q_min) / q_step + 1)                                              # 495
    phi_min, phi_max, n_phi = phirange[0], phirange[1], phirange[2]
    qvals = np.arange(n_q) * q_step + q_min
    theta = 2.0 * np.arcsin(qvals * wavelng / (4.0 * math.pi))
    max_circ_rad_pix = int(round(det_sam * math.tan(theta[-1]) / pixsz))
    maxpix = round(2 * math.pi * max_circ_rad_pix)
    if (maxpix % 2) != 0:
        maxpix += 1
    maxpix = int(maxpix)
    if phirange[3] == 'max':                                                             # 517-522
        n_phi = min(maxpix, n_phi)
    elif phirange[3] == 'min':
        n_phi = max(maxpix, n_phi)
    n_phi = int(n_phi)
    phi = np.arange(n_phi) * (phi_max - phi_min) / float(n_phi) + phi_min
    pol_q = np.outer(np.tan(theta) * det_sam / pixsz, np.ones(n_phi))
    pol_phi = np.outer(np.ones(n_q), phi)
    origin = opt['detector_origin']
    cart_x = pol_q * np.cos(pol_phi) + origin[0]
    cart_y = pol_q * np.sin(pol_phi) + origin[1]
    pos = []
    for sel in qrange_xcca:                                                              # 547-558
        p1 = np.abs(qvals - sel[0]).argmin()
        p2 = np.abs(qvals - sel[1]).argmin()
        pos.append(np.arange(p1, p2 + 1, sel[2]))
    return {'qvals': qvals, 'theta': theta, 'phi': phi, 'n_q': n_q, 'n_phi': n_phi, 'maxpix': maxpix, 'cart_x': cart_x, 'cart_y': cart_y,
            'q1vals_pos': pos[0], 'q2vals_pos': pos[1], 'q1vals': qvals[pos[0]], 'q2vals': qvals[pos[1]]}


def polarization_factor(theta, phi, kind):
    """``_determine_polarization_correction`` (565-582); any other kind leaves ones, as upstream"""
    out = np.ones((len(theta), len(phi)))
    if kind in ('v', 'h'):
        f = np.sin if kind == 'v' else np.cos
        for i, th in enumerate(theta):
            for j, fi in enumerate(phi):
                out[i, j] = 1.0 / (math.cos(th) ** 2 + (math.sin(th) ** 2) * (f(fi) ** 2))
    return out


def solid_angle_factor(theta, n_phi):
    """``_determine_solid_angle_correction`` (587-591)"""
    out = np.empty((len(theta), n_phi))
    for i, th in enumerate(theta):
        out[i] = 1.0 / (math.cos(th) ** 3)
    return out


def read_raw_images(paths, shape):
    """``_read_binary_2D_arr`` (606-620) for a list of files: little-endian float32 frames of the given (H, W), NaN -> 0; returns
    (P, H, W) float32.  A file of another length raises (upstream's struct.unpack does)."""
    if isinstance(paths, (str, bytes)) or hasattr(paths, '__fspath__'):
        paths = [paths]
    H, W = int(shape[0]), int(shape[1])
    out = np.empty((len(paths), H, W), np.float32)
    for i, path in enumerate(paths):
        data = np.fromfile(path, dtype='<f4')
        if data.size != H * W:
            raise ValueError(f'read_raw_images: {path} holds {data.size} values, a {H} x {W} frame has {H * W}')
        out[i] = data.reshape(H, W)
    out[np.isnan(out)] = 0
    return out


def _frames(a, H, W, what, on_device):
    """(P, H, W) from (P, H, W) or (H, W)"""
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or tuple(a.shape[1:]) != (H, W):
        raise ValueError(f'correlate: {what} must have shape (P, {H}, {W}), got {tuple(a.shape)}')
    return a.contiguous() if on_device else np.ascontiguousarray(a)


def ring_median_mad(engine, images, masks, k):
    """``i_median_and_mad`` (correlate.py:471-474) and the filter of line 412 on rows: images (n_rows, n_phi) float64, masks of the same
    shape (non-zero: valid), n_phi = 1 .. 2048.  Returns (median (n_rows), mad (n_rows), masks_out (n_rows, n_phi) uint8) with
    masks_out = mask & ~(|x - median| > k mad); numpy arrays in and out, or torch tensors on the engine's device in and out."""
    on_device = not isinstance(images, np.ndarray) and hasattr(images, 'data_ptr')
    if on_device:
        import torch
        images = images.to(torch.float64).contiguous()
        masks = (torch.as_tensor(masks, device=images.device) != 0).to(torch.uint8).contiguous()
    else:
        images, masks = _lib.as_f64(images), _lib.as_u8(np.asarray(masks) != 0)
    if images.ndim != 2 or tuple(masks.shape) != tuple(images.shape):
        raise ValueError(f'correlate: ring_median_mad takes images and masks of one shape (n_rows, n_phi), got {tuple(images.shape)} '
                         f'and {tuple(masks.shape)}')
    n_rows, n_phi = int(images.shape[0]), int(images.shape[1])
    if on_device:
        med = torch.empty(n_rows, dtype=torch.float64, device=images.device)
        mad, out = torch.empty_like(med), torch.empty_like(masks)
        ptrs = [engine._tp(t) for t in (images, masks, med, mad, out)]
    else:
        med, mad, out = np.empty(n_rows), np.empty(n_rows), np.empty((n_rows, n_phi), np.uint8)
        ptrs = [_lib.ptr(t) for t in (images, masks, med, mad, out)]
    engine._ck(engine.lib.mtip_op_ring_median_mad(engine.ctx, n_rows, n_phi, ptrs[0], ptrs[1], float(k), ptrs[2], ptrs[3], ptrs[4]))
    return med, mad, out


class Resampler:
    """The Cartesian stage of ``process_image`` (382-398) on the engine's device: ``run(images, masks=None)`` takes detector frames
    (P, H, W) float32 / float64 and optional initial masks (P, H, W) or (H, W) of 0 / 1 (default: ones) to
    (images_polar (P, n_q, n_phi) float64, masks_polar (P, n_q, n_phi) uint8), what ``Correlator.add`` takes.  numpy arrays in, numpy
    arrays out; torch tensors on the engine's device in, such tensors out.  binary_mask / background (H, W) are read where the
    settings switch them on (use_binary_mask, subtract_background); the binary mask counts where it is non-zero.

    The mask is static where intensity_pixel_threshold is off and no masks are given: it is then resampled once per handle."""

    def __init__(self, engine, settings=None, binary_mask=None, background=None):
        self.engine = engine
        self.lib = engine.lib
        self.opt = opt = resolve_correlate(settings)
        self.geometry = g = polar_geometry(opt)
        self.n_q, self.n_phi = g['n_q'], g['n_phi']
        self.H, self.W = int(opt['image_dimensions'][0]), int(opt['image_dimensions'][1])
        self.order = opt['interpolation_order']
        if self.order not in SUPPORTED_ORDERS:
            raise NotImplementedError(f'correlate: interpolation_order = {self.order!r} is not built; supported orders: {SUPPORTED_ORDERS}')
        if not (FRAME_DIM_MIN <= self.H <= FRAME_DIM_MAX and FRAME_DIM_MIN <= self.W <= FRAME_DIM_MAX):
            raise NotImplementedError(f'correlate: frames of {self.H} x {self.W} are not built; supported: {FRAME_DIM_MIN} .. '
                                      f'{FRAME_DIM_MAX} along either axis')
        thr = opt['intensity_pixel_threshold']
        self.threshold = bool(thr[0])
        frame = (self.H, self.W)
        self.binary_mask = self.background = None
        if opt['use_binary_mask']:
            if binary_mask is None or np.shape(binary_mask) != frame:
                raise ValueError(f'correlate: use_binary_mask needs a binary_mask of shape {frame}')
            self.binary_mask = _lib.as_u8(np.asarray(binary_mask) != 0)                  # 385: the evident intent
        if opt['subtract_background']:
            if background is None or np.shape(background) != frame:
                raise ValueError(f'correlate: subtract_background needs a background of shape {frame}')
            self.background = _lib.as_f64(background)
        self.cart_x, self.cart_y = _lib.as_f64(g['cart_x']), _lib.as_f64(g['cart_y'])
        cfg = _lib.MtipResampleCfg(self.H, self.W, int(self.order), int(self.threshold), int(self.binary_mask is not None),
                                   int(self.background is not None), self.n_q * self.n_phi, float(thr[1]), float(thr[2]))
        self.handle = self.lib.mtip_resample_create(engine.ctx, C.byref(cfg), _lib.ptr(self.cart_x), _lib.ptr(self.cart_y),
                                                    _lib.ptr(self.binary_mask), _lib.ptr(self.background))
        if not self.handle:
            msg = self.lib.mtip_last_error(engine.ctx).decode()
            if 'GB' in msg:
                raise MemoryError(msg)
            raise _lib.MtipError(msg)

    def close(self):
        if getattr(self, 'handle', None):
            self.lib.mtip_resample_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def is_static(self, masks):
        """the Cartesian mask does not depend on the pattern"""
        return not self.threshold and masks is None

    def prepare(self, images, masks):
        """checked, contiguous inputs and their pointers: (images, masks or None, P, is_float32, on_device, p_img, p_mask)"""
        on_device = not isinstance(images, np.ndarray) and hasattr(images, 'data_ptr')
        if on_device:
            import torch
            if images.dtype not in (torch.float32, torch.float64):
                raise TypeError('correlate: images must be float32 or float64')
            images = _frames(images, self.H, self.W, 'images', True)
            f32 = images.dtype == torch.float32
            if masks is not None:
                masks = torch.as_tensor(masks, device=images.device)
                if bool(((masks != 0) & (masks != 1)).any()):
                    raise ValueError(BAD_MASK)
                masks = _frames(masks.to(torch.uint8), self.H, self.W, 'masks', True)
        else:
            images = np.asarray(images)
            if images.dtype not in (np.float32, np.float64):
                raise TypeError('correlate: images must be float32 or float64')
            images = _frames(images, self.H, self.W, 'images', False)
            f32 = images.dtype == np.float32
            if masks is not None:
                masks = np.asarray(masks)
                if ((masks != 0) & (masks != 1)).any():
                    raise ValueError(BAD_MASK)
                masks = _frames(masks.astype(np.uint8), self.H, self.W, 'masks', False)
        P = int(images.shape[0])
        if masks is not None:
            if masks.shape[0] not in (1, P):
                raise ValueError(f'correlate: masks must have shape (P, H, W) or (H, W), got {tuple(masks.shape)}')
            if masks.shape[0] != P:
                masks = masks.expand(P, -1, -1).contiguous() if on_device else np.ascontiguousarray(np.broadcast_to(masks, images.shape))
        if on_device:
            p_img, p_mask = self.engine._tp(images), (None if masks is None else self.engine._tp(masks))
            if images.is_cuda:                                                           # (torch's stream, see Correlator.add)
                torch.cuda.current_stream(images.device).synchronize()
        else:
            p_img, p_mask = _lib.ptr(images), _lib.ptr(masks)
        return images, masks, P, f32, on_device, p_img, p_mask

    def run(self, images, masks=None):
        images, masks, P, f32, on_device, p_img, p_mask = self.prepare(images, masks)
        shape = (P, self.n_q, self.n_phi)
        if on_device:
            import torch
            out_i = torch.empty(shape, dtype=torch.float64, device=images.device)
            out_m = torch.empty(shape, dtype=torch.uint8, device=images.device)
            p_oi, p_om = self.engine._tp(out_i), self.engine._tp(out_m)
        else:
            out_i, out_m = np.empty(shape), np.empty(shape, np.uint8)
            p_oi, p_om = _lib.ptr(out_i), _lib.ptr(out_m)
        bad = C.c_int64(0)
        self.engine._ck(self.lib.mtip_resample_run(self.handle, P, p_img, int(f32), p_mask, p_oi, p_om, C.byref(bad)))
        if bad.value:
            raise ValueError(BAD_MASK + f' after the resampling ({bad.value} points)')
        return out_i, out_m

    def static_mask(self):
        """the polar mask (n_q, n_phi) uint8 of the static case, as a numpy array"""
        if getattr(self, '_static', None) is None:
            if self.threshold:
                raise ValueError('correlate: with intensity_pixel_threshold on the mask is not static')
            self._static = self.run(np.zeros((1, self.H, self.W), np.float32))[1][0]
        return self._static


class Correlator:
    """Accumulates patterns on the engine's device: ``add(images, masks)`` any number of times, ``result()`` for the reference's result
    dict (it goes through ``io.load_ccd(..., 'direct')`` into ``extract_from_cross_correlation`` unchanged);
    ``add_detector(images, masks=None)`` takes detector frames through a ``Resampler`` (binary_mask / background are its).  ``partial()`` /
    ``merge(partials)`` make the accumulation additive over ranks or GPUs that each take a share of the patterns.

    shared_mask=True: one mask for every pattern; its pair counts are computed once per handle.  An active radial pixel filter makes
    masks per pattern, so the flag is ignored then.

    general_n_phi=True (None: settings['GPU']['general_n_phi'], default False): n_phi may be any even length in 16 .. 2048 whose only
    prime factors are 2, 3 and 5 -- the default settings' 1536 among them -- through ``mtip_correlate_create_ex``; without it the
    lengths are SUPPORTED_N_PHI.  ``general_n_phi_near`` names the nearest such lengths.

    any_n_phi=True (None: settings['GPU']['any_n_phi'], default False): n_phi may be any even length in 16 .. 2048 (``any_n_phi_ok``),
    as phi_range's 'max' and 'min' modes make them from the outermost ring's pixel count.  The lengths above run the same kernels
    and give the same bits as without it; a length with a prime factor above 5 runs chirp-z transforms (``csrc/k_correlate_bs.h``).

    median_mad=True (None: settings['GPU']['median_mad'], default False): intensity_radial_pixel_filter [True, ['median_mad', k]] runs
    on the device (``csrc/k_ringfilter.h``: exact medians, numpy's and scipy's bit for bit); without it that setting raises."""

    def __init__(self, engine, settings=None, shared_mask=False, binary_mask=None, background=None, general_n_phi=None, median_mad=None,
                 any_n_phi=None):
        self.engine = engine
        self._frame_arrays = (binary_mask, background)
        self.resampler = None
        self.lib = engine.lib
        self.opt = opt = resolve_correlate(settings)
        self.compute = analyse_dependencies(opt['compute'])
        self.geometry = g = polar_geometry(opt)
        self.n_q, self.n_phi = g['n_q'], g['n_phi']
        if general_n_phi is None:
            general_n_phi = (opt.get('GPU') or {}).get('general_n_phi', False)
        self.general_n_phi = bool(general_n_phi)
        if any_n_phi is None:
            any_n_phi = (opt.get('GPU') or {}).get('any_n_phi', False)
        self.any_n_phi = bool(any_n_phi)
        hint = ANY_N_PHI_HINT if any_n_phi_ok(self.n_phi) else ''
        if self.any_n_phi:
            if not any_n_phi_ok(self.n_phi):
                raise NotImplementedError(f'correlate: n_phi = {self.n_phi} is not built; any_n_phi takes every even length '
                                          f'{GENERAL_N_PHI_MIN} .. {GENERAL_N_PHI_MAX}')
        elif self.general_n_phi:
            if not general_n_phi_ok(self.n_phi):
                below, above = general_n_phi_near(self.n_phi)
                raise NotImplementedError(f'correlate: n_phi = {self.n_phi} is not built; general_n_phi takes even lengths '
                                          f'{GENERAL_N_PHI_MIN} .. {GENERAL_N_PHI_MAX} whose only prime factors are 2, 3 and 5; the '
                                          f'nearest below: {below}, above: {above}' + hint)
        elif self.n_phi not in SUPPORTED_N_PHI:
            raise NotImplementedError(f'correlate: n_phi = {self.n_phi} is not built; supported lengths: {SUPPORTED_N_PHI}' + hint)
        filt = opt['intensity_radial_pixel_filter']
        self.filter = bool(filt[0])
        if median_mad is None:
            median_mad = (opt.get('GPU') or {}).get('median_mad', False)
        self.median_mad = bool(median_mad)
        if self.filter and filt[1][0] == 'median_mad' and not self.median_mad:
            raise NotImplementedError("correlate: intensity_radial_pixel_filter 'median_mad' (correlate.py:405-406, i_median_and_mad "
                                      "471-474) is opt-in: Correlator(..., median_mad=True) or settings['GPU']['median_mad'] = True; "
                                      'average_sigma needs no flag')
        if self.filter and filt[1][0] not in ('average_sigma', 'median_mad'):
            raise ValueError(f'correlate: unknown intensity_radial_pixel_filter {filt[1][0]!r} (correlate.py:408)')
        filter_kind = 0 if not self.filter else (2 if filt[1][0] == 'median_mad' else 1)
        roi_n, roi_f = opt['ROI_normalization'], opt['ROI_mean_filter']
        qvals = g['qvals']
        roi_lo = roi_hi = 0
        if roi_n[0] or roi_f[0]:                                                         # 186-188: both read ROI_normalization's range
            roi_lo = int(np.abs(qvals - roi_n[1]).argmin())
            roi_hi = int(np.abs(qvals - roi_n[2]).argmin())
        factor = None
        pol = opt['polarization_correction']
        if pol[0]:
            factor = polarization_factor(g['theta'], g['phi'], pol[1])
        if opt['solid_angle_correction'] is True:
            sa = solid_angle_factor(g['theta'], self.n_phi)
            factor = sa if factor is None else factor * sa
        self.factor = None if factor is None else _lib.as_f64(factor)
        self.q1 = np.ascontiguousarray(g['q1vals_pos'], dtype=np.int32)
        self.q2 = np.ascontiguousarray(g['q2vals_pos'], dtype=np.int32)
        self.n_q1, self.n_q2 = len(self.q1), len(self.q2)
        self.shared_mask = bool(shared_mask) and not self.filter
        self._mask0 = None
        cfg = _lib.MtipCorrelateCfg(self.n_q, self.n_phi, self.n_q1, self.n_q2, filter_kind, roi_lo, roi_hi,
                                    1 if roi_f[0] else 0, 1 if roi_n[0] else 0, 1 if self.shared_mask else 0,
                                    float(filt[1][1]) if self.filter else 0.0, float(roi_f[1]), float(roi_f[2]))
        tables = (engine.ctx, C.byref(cfg), _lib.ptr(self.q1), _lib.ptr(self.q2), _lib.ptr(self.factor))
        flags = (_lib.MTIP_CORRELATE_GENERAL_NPHI if self.general_n_phi else 0) | (_lib.MTIP_CORRELATE_ANY_NPHI if self.any_n_phi else 0)
        if flags:
            self.handle = self.lib.mtip_correlate_create_ex(*tables, flags)
        else:
            self.handle = self.lib.mtip_correlate_create(*tables)
        if not self.handle:
            msg = self.lib.mtip_last_error(engine.ctx).decode()
            if 'GB' in msg:
                raise MemoryError(msg)
            raise _lib.MtipError(msg)

    # ------------------------------------------------------------------ bookkeeping
    def close(self):
        if getattr(self, 'resampler', None) is not None:
            self.resampler.close()
            self.resampler = None
        if getattr(self, 'handle', None):
            self.lib.mtip_correlate_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        self.engine._ck(rc)

    @property
    def acc_shape(self):
        return (self.n_q1, self.n_q2, self.n_phi)

    @property
    def num_patterns(self):
        return int(self.lib.mtip_correlate_num_patterns(self.handle))

    # ------------------------------------------------------------------ accumulation
    def add(self, images, masks):
        """images (P, n_q, n_phi) float32 / float64, masks (P, n_q, n_phi) or one (n_q, n_phi) of 0 / 1 (any integer or bool type):
        numpy arrays, or torch tensors on the engine's device.  A single mask for P patterns is expanded unless the handle was made
        with shared_mask."""
        on_device = not isinstance(images, np.ndarray) and hasattr(images, 'data_ptr')
        ring = (self.n_q, self.n_phi)
        if on_device:
            import torch
            if images.dtype not in (torch.float32, torch.float64):
                raise TypeError('correlate: images must be float32 or float64')
            if images.ndim == 2:
                images = images[None]
            images = images.to(torch.float64).contiguous()
            masks = torch.as_tensor(masks, device=images.device)
            if bool(((masks != 0) & (masks != 1)).any()):
                raise ValueError(BAD_MASK)
            masks = masks.to(torch.uint8)
            shape, mshape = tuple(images.shape), tuple(masks.shape)
        else:
            images = np.asarray(images)
            if images.dtype not in (np.float32, np.float64):
                raise TypeError('correlate: images must be float32 or float64')
            if images.ndim == 2:
                images = images[None]
            images = _lib.as_f64(images)
            masks = np.asarray(masks)
            if ((masks != 0) & (masks != 1)).any():
                raise ValueError(BAD_MASK)
            masks = masks.astype(np.uint8)
            shape, mshape = images.shape, masks.shape
        if len(shape) != 3 or tuple(shape[1:]) != ring:
            raise ValueError(f'correlate: images must have shape (P, {self.n_q}, {self.n_phi}), got {tuple(shape)}')
        P = int(shape[0])
        if tuple(mshape) not in (ring, (1,) + ring, (P,) + ring):
            raise ValueError(f'correlate: masks must have shape (P, n_q, n_phi) or (n_q, n_phi), got {tuple(mshape)}')
        one = tuple(mshape) == ring or (tuple(mshape) == (1,) + ring and P != 1)
        masks = masks.reshape((-1,) + ring)
        if self.shared_mask:
            if masks.shape[0] != 1:
                raise ValueError('correlate: a handle made with shared_mask takes one (n_q, n_phi) mask')
            host = masks.cpu().numpy() if on_device else masks
            if self._mask0 is None:
                self._mask0 = host.copy()
            elif not np.array_equal(self._mask0, host):
                raise ValueError('correlate: shared_mask: the mask differs from the one of the first batch')
        elif one or masks.shape[0] != P:
            masks = masks.expand(P, -1, -1) if on_device else np.broadcast_to(masks, (P,) + ring)
        if on_device:
            masks = masks.contiguous()
            p_img, p_mask = self.engine._tp(images), self.engine._tp(masks)
            if images.is_cuda:                                                           # torch's conversions above run on torch's stream,
                torch.cuda.current_stream(images.device).synchronize()                   # the kernels on the context's own
        else:
            masks = np.ascontiguousarray(masks)
            p_img, p_mask = _lib.ptr(images), _lib.ptr(masks)
        self._ck(self.lib.mtip_correlate_add(self.handle, P, p_img, p_mask))
        return self

    def add_detector(self, images, masks=None):
        """detector frames (P, H, W) float32 / float64 and optional initial masks (P, H, W) or (H, W) of 0 / 1 (default: ones): the
        same as ``add(*resampler.run(images, masks))``, bit for bit, without the polar arrays leaving the device.  A handle made
        with shared_mask takes frames only where the mask is static (intensity_pixel_threshold off, no masks)."""
        if self.resampler is None:
            self.resampler = Resampler(self.engine, self.opt, *self._frame_arrays)
        rs = self.resampler
        if self.shared_mask and not rs.is_static(masks):
            raise ValueError('correlate: shared_mask: detector frames are taken only where the mask is static; it is not with '
                             'intensity_pixel_threshold on or with masks given')
        images, masks, P, f32, _, p_img, p_mask = rs.prepare(images, masks)
        if self.shared_mask:
            host = rs.static_mask()[None]
            if self._mask0 is None:
                self._mask0 = host.copy()
            elif not np.array_equal(self._mask0, host):
                raise ValueError('correlate: shared_mask: the mask differs from the one of the first batch')
        bad = C.c_int64(0)
        rc = self.lib.mtip_correlate_add_detector(self.handle, rs.handle, P, p_img, int(f32), p_mask, C.byref(bad))
        if bad.value:
            raise ValueError(BAD_MASK + f' after the resampling ({bad.value} points)')
        self._ck(rc)
        return self

    def partial(self):
        """the additive state: {'sum', 'count' (n_q1, n_q2, n_phi), 'is_good' (M) int32, 'waxs' (M, n_q)} as numpy arrays"""
        n = self.num_patterns
        out = {'sum': np.empty(self.acc_shape), 'count': np.empty(self.acc_shape, np.int32), 'is_good': np.empty(n, np.int32),
               'waxs': np.empty((n, self.n_q))}
        self._ck(self.lib.mtip_correlate_get_partial(self.handle, _lib.ptr(out['sum']), _lib.ptr(out['count']), _lib.ptr(out['is_good']),
                                                     _lib.ptr(out['waxs'])))
        return out

    def merge(self, partials):
        """add the partial results of other correlators (a dict of ``partial()`` or a list of them); their patterns are appended"""
        if isinstance(partials, dict):
            partials = [partials]
        for p in partials:
            s, c = _lib.as_f64(p['sum']), np.ascontiguousarray(p['count'], dtype=np.int32)
            g, w = np.ascontiguousarray(p['is_good'], dtype=np.int32), _lib.as_f64(p['waxs'])
            if s.shape != self.acc_shape or c.shape != self.acc_shape or w.shape != (len(g), self.n_q):
                raise ValueError('correlate: a partial result of another shape')
            self._ck(self.lib.mtip_correlate_merge(self.handle, _lib.ptr(s), _lib.ptr(c), len(g), _lib.ptr(g), _lib.ptr(w)))
        return self

    # ------------------------------------------------------------------ result (correlate.py:249-295)
    def symmetrize_positions(self):
        phi = self.geometry['phi']
        return (int(np.abs(phi - math.pi / 2.0).argmin()), int(np.abs(phi - math.pi).argmin()), int(np.abs(phi - 3 * math.pi / 2.0).argmin()))

    def finalize(self, want_ccf=True, want_fc=False):
        """(ccf (n_q1, n_q2, n_phi) or None, fc (n_q1, n_q2, fc_n_max) or None) from the device"""
        sym = self.opt['ccf_2p_symmetrize'] is True
        pos = self.symmetrize_positions() if sym else (0, 0, 0)
        fc_n = min(int(self.opt['fc_n_max']), self.n_phi)
        ccf = np.empty(self.acc_shape) if want_ccf else None
        fc = np.empty((self.n_q1, self.n_q2, fc_n), complex) if want_fc else None
        self._ck(self.lib.mtip_correlate_finalize(self.handle, int(sym), pos[0], pos[1], pos[2], fc_n, _lib.ptr(ccf), _lib.ptr(fc)))
        return ccf, fc

    def result(self):
        compute, g = self.compute, self.geometry
        want_fc = 'ccf_q1q2_fc' in compute
        want_ccf = 'ccf_q1q2' in compute
        part_n = self.num_patterns
        is_good = np.empty(part_n, np.int32)
        waxs = np.empty((part_n, self.n_q))
        self._ck(self.lib.mtip_correlate_get_partial(self.handle, None, None, _lib.ptr(is_good), _lib.ptr(waxs)))
        mgood = int(np.sum(is_good))                                                     # 249
        result = {}
        if 'waxs_aver' in compute:                                                       # 252-253, 276-278
            aver = np.zeros(self.n_q)
            with np.errstate(invalid='ignore', divide='ignore'), warnings.catch_warnings():
                warnings.simplefilter('ignore', RuntimeWarning)                          # (no good pattern: NaN, as upstream)
                np.mean(waxs, axis=0, where=(is_good[:, None] == 1), out=aver)
            result['average_intensity'] = aver
        if 'xcca' in compute and (want_ccf or want_fc):
            ccf, fc = self.finalize(want_ccf, want_fc)
            if want_ccf:
                result['cross_correlation'] = {'I1I1': ccf}                              # 280-282
            if want_fc:
                result['cross_correlation'] = {'I1I1_fc': fc}                            # 287-288
        result['radial_points'] = g['qvals']
        result['angular_points'] = g['phi']
        result['num_images_processed'] = part_n
        result['num_images_good'] = mgood
        result['xray_wavelength'] = self.opt['wavelength']
        return result

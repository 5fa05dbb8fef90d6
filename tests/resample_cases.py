"""Cases of the route detector frames -> polar patterns (csrc/k_resample.h, fxs/correlate.py Resampler / Correlator.add_detector), shared
by tests/test_emul_resample.py (CPU emulator), tests/test_gpu_resample.py (MI355X) and tests/test_resample_reference.py (no kernel).

Yardsticks:
  * G26 (tests/golden/resample.npz): image_polar / mask_polar of the reference's own DataReader.process_image at interp_order 0, 2, 3, 5
    on 24 x 20 frames (tests/golden/make_golden_resample.py);
  * r_resample: a numpy float64 restatement of process_image 382-398 including scipy.ndimage.map_coordinates (weights from the
    spline's polynomial pieces), held to G26 and to scipy;
  * x_resample: the same in np.longdouble (closed-form mirror start of the recursions, explicit B-spline sum for the weights).

Bound per element of the image:  |device - x_resample| <= 8 eps G_n^2 max|image mask|,  G_n = 1, 1, 2, 3, 4.8, 7.5 for orders 0 .. 5:
the infinity norm of one axis' inverse prefilter, 1 / (beta(0) - 2 |beta(1)| + 2 |beta(2)|); max over the prepared frame of the
pattern.  scipy's own distance to x_resample is at most 0.83 eps G_n^2 max (frames 4 x 5 .. 130 x 67, values up to 1000), which is where
the factor 8 comes from; the CPU test holds scipy and r_resample to a quarter of the bound.
Masks compare exactly, except at points whose longdouble value lies within 1e-9 of a half-integer; those may be at most 0.1 % of a
case's points (the origin offsets are kept off half-pixels: with the inputs below there is none).
Points outside the frame are exactly 0 in image and mask.

Shapes: the issue's four (4 x 5 is smaller than the support of order 5: the mirror is applied more than once) and, from the kernel's
constants, 2 x 3 (the shortest line: RS_MIN_DIM) and 65 x 33 (one row past a row block RS_RT, one column past an LDS tile RS_TW);
130 x 67 takes a third row block, a second column block (RS_CT), a third tile with a tail, and 12 x 32 points (+ the edge points) a
second gather block (RS_GT).  33 patterns make a second chunk (RS_CHUNK)."""
import ctypes
import functools
import os

import numpy as np

from xframe_amd.fxs import _lib, correlate as CR
from ccextract_cases import small_engine

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'resample.npz')
EPS = np.finfo(float).eps
G_N = (1.0, 1.0, 2.0, 3.0, 4.8, 7.5)
BOUND_FACTOR = 8.0
TOL_GOLDEN = 1e-13
NEAR_HALF = 1e-9
MAX_NEAR_SHARE = 1e-3
RS_CT, RS_RT, RS_TW, RS_GT, RS_CHUNK, RS_MIN_DIM = 64, 64, 32, 256, 32, 2
SHAPES = [(4, 5), (37, 53), (64, 64), (130, 67), (RS_MIN_DIM, 3), (RS_RT + 1, RS_TW + 1)]
ORDERS = (0, 1, 2, 3, 4, 5)
SWITCH_NAMES = ('plain', 'threshold', 'binary', 'background', 'masks', 'all')
THRESHOLD = (60.0, 930.0)
G26_ORDERS = (0, 2, 3, 5)
G26_SETS = {'plain': {}, 'threshold': {'thr': True}, 'background': {'bg': True}, 'binary': {'bin': True},
            'all': {'thr': True, 'bg': True, 'bin': True}}


# ---- numpy restatement of map_coordinates (dtype float64) and its longdouble twin --------------------------------------------------------
def poles(order, dt):
    """the poles of the prefilter, correctly rounded to dt (the closed forms of orders 4 and 5 cancel three digits: they are
    evaluated in longdouble whatever dt is)"""
    return [dt(z) for z in _poles(order, np.longdouble)]


def _poles(order, dt):
    s = lambda v: np.sqrt(dt(v))                                                         # noqa: E731
    if order == 2:
        return [s(8) - dt(3)]
    if order == 3:
        return [s(3) - dt(2)]
    if order == 4:
        return [np.sqrt(dt(664) - s(438976)) + s(304) - dt(19), np.sqrt(dt(664) + s(438976)) - s(304) - dt(19)]
    if order == 5:
        return [np.sqrt(dt(67.5) - s(4436.25)) + s(26.25) - dt(6.5), np.sqrt(dt(67.5) + s(4436.25)) - s(26.25) - dt(6.5)]
    return []


def mirror(i, n):
    """whole-sample symmetry about 0 and n - 1 (period 2 n - 2), applied as often as it takes"""
    per = 2 * n - 2
    i = np.mod(i, per)
    return np.where(i < n, i, per - i)


def filter_axis0(a, order, dt):
    """the B-spline prefilter along axis 0 of (N, ...): per pole a causal and an anticausal recursion; the causal start is the sum
    over one whole period of the mirrored line, divided by 1 - z^(2N-2)"""
    c = np.array(a, dtype=dt)
    n = c.shape[0]
    zs = poles(order, dt)
    gain = dt(1)
    for z in zs:
        gain = gain * (dt(1) - z) * (dt(1) - dt(1) / z)
    c *= gain
    k = np.arange(2 * n - 2)
    for z in zs:
        zk = z ** k.astype(dt)
        c0 = np.tensordot(zk, c[mirror(k, n)], axes=(0, 0)) / (dt(1) - z ** dt(2 * n - 2))
        c[0] = c0
        for i in range(1, n):
            c[i] = c[i] + z * c[i - 1]
        c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - dt(1))
        for i in range(n - 2, -1, -1):
            c[i] = z * (c[i + 1] - c[i])
    return c


def spline_coefficients(a, order, dt):
    """(..., H, W) -> coefficients: axis 0 of the frame, then axis 1; orders 0 and 1 have no prefilter"""
    a = np.array(a, dtype=dt)
    if order < 2:
        return a
    c = np.moveaxis(filter_axis0(np.moveaxis(a, -2, 0), order, dt), 0, -2)
    return np.moveaxis(filter_axis0(np.moveaxis(c, -1, 0), order, dt), 0, -1)


def bspline(n, x, dt):
    """the centred cardinal B-spline of degree n: 1 / n! sum_k (-1)^k C(n + 1, k) (x + (n + 1) / 2 - k)_+^n"""
    from math import comb, factorial
    x = np.asarray(x, dtype=dt)
    if n == 0:
        return ((x >= dt(-0.5)) & (x < dt(0.5))).astype(dt)
    out = np.zeros(x.shape, dt)
    for k in range(n + 2):
        t = np.maximum(x + dt(n + 1) / dt(2) - dt(k), dt(0))
        out += dt((-1) ** k * comb(n + 1, k)) * t ** n
    return out / dt(factorial(n))


def bspline_piecewise(n, x):
    """the same spline in float64 by its polynomial pieces in Horner form (no cancellation between large terms)"""
    a = np.abs(np.asarray(x, dtype=np.float64))
    if n == 1:
        return np.maximum(1.0 - a, 0.0)
    if n == 2:
        return np.where(a < 0.5, 0.75 - a * a, np.where(a < 1.5, 0.5 * (1.5 - a) ** 2, 0.0))
    if n == 3:
        return np.where(a < 1.0, (a * a * (a - 2.0) * 3.0 + 4.0) / 6.0, np.where(a < 2.0, (2.0 - a) ** 3 / 6.0, 0.0))
    if n == 4:
        inner = a * a * (a * a * 0.25 - 0.625) + 115.0 / 192.0
        mid = a * (a * (a * (5.0 / 6.0 - a / 6.0) - 1.25) + 5.0 / 24.0) + 55.0 / 96.0
        return np.where(a < 0.5, inner, np.where(a < 1.5, mid, np.where(a < 2.5, (a - 2.5) ** 4 / 24.0, 0.0)))
    inner = a * a * (a * a * (0.25 - a / 12.0) - 0.5) + 0.55
    mid = a * (a * (a * (a * (a / 24.0 - 0.375) + 1.25) - 1.75) + 0.625) + 0.425
    return np.where(a <= 1.0, inner, np.where(a < 2.0, mid, np.where(a < 3.0, (3.0 - a) ** 5 / 120.0, 0.0)))


def taps(x, n, order, dt):
    """(indices (order + 1, npts) through the mirror, weights (order + 1, npts)) of one axis"""
    x = np.asarray(x, dtype=np.float64)
    first = (np.floor(x) if order % 2 else np.floor(x + 0.5)).astype(np.int64) - order // 2
    pos = first[None, :] + np.arange(order + 1)[:, None]
    if order == 0:
        w = np.ones(pos.shape, dt)
    elif dt is np.longdouble:
        w = bspline(order, x.astype(dt)[None, :] - pos.astype(dt), dt)
    else:
        w = bspline_piecewise(order, x[None, :] - pos.astype(np.float64)).astype(dt)
    return mirror(pos, n), w


def interpolate(coef, xs, ys, order, dt):
    """coef (P, H, W) at the points (xs along axis 0, ys along axis 1): (P, npts); 0 outside [0, H - 1] x [0, W - 1] (ends inclusive)"""
    P, H, W = coef.shape
    inside = (xs >= 0) & (xs <= H - 1) & (ys >= 0) & (ys <= W - 1)
    out = np.zeros((P, len(xs)), dt)
    ix, wx = taps(xs[inside], H, order, dt)
    iy, wy = taps(ys[inside], W, order, dt)
    acc = np.zeros((P, int(inside.sum())), dt)
    for r in range(order + 1):
        for s in range(order + 1):
            acc += coef[:, ix[r], iy[s]] * (wx[r] * wy[s])[None, :]
    out[:, inside] = acc
    return out, inside


def round_half_away(v):
    v = np.asarray(v)
    return np.where(v < 0, -np.floor(-v + 0.5), np.floor(v + 0.5)).astype(np.int64)


def prepare(images, masks, thr=None, binary=None, background=None, dt=np.float64):
    """process_image 382-392 for (P, H, W): the prepared images (dt) and the Cartesian masks (int)"""
    images = np.array(images, dtype=np.float64)
    masks = np.ones(images.shape, np.int64) if masks is None else np.array(np.broadcast_to(masks, images.shape), dtype=np.int64)
    if thr is not None:
        masks[(images < thr[0]) | (images > thr[1])] = 0                                  # 383
    if binary is not None:
        masks *= (np.asarray(binary) != 0).astype(np.int64)[None]                         # 385: the evident intent
    img = images.astype(dt)
    if background is not None:
        img = img - np.asarray(background, np.float64).astype(dt)[None]                   # 389
    return img * masks.astype(dt), masks                                                  # 392


def resample(images, masks, xs, ys, order, thr=None, binary=None, background=None, dt=np.float64):
    """process_image 382-398: {'image' (P, npts) dt, 'mask_value' (P, npts) dt before rounding, 'mask' int, 'inside', 'scale' (P)}"""
    img, msk = prepare(images, masks, thr, binary, background, dt)
    vi, inside = interpolate(spline_coefficients(img, order, dt), xs, ys, order, dt)
    vm, _ = interpolate(spline_coefficients(msk, order, dt), xs, ys, order, dt)
    return {'image': vi, 'mask_value': vm, 'mask': round_half_away(vm), 'inside': inside,
            'scale': np.abs(img.astype(np.float64)).reshape(len(img), -1).max(axis=1)}


def r_resample(images, masks, xs, ys, order, **kw):
    return resample(images, masks, xs, ys, order, dt=np.float64, **kw)


def x_resample(images, masks, xs, ys, order, **kw):
    x = resample(images, masks, xs, ys, order, dt=np.longdouble, **kw)
    frac = x['mask_value'] - np.floor(x['mask_value'])
    x['near_half'] = np.abs(frac - np.longdouble(0.5)) < NEAR_HALF
    return x


def scipy_resample(images, masks, xs, ys, order, **kw):
    """the reference's route itself: map_coordinates on the float64 image and on the integer mask"""
    from scipy import ndimage
    img, msk = prepare(images, masks, dt=np.float64, **kw)
    out_i = np.stack([ndimage.map_coordinates(a, [xs, ys], order=order, mode='constant', cval=0, prefilter=True) for a in img])
    out_m = np.stack([ndimage.map_coordinates(a, [xs, ys], order=order, mode='constant', cval=0, prefilter=True) for a in msk])
    return out_i, out_m


def bound(x, order):
    """(P, 1): the bound of every element of pattern p"""
    return (BOUND_FACTOR * EPS * G_N[order] ** 2 * x['scale'])[:, None]


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------------
def polar_points(H, W, n_q=12, n_phi=32):
    """a polar grid around (H / 2 - 0.3, W / 2 + 0.21) whose outer rings leave the frame: 25-40 % of its points lie outside"""
    ox, oy = H / 2 - 0.3, W / 2 + 0.21
    phi = np.arange(n_phi) * 2 * np.pi / n_phi + 0.05
    for f in np.arange(0.5, 4.0, 0.025):
        r = np.arange(n_q) * (f * min(H, W) / 2 / (n_q - 1))
        xs = (r[:, None] * np.cos(phi)[None, :] + ox).ravel()
        ys = (r[:, None] * np.sin(phi)[None, :] + oy).ravel()
        out = 1.0 - np.mean((xs >= 0) & (xs <= H - 1) & (ys >= 0) & (ys <= W - 1))
        if 0.25 <= out <= 0.40:
            return xs, ys
    raise AssertionError((H, W))


def edge_points(H, W):
    """for the image only: the four corners, a hair outside and inside each edge, exact integers, exact half-integers (where the
    even orders switch their first tap)"""
    pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1),
           (-1e-9, W / 2), (H - 1 + 1e-9, W / 2), (H / 2, -1e-9), (H / 2, W - 1 + 1e-9),
           (1e-9, 1e-9), (H - 1 - 1e-9, W - 1 - 1e-9)]
    for i in sorted({0, 1, H // 2, H - 2, H - 1}):
        for j in sorted({0, 1, W // 2, W - 2, W - 1}):
            pts.append((i, j))
            if i + 0.5 <= H - 1:
                pts.append((i + 0.5, j))
            if j + 0.5 <= W - 1:
                pts.append((i, j + 0.5))
            if i + 0.5 <= H - 1 and j + 0.5 <= W - 1:
                pts.append((i + 0.5, j + 0.5))
    a = np.array(pts, dtype=np.float64)
    return a[:, 0].copy(), a[:, 1].copy()


def make_frames(H, W, P, seed, dtype=np.float64):
    """P frames with values up to 1000; initial masks: random dead pixels at 10 %, a dead rectangle, a dead column, in turn; a
    binary mask with a dead corner block and a smooth background"""
    rng = np.random.default_rng(seed)
    images = (1000.0 * rng.random((P, H, W))).astype(dtype)
    masks = np.ones((P, H, W), np.int64)
    for p in range(P):
        kind = p % 3
        if kind == 0:
            masks[p][rng.random((H, W)) < 0.10] = 0
        elif kind == 1:
            masks[p, H // 4:H // 4 + max(1, H // 3), W // 3:W // 3 + max(1, W // 4)] = 0
        else:
            masks[p, :, (2 * W) // 3] = 0
    binary = np.ones((H, W), np.int64)
    binary[:max(1, H // 5), :max(1, W // 5)] = 0
    binary[rng.random((H, W)) < 0.03] = 0
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    background = 20.0 + 5.0 * np.sin(0.3 * ii) * np.cos(0.2 * jj)
    return images, masks, binary, background


def switch_kwargs(name, masks, binary, background):
    """(caller's masks or None, keywords of resample) of a switch set"""
    on = lambda k: name in (k, 'all')                                                     # noqa: E731
    return (masks if on('masks') else None,
            {'thr': THRESHOLD if on('threshold') else None, 'binary': binary if on('binary') else None,
             'background': background if on('background') else None})


@functools.lru_cache(maxsize=None)
def case(H, W, order, switches, dtype_name, P=3, edges=True):
    """inputs and both references of one case, computed once and frozen"""
    images, masks, binary, background = make_frames(H, W, P, 100 * H + W, np.dtype(dtype_name))
    xs, ys = polar_points(H, W)
    n_grid = len(xs)
    if edges:
        ex, ey = edge_points(H, W)
        xs, ys = np.concatenate([xs, ex]), np.concatenate([ys, ey])
    cm, kw = switch_kwargs(switches, masks, binary, background)
    x = x_resample(images, cm, xs, ys, order, **kw)
    r = r_resample(images, cm, xs, ys, order, **kw)
    share = float(x['near_half'][:, :n_grid].mean())
    assert share <= MAX_NEAR_SHARE, share                                                 # the condition on the inputs
    out = {'images': images, 'masks': cm, 'xs': xs, 'ys': ys, 'n_grid': n_grid, 'kw': kw, 'x': x, 'r': r, 'order': order}
    for d in (out, x, r):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return out


def as_signed(msk):
    """the device stores a rounded mask value as its low byte: 255 is -1"""
    msk = np.asarray(msk)
    return (msk.view(np.int8) if msk.dtype == np.uint8 else msk).astype(np.int64)


def check_bad(bad, c, tag):
    """the device's count of rounded mask values other than 0 / 1 is the longdouble reference's (a spline of order >= 2 overshoots: a
    busy mask can reach 1.5 or -0.5), up to the points within 1e-9 of a half-integer"""
    m = c['x']['mask']
    want = int(((m != 0) & (m != 1)).sum())
    assert abs(bad - want) <= int(c['x']['near_half'].sum()), (tag, bad, want)


def compare(img, msk, c, tag, who='device', fraction=1.0):
    """img (P, npts), msk (P, npts) against the longdouble reference of case c: prints and returns the worst ratio to the bound"""
    x, n_grid = c['x'], c['n_grid']
    outside = ~x['inside']
    assert not np.any(img[:, outside]) and not np.any(msk[:, outside]), tag              # exactly 0, not merely small
    err = np.abs((img.astype(np.longdouble) - x['image']).astype(np.float64))
    b = bound(x, c['order'])
    ratio = float((err / b).max())
    near = x['near_half'][:, :n_grid]
    differ = as_signed(msk[:, :n_grid]) != x['mask'][:, :n_grid]
    print(f'{tag}: {who} / bound {ratio:.3f}; masks differing {int(differ.sum())} (near a half-integer: {int(near.sum())})')
    assert ratio <= fraction, (tag, ratio)
    assert not np.any(differ & ~near), tag
    return ratio


# ---- the device through the C ABI (arbitrary points) --------------------------------------------------------------------------------------
def device_run(e, H, W, order, xs, ys, images, masks=None, thr=None, binary=None, background=None, splits=None):
    """mtip_resample_create / run / destroy: (images (P, npts) float64, masks (P, npts) uint8, n_bad); splits: batch sizes"""
    xs, ys = _lib.as_f64(xs), _lib.as_f64(ys)
    b = None if binary is None else _lib.as_u8(np.asarray(binary) != 0)
    g = None if background is None else _lib.as_f64(background)
    lo, hi = thr if thr is not None else (0.0, 0.0)
    cfg = _lib.MtipResampleCfg(H, W, order, int(thr is not None), int(b is not None), int(g is not None), len(xs), lo, hi)
    h = e.lib.mtip_resample_create(e.ctx, ctypes.byref(cfg), _lib.ptr(xs), _lib.ptr(ys), _lib.ptr(b), _lib.ptr(g))
    assert h, e.lib.mtip_last_error(e.ctx).decode()
    images = np.ascontiguousarray(images)
    P = len(images)
    m8 = None if masks is None else _lib.as_u8(np.broadcast_to(masks, images.shape))
    out_i, out_m, n_bad = np.full((P, len(xs)), np.nan), np.full((P, len(xs)), 77, np.uint8), 0
    start = 0
    for n in (splits or [P]):
        bad = ctypes.c_int64(-1)
        oi, om = np.empty((n, len(xs))), np.empty((n, len(xs)), np.uint8)
        rc = e.lib.mtip_resample_run(h, n, _lib.ptr(images[start:start + n]), int(images.dtype == np.float32),
                                     None if m8 is None else _lib.ptr(m8[start:start + n]), _lib.ptr(oi), _lib.ptr(om), ctypes.byref(bad))
        assert rc == 0, e.lib.mtip_last_error(e.ctx).decode()
        out_i[start:start + n], out_m[start:start + n] = oi, om
        n_bad += bad.value
        start += n
    assert start == P
    e.lib.mtip_resample_destroy(h)
    return out_i, out_m, n_bad


def device_case(e, c, **kw):
    return device_run(e, c['images'].shape[1], c['images'].shape[2], c['order'], c['xs'], c['ys'], c['images'], c['masks'],
                      thr=c['kw']['thr'], binary=c['kw']['binary'], background=c['kw']['background'], **kw)


# ---- checks --------------------------------------------------------------------------------------------------------------------------------
def check_shape_order(lib_path, shape, order):
    """one shape at one order: float64 frames with every switch on, float32 frames with the caller's masks alone"""
    e = small_engine(lib_path)
    worst = 0.0
    for sw, dtype in (('all', 'float64'), ('masks', 'float32')):
        c = case(shape[0], shape[1], order, sw, dtype)
        img, msk, bad = device_case(e, c)
        check_bad(bad, c, sw)
        worst = max(worst, compare(img, msk, c, f'{shape[0]} x {shape[1]} order {order} {sw} {dtype}'))
    e.close()
    return worst


def check_switch(lib_path, name, order, shape=(37, 53)):
    """each switch alone (and none, and all)"""
    e = small_engine(lib_path)
    c = case(shape[0], shape[1], order, name, 'float64')
    img, msk, bad = device_case(e, c)
    e.close()
    check_bad(bad, c, name)
    return compare(img, msk, c, f'switch {name} order {order}')


def check_reference_case(shape, order, switches, dtype):
    """no kernel: scipy itself and the float64 restatement stay below a quarter of the bound, masks as the device's must"""
    c = case(shape[0], shape[1], order, switches, dtype)
    r = c['r']
    compare(r['image'], r['mask'], c, f'{shape} order {order} {switches} {dtype}', 'r_resample', 0.25)
    si, sm = scipy_resample(c['images'], c['masks'], c['xs'], c['ys'], order, **c['kw'])
    assert sm.dtype.kind == 'i'
    compare(si, sm, c, f'{shape} order {order} {switches} {dtype}', 'scipy', 0.25)


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def g26_inputs(g, name):
    sw = G26_SETS[name]
    thr = tuple(g['G26_threshold']) if sw.get('thr') else None
    return {'thr': thr, 'binary': g['G26_binary'] if sw.get('bin') else None, 'background': g['G26_background'] if sw.get('bg') else None}


def check_restatement_golden(g):
    """r_resample against the reference's own process_image (G26): 1e-13 of the largest value, masks equal; the geometry the
    fixture was made with is polar_geometry's"""
    geo = CR.polar_geometry(g26_settings(g))
    assert np.array_equal(geo['cart_x'], g['G26_cart_x']) and np.array_equal(geo['cart_y'], g['G26_cart_y'])
    xs, ys = g['G26_cart_x'].ravel(), g['G26_cart_y'].ravel()
    for order in G26_ORDERS:
        for name in G26_SETS:
            r = r_resample(g['G26_images'], g['G26_masks'], xs, ys, order, **g26_inputs(g, name))
            for p in range(len(g['G26_images'])):
                tag = f'G26_o{order}_{name}_p{p}_'
                want = g[tag + 'image'].ravel()
                assert np.all(np.abs(r['image'][p] - want) <= TOL_GOLDEN * np.abs(want).max()), tag
                assert np.array_equal(r['mask'][p], g[tag + 'mask'].ravel()), tag


def g26_settings(g):
    H, W = g['G26_images'].shape[1:]
    return {'qrange': [0.0, float(g['G26_q_max']), float(g['G26_q_step'])], 'qrange_xcca': [[0.0, float(g['G26_q_max']), 1]] * 2,
            'phi_range': (0.0, 2 * np.pi, 16, 'exact'), 'image_dimensions': [int(H), int(W)],
            'detector_origin': [float(v) for v in g['G26_origin']], 'pixel_size': float(g['G26_pixel_size']),
            'sample_distance': float(g['G26_sample_distance']), 'wavelength': float(g['G26_wavelength'])}


def check_device_golden(g, lib_path=None):
    """Resampler on the fixture's settings against the reference's own outputs, at the bound"""
    e = small_engine(lib_path)
    images, masks = g['G26_images'], g['G26_masks']
    xs, ys = g['G26_cart_x'].ravel(), g['G26_cart_y'].ravel()
    for order in G26_ORDERS:
        for name, sw in G26_SETS.items():
            kw = g26_inputs(g, name)
            settings = dict(g26_settings(g), interpolation_order=order, use_binary_mask=bool(sw.get('bin')),
                            subtract_background=bool(sw.get('bg')),
                            intensity_pixel_threshold=[bool(sw.get('thr'))] + [float(v) for v in g['G26_threshold']])
            rs = CR.Resampler(e, settings, binary_mask=g['G26_binary'], background=g['G26_background'])
            img, msk = rs.run(images, masks)
            rs.close()
            x = x_resample(images, masks, xs, ys, order, **kw)
            worst = 0.0
            for p in range(len(images)):
                tag = f'G26_o{order}_{name}_p{p}_'
                # the fixture is float64 arithmetic itself: it sits within a quarter of the bound of the longdouble value (asserted)
                ref_err = np.abs((g[tag + 'image'].astype(np.longdouble) - x['image'][p].reshape(img.shape[1:])).astype(float)).max()
                b = float(bound(x, order)[p, 0])
                assert ref_err <= 0.25 * b, tag
                ratio = float(np.abs(img[p] - g[tag + 'image']).max() / b)
                worst = max(worst, ratio)
                assert ratio <= 1.0, (tag, ratio)
                assert np.array_equal(msk[p], g[tag + 'mask']), tag
            print(f'G26 order {order} {name}: device / bound {worst:.3f}')
    e.close()


def check_chunking(lib_path):
    """RS_CHUNK + 1 patterns of 20 x 24: one chunk plus one pattern, with per-pattern masks and with the static mask"""
    e = small_engine(lib_path)
    for sw in ('masks', 'background'):
        c = case(20, 24, 3, sw, 'float32', P=RS_CHUNK + 1, edges=False)
        img, msk, bad = device_case(e, c)
        check_bad(bad, c, sw)
        compare(img, msk, c, f'chunk {sw}')
    e.close()


def check_batch_independence(lib_path):
    """7 patterns as 7, 3 + 4 and 1 x 7: bit-identical"""
    e = small_engine(lib_path)
    c = case(37, 53, 5, 'all', 'float64', P=7, edges=False)
    outs = [device_case(e, c, splits=s) for s in ([7], [3, 4], [1] * 7)]
    e.close()
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1]) and o[2] == outs[0][2]
    check_bad(outs[0][2], c, 'batch independence')


def check_static_mask(lib_path):
    """no masks and the threshold off (the mask is resampled once per handle) against explicit masks of ones: bit-identical, with
    and without a binary mask; under the emulator the launch log shows the mask's filter running once"""
    import parity_cases as PC
    e = small_engine(lib_path)
    for sw in ('plain', 'binary'):
        c = case(37, 53, 2, sw, 'float64', P=5, edges=False)
        PC.launched_kernels(e, ('k_rs',))
        a = device_case(e, c, splits=[2, 3])
        log = PC.launched_kernels(e, ('k_rs',))
        ones = np.ones(c['images'].shape, np.uint8)
        b = device_run(e, 37, 53, 2, c['xs'], c['ys'], c['images'], ones, splits=[2, 3], **c['kw'])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] == 0
        compare(a[0], a[1], c, f'static mask {sw}')
        if log is not None:
            assert log == ('k_rs_cols', 'k_rs_rows', 'k_rs_gather') * 3, log
    e.close()


def check_host_device(lib_path):
    """numpy arrays and torch tensors on the engine's device through Resampler: identical"""
    import torch
    e = small_engine(lib_path)
    settings = detector_settings(37, 53, 8, 32, interpolation_order=3, intensity_pixel_threshold=[True, *THRESHOLD])
    images, masks, _, _ = make_frames(37, 53, 3, 5, np.float32)
    rs = CR.Resampler(e, settings)
    a = rs.run(images, masks)
    dev = e.torch_device()
    b = rs.run(torch.from_numpy(images).to(dev), torch.from_numpy(masks.astype(bool)).to(dev))
    one = rs.run(images, masks[0])
    rs.close()
    e.close()
    assert isinstance(a[0], np.ndarray) and isinstance(b[0], torch.Tensor) and b[1].dtype == torch.uint8
    assert np.array_equal(a[0], b[0].cpu().numpy()) and np.array_equal(a[1], b[1].cpu().numpy())
    assert np.array_equal(one[0][0], a[0][0]) and np.array_equal(one[1][0], a[1][0])     # one (H, W) mask is every pattern's


def detector_settings(H, W, n_q, n_phi, **top):
    """settings whose polar grid has n_q rings x n_phi angles around (H / 2 - 0.3, W / 2 + 0.21) and leaves the frame on its outer
    rings (pixel size 1 mm at 1 m: ring k has a radius of 1000 tan(theta_k) pixels)"""
    r_max = 0.62 * max(H, W)
    wavelength = 1.0
    q_max = 4 * np.pi / wavelength * np.sin(np.arctan(r_max / 1000.0) / 2)
    s = {'qrange': [0.0, q_max, q_max / (n_q - 1) * (1 - 1e-12)], 'qrange_xcca': [[0.0, q_max, 1], [0.0, q_max, 1]],
         'phi_range': (0.0, 2 * np.pi, n_phi, 'exact'), 'image_dimensions': [H, W], 'detector_origin': [H / 2 - 0.3, W / 2 + 0.21],
         'pixel_size': 1000.0, 'sample_distance': 1000.0, 'wavelength': wavelength, 'compute': ['is_good', 'waxs_aver', 'ccf_q1q2']}
    s.update(top)
    return s


def check_add_detector(lib_path):
    """Correlator.add_detector: bit-identical to add of Resampler.run's output; agrees with add of the scipy-resampled patterns under
    correlate_cases.compare_partial at 37 x 53 -> 8 x 32; a shared_mask handle takes it with a static mask and refuses the threshold"""
    import pytest
    import correlate_cases as CO
    H, W, n_q, n_phi, P = 37, 53, 8, 32, 4
    images, masks, binary, background = make_frames(H, W, P, 11, np.float64)
    images += 50.0                                                                        # (keeps every ring's pair counts positive)
    e = small_engine(lib_path)
    for sw in ('plain', 'all'):
        top = {'interpolation_order': 2}
        cm = None
        if sw == 'all':
            top.update(intensity_pixel_threshold=[True, 80.0, 1e4], use_binary_mask=True, subtract_background=True)
            cm = masks
        settings = detector_settings(H, W, n_q, n_phi, **top)
        geo = CR.polar_geometry(settings)
        assert (geo['n_q'], geo['n_phi']) == (n_q, n_phi)
        a = CR.Correlator(e, settings, binary_mask=binary, background=background)
        a.add_detector(images[:1], None if cm is None else cm[:1]).add_detector(images[1:], None if cm is None else cm[1:])
        rs = CR.Resampler(e, settings, binary_mask=binary, background=background)
        pol_i, pol_m = rs.run(images, cm)
        rs.close()
        assert 0.05 < np.mean(pol_m == 0) < 0.6
        b = CR.Correlator(e, settings)
        b.add(pol_i, pol_m)
        pa, pb = a.partial(), b.partial()
        a.close()
        b.close()
        for k in pa:
            assert np.array_equal(pa[k], pb[k], equal_nan=True), (sw, k)
        kw = switch_kwargs(sw, masks, binary, background)[1]
        if kw['thr'] is not None:
            kw['thr'] = (80.0, 1e4)
        si, sm = scipy_resample(images, cm, geo['cart_x'].ravel(), geo['cart_y'].ravel(), 2, **kw)
        si, sm = si.reshape(P, n_q, n_phi), sm.reshape(P, n_q, n_phi)
        assert np.array_equal(sm, pol_m)
        x = CO.x_correlate(si, sm, CO.params(settings))
        CO.compare_partial(pa, x, f'add_detector {sw} against add of scipy patterns')
    settings = detector_settings(H, W, n_q, n_phi, use_binary_mask=True)
    s = CR.Correlator(e, settings, shared_mask=True, binary_mask=binary)
    s.add_detector(images[:2]).add_detector(images[2:])
    u = CR.Correlator(e, settings, binary_mask=binary)
    u.add_detector(images)
    ps, pu = s.partial(), u.partial()
    for k in ps:
        assert np.array_equal(ps[k], pu[k], equal_nan=True), k
    with pytest.raises(ValueError, match='shared_mask'):
        s.add_detector(images, masks)
    assert s.num_patterns == P
    s.close()
    u.close()
    t = CR.Correlator(e, dict(settings, intensity_pixel_threshold=[True, 80.0, 1e4]), shared_mask=True, binary_mask=binary)
    with pytest.raises(ValueError, match='shared_mask.*intensity_pixel_threshold'):
        t.add_detector(images)
    assert t.num_patterns == 0
    t.close()
    e.close()


def overshoot_mask(H, W, order, i0, j0):
    """a 0 / 1 mask whose spline interpolant exceeds 1.5 at (i0 + 0.5, j0 + 0.5): ones where the cardinal spline of that point is
    positive, so the value there is the sum of the positive cardinal values, (1 + Lebesgue function) / 2"""
    xs, ys = np.array([i0 + 0.5]), np.array([j0 + 0.5])
    card = np.zeros((H, W), np.longdouble)
    for i in range(H):
        for j in range(W):
            d = np.zeros((1, H, W))
            d[0, i, j] = 1.0
            card[i, j] = interpolate(spline_coefficients(d, order, np.longdouble), xs, ys, order, np.longdouble)[0][0, 0]
    return (card > 0).astype(np.int64), float(card[card > 0].sum())


def check_raises(lib_path):
    """what is not built raises and names itself; bad inputs raise; a polar mask value of 2 raises the ValueError of add"""
    import pytest
    e = small_engine(lib_path)
    settings = detector_settings(20, 24, 8, 16)
    with pytest.raises(NotImplementedError, match='interpolation_order = 6'):
        CR.Resampler(e, dict(settings, interpolation_order=6))
    with pytest.raises(NotImplementedError, match='1 x 24'):
        CR.Resampler(e, dict(settings, image_dimensions=[1, 24]))
    for order, dims in ((6, (20, 24)), (-1, (20, 24)), (2, (1, 24)), (2, (20, 4097))):
        cfg = _lib.MtipResampleCfg(dims[0], dims[1], order, 0, 0, 0, 4, 0.0, 0.0)
        pts = np.ones(4)
        assert not e.lib.mtip_resample_create(e.ctx, ctypes.byref(cfg), _lib.ptr(pts), _lib.ptr(pts), None, None)
        assert 'supported' in e.lib.mtip_last_error(e.ctx).decode()
    with pytest.raises(ValueError, match='use_binary_mask'):
        CR.Resampler(e, dict(settings, use_binary_mask=True))
    rs = CR.Resampler(e, settings)
    images, masks, _, _ = make_frames(20, 24, 2, 3)
    with pytest.raises(ValueError, match='shape'):
        rs.run(images[:, :19])
    with pytest.raises(ValueError, match='shape'):
        rs.run(images, masks[:, :, :23])
    for bad in (masks * 2, masks - 1, masks + 0.5):
        with pytest.raises(ValueError, match='0 / 1'):
            rs.run(images, bad)
    with pytest.raises(TypeError):
        rs.run(images.astype(np.int32))
    rs.close()
    # a polar mask value other than 0 / 1: the interpolant of a 0 / 1 mask overshoots past 1.5 at order 3 (proved in longdouble)
    H, W, order = 12, 12, 3
    mask, value = overshoot_mask(H, W, order, 5, 5)
    assert value > 1.5 + 1e-6, value
    xs, ys = np.array([5.5, 2.0]), np.array([5.5, 3.0])
    frames = np.ones((1, H, W))
    assert round_half_away(x_resample(frames, mask[None], xs, ys, order)['mask_value'])[0, 0] == 2
    _, msk, bad = device_run(e, H, W, order, xs, ys, frames, mask[None])
    assert bad == 1 and msk[0, 0] == 2 and msk[0, 1] in (0, 1)
    s2 = detector_settings(H, W, 8, 16, interpolation_order=order, detector_origin=[5.5, 5.5])
    c = CR.Correlator(e, s2)
    assert c.geometry['cart_x'][0, 0] == 5.5 and c.geometry['cart_y'][0, 0] == 5.5      # ring 0 sits on the overshoot
    with pytest.raises(ValueError, match='0 / 1'):
        c.add_detector(frames, mask[None])
    assert c.num_patterns == 0 and not np.any(c.partial()['count'])
    c.resampler.close()
    rs = CR.Resampler(e, s2)
    with pytest.raises(ValueError, match='0 / 1'):
        rs.run(frames, mask[None])
    rs.close()
    c.close()
    e.close()


def check_read_raw_images(tmp_path):
    """read_raw_images: little-endian float32, NaN -> 0, a wrong length raises"""
    import pytest
    a = np.arange(12, dtype='<f4').reshape(3, 4)
    a[1, 2] = np.nan
    paths = []
    for k in range(2):
        p = os.path.join(str(tmp_path), f'frame{k}.raw')
        (a + k).astype('<f4').tofile(p)
        paths.append(p)
    out = CR.read_raw_images(paths, (3, 4))
    want = np.nan_to_num(np.stack([a, a + 1]), nan=0.0)
    assert out.dtype == np.float32 and out.shape == (2, 3, 4) and np.array_equal(out, want)
    with pytest.raises(ValueError, match='12'):
        CR.read_raw_images(paths[0], (3, 5))


GUARD_SCRIPT = r'''
import sys
sys.path.insert(0, {tests!r})
sys.path.insert(0, {root!r})
import resample_cases as RC
for shape in ((4, 5), (37, 53)):
    for order in RC.ORDERS:
        RC.check_shape_order({lib!r}, shape, order)
print('guarded run complete')
'''

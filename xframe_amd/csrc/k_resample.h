// correlate, the Cartesian stage: detector frames -> polar patterns  (gfx950, fp64)
//   xframe/projects/fxs/correlate.py:377-398   process_image up to the two map_coordinates calls
// Included by k_extract.hip behind k_correlate.h (mtip_correlate_add_detector hands its output to mtip_correlate_add on the device).
// scipy.ndimage.map_coordinates(order, mode='constant', cval=0, prefilter=True) is restated as
//   k_rs_cols     B-spline prefilter along axis 0: one thread per column, neighbouring threads read neighbouring columns.  Its first
//                 pass loads THROUGH the preparation (threshold, binary mask, background, image *= mask): no pass of its own.
//   k_rs_rows     the same filter along axis 1: a workgroup owns RS_RT rows and moves them through an LDS tile of RS_TW columns, so
//                 global memory is read and written along the rows while every thread walks its own row in LDS.
//   k_rs_prep     orders 0 and 1 have no prefilter: the preparation alone
//   k_rs_gather   one point per thread: (order + 1)^2 taps at mirrored indices, B-spline weights by the uniform-knot recurrence,
//                 zero outside the frame; the image as float64, the mask rounded half away from zero as uint8, straight into
//                 the (P, n_points) layout mtip_correlate_add reads; rounded mask values other than 0 / 1 are counted.
// Each pole is a causal and an anticausal recursion with the mirror boundary (whole-sample symmetry, period 2 N - 2).  The causal
// start is the exact sum over the whole mirrored line,  c+[0] = (sum_i z^i s[i] + z^(N-1) sum_{0<i<N-1} z^(N-1-i) s[i]) / (1 - z^(2N-2)),
// taken in a pass of its own (a forward power sum and a Horner sum), never a truncated horizon.
// Image and mask coefficients of RS_CHUNK patterns are the working memory.  Where the threshold is off and the caller gives no masks
// the Cartesian mask is the same for every pattern: it is filtered and gathered once per handle by the same kernels (bit-identical).
#pragma once

#define RS_MAX_ORDER 5
#define RS_MIN_DIM 2                   // a line of one sample has no mirror period
#define RS_MAX_DIM 4096
#define RS_CHUNK COR_CHUNK             // patterns per pass: the chunk the correlation behind it takes
#define RS_CT 64                       // columns per workgroup of k_rs_cols (one thread per line)
#define RS_SEG 16                      // samples of a column that go through registers together
#define RS_RT 64                       // rows per workgroup of k_rs_rows
#define RS_TW 32                       // columns of its LDS tile
#define RS_TP (RS_TW + 1)              // padded row length of the tile: the threads of a wave walk one column of it
#define RS_GT 256                      // points per workgroup of k_rs_gather

struct RsSrc {
    const void* img;                   // (P, H, W) float or double; null: only the mask is asked for (static mask)
    const uint8_t* mask;               // (P, H, W) caller's initial masks, or null: ones
    const uint8_t* bin;                // (H, W) or null
    const double* bg;                  // (H, W) or null
    int thr_on;
    double lo, hi;
};

// process_image 382-392 for one pixel: arr 0 the image, 1 the mask
template <typename T>
__device__ __forceinline__ double rs_src(const RsSrc& s, int arr, size_t pix, size_t ij) {
    const double raw = s.img ? (double)((const T*)s.img)[pix] : 0.0;
    int m = s.mask ? (s.mask[pix] != 0 ? 1 : 0) : 1;
    if (s.thr_on && (raw < s.lo || raw > s.hi)) m = 0;                  // 383: on the raw image
    if (s.bin && s.bin[ij] == 0) m = 0;                                 // 385, the evident intent: mask *= (binary_mask != 0)
    if (arr) return (double)m;
    double v = raw;
    if (s.bg) v -= s.bg[ij];                                            // 389
    return v * (double)m;                                               // 392
}

struct RsArgs {
    RsSrc src;
    double* coef[2];                   // (patterns, H, W) image and mask coefficients
    int H, W, arr0, narr;              // blockIdx.y = pattern * narr + (array - arr0)
    double z[2], zn[2], gain;          // poles, z^(N - 1) of this axis, prod (1 - z)(1 - 1 / z)
};

template <typename T>
__global__ void __launch_bounds__(RS_GT) k_rs_prep(RsArgs a) {
    const size_t frame = (size_t)a.H * a.W, ij = (size_t)blockIdx.x * RS_GT + threadIdx.x;
    if (ij >= frame) return;
    const int arr = a.arr0 + (int)(blockIdx.y % a.narr);
    const size_t p = blockIdx.y / a.narr;
    a.coef[arr][p * frame + ij] = rs_src<T>(a.src, arr, p * frame + ij, ij);
}

// RS_SEG samples of one column into registers: the loads of a segment are issued together and do not depend on the recursion
template <bool FIRST, typename T>
__device__ __forceinline__ void rs_col_load(const RsArgs& a, int arr, const double* c, size_t pix0, size_t W, int j, int i0, double* v) {
#pragma unroll
    for (int u = 0; u < RS_SEG; ++u) {
        const size_t off = (size_t)(i0 + u) * W;
        v[u] = FIRST ? a.gain * rs_src<T>(a.src, arr, pix0 + off, off + j) : c[off];
    }
}

template <bool FIRST, typename T>
__device__ __forceinline__ double rs_col_load1(const RsArgs& a, int arr, const double* c, size_t pix0, size_t W, int j, int i) {
    const size_t off = (size_t)i * W;
    return FIRST ? a.gain * rs_src<T>(a.src, arr, pix0 + off, off + j) : c[off];
}

// one pole along one column: the mirror start over the whole line, the causal pass, the anticausal pass; whole segments of RS_SEG
// samples go through registers, the rest of the line one by one
template <bool FIRST, typename T>
__device__ __forceinline__ void rs_col_pole(const RsArgs& a, int arr, double* c, size_t pix0, int j, double z, double zn) {
    const int H = a.H, full = H - H % RS_SEG;
    const size_t W = (size_t)a.W;
    double v[RS_SEG];
    double A = 0.0, B = 0.0, zi = 1.0;
    for (int i0 = 0; i0 < full; i0 += RS_SEG) {
        rs_col_load<FIRST, T>(a, arr, c, pix0, W, j, i0, v);
#pragma unroll
        for (int u = 0; u < RS_SEG; ++u) {
            A += zi * v[u];
            zi *= z;
            B = (i0 + u >= 1 && i0 + u <= H - 2) ? B * z + v[u] : B;
        }
    }
    for (int i = full; i < H; ++i) {
        const double s = rs_col_load1<FIRST, T>(a, arr, c, pix0, W, j, i);
        A += zi * s;
        zi *= z;
        B = (i >= 1 && i <= H - 2) ? B * z + s : B;
    }
    const double c0 = (A + zn * z * B) / (1.0 - zn * zn);
    double prev = 0.0, prev2 = 0.0;
    for (int i0 = 0; i0 < full; i0 += RS_SEG) {
        rs_col_load<FIRST, T>(a, arr, c, pix0, W, j, i0, v);
#pragma unroll
        for (int u = 0; u < RS_SEG; ++u) {
            prev2 = prev;
            prev = i0 + u == 0 ? c0 : v[u] + z * prev;
            v[u] = prev;
        }
#pragma unroll
        for (int u = 0; u < RS_SEG; ++u) c[(size_t)(i0 + u) * W] = v[u];
    }
    for (int i = full; i < H; ++i) {
        const double s = rs_col_load1<FIRST, T>(a, arr, c, pix0, W, j, i);
        prev2 = prev;
        prev = i == 0 ? c0 : s + z * prev;
        c[(size_t)i * W] = prev;
    }
    const double last = (z * prev2 + prev) * z / (z * z - 1.0);
    double nxt = 0.0;
    for (int i = H - 1; i >= full; --i) {
        nxt = i == H - 1 ? last : z * (nxt - c[(size_t)i * W]);
        c[(size_t)i * W] = nxt;
    }
    for (int i0 = full - RS_SEG; i0 >= 0; i0 -= RS_SEG) {
        rs_col_load<false, T>(a, arr, c, pix0, W, j, i0, v);
#pragma unroll
        for (int u = RS_SEG - 1; u >= 0; --u) {
            nxt = i0 + u == H - 1 ? last : z * (nxt - v[u]);
            v[u] = nxt;
        }
#pragma unroll
        for (int u = 0; u < RS_SEG; ++u) c[(size_t)(i0 + u) * W] = v[u];
    }
}

template <int NPOLE, typename T>
__global__ void __launch_bounds__(RS_CT) k_rs_cols(RsArgs a) {
    const int j = blockIdx.x * RS_CT + threadIdx.x;
    if (j >= a.W) return;                                               // (no barrier in this kernel)
    const int arr = a.arr0 + (int)(blockIdx.y % a.narr);
    const size_t pix0 = (size_t)(blockIdx.y / a.narr) * a.H * a.W + j;
    double* c = a.coef[arr] + pix0;
    rs_col_pole<true, T>(a, arr, c, pix0, j, a.z[0], a.zn[0]);
    if (NPOLE > 1) rs_col_pole<false, T>(a, arr, c, pix0, j, a.z[1], a.zn[1]);
}

__device__ __forceinline__ void rs_tile_load(double* s_t, const double* c, int row0, int j0, int H, int W, double g, int tid) {
    for (int e = tid; e < RS_RT * RS_TW; e += RS_RT) {
        const int r = e / RS_TW, cc = e % RS_TW;
        s_t[r * RS_TP + cc] = (row0 + r < H && j0 + cc < W) ? g * c[(size_t)(row0 + r) * W + j0 + cc] : 0.0;
    }
}

__device__ __forceinline__ void rs_tile_store(const double* s_t, double* c, int row0, int j0, int H, int W, int tid) {
    for (int e = tid; e < RS_RT * RS_TW; e += RS_RT) {
        const int r = e / RS_TW, cc = e % RS_TW;
        if (row0 + r < H && j0 + cc < W) c[(size_t)(row0 + r) * W + j0 + cc] = s_t[r * RS_TP + cc];
    }
}

template <int NPOLE>
__global__ void __launch_bounds__(RS_RT) k_rs_rows(RsArgs a) {
    __shared__ double s_t[RS_RT * RS_TP];
    const int tid = threadIdx.x, row0 = blockIdx.x * RS_RT, H = a.H, W = a.W;
    const bool active = row0 + tid < H;
    const int arr = a.arr0 + (int)(blockIdx.y % a.narr), ntile = (W + RS_TW - 1) / RS_TW;
    double* c = a.coef[arr] + (size_t)(blockIdx.y / a.narr) * H * W;
    double* mine = s_t + tid * RS_TP;
#pragma unroll
    for (int k = 0; k < NPOLE; ++k) {
        const double z = a.z[k], zn = a.zn[k], g = k == 0 ? a.gain : 1.0;
        double A = 0.0, B = 0.0, zi = 1.0;
        for (int t = 0; t < ntile; ++t) {
            const int j0 = t * RS_TW, cnt = min(RS_TW, W - j0);
            rs_tile_load(s_t, c, row0, j0, H, W, g, tid);
            __syncthreads();
            if (active)
                for (int cc = 0; cc < cnt; ++cc) {
                    const int j = j0 + cc;
                    const double s = mine[cc];
                    A += zi * s;
                    zi *= z;
                    if (j >= 1 && j <= W - 2) B = B * z + s;
                }
            __syncthreads();
        }
        double prev = (A + zn * z * B) / (1.0 - zn * zn), prev2 = 0.0;
        for (int t = 0; t < ntile; ++t) {
            const int j0 = t * RS_TW, cnt = min(RS_TW, W - j0);
            rs_tile_load(s_t, c, row0, j0, H, W, g, tid);
            __syncthreads();
            if (active)
                for (int cc = 0; cc < cnt; ++cc) {
                    if (j0 + cc > 0) {
                        prev2 = prev;
                        prev = mine[cc] + z * prev;
                    }
                    mine[cc] = prev;
                }
            __syncthreads();
            rs_tile_store(s_t, c, row0, j0, H, W, tid);
            __syncthreads();
        }
        double nxt = (z * prev2 + prev) * z / (z * z - 1.0);
        for (int t = ntile - 1; t >= 0; --t) {
            const int j0 = t * RS_TW, cnt = min(RS_TW, W - j0);
            rs_tile_load(s_t, c, row0, j0, H, W, 1.0, tid);
            __syncthreads();
            if (active)
                for (int cc = cnt - 1; cc >= 0; --cc) {
                    if (j0 + cc < W - 1) nxt = z * (nxt - mine[cc]);
                    mine[cc] = nxt;
                }
            __syncthreads();
            rs_tile_store(s_t, c, row0, j0, H, W, tid);
            __syncthreads();
        }
    }
}

// an index beyond the edges through the mirror (period 2 n - 2), as often as it takes
__device__ __forceinline__ int rs_mirror(int i, int n) {
    const int per = 2 * n - 2;
    i %= per;
    if (i < 0) i += per;
    return i < n ? i : per - i;
}

// the ORDER + 1 taps of one axis: mirrored indices and the values of the centred cardinal B-spline.  Odd orders have their knots at
// the samples, even orders midway between them; either way x = knot + t with 0 <= t < 1, and the uniform-knot recurrence
// (de Boor: every denominator of degree j is j) gives the non-zero splines from the leftmost on.
template <int ORDER>
__device__ __forceinline__ void rs_taps(double x, int n, int* idx, double* w) {
    const double f = (ORDER & 1) ? floor(x) : floor(x + 0.5);
    const double t = (ORDER & 1) ? x - f : (x - f) + 0.5;
    const int start = (int)f - ORDER / 2;
    w[0] = 1.0;
#pragma unroll
    for (int j = 1; j <= ORDER; ++j) {
        const double inv = 1.0 / (double)j;
        double saved = 0.0;
#pragma unroll
        for (int r = 0; r < j; ++r) {
            const double term = w[r] * inv;
            w[r] = saved + ((double)(r + 1) - t) * term;
            saved = (t + (double)(j - r - 1)) * term;
        }
        w[j] = saved;
    }
#pragma unroll
    for (int r = 0; r <= ORDER; ++r) idx[r] = rs_mirror(start + r, n);
}

struct RsGatherArgs {
    const double* ci;                  // (P, H, W) image coefficients, or null
    const double* cm;                  // (P or 1, H, W) mask coefficients, or null: the mask comes from mstat
    size_t cm_stride;
    const uint8_t* mstat;              // (n_points) the static mask's polar values
    const double *x, *y;               // (n_points) coordinates along axis 0 and axis 1
    double* out_img;                   // (P, n_points) or null
    uint8_t* out_mask;                 // (P, n_points)
    int* bad;
    int H, W;
    long long n_points;
};

template <int ORDER>
__global__ void __launch_bounds__(RS_GT) k_rs_gather(RsGatherArgs a) {
    const long long pt = (long long)blockIdx.x * RS_GT + threadIdx.x;
    if (pt >= a.n_points) return;
    const size_t p = blockIdx.y, frame = (size_t)a.H * a.W;
    const double x = a.x[pt], y = a.y[pt];
    double vi = 0.0, vm = 0.0;
    if (x >= 0.0 && x <= (double)(a.H - 1) && y >= 0.0 && y <= (double)(a.W - 1)) {   // both ends inclusive; a NaN is outside
        int ix[ORDER + 1], iy[ORDER + 1];
        double wx[ORDER + 1], wy[ORDER + 1];
        rs_taps<ORDER>(x, a.H, ix, wx);
        rs_taps<ORDER>(y, a.W, iy, wy);
        const double* ci = a.ci ? a.ci + p * frame : nullptr;
        const double* cm = a.cm ? a.cm + p * a.cm_stride : nullptr;
#pragma unroll
        for (int r = 0; r <= ORDER; ++r) {
            const size_t row = (size_t)ix[r] * a.W;
            double si = 0.0, sm = 0.0;
#pragma unroll
            for (int s = 0; s <= ORDER; ++s) {
                if (ci) si += wy[s] * ci[row + iy[s]];
                if (cm) sm += wy[s] * cm[row + iy[s]];
            }
            vi += wx[r] * si;
            vm += wx[r] * sm;
        }
    }
    if (a.out_img) a.out_img[p * (size_t)a.n_points + pt] = vi;
    int r;
    if (a.cm) r = (int)(vm < 0.0 ? vm - 0.5 : vm + 0.5);                // an integer output array: rounded half away from zero
    else r = (int)(int8_t)a.mstat[pt];
    if (r != 0 && r != 1) atomicAdd(a.bad, 1);
    a.out_mask[p * (size_t)a.n_points + pt] = (uint8_t)r;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
struct mtip_resample {
    mtip_ctx* c = nullptr;
    mtip_resample_cfg cfg{};
    int npole = 0;
    double z[2] = {0.0, 0.0}, zn_h[2] = {0.0, 0.0}, zn_w[2] = {0.0, 0.0}, gain = 1.0;
    DevBuf<double> d_x, d_y, d_bg;
    DevBuf<uint8_t> d_bin;
    DevBuf<double> d_ci;               // (RS_CHUNK, H, W)
    DevBuf<double> d_cm;               // (RS_CHUNK, H, W), allocated by the first batch with per-pattern masks
    DevBuf<double> d_cms;              // (H, W) the static mask's coefficients
    DevBuf<uint8_t> d_mstat;           // (n_points) its polar values
    bool have_static = false;
    DevBuf<int> d_bad;                 // [0] of the batch, [1] of the static set-up
};

extern "C" mtip_resample* mtip_resample_create(mtip_ctx* c, const mtip_resample_cfg* cfg, const double* cart_x, const double* cart_y,
                                               const uint8_t* binary_mask, const double* background) {
    if (!c) return nullptr;
    char msg[400];
    if (!cfg || !cart_x || !cart_y || cfg->n_points < 1 || (cfg->has_binary_mask && !binary_mask) || (cfg->has_background && !background)) {
        c->err = "resample_create: null argument or no point";
        return nullptr;
    }
    if (cfg->order < 0 || cfg->order > RS_MAX_ORDER) {
        snprintf(msg, sizeof msg, "resample_create: interpolation order %d is not built; supported: 0 .. %d", cfg->order, RS_MAX_ORDER);
        c->err = msg;
        return nullptr;
    }
    if (cfg->H < RS_MIN_DIM || cfg->H > RS_MAX_DIM || cfg->W < RS_MIN_DIM || cfg->W > RS_MAX_DIM) {
        snprintf(msg, sizeof msg, "resample_create: frames of %d x %d are not built; supported: %d .. %d along either axis", cfg->H, cfg->W,
                 RS_MIN_DIM, RS_MAX_DIM);
        c->err = msg;
        return nullptr;
    }
    (void)hipSetDevice(c->device);
    const size_t frame = (size_t)cfg->H * cfg->W, np = (size_t)cfg->n_points;
    const size_t need = frame * 8 * (2 * RS_CHUNK + 2) + frame + np * 17, fr = mtip_free_memory();
    if (need > fr) {
        snprintf(msg, sizeof msg, "resample_create: %d patterns of %d x %d coefficients need %.3f GB; %.3f GB of device memory are free",
                 RS_CHUNK, cfg->H, cfg->W, (double)need * 1e-9, (double)fr * 1e-9);
        c->err = msg;
        return nullptr;
    }
    mtip_resample* r = new mtip_resample;
    r->c = c;
    r->cfg = *cfg;
    // the poles of the B-spline prefilter (Unser, Aldroubi, Eden 1993), in long double
    long double zl[2] = {0.0L, 0.0L};
    if (cfg->order == 2) zl[0] = sqrtl(8.0L) - 3.0L;
    if (cfg->order == 3) zl[0] = sqrtl(3.0L) - 2.0L;
    if (cfg->order == 4) {
        zl[0] = sqrtl(664.0L - sqrtl(438976.0L)) + sqrtl(304.0L) - 19.0L;
        zl[1] = sqrtl(664.0L + sqrtl(438976.0L)) - sqrtl(304.0L) - 19.0L;
    }
    if (cfg->order == 5) {
        zl[0] = sqrtl(67.5L - sqrtl(4436.25L)) + sqrtl(26.25L) - 6.5L;
        zl[1] = sqrtl(67.5L + sqrtl(4436.25L)) - sqrtl(26.25L) - 6.5L;
    }
    r->npole = cfg->order < 2 ? 0 : (cfg->order < 4 ? 1 : 2);
    long double gain = 1.0L;
    for (int k = 0; k < r->npole; ++k) {
        r->z[k] = (double)zl[k];
        r->zn_h[k] = (double)powl(zl[k], (long double)(cfg->H - 1));
        r->zn_w[k] = (double)powl(zl[k], (long double)(cfg->W - 1));
        gain *= (1.0L - zl[k]) * (1.0L - 1.0L / zl[k]);
    }
    r->gain = (double)gain;
    hipError_t e = r->d_x.alloc(np);
    if (e == hipSuccess) e = r->d_y.alloc(np);
    if (e == hipSuccess) e = r->d_ci.alloc(frame * RS_CHUNK);
    if (e == hipSuccess) e = r->d_bad.alloc(2);
    if (e == hipSuccess && cfg->has_binary_mask) e = r->d_bin.alloc(frame);
    if (e == hipSuccess && cfg->has_background) e = r->d_bg.alloc(frame);
    if (e == hipSuccess) e = mtip_copy(c, r->d_x, cart_x, np * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = mtip_copy(c, r->d_y, cart_y, np * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && cfg->has_binary_mask) e = mtip_copy(c, r->d_bin, binary_mask, frame, hipMemcpyHostToDevice);
    if (e == hipSuccess && cfg->has_background) e = mtip_copy(c, r->d_bg, background, frame * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        c->err = std::string("resample_create: ") + hipGetErrorString(e);
        delete r;
        return nullptr;
    }
    return r;
}

extern "C" void mtip_resample_destroy(mtip_resample* r) {
    if (!r) return;
    (void)hipSetDevice(r->c->device);
    (void)hipStreamSynchronize(r->c->stream);
    delete r;
}

// the Cartesian mask does not depend on the pattern
static inline bool rs_static(const mtip_resample* r, const uint8_t* masks) { return !r->cfg.threshold_on && masks == nullptr; }

// preparation and prefilter of pc patterns: arrays arr0 .. arr0 + narr - 1 into a.coef
static inline void rs_filter(mtip_resample* r, RsArgs a, int pc, bool f32) {
    mtip_ctx* c = r->c;
    const int H = r->cfg.H, W = r->cfg.W;
    const unsigned ny = (unsigned)(pc * a.narr);
    a.H = H;
    a.W = W;
    a.gain = r->gain;
    for (int k = 0; k < 2; ++k) a.z[k] = r->z[k];
    ProfScope ps(c, "rs_filter");
    if (r->npole == 0) {
        const dim3 g((unsigned)div_up((long long)H * W, RS_GT), ny), b(RS_GT);
        if (f32) hipLaunchKernelGGL(k_rs_prep<float>, g, b, 0, c->stream, a);
        else hipLaunchKernelGGL(k_rs_prep<double>, g, b, 0, c->stream, a);
        return;
    }
    for (int k = 0; k < 2; ++k) a.zn[k] = r->zn_h[k];
    const dim3 gc((unsigned)div_up(W, RS_CT), ny), bc(RS_CT);
    if (r->npole == 1) {
        if (f32) hipLaunchKernelGGL((k_rs_cols<1, float>), gc, bc, 0, c->stream, a);
        else hipLaunchKernelGGL((k_rs_cols<1, double>), gc, bc, 0, c->stream, a);
    } else {
        if (f32) hipLaunchKernelGGL((k_rs_cols<2, float>), gc, bc, 0, c->stream, a);
        else hipLaunchKernelGGL((k_rs_cols<2, double>), gc, bc, 0, c->stream, a);
    }
    for (int k = 0; k < 2; ++k) a.zn[k] = r->zn_w[k];
    const dim3 gr((unsigned)div_up(H, RS_RT), ny), br(RS_RT);
    if (r->npole == 1) hipLaunchKernelGGL(k_rs_rows<1>, gr, br, 0, c->stream, a);
    else hipLaunchKernelGGL(k_rs_rows<2>, gr, br, 0, c->stream, a);
}

static inline void rs_gather(mtip_resample* r, const RsGatherArgs& g, int pc) {
    mtip_ctx* c = r->c;
    const dim3 grid((unsigned)div_up(g.n_points, RS_GT), (unsigned)pc), b(RS_GT);
    ProfScope ps(c, "rs_gather");
    switch (r->cfg.order) {
        case 0: hipLaunchKernelGGL(k_rs_gather<0>, grid, b, 0, c->stream, g); break;
        case 1: hipLaunchKernelGGL(k_rs_gather<1>, grid, b, 0, c->stream, g); break;
        case 2: hipLaunchKernelGGL(k_rs_gather<2>, grid, b, 0, c->stream, g); break;
        case 3: hipLaunchKernelGGL(k_rs_gather<3>, grid, b, 0, c->stream, g); break;
        case 4: hipLaunchKernelGGL(k_rs_gather<4>, grid, b, 0, c->stream, g); break;
        default: hipLaunchKernelGGL(k_rs_gather<5>, grid, b, 0, c->stream, g); break;
    }
}

// every pointer is device memory; the stream is synchronised when this returns without an error
static inline hipError_t rs_run(mtip_resample* r, int P, const void* images, bool f32, const uint8_t* masks, double* out_img, uint8_t* out_mask,
                                int64_t* n_bad) {
    mtip_ctx* c = r->c;
    const mtip_resample_cfg& f = r->cfg;
    const size_t frame = (size_t)f.H * f.W, np = (size_t)f.n_points;
    const bool stat = rs_static(r, masks);
    hipError_t e = hipMemsetAsync(r->d_bad, 0, 2 * sizeof(int), c->stream);
    RsArgs a{};
    a.src.bin = r->d_bin;
    a.src.bg = r->d_bg;
    a.src.thr_on = f.threshold_on;
    a.src.lo = f.threshold_lo;
    a.src.hi = f.threshold_hi;
    RsGatherArgs g{};
    g.x = r->d_x;
    g.y = r->d_y;
    g.H = f.H;
    g.W = f.W;
    g.n_points = f.n_points;
    if (e == hipSuccess && stat && !r->have_static) {
        e = r->d_cms.alloc(frame);
        if (e == hipSuccess) e = r->d_mstat.alloc(np);
        if (e == hipSuccess) {
            RsArgs am = a;
            am.coef[1] = r->d_cms;
            am.arr0 = 1;
            am.narr = 1;
            rs_filter(r, am, 1, false);
            RsGatherArgs gm = g;
            gm.cm = r->d_cms;
            gm.out_mask = r->d_mstat;
            gm.bad = r->d_bad + 1;
            rs_gather(r, gm, 1);
            r->have_static = true;
        }
    }
    if (e == hipSuccess && !stat && !r->d_cm) e = r->d_cm.alloc(frame * RS_CHUNK);
    const size_t px = f32 ? sizeof(float) : sizeof(double);
    for (int p0 = 0; e == hipSuccess && p0 < P; p0 += RS_CHUNK) {
        const int pc = std::min(RS_CHUNK, P - p0);
        a.src.img = (const char*)images + (size_t)p0 * frame * px;
        a.src.mask = masks ? masks + (size_t)p0 * frame : nullptr;
        a.coef[0] = r->d_ci;
        a.coef[1] = r->d_cm;
        a.arr0 = 0;
        a.narr = stat ? 1 : 2;
        rs_filter(r, a, pc, f32);
        g.ci = r->d_ci;
        g.cm = stat ? nullptr : (const double*)r->d_cm;
        g.cm_stride = frame;
        g.mstat = stat ? (const uint8_t*)r->d_mstat : nullptr;
        g.out_img = out_img + (size_t)p0 * np;
        g.out_mask = out_mask + (size_t)p0 * np;
        g.bad = r->d_bad;
        rs_gather(r, g, pc);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    int bad[2] = {0, 0};
    if (e == hipSuccess) e = mtip_copy(c, bad, r->d_bad, sizeof bad, hipMemcpyDeviceToHost);
    if (n_bad) *n_bad = (int64_t)bad[0];
    return e;
}

static inline int rs_check(mtip_resample* r, int n_patterns, const void* images, const char* who) {
    if (n_patterns < 1 || !images) {
        r->c->err = std::string(who) + ": null buffer or no pattern";
        return MTIP_EINVAL;
    }
    return MTIP_OK;
}

extern "C" int mtip_resample_run(mtip_resample* r, int n_patterns, const void* images, int is_float32, const uint8_t* masks, double* images_out,
                                 uint8_t* masks_out, int64_t* n_bad_mask) {
    if (!r) return MTIP_EINVAL;
    mtip_ctx* c = r->c;
    if (rs_check(r, n_patterns, images, "resample_run") != MTIP_OK) return MTIP_EINVAL;
    if (!images_out || !masks_out) {
        c->err = "resample_run: null output buffer";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    const size_t frame = (size_t)r->cfg.H * r->cfg.W, np = (size_t)r->cfg.n_points, P = (size_t)n_patterns;
    DevView v_img(c, images, P * frame * (is_float32 ? sizeof(float) : sizeof(double)), true, false);
    DevView v_mask(c, masks, P * frame, true, false);
    DevView v_oi(c, images_out, P * np * sizeof(double), false, true);
    DevView v_om(c, masks_out, P * np, false, true);
    hipError_t e = v_img.err != hipSuccess ? v_img.err : (v_mask.err != hipSuccess ? v_mask.err : (v_oi.err != hipSuccess ? v_oi.err : v_om.err));
    if (e == hipSuccess)
        e = rs_run(r, n_patterns, v_img.dev, is_float32 != 0, (const uint8_t*)v_mask.dev, (double*)v_oi.dev, (uint8_t*)v_om.dev, n_bad_mask);
    if (e == hipSuccess) e = v_oi.finish();
    if (e == hipSuccess) e = v_om.finish();
    if (e != hipSuccess) {
        c->err = std::string("resample_run: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? MTIP_ENOMEM : MTIP_EHIP;
    }
    return MTIP_OK;
}

extern "C" int mtip_correlate_add_detector(mtip_correlate* h, mtip_resample* r, int n_patterns, const void* images, int is_float32,
                                           const uint8_t* masks, int64_t* n_bad_mask) {
    if (!h || !r) return MTIP_EINVAL;
    mtip_ctx* c = h->c;
    if (r->c != c || r->cfg.n_points != (int64_t)h->cfg.n_q * h->cfg.n_phi) {
        c->err = "correlate_add_detector: the resample handle belongs to another context, or its points are not this handle's n_q x n_phi";
        return MTIP_EINVAL;
    }
    if (rs_check(r, n_patterns, images, "correlate_add_detector") != MTIP_OK) return MTIP_EINVAL;
    if (h->cfg.shared_mask && !rs_static(r, masks)) {
        c->err = "correlate_add_detector: a handle made with shared_mask takes detector frames only where the mask is static "
                 "(intensity_pixel_threshold off and no per-pattern masks)";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    const size_t frame = (size_t)r->cfg.H * r->cfg.W, np = (size_t)r->cfg.n_points, P = (size_t)n_patterns;
    DevView v_img(c, images, P * frame * (is_float32 ? sizeof(float) : sizeof(double)), true, false);
    DevView v_mask(c, masks, P * frame, true, false);
    DevBuf<double> d_pi;
    DevBuf<uint8_t> d_pm;
    int64_t bad = 0;
    hipError_t e = v_img.err != hipSuccess ? v_img.err : v_mask.err;
    if (e == hipSuccess) e = d_pi.alloc(P * np);
    if (e == hipSuccess) e = d_pm.alloc(P * np);
    if (e == hipSuccess) e = rs_run(r, n_patterns, v_img.dev, is_float32 != 0, (const uint8_t*)v_mask.dev, d_pi, d_pm, &bad);
    if (n_bad_mask) *n_bad_mask = bad;
    if (e != hipSuccess) {
        c->err = std::string("correlate_add_detector: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? MTIP_ENOMEM : MTIP_EHIP;
    }
    if (bad != 0) {
        c->err = "correlate_add_detector: mask values other than 0 / 1 after the resampling; nothing was accumulated";
        return MTIP_EINVAL;
    }
    return mtip_correlate_add(h, n_patterns, d_pi, d_pm);
}

// Grid arithmetic of the averaging worker for dimensions = 2 (xframe/projects/fxs/average.py:123-358, run_2d), between the polar
// transforms of k_polar2d.hip, which includes this file: the 2-D counterparts of csrc/k_average.hip on stacks of n polar grids
// (n, Nq, n_phi) complex128 that the caller owns (device OR host pointers; host arrays are staged through a temporary).
//   centre of mass, PolarIntegrator      misk.py:295-312, mathLibrary.py:1254-1262     -> mtip2d_avg_grid_stats [0..2]
//   normalisation factors                average.py:168-180                            -> mtip2d_avg_grid_stats [3..6]
//   shift operator                       fxs_Projections.py:1426-1434                  -> mtip2d_op_grid_phase_ramp
//   point-inversion decision             average.py:216-217                            -> mtip2d_avg_inversion_metric
//   conj / division / means              average.py:174, 180, 222, 238-242             -> mtip2d_op_grid_combine
//   PRTF (four variants), pseudo FSC     resolution_metrics.py:23-33, 63-79            -> mtip2d_avg_curves
//   FQCB                                 resolution_metrics.py:146-187                 -> mtip2d_avg_fqcb, mtip2d_op_deg2_from_table
// The grids are small (128 x 129 values at most in practice): one workgroup per grid (or per shell) with wave reductions in a
// fixed order, so that a grid's result depends on nothing but the grid -- not on n, its position in the stack or n_batch.
#pragma once

#define A2_THREADS 256
#define A2_WAVES (A2_THREADS / 64)
#define A2_NSTAT 9

// numpy's max / min: a NaN is returned, where fmax / fmin would drop it
__device__ __forceinline__ double a2_op(int op, double a, double b) {
    if (op == 0) return a + b;
    if (a != a || b != b) return a + b;
    return op == 1 ? fmax(a, b) : fmin(a, b);
}
// sum (op 0), max (1) or min (2) over the workgroup, returned to every thread: lanes by shuffles, then the waves in order
__device__ __forceinline__ double a2_block_red(int op, double v, double* red) {
    for (int o = 32; o > 0; o >>= 1) v = a2_op(op, v, __shfl_down(v, o, 64));      // (lane 0 holds the wave's result)
    __syncthreads();                                          // (red may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = red[0];
    for (int w = 1; w < A2_WAVES; ++w) s = a2_op(op, s, red[w]);
    return s;
}
__device__ __forceinline__ double a2_block_sum(double v, double* red) { return a2_block_red(0, v, red); }

// per grid: [0] int Re, [1], [2] int Re {x, y} (PolarIntegrator: trapezoids in phi and in r with the weight r, as w_r[q] w_phi[p]),
// [3] the largest real part among the entries "> 0" in numpy's lexicographic order on complex numbers (Re > 0, or Re == 0 and
// Im > 0; -inf if there is none), [4], [5] the complex sum of those entries, [6] their count, [7] max Re, [8] min Re (numpy's: a NaN
// is returned; average.py:721-727).  The nine values are reduced together: shuffles inside every wave, one trip through LDS.
__global__ void __launch_bounds__(A2_THREADS) k2a_stats(const double2* __restrict__ g, const double* __restrict__ wr,
                                                        const double* __restrict__ wp, const double* __restrict__ rs, int N, int n,
                                                        double* __restrict__ out) {
    __shared__ double red[A2_WAVES][A2_NSTAT];
    const int b = blockIdx.x, G = N * n;
    const double2* gb = g + (size_t)b * G;
    const double dphi = 2.0 * 3.14159265358979323846 / n;
    double s[A2_NSTAT];
#pragma unroll
    for (int k = 0; k < A2_NSTAT; ++k) s[k] = 0.0;
    s[3] = s[7] = -__builtin_huge_val();
    s[8] = __builtin_huge_val();
    for (int i = threadIdx.x; i < G; i += A2_THREADS) {
        const int q = i / n, p = i - q * n;
        const double2 v = gb[i];
        double sp, cp;
        sincos(dphi * p, &sp, &cp);
        const double wv = wr[q] * wp[p] * v.x, r = rs[q];
        s[0] += wv;
        s[1] = fma(wv, r * cp, s[1]);
        s[2] = fma(wv, r * sp, s[2]);
        s[7] = a2_op(1, s[7], v.x);
        s[8] = a2_op(2, s[8], v.x);
        if (v.x > 0.0 || (v.x == 0.0 && v.y > 0.0)) {
            s[3] = fmax(s[3], v.x);
            s[4] += v.x;
            s[5] += v.y;
            s[6] += 1.0;
        }
    }
#pragma unroll
    for (int k = 0; k < A2_NSTAT; ++k) {
        const int op = (k == 3 || k == 7) ? 1 : (k == 8 ? 2 : 0);
        double v = s[k];
        for (int o = 32; o > 0; o >>= 1) v = a2_op(op, v, __shfl_down(v, o, 64));
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < A2_NSTAT) {
        const int k = threadIdx.x, op = (k == 3 || k == 7) ? 1 : (k == 8 ? 2 : 0);
        double t = red[0][k];
        for (int w = 1; w < A2_WAVES; ++w) t = a2_op(op, t, red[w][k]);           // the waves in order
        out[(size_t)b * A2_NSTAT + k] = t;
    }
}

// grids[b] *= exp(-i sign k . c_b), k = q (cos phi, sin phi) (fxs_Projections.py:1426-1434), one Cartesian centre per grid
__global__ void __launch_bounds__(A2_THREADS) k2a_phase(double2* __restrict__ g, const double* __restrict__ cc, double sgn,
                                                        const double* __restrict__ qs, int N, int n) {
    const int b = blockIdx.y, G = N * n;
    const double cx = cc[2 * b], cy = cc[2 * b + 1];
    const double dphi = 2.0 * 3.14159265358979323846 / n;
    double2* gb = g + (size_t)b * G;
    for (int i = blockIdx.x * A2_THREADS + threadIdx.x; i < G; i += gridDim.x * A2_THREADS) {
        const int q = i / n, p = i - q * n;
        double sp, cp, sn, cs;
        sincos(dphi * p, &sp, &cp);
        const double kc = qs[q] * cp * cx + qs[q] * sp * cy;
        sincos(-sgn * kc, &sn, &cs);
        gb[i] = cmul(gb[i], make_double2(cs, sn));
    }
}

// per grid: int |Im F - Im F_ref| and int |Im F - Im conj(F_ref)| on the reciprocal grid, one read of F (average.py:216-217)
__global__ void __launch_bounds__(A2_THREADS) k2a_invmetric(const double2* __restrict__ F, const double2* __restrict__ ref,
                                                            const double* __restrict__ wq, const double* __restrict__ wp, int N, int n,
                                                            double* __restrict__ out) {
    __shared__ double red[A2_WAVES];
    const int b = blockIdx.x, G = N * n;
    const double2* Fb = F + (size_t)b * G;
    double d0 = 0.0, d1 = 0.0;
    for (int i = threadIdx.x; i < G; i += A2_THREADS) {
        const int q = i / n, p = i - q * n;
        const double w = wq[q] * wp[p], a = Fb[i].y, r = ref[i].y;
        d0 = fma(w, fabs(a - r), d0);
        d1 = fma(w, fabs(a + r), d1);
    }
    d0 = a2_block_sum(d0, red);
    d1 = a2_block_sum(d1, red);
    if (threadIdx.x == 0) {
        out[2 * b] = d0;
        out[2 * b + 1] = d1;
    }
}

// 0 conj: dst[b] = conj(a[b]);  1 div: dst[b] = a[b] / s[b] (complex per grid);  2 mean: dst = (sum_b a[b]) / Re s[0];
// 3 abs2 mean: dst = (sum_b |a[b]|^2) / Re s[0] (as complex);  4 affine: dst[b] = (a[b] - Re s[0]) / Re s[1] (average.py:721-727).
// The sums run over the stack in its order, as numpy's do over axis 0
enum { A2_CONJ = 0, A2_DIV = 1, A2_MEAN = 2, A2_ABS2MEAN = 3, A2_AFFINE = 4 };
__global__ void __launch_bounds__(A2_THREADS) k2a_combine(int op, double2* dst, const double2* a,      // (dst may be a)
                                                          const double2* __restrict__ s, int nb, int G) {
    for (int i = blockIdx.x * A2_THREADS + threadIdx.x; i < G; i += gridDim.x * A2_THREADS) {
        if (op == A2_MEAN || op == A2_ABS2MEAN) {
            double2 acc = make_double2(0.0, 0.0);
            for (int b = 0; b < nb; ++b) {
                const double2 v = a[(size_t)b * G + i];
                if (op == A2_MEAN) acc = cadd(acc, v);
                else acc.x += v.x * v.x + v.y * v.y;
            }
            const double d = s[0].x;
            dst[i] = make_double2(acc.x / d, acc.y / d);
        } else {
            for (int b = 0; b < nb; ++b) {
                const double2 v = a[(size_t)b * G + i];
                double2 r;
                if (op == A2_CONJ) {
                    r = make_double2(v.x, -v.y);
                } else if (op == A2_AFFINE) {
                    r = make_double2((v.x - s[0].x) / s[1].x, v.y / s[1].x);
                } else {
                    const double2 d = s[b];
                    if (d.y == 0.0) {
                        r = make_double2(v.x / d.x, v.y / d.x);
                    } else {
                        const double m = d.x * d.x + d.y * d.y;
                        r = make_double2((v.x * d.x + v.y * d.y) / m, (v.y * d.x - v.x * d.y) / m);
                    }
                }
                dst[(size_t)b * G + i] = r;
            }
        }
    }
}

// ---- per-shell curves: the shell is a row of n_phi.  blockIdx.y 0..3: PRTF (resolution_metrics.py:63-79) of
//      (a_d, a_ft, I_d, I_ft), (a_d, a_d, I_d, I_d), (a_ft, a_ft, I_ft, I_ft), (a_d, a_d, I_ft, I_ft) -- average.py:250-263;
//      blockIdx.y 4: _fsc(a_d, a_ft) (resolution_metrics.py:23-33)
__device__ __forceinline__ double2 a2_csqrt(double2 z) {
    const double m = sqrt(sqrt(z.x * z.x + z.y * z.y));
    if (m == 0.0) return make_double2(0.0, 0.0);
    double sn, cs;
    sincos(0.5 * atan2(z.y, z.x), &sn, &cs);
    return make_double2(m * cs, m * sn);
}
// nd = sqrt(a1 conj(a2) / (b1 b2)), b = sqrt(I), where both b are non-zero; 0 where a b vanishes and both a do not; 1 elsewhere
__device__ __forceinline__ double2 a2_prtf_point(double2 a1, double2 a2, double i1, double i2) {
    const double b1 = sqrt(i1), b2 = sqrt(i2);
    double2 nd = make_double2(1.0, 0.0);
    if ((b1 != 0.0) && (b2 != 0.0)) {
        const double den = b1 * b2;
        const double2 num = cmulc(a1, a2);
        // (numpy divides by the complex number den + 0i: a zero imaginary part of the quotient comes out as +0)
        nd = make_double2(num.x / den, num.y == 0.0 ? 0.0 : num.y / den);
    } else if ((a1.x != 0.0 || a1.y != 0.0) && (a2.x != 0.0 || a2.y != 0.0)) {
        nd = make_double2(0.0, 0.0);
    }
    return a2_csqrt(nd);
}
__global__ void __launch_bounds__(A2_THREADS) k2a_curves(const double2* __restrict__ a_d, const double2* __restrict__ a_ft,
                                                         const double2* __restrict__ I_d, const double2* __restrict__ I_ft, int N, int n,
                                                         double2* __restrict__ mean, double* __restrict__ sd, double* __restrict__ fsc) {
    __shared__ double red[A2_WAVES];
    const int q = blockIdx.x, var = blockIdx.y;
    const size_t o = (size_t)q * n;
    if (var == 4) {
        double nx = 0.0, s1 = 0.0, s2 = 0.0;
        for (int i = threadIdx.x; i < n; i += A2_THREADS) {
            const double2 x = a_d[o + i], y = a_ft[o + i];
            nx += x.x * y.x + x.y * y.y;
            s1 += x.x * x.x + x.y * x.y;
            s2 += y.x * y.x + y.y * y.y;
        }
        nx = a2_block_sum(nx, red);
        s1 = a2_block_sum(s1, red);
        s2 = a2_block_sum(s2, red);
        if (threadIdx.x == 0) {
            const double den = sqrt(s1 * s2);
            fsc[q] = den != 0.0 ? nx / den : 1.0;
        }
        return;
    }
    const double2* a1 = a_d;
    const double2* a2 = var == 0 ? a_ft : a_d;
    const double2* i1 = (var == 0 || var == 1) ? I_d : I_ft;
    const double2* i2 = var == 1 ? I_d : I_ft;
    if (var == 2) a1 = a2 = a_ft;
    double sx = 0.0, sy = 0.0;
    for (int i = threadIdx.x; i < n; i += A2_THREADS) {
        const double2 v = a2_prtf_point(a1[o + i], a2[o + i], i1[o + i].x, i2[o + i].x);
        sx += v.x;
        sy += v.y;
    }
    const double mx = a2_block_sum(sx, red) / n, my = a2_block_sum(sy, red) / n;
    double v2 = 0.0;
    for (int i = threadIdx.x; i < n; i += A2_THREADS) {
        const double2 v = a2_prtf_point(a1[o + i], a2[o + i], i1[o + i].x, i2[o + i].x);
        const double dx = v.x - mx, dy = v.y - my;
        v2 += dx * dx + dy * dy;
    }
    v2 = a2_block_sum(v2, red);
    if (threadIdx.x == 0) {
        mean[(size_t)var * N + q] = make_double2(mx, my);
        sd[(size_t)var * N + q] = sqrt(v2 / n);
    }
}

// ---- FQCB (resolution_metrics.py:146-187).  An input is a coefficient table I_n(q) (kind 0: rows of ld values, order n in column
//      n; B_n(q, q') = I_n(q) conj(I_n(q')), fxs_invariant_tools.py:906-914) or a B_n stack (kind 1: (n, N, N)).  One workgroup
//      per row q: B_n is symmetrised in (q, q'), the orders o_start, o_start + o_step, ... < o_stop are reduced to the numerator
//      and the two norms, bb = |num / den| (1 where den == 0), then the mean and the population standard deviation over q' <= q.
//      Nothing of size orders x N x N is written.
__device__ __forceinline__ double2 a2_bn(const double2* __restrict__ src, int kind, int ld, int N, int o, int q, int k) {
    if (kind == 0) return cmulc(src[(size_t)q * ld + o], src[(size_t)k * ld + o]);
    return src[((size_t)o * N + q) * N + k];
}
__device__ __forceinline__ double a2_fqcb_point(const double2* __restrict__ s1, int kind1, int ld1, const double2* __restrict__ s2, int kind2,
                                                int ld2, int N, int o_start, int o_stop, int o_step, int q, int k) {
    double num = 0.0, n1 = 0.0, n2 = 0.0;
    for (int o = o_start; o < o_stop; o += o_step) {
        const double2 u = a2_bn(s1, kind1, ld1, N, o, q, k), ut = a2_bn(s1, kind1, ld1, N, o, k, q);
        const double2 v = a2_bn(s2, kind2, ld2, N, o, q, k), vt = a2_bn(s2, kind2, ld2, N, o, k, q);
        const double2 b1 = make_double2((u.x + ut.x) / 2, (u.y + ut.y) / 2), b2 = make_double2((v.x + vt.x) / 2, (v.y + vt.y) / 2);
        num += b1.x * b2.x + b1.y * b2.y;
        n1 += b1.x * b1.x + b1.y * b1.y;
        n2 += b2.x * b2.x + b2.y * b2.y;
    }
    const double den = sqrt(n1 * n2);
    return den != 0.0 ? fabs(num / den) : 1.0;
}
__global__ void __launch_bounds__(A2_THREADS) k2a_fqcb(const double2* __restrict__ s1, int kind1, int ld1, const double2* __restrict__ s2,
                                                       int kind2, int ld2, int N, int o_start, int o_stop, int o_step,
                                                       double* __restrict__ mean, double* __restrict__ sd) {
    __shared__ double red[A2_WAVES];
    const int q = blockIdx.x;
    double s = 0.0;
    for (int k = threadIdx.x; k <= q; k += A2_THREADS) s += a2_fqcb_point(s1, kind1, ld1, s2, kind2, ld2, N, o_start, o_stop, o_step, q, k);
    const double m = a2_block_sum(s, red) / (q + 1);
    double v2 = 0.0;
    for (int k = threadIdx.x; k <= q; k += A2_THREADS) {
        const double d = a2_fqcb_point(s1, kind1, ld1, s2, kind2, ld2, N, o_start, o_stop, o_step, q, k) - m;
        v2 = fma(d, d, v2);
    }
    v2 = a2_block_sum(v2, red);
    if (threadIdx.x == 0) {
        mean[q] = m;
        sd[q] = sqrt(v2 / (q + 1));
    }
}
// B_n(q, q') = I_n(q) conj(I_n(q')) of a table, for the callers that ask for the arrays: out (n, N, N)
__global__ void __launch_bounds__(A2_THREADS) k2a_deg2(const double2* __restrict__ tab, int ld, int N, int n, double2* __restrict__ out) {
    const long long total = (long long)n * N * N;
    for (long long i = (long long)blockIdx.x * A2_THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * A2_THREADS) {
        const int k = (int)(i % N), q = (int)((i / N) % N), o = (int)(i / ((long long)N * N));
        out[i] = cmulc(tab[(size_t)q * ld + o], tab[(size_t)k * ld + o]);
    }
}

// ----------------------------------------------------------------------------------------------------------------------------------
// a caller's array as device memory: itself when it is device memory, else a temporary that is filled / copied back
struct View2d {
    hipStream_t stream = nullptr;
    void* dev = nullptr;
    void* host = nullptr;
    size_t bytes = 0;
    bool writeback = false;
    hipError_t err = hipSuccess;
    DevBuf<char> temp;
    View2d(mtip2d_ctx* c, const void* p, size_t n, bool read, bool write) : stream(c->stream), bytes(n), writeback(write) {
        if (p == nullptr || n == 0) return;
        if (mtip_is_device_pointer(p)) {
            dev = const_cast<void*>(p);
            return;
        }
        host = const_cast<void*>(p);
        err = temp.alloc(n);
        dev = temp;
        if (err == hipSuccess && read) err = mtip_copy(stream, dev, p, n);
    }
    hipError_t finish() {                           // after the stream has been synchronised
        if (temp && writeback && err == hipSuccess) err = mtip_copy(stream, host, dev, bytes);
        return err;
    }
};

static int a2_require_grid(mtip2d_ctx* c, const char* who) {
    if (!c->a_ready) C2_FAIL(c, MTIP_ESTATE, std::string(who) + ": mtip2d_avg_set_grid has not been called");
    return MTIP_OK;
}
static int a2_blocks(const mtip2d_ctx* c) { return std::max(1, div_up((long long)c->N * c->n_phi, A2_THREADS * 4)); }

extern "C" {

int mtip2d_avg_set_grid(mtip2d_ctx* c, const double* rs, const double* qs, const double* w_r, const double* w_q, const double* w_phi) {
    if (!c) return MTIP_EINVAL;
    if (!rs || !qs || !w_r || !w_q || !w_phi) C2_FAIL(c, MTIP_EINVAL, "avg_set_grid: null buffer");
    (void)hipSetDevice(c->device);
    c->a_ready = false;
    MTIP_HIP_CHECK(c, c->a_tab.alloc((size_t)4 * c->N + c->n_phi));
    double* t = c->a_tab;
    const size_t nb = (size_t)c->N * sizeof(double);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, t, rs, nb));
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, t + c->N, qs, nb));
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, t + 2 * c->N, w_r, nb));
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, t + 3 * c->N, w_q, nb));
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, t + 4 * c->N, w_phi, (size_t)c->n_phi * sizeof(double)));
    c->a_ready = true;
    return MTIP_OK;
}

int mtip2d_avg_grid_stats(mtip2d_ctx* c, const mtip_cdouble* grids, int n, double* out) {
    if (!c) return MTIP_EINVAL;
    if (!grids || n <= 0 || !out) C2_FAIL(c, MTIP_EINVAL, "avg_grid_stats: null buffer / empty stack");
    int r = a2_require_grid(c, "avg_grid_stats");
    if (r) return r;
    (void)hipSetDevice(c->device);
    MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    View2d vg(c, grids, (size_t)n * c->N * c->n_phi * sizeof(double2), true, false);
    View2d vo(c, out, (size_t)n * A2_NSTAT * sizeof(double), false, true);
    MTIP_HIP_CHECK(c, vg.err);
    MTIP_HIP_CHECK(c, vo.err);
    const double* t = c->a_tab;
    hipLaunchKernelGGL(k2a_stats, dim3((unsigned)n), dim3(A2_THREADS), 0, c->stream, (const double2*)vg.dev, t + 2 * c->N, t + 4 * c->N, t,
                       c->N, c->n_phi, (double*)vo.dev);
    MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    MTIP_HIP_CHECK(c, vo.finish());
    MTIP_HIP_CHECK(c, hipGetLastError());
    return MTIP_OK;
}

int mtip2d_avg_inversion_metric(mtip2d_ctx* c, const mtip_cdouble* F, int n, const mtip_cdouble* F_ref, double* out) {
    if (!c) return MTIP_EINVAL;
    if (!F || n <= 0 || !F_ref || !out) C2_FAIL(c, MTIP_EINVAL, "avg_inversion_metric: null buffer / empty stack");
    int r = a2_require_grid(c, "avg_inversion_metric");
    if (r) return r;
    (void)hipSetDevice(c->device);
    MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    const size_t gb = (size_t)c->N * c->n_phi * sizeof(double2);
    View2d vf(c, F, (size_t)n * gb, true, false);
    View2d vr(c, F_ref, gb, true, false);
    View2d vo(c, out, (size_t)n * 2 * sizeof(double), false, true);
    MTIP_HIP_CHECK(c, vf.err);
    MTIP_HIP_CHECK(c, vr.err);
    MTIP_HIP_CHECK(c, vo.err);
    const double* t = c->a_tab;
    hipLaunchKernelGGL(k2a_invmetric, dim3((unsigned)n), dim3(A2_THREADS), 0, c->stream, (const double2*)vf.dev, (const double2*)vr.dev,
                       t + 3 * c->N, t + 4 * c->N, c->N, c->n_phi, (double*)vo.dev);
    MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    MTIP_HIP_CHECK(c, vo.finish());
    MTIP_HIP_CHECK(c, hipGetLastError());
    return MTIP_OK;
}

int mtip2d_op_grid_phase_ramp(mtip2d_ctx* c, mtip_cdouble* grids, int n, const double* centers_cartesian, double sign) {
    if (!c) return MTIP_EINVAL;
    if (!grids || n <= 0 || !centers_cartesian) C2_FAIL(c, MTIP_EINVAL, "grid_phase_ramp: null buffer / empty stack");
    int r = a2_require_grid(c, "grid_phase_ramp");
    if (r) return r;
    (void)hipSetDevice(c->device);
    MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    View2d vg(c, grids, (size_t)n * c->N * c->n_phi * sizeof(double2), true, true);
    View2d vc(c, centers_cartesian, (size_t)n * 2 * sizeof(double), true, false);
    MTIP_HIP_CHECK(c, vg.err);
    MTIP_HIP_CHECK(c, vc.err);
    const double* t = c->a_tab;
    hipLaunchKernelGGL(k2a_phase, dim3((unsigned)a2_blocks(c), (unsigned)n), dim3(A2_THREADS), 0, c->stream, (double2*)vg.dev,
                       (const double*)vc.dev, sign, t + c->N, c->N, c->n_phi);
    MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    MTIP_HIP_CHECK(c, vg.finish());
    MTIP_HIP_CHECK(c, hipGetLastError());
    return MTIP_OK;
}

int mtip2d_op_grid_combine(mtip2d_ctx* c, int op, mtip_cdouble* dst, const mtip_cdouble* a, int n, const mtip_cdouble* scalars) {
    if (!c) return MTIP_EINVAL;
    if (!dst || !a || n <= 0 || op < A2_CONJ || op > A2_AFFINE) C2_FAIL(c, MTIP_EINVAL, "grid_combine: null buffer / empty stack / unknown op");
    if (op != A2_CONJ && !scalars) C2_FAIL(c, MTIP_EINVAL, "grid_combine: this op needs scalars");
    (void)hipSetDevice(c->device);
    MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    const bool reduce = op == A2_MEAN || op == A2_ABS2MEAN;
    const size_t gb = (size_t)c->N * c->n_phi * sizeof(double2);
    View2d va(c, a, (size_t)n * gb, true, false);
    View2d vd(c, dst, reduce ? gb : (size_t)n * gb, false, true);
    View2d vs(c, scalars, (op == A2_DIV ? (size_t)n : (op == A2_AFFINE ? (size_t)2 : (size_t)1)) * sizeof(double2), true, false);
    MTIP_HIP_CHECK(c, va.err);
    MTIP_HIP_CHECK(c, vd.err);
    MTIP_HIP_CHECK(c, vs.err);
    // (dst == a on device memory: every point is read before it is written by the same thread)
    hipLaunchKernelGGL(k2a_combine, dim3((unsigned)a2_blocks(c)), dim3(A2_THREADS), 0, c->stream, op, (double2*)vd.dev, (const double2*)va.dev,
                       (const double2*)vs.dev, n, c->N * c->n_phi);
    MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    MTIP_HIP_CHECK(c, vd.finish());
    MTIP_HIP_CHECK(c, hipGetLastError());
    return MTIP_OK;
}

int mtip2d_avg_curves(mtip2d_ctx* c, const mtip_cdouble* a_d, const mtip_cdouble* a_ft, const mtip_cdouble* I_d, const mtip_cdouble* I_ft,
                      mtip_cdouble* prtf_mean, double* prtf_std, double* fsc) {
    if (!c) return MTIP_EINVAL;
    if (!a_d || !a_ft || !I_d || !I_ft || !prtf_mean || !prtf_std || !fsc) C2_FAIL(c, MTIP_EINVAL, "avg_curves: null buffer");
    (void)hipSetDevice(c->device);
    MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    const size_t gb = (size_t)c->N * c->n_phi * sizeof(double2), N = (size_t)c->N;
    View2d v1(c, a_d, gb, true, false), v2(c, a_ft, gb, true, false), v3(c, I_d, gb, true, false), v4(c, I_ft, gb, true, false);
    View2d vm(c, prtf_mean, 4 * N * sizeof(double2), false, true), vs(c, prtf_std, 4 * N * sizeof(double), false, true);
    View2d vf(c, fsc, N * sizeof(double), false, true);
    MTIP_HIP_CHECK(c, v1.err);
    MTIP_HIP_CHECK(c, v2.err);
    MTIP_HIP_CHECK(c, v3.err);
    MTIP_HIP_CHECK(c, v4.err);
    MTIP_HIP_CHECK(c, vm.err);
    MTIP_HIP_CHECK(c, vs.err);
    MTIP_HIP_CHECK(c, vf.err);
    hipLaunchKernelGGL(k2a_curves, dim3((unsigned)c->N, 5u), dim3(A2_THREADS), 0, c->stream, (const double2*)v1.dev, (const double2*)v2.dev,
                       (const double2*)v3.dev, (const double2*)v4.dev, c->N, c->n_phi, (double2*)vm.dev, (double*)vs.dev, (double*)vf.dev);
    MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    MTIP_HIP_CHECK(c, vm.finish());
    MTIP_HIP_CHECK(c, vs.finish());
    MTIP_HIP_CHECK(c, vf.finish());
    MTIP_HIP_CHECK(c, hipGetLastError());
    return MTIP_OK;
}

static size_t a2_fqcb_bytes(const mtip2d_ctx* c, int kind, int n, int ld) {
    return (kind == 0 ? (size_t)c->N * ld : (size_t)n * c->N * c->N) * sizeof(double2);
}

int mtip2d_avg_fqcb(mtip2d_ctx* c, const mtip_cdouble* in1, int kind1, int n1, int ld1, const mtip_cdouble* in2, int kind2, int n2, int ld2,
                    int o_start, int o_step, double* mean, double* std_dev) {
    if (!c) return MTIP_EINVAL;
    if (!in1 || !in2 || !mean || !std_dev) C2_FAIL(c, MTIP_EINVAL, "avg_fqcb: null buffer");
    if (kind1 < 0 || kind1 > 1 || kind2 < 0 || kind2 > 1 || n1 < 1 || n2 < 1 || o_start < 0 || o_step < 1 ||
        (kind1 == 0 && ld1 < n1) || (kind2 == 0 && ld2 < n2))
        C2_FAIL(c, MTIP_EINVAL, "avg_fqcb: kind 0 (table, ld >= n) or 1 (stack), n >= 1, o_start >= 0, o_step >= 1");
    (void)hipSetDevice(c->device);
    MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    View2d v1(c, in1, a2_fqcb_bytes(c, kind1, n1, ld1), true, false), v2(c, in2, a2_fqcb_bytes(c, kind2, n2, ld2), true, false);
    View2d vm(c, mean, (size_t)c->N * sizeof(double), false, true), vs(c, std_dev, (size_t)c->N * sizeof(double), false, true);
    MTIP_HIP_CHECK(c, v1.err);
    MTIP_HIP_CHECK(c, v2.err);
    MTIP_HIP_CHECK(c, vm.err);
    MTIP_HIP_CHECK(c, vs.err);
    hipLaunchKernelGGL(k2a_fqcb, dim3((unsigned)c->N), dim3(A2_THREADS), 0, c->stream, (const double2*)v1.dev, kind1, ld1, (const double2*)v2.dev,
                       kind2, ld2, c->N, o_start, std::min(n1, n2), o_step, (double*)vm.dev, (double*)vs.dev);
    MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    MTIP_HIP_CHECK(c, vm.finish());
    MTIP_HIP_CHECK(c, vs.finish());
    MTIP_HIP_CHECK(c, hipGetLastError());
    return MTIP_OK;
}

int mtip2d_op_deg2_from_table(mtip2d_ctx* c, const mtip_cdouble* table, int n, int ld, mtip_cdouble* out) {
    if (!c) return MTIP_EINVAL;
    if (!table || !out || n < 1 || ld < n) C2_FAIL(c, MTIP_EINVAL, "deg2_from_table: null buffer / n < 1 / ld < n");
    (void)hipSetDevice(c->device);
    MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    const long long total = (long long)n * c->N * c->N;
    View2d vt(c, table, (size_t)c->N * ld * sizeof(double2), true, false), vo(c, out, (size_t)total * sizeof(double2), false, true);
    MTIP_HIP_CHECK(c, vt.err);
    MTIP_HIP_CHECK(c, vo.err);
    hipLaunchKernelGGL(k2a_deg2, dim3((unsigned)std::max(1, std::min(1024, div_up(total, A2_THREADS)))), dim3(A2_THREADS), 0, c->stream,
                       (const double2*)vt.dev, ld, c->N, n, (double2*)vo.dev);
    MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    MTIP_HIP_CHECK(c, vo.finish());
    MTIP_HIP_CHECK(c, hipGetLastError());
    return MTIP_OK;
}

}  // extern "C"

// The 2-D (polar) variant of the hot path, operator level: the circular harmonic transforms, the polar
// Hankel transform, the Fourier pair built from them and the 2-D reciprocal projection of xFrame's fxs project
//   circularHarmonicTransform_{complex,real}_{forward,inverse}   xframe/library/mathLibrary.py:469-496
//   generate_polar_ht (midpoint branch)                          projects/fxs/projectLibrary/hankel_transforms.py:602-640
//   generate_ft, dimensions = 2                                  projectLibrary/fourier_transforms.py:49-88
//   approximate_unknowns / mtip_projection / fixed_projection    projectLibrary/fxs_Projections.py:723-745, 803-826, 855-863
// Layout: grids (B, Nq, n_phi) complex128, n_phi = 2 M + 1 (harmonic_transforms.py:44-47: odd, so the phi transform is a dense DFT,
// not a radix FFT); harmonic coefficients (B, Nq, n_phi) in numpy's FFT order (orders 0..M, -M..-1); coefficients of the real
// transform (B, Nq, M + 1).  A 2-D grid is 128 x 129 values: the whole problem of a restart is 260 KB, so these are bandwidth-trivial
// kernels -- one workgroup per (restart, shell) with the twiddles in LDS for the DFTs, coalesced reads of the (p, k, order) weight
// array for the Hankel transform (its 8.5 MB at 128 x M64 come from L2 / HBM once per application) -- written for parity, not tuned.
// The second half of the file is the RESIDENT loop on the same context (mtip2d_set_density ... mtip2d_run): fused step kernels, state in HBM.
#include "mtip_internal.h"
#include <algorithm>
#include <cmath>

struct mtip2d_ctx {
    int N = 0, n_phi = 0, M = 0, B = 0, device = 0;
    hipStream_t stream = nullptr;
    DevBuf<double2> d_tw;                          // n_phi: exp(-2 pi i j / n_phi)
    DevBuf<double2> d_wf, d_wi;                    // (N, N, n_phi) forward / inverse Hankel weights (summed p, new k, order)
    DevBuf<uint8_t> d_unused;                      // n_phi: order zeroed by the Hankel pair
    DevBuf<double2> d_a, d_b;                      // (B, N, n_phi) work grids
    // projection
    int n_used = 0, zero_pos = -1, zero_id = -1;
    int so_pos = -1;                  // SO_freedom: position (among the used orders) of the order whose unknown is set to 1, or -1
    DevBuf<int> d_order_ids;                       // n_used
    DevBuf<double2> d_pm;                          // (n_used, N)
    DevBuf<uint8_t> d_rmask;                       // (n_used, N): radial mask of the used orders
    DevBuf<double> d_q;                            // N
    DevBuf<double2> d_unk;                         // (B, n_used)
    double n_particles = 1.0;
    bool have_weights = false;
    // loop operators (step, shrink-wrap)
    RealParams rp{};
    DevBuf<double> d_errw;                         // (N, n_phi) weights of the real error metric (integrator weights x metric mask)
    DevBuf<double2> d_c, d_d, d_e;                 // more (B, N, n_phi) work grids
    DevBuf<uint8_t> d_sup;                         // (B, N, n_phi)
    DevBuf<double> d_red;                          // (B, 4) reductions
    bool have_errw = false;
    // ---- resident loop (second half of this file): the state of a batch of restarts stays in HBM between the steps
    bool r_alloc = false, r_ready = false, r_fixed_valid = false, r_ft_mixed = false;
    int r_cur = 0;                                 // which of the two (F, rho) pairs is the latest; the other one is the stale pair
    int r_n_used = 0;                              // n_used the per-order buffers were sized for
    long long r_steps = 0, r_cap = 0;              // steps done, capacity of the histories (steps)
    DevBuf<double2> r_F[2], r_R[2];                // (B, N, n_phi) pairs
    DevBuf<double2> r_C, r_H, r_D;                 // harmonic coefficients of rho, of F (Hankel output), of F'
    DevBuf<double2> r_wf, r_wi;                    // the Hankel weights repacked shell-major (new k, summed p, order)
    bool r_w_dirty = true;
    DevBuf<double2> r_Ft;                          // F = FT(rho) of the step in flight (the pair's own F is the F' that produced rho)
    DevBuf<double2> r_Im, r_sp;                    // (B, N, M + 1) I_m of |F|^2; (B, n_used, N) terms of the scalar products
    DevBuf<double2> r_bestF, r_bestR, r_guess, r_unk;
    DevBuf<double> r_fixed;                        // (B, N, n_phi) intensity grid of the *_non_FXS methods
    DevBuf<uint8_t> r_sup, r_bestsup, r_swnew, r_S0;   // effective / best / new (B, G); initial (G)
    DevBuf<uint8_t> r_flag, r_ft, r_enf, r_sel;    // (B) each
    DevBuf<double> r_part, r_part2, r_besterr;     // (B, N, 2) x 2, (B)
    DevBuf<double> r_herr, r_hmain, r_hrl2, r_hdeg2;   // histories (cap, B[, n_used])
    bool r_have_S0 = false;
    uint32_t r_metrics = 0;                        // 1: deg2_invariant_l2_diff, 2: l2_projection_diff (reciprocal)
    DevBuf<double2> r_deg2ref;                     // (n_used, N, N)
    DevBuf<double> r_deg2norm, r_recw;             // (n_used), (N, n_phi)
    int r_main_type = 0, r_main_n = 1, r_main_items[8] = {0, 0, 0, 0, 0, 0, 0, 0};       // 0 real, 1 deg2, 2 reciprocal l2
    // ---- averaging (k_average2d.h): r (N), q (N), integrator weights in r (N), in q (N), in phi (n_phi)
    DevBuf<double> a_tab;
    bool a_ready = false;
    std::string err;
};

// out[m] = scale * sum_p in[p] exp(sign 2 pi i m p / n) for one (restart, shell) per workgroup; n_out outputs (n for the complex
// transform, M + 1 for the real one); real_in: only Re(in) enters (circularHarmonicTransform_real_forward)
__global__ void __launch_bounds__(256) k2d_dft(const double2* __restrict__ in, double2* __restrict__ out, const double2* __restrict__ tw_g,
                                               int n, int n_out, int sign, double scale, int real_in) {
    HIP_DYNAMIC_SHARED(double2, sm)
    double2* tw = sm;                    // n
    double2* x = sm + n;                 // n
    const size_t row = blockIdx.x;
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        tw[e] = tw_g[e];
        const double2 v = in[row * n + e];
        x[e] = real_in == 2 ? make_double2(v.x * v.x + v.y * v.y, 0.0) : (real_in ? make_double2(v.x, 0.0) : v);
    }
    __syncthreads();
    for (int m = threadIdx.x; m < n_out; m += blockDim.x) {
        double2 acc = make_double2(0.0, 0.0);
        int idx = 0;                                                   // (m p) mod n
        for (int p = 0; p < n; ++p) {
            double2 w = tw[idx];
            if (sign > 0) w.y = -w.y;
            acc = cadd(acc, cmul(x[p], w));
            idx += m;
            if (idx >= n) idx -= n;
        }
        out[row * n_out + m] = cscale(acc, scale);
    }
}

// circularHarmonicTransform_real_inverse: x[p] = irfft(c * n, n)[p] = Re c_0 + 2 sum_{m=1..M} Re(c_m e^{2 pi i m p / n}) (odd n); real output
__global__ void __launch_bounds__(256) k2d_irdft(const double2* __restrict__ coef, double* __restrict__ out, const double2* __restrict__ tw_g,
                                                 int n, int M) {
    HIP_DYNAMIC_SHARED(double2, sm)
    double2* tw = sm;
    double2* c = sm + n;
    const size_t row = blockIdx.x;
    for (int e = threadIdx.x; e < n; e += blockDim.x) tw[e] = tw_g[e];
    for (int e = threadIdx.x; e <= M; e += blockDim.x) c[e] = coef[row * (M + 1) + e];
    __syncthreads();
    for (int p = threadIdx.x; p < n; p += blockDim.x) {
        double acc = c[0].x;
        int idx = 0;
        for (int m = 1; m <= M; ++m) {
            idx += p;
            if (idx >= n) idx -= n;
            const double2 w = tw[idx];                                 // e^{-2 pi i m p / n}: conj for the inverse
            acc += 2.0 * (c[m].x * w.x + c[m].y * w.y);
        }
        out[row * n + p] = acc;
    }
}

// out[b, k, m] = sum_p W[p, k, m] c[b, p, m]; unused orders -> 0.  grid (k, b), threads over m (coalesced rows of W and c)
__global__ void __launch_bounds__(256) k2d_hankel(const double2* __restrict__ c, double2* __restrict__ out, const double2* __restrict__ W,
                                                  const uint8_t* __restrict__ unused, int N, int n) {
    const int k = blockIdx.x, b = blockIdx.y;
    for (int m = threadIdx.x; m < n; m += blockDim.x) {
        double2 acc = make_double2(0.0, 0.0);
        if (!unused[m])
            for (int p = 0; p < N; ++p) acc = cadd(acc, cmul(W[((size_t)p * N + k) * n + m], c[((size_t)b * N + p) * n + m]));
        out[((size_t)b * N + k) * n + m] = acc;
    }
}

// one workgroup per restart: u_j = <I[:, id_j], v_j>_q / |.| (1 when the scalar product vanishes), then I' (fxs_Projections.py:723-745,
// 803-826, 855-863)
__global__ void __launch_bounds__(256) k2d_project(const double2* __restrict__ I, double2* __restrict__ out, double2* __restrict__ unk,
                                                   const double2* __restrict__ pm, const uint8_t* __restrict__ rmask,
                                                   const int* __restrict__ order_ids, const double* __restrict__ q, int N, int n_coef,
                                                   int n_used, int zero_pos, int zero_id, double inv_sqrt_np, int so_pos) {
    HIP_DYNAMIC_SHARED(double2, sm)                // n_used unknowns
    const int b = blockIdx.x;
    const double2* Ib = I + (size_t)b * N * n_coef;
    double2* ob = out + (size_t)b * N * n_coef;
    for (int j = threadIdx.x; j < n_used; j += blockDim.x) {
        const int id = order_ids[j];
        double2 sp = make_double2(0.0, 0.0);
        for (int qq = 0; qq < N; ++qq) sp = cadd(sp, cscale(cmulc(Ib[(size_t)qq * n_coef + id], pm[(size_t)j * N + qq]), q[qq]));
        const double a = sqrt(cabs2(sp));
        double2 u = (sp.x != 0.0 || sp.y != 0.0) ? make_double2(sp.x / a, sp.y / a) : make_double2(1.0, 0.0);
        if (j == so_pos) u = make_double2(1.0, 0.0);                 // SO_freedom (fxs_Projections.py:744-750)
        sm[j] = u;
        unk[(size_t)b * n_used + j] = u;
    }
    for (int e = threadIdx.x; e < N * n_coef; e += blockDim.x) ob[e] = Ib[e];
    __syncthreads();
    for (int e = threadIdx.x; e < N * n_used; e += blockDim.x) {
        const int qq = e / n_used, j = e - qq * n_used;
        if (!rmask[(size_t)j * N + qq]) continue;
        const double2 v = pm[(size_t)j * N + qq];
        ob[(size_t)qq * n_coef + order_ids[j]] = (j == zero_pos) ? v : cmul(v, sm[j]);
    }
    __syncthreads();
    if (zero_id >= 0)
        for (int qq = threadIdx.x; qq < N; qq += blockDim.x) ob[(size_t)qq * n_coef + zero_id] = cscale(ob[(size_t)qq * n_coef + zero_id], inv_sqrt_np);
}

// F' = F sqrt(I' / |F|^2) where |F|^2 >= 0 and I' >= 0, else 0 (project_to_modified_intensity, fxs_Projections.py:899-909);
// I' real grid (B, N, n)
__global__ void __launch_bounds__(256) k2d_modulus(const double2* __restrict__ F, const double* __restrict__ Inew, double2* __restrict__ out,
                                                   long long total) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const double2 f = F[e];
    const double I = f.x * f.x + f.y * f.y, In = Inew[e];
    const bool ok = (I >= 0.0) && (In >= 0.0);
    out[e] = cscale(f, ok ? sqrt(In / I) : 0.0);
}

// the real-space stage of a step (one workgroup per restart): w = rho' (+ (rho_in - IFT(F)) above shell 0 with ft_stab:
// add_above_zero_index, misk.py:326-329), P = real projection, HIO / ER, and the l2_projection_diff sums with the metric weights
__global__ void __launch_bounds__(256) k2d_real_update(const double2* __restrict__ rho_p, const double2* __restrict__ rho_in,
                                                       const double2* __restrict__ rho_rt, const uint8_t* __restrict__ sup,
                                                       const double* __restrict__ errw, double2* __restrict__ out, double* __restrict__ red,
                                                       RealParams rp, int method, double beta, int ft_stab, int N, int n) {
    __shared__ double s_n[4], s_d[4];
    const int b = blockIdx.x;
    const size_t G = (size_t)N * n;
    double num = 0.0, den = 0.0;
    for (size_t e = threadIdx.x; e < G; e += blockDim.x) {
        const size_t i = (size_t)b * G + e;
        double2 w = rho_p[i];
        const double2 pv = rho_in[i];
        if (ft_stab && e >= (size_t)n) w = cadd(w, csub(pv, rho_rt[i]));
        double2 P;
        out[i] = real_update_point(rp, method, beta, w, pv, sup[i] != 0, P);
        const double wg = errw[e];
        const double dx = w.x - P.x, dy = w.y - P.y;
        num = fma(wg, dx * dx + dy * dy, num);
        den = fma(wg, w.x * w.x + w.y * w.y, den);
    }
    for (int o = 32; o > 0; o >>= 1) {
        num += __shfl_xor(num, o, 64);
        den += __shfl_xor(den, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        s_n[threadIdx.x >> 6] = num;
        s_d[threadIdx.x >> 6] = den;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, d = 0.0;
        for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) {
            a += s_n[wv];
            d += s_d[wv];
        }
        red[2 * b] = a;
        red[2 * b + 1] = d;
    }
}

// shrink-wrap (fxs_Projections.py:245-258, 294-298): |rho| -> FT -> x Gaussian(q, sigma) -> IFT is done by the caller's launches;
// these two kernels are the elementwise ends: abs, the Gaussian factor, and the threshold between min and max of the clamped result
__global__ void __launch_bounds__(256) k2d_abs(const double2* __restrict__ in, double2* __restrict__ out, long long total) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < total) out[e] = make_double2(sqrt(in[e].x * in[e].x + in[e].y * in[e].y), 0.0);
}

__global__ void __launch_bounds__(256) k2d_gauss(double2* __restrict__ F, const double* __restrict__ q, double sigma, int N, int n, long long total) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int qi = (int)((e / n) % N);
    const double a = 1.0 / (2.0 * sigma * sigma), pi = 3.14159265358979323846;
    const double q2 = q[qi] * q[qi];
    F[e] = cscale(F[e], sqrt(pi / a) * exp(-pi * pi * q2 * q2 / a));                  // gaussian_fourier_transformed_spherical: q^4 (mathLibrary.py:616-624)
}

__global__ void __launch_bounds__(256) k2d_sw_mask(const double2* __restrict__ conv, uint8_t* __restrict__ mask, double threshold, int N, int n) {
    __shared__ double s_lo[4], s_hi[4];
    const int b = blockIdx.x;
    const size_t G = (size_t)N * n;
    double lo = HUGE_VAL, hi = -HUGE_VAL;
    for (size_t e = threadIdx.x; e < G; e += blockDim.x) {
        const double c = fmax(conv[(size_t)b * G + e].x, 0.0);
        lo = fmin(lo, c);
        hi = fmax(hi, c);
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, o, 64));
        hi = fmax(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.x >> 6] = lo;
        s_hi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    lo = s_lo[0];
    hi = s_hi[0];
    for (int wv = 1; wv < (int)(blockDim.x >> 6); ++wv) {
        lo = fmin(lo, s_lo[wv]);
        hi = fmax(hi, s_hi[wv]);
    }
    const double cut = lo + threshold * (hi - lo);
    for (size_t e = threadIdx.x; e < G; e += blockDim.x) mask[(size_t)b * G + e] = fmax(conv[(size_t)b * G + e].x, 0.0) >= cut ? 1 : 0;
}

static void c2_dft(mtip2d_ctx* c, const double2* in, double2* out, int inverse) {
    const size_t lds = (size_t)2 * c->n_phi * sizeof(double2);
    hipLaunchKernelGGL(k2d_dft, dim3((unsigned)(c->B * c->N)), dim3(256), lds, c->stream, in, out, (const double2*)c->d_tw, c->n_phi, c->n_phi,
                       inverse ? +1 : -1, inverse ? 1.0 : 1.0 / c->n_phi, 0);
}

static void c2_hankel(mtip2d_ctx* c, const double2* in, double2* out, int inverse) {
    hipLaunchKernelGGL(k2d_hankel, dim3((unsigned)c->N, (unsigned)c->B), dim3(256), 0, c->stream, in, out,
                       (const double2*)(inverse ? c->d_wi : c->d_wf), (const uint8_t*)c->d_unused, c->N, c->n_phi);
}

extern "C" {

mtip2d_ctx* mtip2d_create(int n_radial, int n_phi, int n_batch, int device) {
    if (n_radial < 2 || n_phi < 3 || !(n_phi & 1) || n_phi > 2047 || n_batch < 1) return nullptr;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return nullptr;
    mtip2d_ctx* c = new mtip2d_ctx();
    c->N = n_radial; c->n_phi = n_phi; c->M = (n_phi - 1) / 2; c->B = n_batch; c->device = device;
    (void)hipSetDevice(device);
    const size_t G = (size_t)n_batch * n_radial * n_phi;
    bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess &&
              c->d_tw.alloc(n_phi) == hipSuccess &&
              c->d_wf.alloc((size_t)n_radial * n_radial * n_phi) == hipSuccess &&
              c->d_wi.alloc((size_t)n_radial * n_radial * n_phi) == hipSuccess &&
              c->d_unused.alloc(n_phi) == hipSuccess && c->d_a.alloc(G) == hipSuccess &&
              c->d_b.alloc(G) == hipSuccess;
    if (ok) {
        std::vector<double2> tw(n_phi);
        const double pi = 3.14159265358979323846;
        for (int j = 0; j < n_phi; ++j) tw[j] = make_double2(std::cos(2 * pi * j / n_phi), -std::sin(2 * pi * j / n_phi));
        ok = mtip_copy(c->stream, c->d_tw, tw.data(), n_phi * sizeof(double2)) == hipSuccess;
    }
    if (!ok) {
        mtip2d_destroy(c);
        return nullptr;
    }
    return c;
}

void mtip2d_destroy(mtip2d_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamDestroy(c->stream);
    }
    delete c;                                            // the device buffers go with it
}

const char* mtip2d_last_error(const mtip2d_ctx* c) { return c ? c->err.c_str() : "null context"; }

int mtip2d_set_hankel_weights(mtip2d_ctx* c, const mtip_cdouble* forward, const mtip_cdouble* inverse, const uint8_t* unused_orders) {
    if (!c) return MTIP_EINVAL;
    if (!forward || !inverse || !unused_orders) {
        c->err = "hankel weights: null buffer";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    const size_t n = (size_t)c->N * c->N * c->n_phi * sizeof(double2);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->d_wf, forward, n));
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->d_wi, inverse, n));
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->d_unused, unused_orders, c->n_phi));
    c->have_weights = true;
    c->r_w_dirty = true;                           // (the resident loop repacks them in mtip2d_init_state)
    return MTIP_OK;
}

int mtip2d_set_projection(mtip2d_ctx* c, int n_used, const int32_t* order_ids, const mtip_cdouble* pm, const uint8_t* radial_mask,
                          const double* radial_points, double n_particles) {
    if (!c) return MTIP_EINVAL;
    if (n_used < 1 || n_used > c->M + 1 || !order_ids || !pm || !radial_mask || !radial_points || !(n_particles > 0)) {
        c->err = "projection: 1 <= n_used <= M + 1, buffers not null, n_particles > 0";
        return MTIP_EINVAL;
    }
    c->zero_pos = -1;
    c->zero_id = -1;
    for (int j = 0; j < n_used; ++j) {
        if (order_ids[j] < 0 || order_ids[j] > c->M || (j > 0 && order_ids[j] <= order_ids[j - 1])) {
            // (upstream assigns through boolean masks in row-major order: only ascending ids keep columns and vectors paired, 806-818)
            c->err = "projection: order ids must be ascending and within 0..M";
            return MTIP_EINVAL;
        }
        if (order_ids[j] == 0) {
            c->zero_pos = j;
            c->zero_id = 0;
        }
    }
    if (c->zero_id < 0) {
        c->err = "projection: order 0 must be among the used orders (fxs_Projections.py:852-861 indexes it unconditionally)";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    c->d_order_ids.reset();                              // all of the old tables go before the first new one comes
    c->d_pm.reset();
    c->d_rmask.reset();
    c->d_q.reset();
    c->d_unk.reset();
    MTIP_HIP_CHECK(c, c->d_order_ids.alloc(n_used));
    MTIP_HIP_CHECK(c, c->d_pm.alloc((size_t)n_used * c->N));
    MTIP_HIP_CHECK(c, c->d_rmask.alloc((size_t)n_used * c->N));
    MTIP_HIP_CHECK(c, c->d_q.alloc(c->N));
    MTIP_HIP_CHECK(c, c->d_unk.alloc((size_t)c->B * n_used));
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->d_order_ids, order_ids, n_used * sizeof(int)));
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->d_pm, pm, (size_t)n_used * c->N * sizeof(double2)));
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->d_rmask, radial_mask, (size_t)n_used * c->N));
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->d_q, radial_points, c->N * sizeof(double)));
    c->n_used = n_used;
    c->n_particles = n_particles;
    c->so_pos = -1;
    c->r_ready = false;                            // the resident state's per-order buffers follow the projection: mtip2d_init_state again
    c->r_metrics &= ~1u;                           // (and the deg2 reference table is per used order: mtip2d_set_reciprocal_metrics again)
    for (int i = 0; i < c->r_main_n; ++i)
        if (c->r_main_items[i] == 1) { c->r_main_n = 1; c->r_main_items[0] = 0; }
    return MTIP_OK;
}

int mtip2d_op_harmonic(mtip2d_ctx* c, const mtip_cdouble* in, mtip_cdouble* out, int inverse) {
    if (!c) return MTIP_EINVAL;
    if (!in || !out) {
        c->err = "harmonic transform: null buffer";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    const size_t n = (size_t)c->B * c->N * c->n_phi * sizeof(double2);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->d_a, in, n));
    c2_dft(c, c->d_a, c->d_b, inverse);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, out, c->d_b, n));
    MTIP_HIP_CHECK(c, hipGetLastError());
    return MTIP_OK;
}

int mtip2d_op_real_harmonic_forward(mtip2d_ctx* c, const mtip_cdouble* grid, mtip_cdouble* coef) {
    if (!c) return MTIP_EINVAL;
    if (!grid || !coef) {
        c->err = "real harmonic transform: null buffer";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->d_a, grid, (size_t)c->B * c->N * c->n_phi * sizeof(double2)));
    hipLaunchKernelGGL(k2d_dft, dim3((unsigned)(c->B * c->N)), dim3(256), (size_t)2 * c->n_phi * sizeof(double2), c->stream, (const double2*)c->d_a,
                       c->d_b, (const double2*)c->d_tw, c->n_phi, c->M + 1, -1, 1.0 / c->n_phi, 1);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, coef, c->d_b, (size_t)c->B * c->N * (c->M + 1) * sizeof(double2)));
    MTIP_HIP_CHECK(c, hipGetLastError());
    return MTIP_OK;
}

int mtip2d_op_real_harmonic_inverse(mtip2d_ctx* c, const mtip_cdouble* coef, double* grid) {
    if (!c) return MTIP_EINVAL;
    if (!grid || !coef) {
        c->err = "real harmonic transform: null buffer";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->d_a, coef, (size_t)c->B * c->N * (c->M + 1) * sizeof(double2)));
    hipLaunchKernelGGL(k2d_irdft, dim3((unsigned)(c->B * c->N)), dim3(256), (size_t)2 * c->n_phi * sizeof(double2), c->stream, (const double2*)c->d_a,
                       reinterpret_cast<double*>((double2*)c->d_b), (const double2*)c->d_tw, c->n_phi, c->M);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, grid, c->d_b, (size_t)c->B * c->N * c->n_phi * sizeof(double)));
    MTIP_HIP_CHECK(c, hipGetLastError());
    return MTIP_OK;
}

int mtip2d_op_hankel(mtip2d_ctx* c, const mtip_cdouble* in, mtip_cdouble* out, int inverse) {
    if (!c) return MTIP_EINVAL;
    if (!c->have_weights) {
        c->err = "mtip2d_set_hankel_weights has not been called";
        return MTIP_ESTATE;
    }
    if (!in || !out) {
        c->err = "hankel: null buffer";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    const size_t n = (size_t)c->B * c->N * c->n_phi * sizeof(double2);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->d_a, in, n));
    c2_hankel(c, c->d_a, c->d_b, inverse);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, out, c->d_b, n));
    MTIP_HIP_CHECK(c, hipGetLastError());
    return MTIP_OK;
}

/* generate_ft (fourier_transforms.py:57-88): harmonic forward, Hankel (forward / inverse weights), harmonic inverse */
int mtip2d_op_fourier_transform(mtip2d_ctx* c, const mtip_cdouble* in, mtip_cdouble* out, int inverse) {
    if (!c) return MTIP_EINVAL;
    if (!c->have_weights) {
        c->err = "mtip2d_set_hankel_weights has not been called";
        return MTIP_ESTATE;
    }
    if (!in || !out) {
        c->err = "fourier transform: null buffer";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    const size_t n = (size_t)c->B * c->N * c->n_phi * sizeof(double2);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->d_a, in, n));
    c2_dft(c, c->d_a, c->d_b, 0);
    c2_hankel(c, c->d_b, c->d_a, inverse);
    c2_dft(c, c->d_a, c->d_b, 1);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, out, c->d_b, n));
    MTIP_HIP_CHECK(c, hipGetLastError());
    return MTIP_OK;
}

int mtip2d_set_so_freedom(mtip2d_ctx* c, int position) {
    if (!c) return MTIP_EINVAL;
    if (position < -1 || position >= c->n_used) {
        c->err = "so_freedom: position among the used orders of the current projection, or -1";
        return MTIP_EINVAL;
    }
    c->so_pos = position;
    return MTIP_OK;
}

int mtip2d_op_project(mtip2d_ctx* c, const mtip_cdouble* I, mtip_cdouble* out, mtip_cdouble* unknowns) {
    if (!c) return MTIP_EINVAL;
    if (c->n_used == 0) {
        c->err = "mtip2d_set_projection has not been called";
        return MTIP_ESTATE;
    }
    if (!I || !out) {
        c->err = "project: null buffer";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    const int n_coef = c->M + 1;
    const size_t n = (size_t)c->B * c->N * n_coef * sizeof(double2);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->d_a, I, n));
    hipLaunchKernelGGL(k2d_project, dim3((unsigned)c->B), dim3(256), (size_t)c->n_used * sizeof(double2), c->stream, (const double2*)c->d_a, c->d_b,
                       c->d_unk, (const double2*)c->d_pm, (const uint8_t*)c->d_rmask, (const int*)c->d_order_ids, (const double*)c->d_q, c->N,
                       n_coef, c->n_used, c->zero_pos, c->zero_id, 1.0 / std::sqrt(c->n_particles), c->so_pos);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, out, c->d_b, n));
    if (unknowns) MTIP_HIP_CHECK(c, mtip_copy(c->stream, unknowns, c->d_unk, (size_t)c->B * c->n_used * sizeof(double2)));
    MTIP_HIP_CHECK(c, hipGetLastError());
    return MTIP_OK;
}

int mtip2d_set_real_constraints(mtip2d_ctx* c, uint32_t flags, double lo, double hi, double imag_thr, uint32_t hio_flags) {
    if (!c) return MTIP_EINVAL;
    c->rp.flags = flags; c->rp.hio_flags = hio_flags; c->rp.lo = lo; c->rp.hi = hi; c->rp.imag_thr = imag_thr;
    return MTIP_OK;
}

/* weights (Nq, n_phi) of the real error metric: integrator weights times the metric's mask (fxs_IO_methods.py:97-128 with
 * PolarIntegrator, mathLibrary.py:1242-1265) */
int mtip2d_set_error_weights(mtip2d_ctx* c, const double* weights) {
    if (!c || !weights) return MTIP_EINVAL;
    (void)hipSetDevice(c->device);
    const size_t G = (size_t)c->N * c->n_phi, BG = (size_t)c->B * G;
    // (each buffer on its own: a call that failed half way is completed by the next one)
    if (!c->d_errw) MTIP_HIP_CHECK(c, c->d_errw.alloc(G));
    if (!c->d_c) MTIP_HIP_CHECK(c, c->d_c.alloc(BG));
    if (!c->d_d) MTIP_HIP_CHECK(c, c->d_d.alloc(BG));
    if (!c->d_e) MTIP_HIP_CHECK(c, c->d_e.alloc(BG));
    if (!c->d_sup) MTIP_HIP_CHECK(c, c->d_sup.alloc(BG));
    if (!c->d_red) MTIP_HIP_CHECK(c, c->d_red.alloc((size_t)c->B * 4));
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->d_errw, weights, G * sizeof(double)));
    c->have_errw = true;
    return MTIP_OK;
}

/* one HIO (method 0) / ER (method 1) step of the 2-D loop (sketches reconstruct.py:518-528, 576-593 with the 2-D operators):
 * F = FT(rho); I_m = real harmonic transform of |F|^2; unknowns + projection; I' back on the grid; F' = F sqrt(I' / |F|^2);
 * rho' = IFT(F') (+ rho - IFT(F) above shell 0 with ft_stab); real-space projection with `support` (n_batch, Nq, n_phi; the
 * effective one) + HIO / ER; error = l2_projection_diff.  F_new, rho_new (n_batch, Nq, n_phi), err (n_batch), unknowns
 * (n_batch, n_used) or NULL. */
int mtip2d_op_step(mtip2d_ctx* c, int method, int ft_stab, double beta, const mtip_cdouble* rho, const uint8_t* support,
                   mtip_cdouble* F_new, mtip_cdouble* rho_new, double* err, mtip_cdouble* unknowns) {
    return mtip2d_op_step_ex(c, method, ft_stab, beta, rho, support, nullptr, F_new, rho_new, err, unknowns, nullptr, nullptr);
}

int mtip2d_op_step_ex(mtip2d_ctx* c, int method, int ft_stab, double beta, const mtip_cdouble* rho, const uint8_t* support,
                      const double* fixed_intensity, mtip_cdouble* F_new, mtip_cdouble* rho_new, double* err, mtip_cdouble* unknowns,
                      mtip_cdouble* F_out, mtip_cdouble* I_out) {
    if (!c) return MTIP_EINVAL;
    if (!c->have_weights || c->n_used == 0 || !c->have_errw) {
        c->err = "step: hankel weights, projection and error weights must be set first";
        return MTIP_ESTATE;
    }
    const bool fxs = (method == MTIP_HIO || method == MTIP_ER);
    if (method < 0 || method > 3 || !rho || !support || !F_new || !rho_new || !err) {
        c->err = "step: method 0 (HIO), 1 (ER), 2 (HIO_non_FXS) or 3 (ER_non_FXS), buffers not null";
        return MTIP_EINVAL;
    }
    if (!fxs && !fixed_intensity) {
        c->err = "step: the *_non_FXS methods need the fixed intensity grid";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    const int N = c->N, n = c->n_phi, M1 = c->M + 1, B = c->B;
    const size_t BG = (size_t)B * N * n;
    const long long total = (long long)BG;
    const size_t lds = (size_t)2 * n * sizeof(double2);
    const unsigned rows = (unsigned)(B * N);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->d_e, rho, BG * sizeof(double2)));                      // rho_in
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->d_sup, support, BG));
    // F = FT(rho) -> d_c
    c2_dft(c, c->d_e, c->d_a, 0);
    c2_hankel(c, c->d_a, c->d_b, 0);
    c2_dft(c, c->d_b, c->d_c, 1);
    if (F_out) MTIP_HIP_CHECK(c, mtip_copy(c->stream, F_out, c->d_c, BG * sizeof(double2)));
    if (!fxs) {
        // MTIP_start_non_FXS (reconstruct.py:530-535): F' = F sqrt(fixed / |F|^2), no harmonic transform and no unknowns
        MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->d_a, fixed_intensity, BG * sizeof(double)));
        unknowns = nullptr;
    } else {
    // I_m of |F|^2 -> d_a (B, N, M + 1); projection -> d_b; I' (real grid) -> d_a (as doubles)
    hipLaunchKernelGGL(k2d_dft, dim3(rows), dim3(256), lds, c->stream, (const double2*)c->d_c, c->d_a, (const double2*)c->d_tw, n, M1, -1, 1.0 / n, 2);
    if (I_out) MTIP_HIP_CHECK(c, mtip_copy(c->stream, I_out, c->d_a, (size_t)B * N * M1 * sizeof(double2)));
    hipLaunchKernelGGL(k2d_project, dim3((unsigned)B), dim3(256), (size_t)c->n_used * sizeof(double2), c->stream, (const double2*)c->d_a, c->d_b,
                       c->d_unk, (const double2*)c->d_pm, (const uint8_t*)c->d_rmask, (const int*)c->d_order_ids, (const double*)c->d_q, N, M1,
                       c->n_used, c->zero_pos, c->zero_id, 1.0 / std::sqrt(c->n_particles), c->so_pos);
    hipLaunchKernelGGL(k2d_irdft, dim3(rows), dim3(256), lds, c->stream, (const double2*)c->d_b, reinterpret_cast<double*>((double2*)c->d_a),
                       (const double2*)c->d_tw, n, c->M);
    }
    // F' -> d_d
    hipLaunchKernelGGL(k2d_modulus, dim3((unsigned)div_up(total, 256)), dim3(256), 0, c->stream, (const double2*)c->d_c,
                       (const double*)reinterpret_cast<double*>((double2*)c->d_a), c->d_d, total);
    // rho' = IFT(F') -> d_a
    c2_dft(c, c->d_d, c->d_a, 0);
    c2_hankel(c, c->d_a, c->d_b, 1);
    c2_dft(c, c->d_b, c->d_a, 1);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, F_new, c->d_d, BG * sizeof(double2)));                   // F' delivered: d_d is free for the outputs below
    if (ft_stab) {                                                                  // IFT(F) -> d_b (through d_d)
        c2_dft(c, c->d_c, c->d_b, 0);
        c2_hankel(c, c->d_b, c->d_d, 1);
        c2_dft(c, c->d_d, c->d_b, 1);
    }
    hipLaunchKernelGGL(k2d_real_update, dim3((unsigned)B), dim3(256), 0, c->stream, (const double2*)c->d_a, (const double2*)c->d_e,
                       (const double2*)c->d_b, (const uint8_t*)c->d_sup, (const double*)c->d_errw, c->d_d, c->d_red, c->rp, method & 1, beta,
                       ft_stab ? 1 : 0, N, n);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, rho_new, c->d_d, BG * sizeof(double2)));
    std::vector<double> red((size_t)B * 2);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, red.data(), c->d_red, red.size() * sizeof(double)));
    for (int b = 0; b < B; ++b) err[b] = red[2 * b + 1] != 0.0 ? red[2 * b] / red[2 * b + 1] : HUGE_VAL;   // fxs_IO_methods.py:121-126
    if (unknowns) MTIP_HIP_CHECK(c, mtip_copy(c->stream, unknowns, c->d_unk, (size_t)B * c->n_used * sizeof(double2)));
    MTIP_HIP_CHECK(c, hipGetLastError());
    return MTIP_OK;
}

/* the SW sketch (reconstruct.py:598-605; fxs_Projections.py:245-258, 294-298): mask = c >= min + threshold (max - min) of
 * c = max(Re IFT(FT(|rho|) gaussian(q, sigma)), 0); mask (n_batch, Nq, n_phi) */
int mtip2d_op_shrinkwrap(mtip2d_ctx* c, const mtip_cdouble* rho, double sigma, double threshold, uint8_t* mask) {
    if (!c) return MTIP_EINVAL;
    if (!c->have_weights || !c->have_errw || c->d_q == nullptr) {
        c->err = "shrinkwrap: hankel weights, projection (radial points) and error weights must be set first";
        return MTIP_ESTATE;
    }
    if (!rho || !mask || !(sigma > 0.0)) {
        c->err = "shrinkwrap: null buffer or sigma <= 0";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    const size_t BG = (size_t)c->B * c->N * c->n_phi;
    const long long total = (long long)BG;
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->d_e, rho, BG * sizeof(double2)));
    hipLaunchKernelGGL(k2d_abs, dim3((unsigned)div_up(total, 256)), dim3(256), 0, c->stream, (const double2*)c->d_e, c->d_c, total);
    c2_dft(c, c->d_c, c->d_a, 0);
    c2_hankel(c, c->d_a, c->d_b, 0);
    c2_dft(c, c->d_b, c->d_c, 1);
    hipLaunchKernelGGL(k2d_gauss, dim3((unsigned)div_up(total, 256)), dim3(256), 0, c->stream, c->d_c, (const double*)c->d_q, sigma, c->N, c->n_phi, total);
    c2_dft(c, c->d_c, c->d_a, 0);
    c2_hankel(c, c->d_a, c->d_b, 1);
    c2_dft(c, c->d_b, c->d_c, 1);
    hipLaunchKernelGGL(k2d_sw_mask, dim3((unsigned)c->B), dim3(256), 0, c->stream, (const double2*)c->d_c, c->d_sup, threshold, c->N, c->n_phi);
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, mask, c->d_sup, BG));
    MTIP_HIP_CHECK(c, hipGetLastError());
    return MTIP_OK;
}

}  // extern "C"

// =====================================================================================================================
// The resident 2-D loop: the state of a batch of restarts stays in HBM and a step is a chain of fused kernels, one workgroup per
// (shell, group of up to RS_BC restarts).  A step has three global joins -- the Hankel contraction couples all shells of an order,
// the scalar products of the projection run over q, the inverse Hankel contraction couples the shells again -- so it is
//   k2d_rs_head   : F = FT(rho) from the harmonic coefficients of rho (forward Hankel for the whole group: every weight is read
//                   once per group, then the inverse DFT of the shell), I_m of |F|^2, the terms of <I_m, v_m>_q of this shell
//   k2d_rs_mid    : unknowns (summed over the shells in a fixed order by every workgroup), projection, I' on the grid, modulus
//                   replacement, harmonic coefficients of F' (and the sums of the reciprocal l2_projection_diff)
//   k2d_rs_tail   : rho' = IFT(F') -- with ft_stab IFT(F' - F) + rho above shell 0 (linearity: IFT(F') + rho - IFT(F)), per
//                   restart --, real-space projection + HIO / ER, error sums of the shell, harmonic coefficients of the new rho
//   k2d_rs_finish : one workgroup: error ratios, main error, best error and the "better" flags, the history rows
//   k2d_rs_keep   : the pair and the support of the restarts that improved -> best buffers
// (+ k2d_rs_deg2 when deg2_invariant_l2_diff is enabled).  Every sum has a fixed order: no atomics.  The *_non_FXS methods
// skip the harmonic part of the head and the projection of the middle kernel and read the resident intensity grid.
// The (F, rho) pairs ping-pong between two buffers: the one a step reads is the pair "before the most recent step" afterwards,
// which is what upstream's stale `hist` holds (reconstruct.py:859, 893, 901).
// Workgroups of 1024 threads: the grid is only N x ceil(B / 8) workgroups (128 at 128 shells x 8 restarts, half the CUs), so the waves
// that hide the latency of the weight stream and of the LDS loops of the DFTs have to come from inside the workgroup.  LDS per
// workgroup: (1 + 2 RS_BC + S RS_BC) n_phi + RS_BC (M + 1) complex values, S <= 4 slices of the Hankel sum: 109 KB at n_phi = 129.
#define RS_BC 8
#define RS_THREADS 1024

struct RsMain { int type, n, items[8]; };

__device__ __forceinline__ void rs_wave_sum2(double& a, double& b) {
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
}

// How the n_out outputs of each of the nb rows of a row transform are shared out: one output per thread and round (the loops of k2d_dft
// / k2d_irdft) for the first `full` columns, and where the last round would be nearly empty (8 rows x 129 columns on 1024 threads
// leave one column) a wave per left-over output instead, its lanes taking the summands in strides of 64 and adding up by the
// butterfly.  The split depends on the column count and the block size alone, not on the number of restarts in the group: a restart
// computes the same thing alone and in a batch.
__device__ __forceinline__ void rs_split(int n_out, int& full, int& rem) {
    const int per_round = blockDim.x / RS_BC;
    full = per_round > 0 ? (n_out / per_round) * per_round : n_out;
    rem = n_out - full;
    if (rem * RS_BC > (int)(blockDim.x >> 6)) {
        full = n_out;
        rem = 0;
    }
}

// rows of a DFT in LDS: y[bb][m] = scale sum_p x[bb][p] exp(sign 2 pi i m p / n), m < n_out; rows of x and y have stride n; y and / or the
// global rows g (row stride g_stride, n_out values each) receive the result
__device__ __forceinline__ void rs_dft(const double2* x, double2* y, const double2* tw, int nb, int n, int n_out, int sign, double scale,
                                       double2* g, size_t g_stride) {
    int full, rem;
    rs_split(n_out, full, rem);
    for (int it = threadIdx.x; it < nb * full; it += blockDim.x) {
        const int bb = it / full, m = it - bb * full;
        const double2* xr = x + (size_t)bb * n;
        double2 acc = make_double2(0.0, 0.0);
        int idx = 0;
        for (int p = 0; p < n; ++p) {
            double2 w = tw[idx];
            if (sign > 0) w.y = -w.y;
            acc = cadd(acc, cmul(xr[p], w));
            idx += m;
            if (idx >= n) idx -= n;
        }
        acc = cscale(acc, scale);
        if (y) y[(size_t)bb * n + m] = acc;
        if (g) g[(size_t)bb * g_stride + m] = acc;
    }
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wv < nb * rem) {
        const int bb = wv / rem, m = full + (wv - bb * rem);
        const double2* xr = x + (size_t)bb * n;
        double ax = 0.0, ay = 0.0;
        for (int p = lane; p < n; p += 64) {
            double2 w = tw[(int)(((long long)m * p) % n)];
            if (sign > 0) w.y = -w.y;
            const double2 t = cmul(xr[p], w);
            ax += t.x;
            ay += t.y;
        }
        rs_wave_sum2(ax, ay);
        if (lane == 0) {
            const double2 acc = make_double2(ax * scale, ay * scale);
            if (y) y[(size_t)bb * n + m] = acc;
            if (g) g[(size_t)bb * g_stride + m] = acc;
        }
    }
}

// circularHarmonicTransform_real_inverse of nb coefficient rows c (stride n): out[bb][p].x = Re c_0 + 2 sum_{m=1..M} Re(c_m e^{2 pi i m p / n})
__device__ __forceinline__ void rs_irdft(const double2* c_all, double2* out, const double2* tw, int nb, int n, int M) {
    int full, rem;
    rs_split(n, full, rem);
    for (int it = threadIdx.x; it < nb * full; it += blockDim.x) {          // the loop of k2d_irdft
        const int bb = it / full, p = it - bb * full;
        const double2* c = c_all + (size_t)bb * n;
        double acc = c[0].x;
        int idx = 0;
        for (int m = 1; m <= M; ++m) {
            idx += p;
            if (idx >= n) idx -= n;
            const double2 w = tw[idx];
            acc += 2.0 * (c[m].x * w.x + c[m].y * w.y);
        }
        out[(size_t)bb * n + p] = make_double2(acc, 0.0);
    }
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wv < nb * rem) {
        const int bb = wv / rem, p = full + (wv - bb * rem);
        const double2* c = c_all + (size_t)bb * n;
        double acc = 0.0, unused_sum = 0.0;
        for (int m = 1 + lane; m <= M; m += 64) {
            const double2 w = tw[(int)(((long long)m * p) % n)];
            acc += 2.0 * (c[m].x * w.x + c[m].y * w.y);
        }
        rs_wave_sum2(acc, unused_sum);
        if (lane == 0) out[(size_t)bb * n + p] = make_double2(c[0].x + acc, 0.0);
    }
}

// out[bb][m] = sum_p W[k, p, m] (c[b, p, m] - (sub[bb] ? c2[b, p, m] : 0)) for the restarts of the group, W repacked shell-major (a
// workgroup streams one contiguous (N, n) block).  A thread owns an order and one of S slices of p and keeps the group's sums in
// registers, so a weight is loaded once per group; the slices' partial sums meet in LDS (P: S x RS_BC x n) and are added in slice order
__device__ __forceinline__ void rs_hankel(const double2* __restrict__ c, const double2* __restrict__ c2, const bool* sub,
                                          const double2* __restrict__ W, const uint8_t* __restrict__ unused, double2* out, double2* P, int S,
                                          int b0, int nb, int k, int N, int n) {
    const int chunk = (N + S - 1) / S;
    for (int t = threadIdx.x; t < S * n; t += blockDim.x) {
        const int sl = t / n, m = t - sl * n;
        const int p0 = sl * chunk, p1 = min(N, p0 + chunk);
        double2 acc[RS_BC];
#pragma unroll
        for (int bb = 0; bb < RS_BC; ++bb) acc[bb] = make_double2(0.0, 0.0);
        if (!unused[m])
            for (int p = p0; p < p1; ++p) {
                const double2 w = W[((size_t)k * N + p) * n + m];
#pragma unroll
                for (int bb = 0; bb < RS_BC; ++bb)
                    if (bb < nb) {
                        const size_t i = ((size_t)(b0 + bb) * N + p) * n + m;
                        const double2 v = (c2 && sub[bb]) ? csub(c[i], c2[i]) : c[i];
                        acc[bb] = cadd(acc[bb], cmul(w, v));
                    }
            }
#pragma unroll
        for (int bb = 0; bb < RS_BC; ++bb)
            if (bb < nb) P[((size_t)sl * RS_BC + bb) * n + m] = acc[bb];
    }
    __syncthreads();
    for (int it = threadIdx.x; it < nb * n; it += blockDim.x) {
        const int bb = it / n, m = it - bb * n;
        double2 a = P[(size_t)bb * n + m];
        for (int sl = 1; sl < S; ++sl) a = cadd(a, P[((size_t)sl * RS_BC + bb) * n + m]);
        out[it] = a;
    }
}

__device__ __forceinline__ void rs_head_body(double2* sm, const double2* __restrict__ C, const double2* __restrict__ W, const uint8_t* __restrict__ unused,
                                                   const double2* __restrict__ tw_g, double2* __restrict__ H, double2* __restrict__ F,
                                                   double2* __restrict__ Im, double2* __restrict__ sp, const double2* __restrict__ pm,
                                                   const int* __restrict__ order_ids, const double* __restrict__ q, int B, int N, int n, int n_used,
                                                   int fxs, int S) {
    double2 *tw = sm, *A = sm + n, *Bf = A + (size_t)RS_BC * n, *P = Bf + (size_t)RS_BC * n + (size_t)RS_BC * ((n + 1) / 2);
    const int k = blockIdx.x, b0 = blockIdx.y * RS_BC, nb = min(RS_BC, B - b0), M1 = (n + 1) / 2;
    for (int e = threadIdx.x; e < n; e += blockDim.x) tw[e] = tw_g[e];
    rs_hankel(C, nullptr, nullptr, W, unused, A, P, S, b0, nb, k, N, n);
    __syncthreads();
    for (int it = threadIdx.x; it < nb * n; it += blockDim.x) {
        const int bb = it / n, m = it - bb * n;
        H[((size_t)(b0 + bb) * N + k) * n + m] = A[it];
    }
    rs_dft(A, Bf, tw, nb, n, n, +1, 1.0, F + ((size_t)b0 * N + k) * n, (size_t)N * n);
    __syncthreads();
    if (!fxs) return;
    for (int it = threadIdx.x; it < nb * n; it += blockDim.x) A[it] = make_double2(Bf[it].x * Bf[it].x + Bf[it].y * Bf[it].y, 0.0);
    __syncthreads();
    rs_dft(A, Bf, tw, nb, n, M1, -1, 1.0 / n, Im + ((size_t)b0 * N + k) * M1, (size_t)N * M1);
    __syncthreads();
    for (int it = threadIdx.x; it < nb * n_used; it += blockDim.x) {
        const int bb = it / n_used, j = it - bb * n_used;
        sp[((size_t)(b0 + bb) * n_used + j) * N + k] = cscale(cmulc(Bf[(size_t)bb * n + order_ids[j]], pm[(size_t)j * N + k]), q[k]);
    }
}

__device__ __forceinline__ void rs_mid_body(double2* sm, const double2* __restrict__ Fin, const double2* __restrict__ Im, const double2* __restrict__ sp,
                                                  double2* __restrict__ unk, const double2* __restrict__ pm, const uint8_t* __restrict__ rmask,
                                                  const int* __restrict__ order_ids, const double2* __restrict__ tw_g,
                                                  const double* __restrict__ fixed, double2* __restrict__ Fn, double2* __restrict__ D,
                                                  const double* __restrict__ recw, double* __restrict__ part2, int B, int N, int n, int n_used,
                                                  int zero_pos, int zero_id, double inv_sqrt_np, int so_pos, int fxs) {
    double2 *tw = sm, *A = sm + n, *Bf = A + (size_t)RS_BC * n, *U = Bf + (size_t)RS_BC * n;
    const int k = blockIdx.x, b0 = blockIdx.y * RS_BC, nb = min(RS_BC, B - b0), M1 = (n + 1) / 2, M = M1 - 1;
    for (int e = threadIdx.x; e < n; e += blockDim.x) tw[e] = tw_g[e];
    if (fxs) {
        // approximate_unknowns (fxs_Projections.py:723-745): every workgroup sums the shells' terms itself, in ascending order (the order
        // of k2d_project: an order without signal has a scalar product of rounding noise, whose phase the summation order would decide)
        for (int it = threadIdx.x; it < nb * n_used; it += blockDim.x) {
            const int bb = it / n_used, j = it - bb * n_used;
            const double2* t = sp + ((size_t)(b0 + bb) * n_used + j) * N;
            double2 s = make_double2(0.0, 0.0);
            for (int qq = 0; qq < N; ++qq) s = cadd(s, t[qq]);
            const double a = sqrt(cabs2(s));
            double2 u = (s.x != 0.0 || s.y != 0.0) ? make_double2(s.x / a, s.y / a) : make_double2(1.0, 0.0);
            if (j == so_pos) u = make_double2(1.0, 0.0);
            U[(size_t)bb * M1 + j] = u;
            if (k == 0) unk[(size_t)(b0 + bb) * n_used + j] = u;
        }
        for (int it = threadIdx.x; it < nb * M1; it += blockDim.x) {
            const int bb = it / M1, m = it - bb * M1;
            A[(size_t)bb * n + m] = Im[((size_t)(b0 + bb) * N + k) * M1 + m];
        }
        __syncthreads();
        for (int it = threadIdx.x; it < nb * n_used; it += blockDim.x) {
            const int bb = it / n_used, j = it - bb * n_used;
            if (!rmask[(size_t)j * N + k]) continue;
            const double2 v = pm[(size_t)j * N + k];
            A[(size_t)bb * n + order_ids[j]] = (j == zero_pos) ? v : cmul(v, U[(size_t)bb * M1 + j]);
        }
        __syncthreads();
        if (zero_id >= 0 && (int)threadIdx.x < nb) A[(size_t)threadIdx.x * n + zero_id] = cscale(A[(size_t)threadIdx.x * n + zero_id], inv_sqrt_np);
        __syncthreads();
        rs_irdft(A, Bf, tw, nb, n, M);
        __syncthreads();
    } else {
        for (int it = threadIdx.x; it < nb * n; it += blockDim.x) {
            const int bb = it / n, p = it - bb * n;
            Bf[it] = make_double2(fixed[((size_t)(b0 + bb) * N + k) * n + p], 0.0);
        }
        __syncthreads();
    }
    for (int it = threadIdx.x; it < nb * n; it += blockDim.x) {                   // project_to_modified_intensity (k2d_modulus)
        const int bb = it / n, p = it - bb * n;
        const size_t g = ((size_t)(b0 + bb) * N + k) * n + p;
        const double2 f = Fin[g];
        const double I = f.x * f.x + f.y * f.y, In = Bf[it].x;
        const bool ok = (I >= 0.0) && (In >= 0.0);
        const double2 o = cscale(f, ok ? sqrt(In / I) : 0.0);
        Fn[g] = o;
        A[it] = o;
    }
    __syncthreads();
    if (recw) {                                                                   // reciprocal l2_projection_diff of (F, F'): a wave per restart
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
        for (int bb = wv; bb < nb; bb += nw) {
            double num = 0.0, den = 0.0;
            for (int p = lane; p < n; p += 64) {
                const double2 f = Fin[((size_t)(b0 + bb) * N + k) * n + p], o = A[(size_t)bb * n + p];
                const double wg = recw[(size_t)k * n + p], dx = f.x - o.x, dy = f.y - o.y;
                num = fma(wg, dx * dx + dy * dy, num);
                den = fma(wg, f.x * f.x + f.y * f.y, den);
            }
            rs_wave_sum2(num, den);
            if (lane == 0) {
                part2[((size_t)(b0 + bb) * N + k) * 2] = num;
                part2[((size_t)(b0 + bb) * N + k) * 2 + 1] = den;
            }
        }
    }
    rs_dft(A, nullptr, tw, nb, n, n, -1, 1.0 / n, D + ((size_t)b0 * N + k) * n, (size_t)N * n);
}

// the kernels of the FXS methods, and of the *_non_FXS methods (no harmonic part, no scalar products / no projection: the resident
// intensity grid instead, sketch MTIP_start_non_FXS, reconstruct.py:530-535)
__global__ void __launch_bounds__(RS_THREADS) k2d_rs_head(const double2* __restrict__ C, const double2* __restrict__ W, const uint8_t* __restrict__ unused,
                                                   const double2* __restrict__ tw_g, double2* __restrict__ H, double2* __restrict__ F,
                                                   double2* __restrict__ Im, double2* __restrict__ sp, const double2* __restrict__ pm,
                                                   const int* __restrict__ order_ids, const double* __restrict__ q, int B, int N, int n, int n_used,
                                                   int S) {
    HIP_DYNAMIC_SHARED(double2, sm)
    rs_head_body(sm, C, W, unused, tw_g, H, F, Im, sp, pm, order_ids, q, B, N, n, n_used, 1, S);
}

__global__ void __launch_bounds__(RS_THREADS) k2d_rs_head_nonfxs(const double2* __restrict__ C, const double2* __restrict__ W,
                                                          const uint8_t* __restrict__ unused, const double2* __restrict__ tw_g,
                                                          double2* __restrict__ H, double2* __restrict__ F, int B, int N, int n, int S) {
    HIP_DYNAMIC_SHARED(double2, sm)
    rs_head_body(sm, C, W, unused, tw_g, H, F, nullptr, nullptr, nullptr, nullptr, nullptr, B, N, n, 0, 0, S);
}

__global__ void __launch_bounds__(RS_THREADS) k2d_rs_mid(const double2* __restrict__ Fin, const double2* __restrict__ Im, const double2* __restrict__ sp,
                                                  double2* __restrict__ unk, const double2* __restrict__ pm, const uint8_t* __restrict__ rmask,
                                                  const int* __restrict__ order_ids, const double2* __restrict__ tw_g, double2* __restrict__ Fn,
                                                  double2* __restrict__ D, const double* __restrict__ recw, double* __restrict__ part2, int B, int N,
                                                  int n, int n_used, int zero_pos, int zero_id, double inv_sqrt_np, int so_pos) {
    HIP_DYNAMIC_SHARED(double2, sm)
    rs_mid_body(sm, Fin, Im, sp, unk, pm, rmask, order_ids, tw_g, nullptr, Fn, D, recw, part2, B, N, n, n_used, zero_pos, zero_id, inv_sqrt_np, so_pos, 1);
}

__global__ void __launch_bounds__(RS_THREADS) k2d_rs_mid_nonfxs(const double2* __restrict__ Fin, const double2* __restrict__ tw_g,
                                                         const double* __restrict__ fixed, double2* __restrict__ Fn, double2* __restrict__ D,
                                                         const double* __restrict__ recw, double* __restrict__ part2, int B, int N, int n) {
    HIP_DYNAMIC_SHARED(double2, sm)
    rs_mid_body(sm, Fin, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, tw_g, fixed, Fn, D, recw, part2, B, N, n, 0, -1, -1, 1.0, -1, 0);
}

__global__ void __launch_bounds__(RS_THREADS) k2d_rs_tail(const double2* __restrict__ D, const double2* __restrict__ H, const double2* __restrict__ W,
                                                   const uint8_t* __restrict__ unused, const double2* __restrict__ tw_g,
                                                   const double2* __restrict__ Rin, const uint8_t* __restrict__ sup, const double* __restrict__ errw,
                                                   double2* __restrict__ Rout, double2* __restrict__ C, double* __restrict__ part, RealParams rp,
                                                   int method, double beta, int ft_mode, const uint8_t* __restrict__ ftmask, int B, int N, int n,
                                                   int S) {
    HIP_DYNAMIC_SHARED(double2, sm)
    double2 *tw = sm, *A = sm + n, *Bf = A + (size_t)RS_BC * n, *P = Bf + (size_t)RS_BC * n + (size_t)RS_BC * ((n + 1) / 2);
    const int k = blockIdx.x, b0 = blockIdx.y * RS_BC, nb = min(RS_BC, B - b0);
    for (int e = threadIdx.x; e < n; e += blockDim.x) tw[e] = tw_g[e];
    bool sub[RS_BC];                                  // add_above_zero_index (misk.py:326-329): the add-back leaves shell 0 alone
#pragma unroll
    for (int bb = 0; bb < RS_BC; ++bb) sub[bb] = k > 0 && bb < nb && (ft_mode == 1 || (ft_mode == 2 && ftmask[b0 + bb] != 0));
    rs_hankel(D, ft_mode ? H : nullptr, sub, W, unused, A, P, S, b0, nb, k, N, n);
    __syncthreads();
    rs_dft(A, Bf, tw, nb, n, n, +1, 1.0, nullptr, 0);
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int bb = wv; bb < nb; bb += nw) {
        const bool add = k > 0 && (ft_mode == 1 || (ft_mode == 2 && ftmask[b0 + bb] != 0));
        double num = 0.0, den = 0.0;
        for (int p = lane; p < n; p += 64) {
            const size_t g = ((size_t)(b0 + bb) * N + k) * n + p;
            double2 w = Bf[(size_t)bb * n + p];
            const double2 pv = Rin[g];
            if (add) w = cadd(w, pv);
            double2 P;
            const double2 o = real_update_point(rp, method, beta, w, pv, sup[g] != 0, P);
            Rout[g] = o;
            A[(size_t)bb * n + p] = o;
            const double wg = errw[(size_t)k * n + p], dx = w.x - P.x, dy = w.y - P.y;
            num = fma(wg, dx * dx + dy * dy, num);
            den = fma(wg, w.x * w.x + w.y * w.y, den);
        }
        rs_wave_sum2(num, den);
        if (lane == 0) {
            part[((size_t)(b0 + bb) * N + k) * 2] = num;
            part[((size_t)(b0 + bb) * N + k) * 2 + 1] = den;
        }
    }
    __syncthreads();
    rs_dft(A, nullptr, tw, nb, n, n, -1, 1.0 / n, C + ((size_t)b0 * N + k) * n, (size_t)N * n);
}

// deg2_invariant_l2_diff, 2-D flavour (fxs_IO_methods.py:370-400): per used order sum_{q, q'} |ref_m(q, q') - I_m(q) I_m(q')^*|^2 / norm_m,
// -1 where the norm vanishes; grid (n_used, B)
__global__ void __launch_bounds__(256) k2d_rs_deg2(const double2* __restrict__ Im, const double2* __restrict__ ref, const double* __restrict__ norm,
                                                   const int* __restrict__ order_ids, double* __restrict__ out, int N, int M1, int n_used) {
    HIP_DYNAMIC_SHARED(double2, sm)                   // N values of I_m
    __shared__ double s_w[4];
    const int j = blockIdx.x, b = blockIdx.y, id = order_ids[j];
    for (int qq = threadIdx.x; qq < N; qq += blockDim.x) sm[qq] = Im[((size_t)b * N + qq) * M1 + id];
    __syncthreads();
    double acc = 0.0, dummy = 0.0;
    const double2* r = ref + (size_t)j * N * N;
    for (int e = threadIdx.x; e < N * N; e += blockDim.x) {
        const int qa = e / N, qb = e - qa * N;
        const double2 d = csub(r[e], cmulc(sm[qa], sm[qb]));
        acc += d.x * d.x + d.y * d.y;
    }
    rs_wave_sum2(acc, dummy);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int wv = 0; wv < (int)(blockDim.x >> 6); ++wv) t += s_w[wv];
        out[(size_t)b * n_used + j] = norm[j] != 0.0 ? t / norm[j] : -1.0;
    }
}

// one workgroup: the error ratios (fxs_IO_methods.py:121-126), the main error (746-765), best error and the flags of the restarts that
// improved (reconstruct.py:934-938), the history rows of this step
__global__ void __launch_bounds__(256) k2d_rs_finish(const double* __restrict__ part, const double* __restrict__ part2, double* __restrict__ herr,
                                                    double* __restrict__ hmain, double* __restrict__ hrl2, const double* __restrict__ hdeg2,
                                                    double* __restrict__ besterr, uint8_t* __restrict__ flag, int B, int N, int n_used, RsMain mc) {
    // a wave per restart: the lanes add the shells' sums in strides of 64, then the butterfly (a fixed order)
    const int lane = threadIdx.x & 63;
    for (int b = threadIdx.x >> 6; b < B; b += (int)(blockDim.x >> 6)) {
        double num = 0.0, den = 0.0;
        for (int k = lane; k < N; k += 64) {
            num += part[((size_t)b * N + k) * 2];
            den += part[((size_t)b * N + k) * 2 + 1];
        }
        rs_wave_sum2(num, den);
        const double err = den != 0.0 ? num / den : HUGE_VAL;
        double rl2 = 0.0;
        if (part2) {
            num = den = 0.0;
            for (int k = lane; k < N; k += 64) {
                num += part2[((size_t)b * N + k) * 2];
                den += part2[((size_t)b * N + k) * 2 + 1];
            }
            rs_wave_sum2(num, den);
            rl2 = den != 0.0 ? num / den : HUGE_VAL;
        }
        if (lane != 0) continue;
        herr[b] = err;
        if (part2) hrl2[b] = rl2;
        double acc = 0.0;
        long long cnt = 0;
        for (int i = 0; i < mc.n; ++i) {
            const int item = mc.items[i], len = item == 1 ? n_used : 1;
            for (int e = 0; e < len; ++e) {
                const double v = item == 0 ? err : (item == 2 ? rl2 : hdeg2[(size_t)b * n_used + e]);
                if (cnt == 0) acc = v;
                else if (mc.type == 0) acc += v;
                else if (mc.type == 1) acc = (v < acc || v != v) ? v : acc;
                else if (mc.type == 2) acc = (v > acc || v != v) ? v : acc;
                else acc *= v;
                ++cnt;
            }
        }
        const double main_err = mc.type == 0 ? acc / (double)cnt : acc;
        hmain[b] = main_err;
        const bool better = besterr[b] > main_err;
        if (better) besterr[b] = main_err;
        flag[b] = better ? 1 : 0;
    }
}

// grid (chunks of the grid, B): the pair and the effective support of a restart that improved become its best ones
__global__ void __launch_bounds__(256) k2d_rs_keep(const uint8_t* __restrict__ flag, const double2* __restrict__ F, const double2* __restrict__ R,
                                                   const uint8_t* __restrict__ sup, double2* __restrict__ bF, double2* __restrict__ bR,
                                                   uint8_t* __restrict__ bsup, long long G) {
    const int b = blockIdx.y;
    if (!flag[b]) return;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G) return;
    const size_t i = (size_t)b * G + e;
    bF[i] = F[i];
    bR[i] = R[i];
    bsup[i] = sup[i];
}

// the support setter (fxs_Projections.py:53-58) with the enforce decision of reconstruct.py:877-885 taken on the device:
// enforce_b = last main error_b > limit (no step yet: not enforced)
__global__ void __launch_bounds__(256) k2d_rs_support(const uint8_t* __restrict__ fresh, const uint8_t* __restrict__ S0, uint8_t* __restrict__ sup,
                                                      const double* __restrict__ last_main, double limit, uint8_t* __restrict__ enf, long long G) {
    const int b = blockIdx.y;
    const bool enforce = last_main && last_main[b] > limit;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G) return;
    const size_t i = (size_t)b * G + e;
    sup[i] = enforce ? (fresh[i] && S0[e]) : (fresh[i] != 0);
    if (e == 0) enf[b] = enforce ? 1 : 0;
}

__global__ void __launch_bounds__(256) k2d_rs_select(const uint8_t* __restrict__ sel, double2* __restrict__ F, double2* __restrict__ R,
                                                     uint8_t* __restrict__ sup, const double2* __restrict__ bF, const double2* __restrict__ bR,
                                                     const uint8_t* __restrict__ bsup, long long G) {
    const int b = blockIdx.y;
    if (sel && !sel[b]) return;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G) return;
    const size_t i = (size_t)b * G + e;
    F[i] = bF[i];
    R[i] = bR[i];
    sup[i] = bsup[i];
}

// (p, k, order) -> (k, p, order)
__global__ void __launch_bounds__(256) k2d_rs_repack(const double2* __restrict__ in, double2* __restrict__ out, int N, int n) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)N * N * n) return;
    const int m = (int)(e % n), p = (int)((e / n) % N), k = (int)(e / ((long long)n * N));
    out[e] = in[((size_t)p * N + k) * n + m];
}

__global__ void __launch_bounds__(256) k2d_rs_absgrid(const double2* __restrict__ F, double* __restrict__ out, long long total) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < total) out[e] = sqrt(F[e].x * F[e].x + F[e].y * F[e].y);
}

__global__ void __launch_bounds__(256) k2d_rs_fill_state(const uint8_t* __restrict__ S0, uint8_t* __restrict__ sup, uint8_t* __restrict__ bsup,
                                                         double* __restrict__ besterr, long long G) {
    const int b = blockIdx.y;
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G) return;
    sup[(size_t)b * G + e] = S0[e];
    bsup[(size_t)b * G + e] = S0[e];
    if (e == 0) besterr[b] = HUGE_VAL;
}

#define C2_FAIL(c, code, msg)  \
    do {                       \
        (c)->err = (msg);      \
        return (code);         \
    } while (0)

// slices of the Hankel sum per workgroup: as many as the threads allow, at most 4
static int rs_slices(const mtip2d_ctx* c) { return std::max(1, std::min(4, RS_THREADS / c->n_phi)); }

static size_t rs_lds_bytes(const mtip2d_ctx* c) {
    return ((size_t)(1 + 2 * RS_BC + rs_slices(c) * RS_BC) * c->n_phi + (size_t)RS_BC * (c->M + 1)) * sizeof(double2);
}

// the buffers that do not depend on the projection; allocated by the first resident call
static int rs_ensure(mtip2d_ctx* c) {
    if (c->r_alloc) return MTIP_OK;
    if (rs_lds_bytes(c) > 144 * 1024) C2_FAIL(c, MTIP_EINVAL, "resident 2-D loop: n_phi too large for the fused step kernels (LDS per workgroup > 144 KB)");
    (void)hipSetDevice(c->device);
    const size_t G = (size_t)c->N * c->n_phi, BG = (size_t)c->B * G, B = (size_t)c->B;
    for (int i = 0; i < 2; ++i) {
        MTIP_HIP_CHECK(c, c->r_F[i].alloc(BG));
        MTIP_HIP_CHECK(c, c->r_R[i].alloc(BG));
    }
    MTIP_HIP_CHECK(c, c->r_C.alloc(BG));
    MTIP_HIP_CHECK(c, c->r_H.alloc(BG));
    MTIP_HIP_CHECK(c, c->r_D.alloc(BG));
    MTIP_HIP_CHECK(c, c->r_Ft.alloc(BG));
    MTIP_HIP_CHECK(c, c->r_wf.alloc((size_t)c->N * c->N * c->n_phi));
    MTIP_HIP_CHECK(c, c->r_wi.alloc((size_t)c->N * c->N * c->n_phi));
    MTIP_HIP_CHECK(c, c->r_Im.alloc(B * c->N * (c->M + 1)));
    MTIP_HIP_CHECK(c, c->r_bestF.alloc(BG));
    MTIP_HIP_CHECK(c, c->r_bestR.alloc(BG));
    MTIP_HIP_CHECK(c, c->r_guess.alloc(BG));
    MTIP_HIP_CHECK(c, c->r_fixed.alloc(BG));
    MTIP_HIP_CHECK(c, c->r_sup.alloc(BG));
    MTIP_HIP_CHECK(c, c->r_bestsup.alloc(BG));
    MTIP_HIP_CHECK(c, c->r_swnew.alloc(BG));
    MTIP_HIP_CHECK(c, c->r_S0.alloc(G));
    MTIP_HIP_CHECK(c, c->r_flag.alloc(B));
    MTIP_HIP_CHECK(c, c->r_ft.alloc(B));
    MTIP_HIP_CHECK(c, c->r_enf.alloc(B));
    MTIP_HIP_CHECK(c, c->r_sel.alloc(B));
    MTIP_HIP_CHECK(c, c->r_part.alloc(B * c->N * 2));
    MTIP_HIP_CHECK(c, c->r_part2.alloc(B * c->N * 2));
    MTIP_HIP_CHECK(c, c->r_besterr.alloc(B));
    MTIP_HIP_CHECK(c, c->r_recw.alloc(G));
    c->r_alloc = true;
    return MTIP_OK;
}

// histories for `need` steps (doubling, as the 3-D context does); the per-order buffers follow the projection in use
static int rs_ensure_hist(mtip2d_ctx* c, long long need) {
    if (need <= c->r_cap) return MTIP_OK;
    long long cap = c->r_cap > 0 ? c->r_cap : 256;
    while (cap < need) cap *= 2;
    const size_t B = (size_t)c->B, nu = (size_t)(c->r_n_used > 0 ? c->r_n_used : 1);
    DevBuf<double> e, m, l, d;
    MTIP_HIP_CHECK(c, e.alloc(cap * B));
    MTIP_HIP_CHECK(c, m.alloc(cap * B));
    MTIP_HIP_CHECK(c, l.alloc(cap * B));
    MTIP_HIP_CHECK(c, d.alloc(cap * B * nu));
    MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    if (c->r_steps > 0) {
        MTIP_HIP_CHECK(c, hipMemcpy(e, c->r_herr, c->r_steps * B * sizeof(double), hipMemcpyDeviceToDevice));
        MTIP_HIP_CHECK(c, hipMemcpy(m, c->r_hmain, c->r_steps * B * sizeof(double), hipMemcpyDeviceToDevice));
        MTIP_HIP_CHECK(c, hipMemcpy(l, c->r_hrl2, c->r_steps * B * sizeof(double), hipMemcpyDeviceToDevice));
        MTIP_HIP_CHECK(c, hipMemcpy(d, c->r_hdeg2, c->r_steps * B * nu * sizeof(double), hipMemcpyDeviceToDevice));
        MTIP_HIP_CHECK(c, hipDeviceSynchronize());
    }
    c->r_herr = std::move(e);
    c->r_hmain = std::move(m);
    c->r_hrl2 = std::move(l);
    c->r_hdeg2 = std::move(d);
    c->r_cap = cap;
    return MTIP_OK;
}

static int rs_require_state(mtip2d_ctx* c, const char* who) {
    if (!c->r_ready) C2_FAIL(c, MTIP_ESTATE, std::string(who) + ": mtip2d_init_state has not been called (or the projection changed since)");
    (void)hipSetDevice(c->device);
    return MTIP_OK;
}

// generate_ft on device buffers (in, out not the work grids d_a / d_b)
static void rs_ft(mtip2d_ctx* c, const double2* in, double2* out, int inverse) {
    c2_dft(c, in, c->d_a, 0);
    c2_hankel(c, c->d_a, c->d_b, inverse);
    c2_dft(c, c->d_b, out, 1);
}

// harmonic coefficients of the latest density: what the head kernel of the next step starts from
static void rs_refresh_coefficients(mtip2d_ctx* c) { c2_dft(c, c->r_R[c->r_cur], c->r_C, 0); }

static dim3 rs_grid_points(const mtip2d_ctx* c) { return dim3((unsigned)div_up((long long)c->N * c->n_phi, 256), (unsigned)c->B); }

static int rs_copy_d2d(mtip2d_ctx* c, void* dst, const void* src, size_t n) {
    MTIP_HIP_CHECK(c, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, c->stream));
    return MTIP_OK;
}

static int rs_enqueue_step(mtip2d_ctx* c, int method, int ft_mode, double beta) {
    const int N = c->N, n = c->n_phi, B = c->B, cur = c->r_cur, nxt = 1 - cur;
    const bool fxs = (method == MTIP_HIO || method == MTIP_ER);
    const dim3 grid((unsigned)N, (unsigned)div_up(B, RS_BC));
    const size_t lds = rs_lds_bytes(c);
    const int S = rs_slices(c);
    const long long s = c->r_steps;
    const bool deg2 = fxs && (c->r_metrics & 1), rl2 = (c->r_metrics & 2) != 0;
    if (fxs)
        hipLaunchKernelGGL(k2d_rs_head, grid, dim3(RS_THREADS), lds, c->stream, (const double2*)c->r_C, (const double2*)c->r_wf, (const uint8_t*)c->d_unused,
                           (const double2*)c->d_tw, c->r_H, c->r_Ft, c->r_Im, c->r_sp, (const double2*)c->d_pm, (const int*)c->d_order_ids,
                           (const double*)c->d_q, B, N, n, c->n_used, S);
    else
        hipLaunchKernelGGL(k2d_rs_head_nonfxs, grid, dim3(RS_THREADS), lds, c->stream, (const double2*)c->r_C, (const double2*)c->r_wf,
                           (const uint8_t*)c->d_unused, (const double2*)c->d_tw, c->r_H, c->r_Ft, B, N, n, S);
    if (deg2)
        hipLaunchKernelGGL(k2d_rs_deg2, dim3((unsigned)c->n_used, (unsigned)B), dim3(256), (size_t)N * sizeof(double2), c->stream,
                           (const double2*)c->r_Im, (const double2*)c->r_deg2ref, (const double*)c->r_deg2norm, (const int*)c->d_order_ids,
                           c->r_hdeg2 + (size_t)s * B * c->n_used, N, c->M + 1, c->n_used);
    const double* recw = rl2 ? (const double*)c->r_recw : (const double*)nullptr;
    if (fxs)
        hipLaunchKernelGGL(k2d_rs_mid, grid, dim3(RS_THREADS), lds, c->stream, (const double2*)c->r_Ft, (const double2*)c->r_Im, (const double2*)c->r_sp,
                           c->r_unk, (const double2*)c->d_pm, (const uint8_t*)c->d_rmask, (const int*)c->d_order_ids, (const double2*)c->d_tw,
                           c->r_F[nxt], c->r_D, recw, c->r_part2, B, N, n, c->n_used, c->zero_pos, c->zero_id, 1.0 / std::sqrt(c->n_particles),
                           c->so_pos);
    else
        hipLaunchKernelGGL(k2d_rs_mid_nonfxs, grid, dim3(RS_THREADS), lds, c->stream, (const double2*)c->r_Ft, (const double2*)c->d_tw,
                           (const double*)c->r_fixed, c->r_F[nxt], c->r_D, recw, c->r_part2, B, N, n);
    hipLaunchKernelGGL(k2d_rs_tail, grid, dim3(RS_THREADS), lds, c->stream, (const double2*)c->r_D, (const double2*)c->r_H, (const double2*)c->r_wi,
                       (const uint8_t*)c->d_unused, (const double2*)c->d_tw, (const double2*)c->r_R[cur], (const uint8_t*)c->r_sup,
                       (const double*)c->d_errw, c->r_R[nxt], c->r_C, c->r_part, c->rp, method & 1, beta, ft_mode, (const uint8_t*)c->r_ft, B, N, n, S);
    RsMain mc;
    mc.type = c->r_main_type;
    mc.n = c->r_main_n;
    for (int i = 0; i < 8; ++i) mc.items[i] = c->r_main_items[i];
    hipLaunchKernelGGL(k2d_rs_finish, dim3(1), dim3(256), 0, c->stream, (const double*)c->r_part, rl2 ? (const double*)c->r_part2 : (const double*)nullptr,
                       c->r_herr + (size_t)s * B, c->r_hmain + (size_t)s * B, c->r_hrl2 + (size_t)s * B,
                       (const double*)(c->r_hdeg2 + (size_t)s * B * (c->r_n_used > 0 ? c->r_n_used : 1)), c->r_besterr, c->r_flag, B, N, c->n_used, mc);
    hipLaunchKernelGGL(k2d_rs_keep, rs_grid_points(c), dim3(256), 0, c->stream, (const uint8_t*)c->r_flag, (const double2*)c->r_F[nxt],
                       (const double2*)c->r_R[nxt], (const uint8_t*)c->r_sup, c->r_bestF, c->r_bestR, c->r_bestsup, (long long)N * n);
    c->r_cur = nxt;
    c->r_steps += 1;
    return MTIP_OK;
}

extern "C" {

/* ---- state */
int mtip2d_set_density(mtip2d_ctx* c, int batch, const mtip_cdouble* rho) {
    if (!c) return MTIP_EINVAL;
    if (batch < 0 || batch >= c->B || !rho) C2_FAIL(c, MTIP_EINVAL, "set_density: batch index / null buffer");
    int r = rs_ensure(c);
    if (r) return r;
    const size_t G = (size_t)c->N * c->n_phi;
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->r_guess + (size_t)batch * G, rho, G * sizeof(double2)));
    return MTIP_OK;
}

int mtip2d_set_initial_support(mtip2d_ctx* c, const uint8_t* support) {
    if (!c) return MTIP_EINVAL;
    if (!support) C2_FAIL(c, MTIP_EINVAL, "set_initial_support: null buffer");
    int r = rs_ensure(c);
    if (r) return r;
    const size_t G = (size_t)c->N * c->n_phi;
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->r_S0, support, G));
    for (int b = 0; b < c->B; ++b) MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->r_sup + (size_t)b * G, support, G));
    c->r_have_S0 = true;
    return MTIP_OK;
}

int mtip2d_set_support(mtip2d_ctx* c, int batch, const uint8_t* support) {
    if (!c) return MTIP_EINVAL;
    if (batch < 0 || batch >= c->B || !support) C2_FAIL(c, MTIP_EINVAL, "set_support: batch index / null buffer");
    int r = rs_ensure(c);
    if (r) return r;
    const size_t G = (size_t)c->N * c->n_phi;
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->r_sup + (size_t)batch * G, support, G));
    return MTIP_OK;
}

int mtip2d_init_state(mtip2d_ctx* c) {
    if (!c) return MTIP_EINVAL;
    if (!c->have_weights || !c->have_errw) C2_FAIL(c, MTIP_ESTATE, "init_state: hankel weights and error weights must be set first");
    if (!c->r_alloc || !c->r_have_S0) C2_FAIL(c, MTIP_ESTATE, "init_state: mtip2d_set_density (every restart) and mtip2d_set_initial_support come first");
    (void)hipSetDevice(c->device);
    const size_t BG = (size_t)c->B * c->N * c->n_phi;
    MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    // the per-order buffers follow the projection (none yet: the *_non_FXS methods alone can run)
    const int nu = c->n_used > 0 ? c->n_used : 1;
    if (nu != c->r_n_used) {
        c->r_sp.reset();
        c->r_unk.reset();
        c->r_herr.reset();
        c->r_hmain.reset();
        c->r_hrl2.reset();
        c->r_hdeg2.reset();
        c->r_cap = 0;
        c->r_n_used = nu;
        MTIP_HIP_CHECK(c, c->r_sp.alloc((size_t)c->B * nu * c->N));
        MTIP_HIP_CHECK(c, c->r_unk.alloc((size_t)c->B * nu));
    }
    c->r_steps = 0;
    int r = rs_ensure_hist(c, 256);
    if (r) return r;
    if (c->r_w_dirty) {
        const long long nw = (long long)c->N * c->N * c->n_phi;
        hipLaunchKernelGGL(k2d_rs_repack, dim3((unsigned)div_up(nw, 256)), dim3(256), 0, c->stream, (const double2*)c->d_wf, c->r_wf, c->N, c->n_phi);
        hipLaunchKernelGGL(k2d_rs_repack, dim3((unsigned)div_up(nw, 256)), dim3(256), 0, c->stream, (const double2*)c->d_wi, c->r_wi, c->N, c->n_phi);
        c->r_w_dirty = false;
    }
    // reconstruct.py:962-963: the state starts from F0 = FT(guess), rho0 = IFT(F0)
    rs_ft(c, c->r_guess, c->r_F[0], 0);
    rs_ft(c, c->r_F[0], c->r_R[0], 1);
    for (double2* dst : {(double2*)c->r_F[1], (double2*)c->r_bestF}) if ((r = rs_copy_d2d(c, dst, c->r_F[0], BG * sizeof(double2)))) return r;
    for (double2* dst : {(double2*)c->r_R[1], (double2*)c->r_bestR}) if ((r = rs_copy_d2d(c, dst, c->r_R[0], BG * sizeof(double2)))) return r;
    hipLaunchKernelGGL(k2d_rs_fill_state, rs_grid_points(c), dim3(256), 0, c->stream, (const uint8_t*)c->r_S0, c->r_sup, c->r_bestsup, c->r_besterr,
                       (long long)c->N * c->n_phi);
    c->r_cur = 0;
    c->r_fixed_valid = false;
    c->r_ft_mixed = false;
    rs_refresh_coefficients(c);
    MTIP_HIP_CHECK(c, hipGetLastError());
    c->r_ready = true;
    return MTIP_OK;
}

int mtip2d_set_ft_stab_mask(mtip2d_ctx* c, const uint8_t* mask) {
    if (!c) return MTIP_EINVAL;
    if (!mask) {
        c->r_ft_mixed = false;
        return MTIP_OK;
    }
    int r = rs_ensure(c);
    if (r) return r;
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->r_ft, mask, (size_t)c->B));
    c->r_ft_mixed = true;
    return MTIP_OK;
}

int mtip2d_set_reciprocal_metrics(mtip2d_ctx* c, uint32_t which, const mtip_cdouble* deg2_reference, const double* deg2_norms,
                                  const double* l2_weights) {
    if (!c) return MTIP_EINVAL;
    if (which & ~3u) C2_FAIL(c, MTIP_EINVAL, "reciprocal metrics: 1 (deg2_invariant_l2_diff) | 2 (l2_projection_diff)");
    if ((which & 1) && (c->n_used == 0 || !deg2_reference || !deg2_norms))
        C2_FAIL(c, c->n_used == 0 ? MTIP_ESTATE : MTIP_EINVAL, "reciprocal metrics: deg2_invariant_l2_diff needs the projection set and its reference table / norms");
    if ((which & 2) && !l2_weights) C2_FAIL(c, MTIP_EINVAL, "reciprocal metrics: l2_projection_diff needs its weights");
    int r = rs_ensure(c);
    if (r) return r;
    if (which & 1) {
        MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
        const size_t nn = (size_t)c->n_used * c->N * c->N;
        MTIP_HIP_CHECK(c, c->r_deg2ref.alloc(nn));
        MTIP_HIP_CHECK(c, c->r_deg2norm.alloc((size_t)c->n_used));
        MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->r_deg2ref, deg2_reference, nn * sizeof(double2)));
        MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->r_deg2norm, deg2_norms, (size_t)c->n_used * sizeof(double)));
    }
    if (which & 2) MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->r_recw, l2_weights, (size_t)c->N * c->n_phi * sizeof(double)));
    c->r_metrics = which;
    return MTIP_OK;
}

int mtip2d_set_main_error(mtip2d_ctx* c, int type, int n_items, const int32_t* items) {
    if (!c) return MTIP_EINVAL;
    if (type < 0 || type > 3 || n_items < 1 || n_items > 8 || !items) C2_FAIL(c, MTIP_EINVAL, "main error: type 0..3, 1..8 items");
    bool vec = false, scalar = false;
    for (int i = 0; i < n_items; ++i) {
        if (items[i] < 0 || items[i] > 2) C2_FAIL(c, MTIP_EINVAL, "main error: items 0 (real l2), 1 (deg2), 2 (reciprocal l2)");
        (items[i] == 1 ? vec : scalar) = true;
    }
    if (vec && scalar) C2_FAIL(c, MTIP_EINVAL, "main error over a scalar metric and a per-order one: the reference raises (fxs_IO_methods.py:758)");
    c->r_main_type = type;
    c->r_main_n = n_items;
    for (int i = 0; i < n_items; ++i) c->r_main_items[i] = items[i];
    return MTIP_OK;
}

/* ---- the loop */
int mtip2d_run_async(mtip2d_ctx* c, int method, int ft_stab, int n_steps, const double* betas) {
    if (!c) return MTIP_EINVAL;
    int r = rs_require_state(c, "run");
    if (r) return r;
    if (method < 0 || method > 3) C2_FAIL(c, MTIP_EINVAL, "run: method 0 (HIO), 1 (ER), 2 (HIO_non_FXS) or 3 (ER_non_FXS)");
    if (n_steps < 0 || (n_steps > 0 && !betas)) C2_FAIL(c, MTIP_EINVAL, "run: bad n_steps / betas");
    const bool fxs = (method == MTIP_HIO || method == MTIP_ER);
    if (fxs && (c->n_used == 0 || c->n_used != c->r_n_used)) C2_FAIL(c, MTIP_ESTATE, "run: an FXS method needs mtip2d_set_projection (before mtip2d_init_state)");
    for (int i = 0; i < c->r_main_n; ++i) {
        if (c->r_main_items[i] == 1 && !((c->r_metrics & 1) && fxs)) C2_FAIL(c, MTIP_ESTATE, "run: main error over deg2_invariant_l2_diff needs that metric and an FXS method");
        if (c->r_main_items[i] == 2 && !(c->r_metrics & 2)) C2_FAIL(c, MTIP_ESTATE, "run: main error over the reciprocal l2_projection_diff needs that metric");
    }
    if (!fxs && c->r_metrics) C2_FAIL(c, MTIP_ESTATE, "run: the *_non_FXS methods with reciprocal metrics enabled (the reference raises)");
    r = rs_ensure_hist(c, c->r_steps + n_steps);
    if (r) return r;
    if (!fxs) {
        if (!c->r_fixed_valid) {                 // reconstruct.py:899-902: |F| of the stale pair, kept for the block of non-FXS keys
            const long long total = (long long)c->B * c->N * c->n_phi;
            hipLaunchKernelGGL(k2d_rs_absgrid, dim3((unsigned)div_up(total, 256)), dim3(256), 0, c->stream, (const double2*)c->r_F[1 - c->r_cur],
                               c->r_fixed, total);
            c->r_fixed_valid = true;
        }
    } else {
        c->r_fixed_valid = false;
    }
    const int ft_mode = !ft_stab ? 0 : (c->r_ft_mixed ? 2 : 1);
    for (int s = 0; s < n_steps; ++s) rs_enqueue_step(c, method, ft_mode, betas[s]);
    MTIP_HIP_CHECK(c, hipGetLastError());
    return MTIP_OK;
}

int mtip2d_fetch_errors(mtip2d_ctx* c, int64_t first, int64_t n, double* real_err) {
    if (!c) return MTIP_EINVAL;
    if (first < 0 || n < 0 || first + n > c->r_steps || !real_err) C2_FAIL(c, MTIP_EINVAL, "fetch_errors: range beyond the steps done / null buffer");
    (void)hipSetDevice(c->device);
    if (n) MTIP_HIP_CHECK(c, mtip_copy(c->stream, real_err, c->r_herr + (size_t)first * c->B, (size_t)n * c->B * sizeof(double)));
    return MTIP_OK;
}

int mtip2d_fetch_main_errors(mtip2d_ctx* c, int64_t first, int64_t n, double* main_err) {
    if (!c) return MTIP_EINVAL;
    if (first < 0 || n < 0 || first + n > c->r_steps || !main_err) C2_FAIL(c, MTIP_EINVAL, "fetch_main_errors: range beyond the steps done / null buffer");
    (void)hipSetDevice(c->device);
    if (n) MTIP_HIP_CHECK(c, mtip_copy(c->stream, main_err, c->r_hmain + (size_t)first * c->B, (size_t)n * c->B * sizeof(double)));
    return MTIP_OK;
}

int mtip2d_fetch_reciprocal_metrics(mtip2d_ctx* c, int64_t first, int64_t n, double* deg2, double* l2) {
    if (!c) return MTIP_EINVAL;
    if (first < 0 || n < 0 || first + n > c->r_steps) C2_FAIL(c, MTIP_EINVAL, "fetch_reciprocal_metrics: range beyond the steps done");
    if ((deg2 && !(c->r_metrics & 1)) || (l2 && !(c->r_metrics & 2))) C2_FAIL(c, MTIP_ESTATE, "fetch_reciprocal_metrics: metric not enabled");
    (void)hipSetDevice(c->device);
    if (n && deg2) MTIP_HIP_CHECK(c, mtip_copy(c->stream, deg2, c->r_hdeg2 + (size_t)first * c->B * c->r_n_used, (size_t)n * c->B * c->r_n_used * sizeof(double)));
    if (n && l2) MTIP_HIP_CHECK(c, mtip_copy(c->stream, l2, c->r_hrl2 + (size_t)first * c->B, (size_t)n * c->B * sizeof(double)));
    return MTIP_OK;
}

int mtip2d_run(mtip2d_ctx* c, int method, int ft_stab, int n_steps, const double* betas, double* real_err) {
    int r = mtip2d_run_async(c, method, ft_stab, n_steps, betas);
    if (r) return r;
    if (!real_err) {
        MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
        return MTIP_OK;
    }
    return mtip2d_fetch_errors(c, c->r_steps - n_steps, n_steps, real_err);
}

int mtip2d_shrinkwrap(mtip2d_ctx* c, double sigma, double threshold, double error_limit, uint8_t* enforced) {
    if (!c) return MTIP_EINVAL;
    int r = rs_require_state(c, "shrinkwrap");
    if (r) return r;
    if (c->d_q == nullptr) C2_FAIL(c, MTIP_ESTATE, "shrinkwrap: the projection (radial points) must be set first");
    if (!(sigma > 0.0)) C2_FAIL(c, MTIP_EINVAL, "shrinkwrap: sigma <= 0");
    const size_t BG = (size_t)c->B * c->N * c->n_phi;
    const long long total = (long long)BG;
    // the launches of mtip2d_op_shrinkwrap on the resident density
    hipLaunchKernelGGL(k2d_abs, dim3((unsigned)div_up(total, 256)), dim3(256), 0, c->stream, (const double2*)c->r_R[c->r_cur], c->d_c, total);
    c2_dft(c, c->d_c, c->d_a, 0);
    c2_hankel(c, c->d_a, c->d_b, 0);
    c2_dft(c, c->d_b, c->d_c, 1);
    hipLaunchKernelGGL(k2d_gauss, dim3((unsigned)div_up(total, 256)), dim3(256), 0, c->stream, c->d_c, (const double*)c->d_q, sigma, c->N, c->n_phi, total);
    c2_dft(c, c->d_c, c->d_a, 0);
    c2_hankel(c, c->d_a, c->d_b, 1);
    c2_dft(c, c->d_b, c->d_c, 1);
    hipLaunchKernelGGL(k2d_sw_mask, dim3((unsigned)c->B), dim3(256), 0, c->stream, (const double2*)c->d_c, c->r_swnew, threshold, c->N, c->n_phi);
    hipLaunchKernelGGL(k2d_rs_support, rs_grid_points(c), dim3(256), 0, c->stream, (const uint8_t*)c->r_swnew, (const uint8_t*)c->r_S0, c->r_sup,
                       c->r_steps > 0 ? (const double*)(c->r_hmain + (size_t)(c->r_steps - 1) * c->B) : (const double*)nullptr, error_limit, c->r_enf,
                       (long long)c->N * c->n_phi);
    MTIP_HIP_CHECK(c, hipGetLastError());
    if (enforced) MTIP_HIP_CHECK(c, mtip_copy(c->stream, enforced, c->r_enf, (size_t)c->B));
    return MTIP_OK;
}

int mtip2d_refresh_reciprocal_density(mtip2d_ctx* c) {
    if (!c) return MTIP_EINVAL;
    int r = rs_require_state(c, "refresh_reciprocal_density");
    if (r) return r;
    const size_t bytes = (size_t)c->B * c->N * c->n_phi * sizeof(double2);
    rs_ft(c, c->r_R[c->r_cur], c->d_c, 0);
    if ((r = rs_copy_d2d(c, c->r_F[c->r_cur], c->r_R[c->r_cur], bytes))) return r;
    if ((r = rs_copy_d2d(c, c->r_R[c->r_cur], c->d_c, bytes))) return r;
    rs_refresh_coefficients(c);
    MTIP_HIP_CHECK(c, hipGetLastError());
    return MTIP_OK;
}

int mtip2d_begin_sub_loop(mtip2d_ctx* c) {
    if (!c) return MTIP_EINVAL;
    int r = rs_require_state(c, "begin_sub_loop");
    if (r) return r;
    const size_t bytes = (size_t)c->B * c->N * c->n_phi * sizeof(double2);
    if ((r = rs_copy_d2d(c, c->r_F[1 - c->r_cur], c->r_F[c->r_cur], bytes))) return r;
    if ((r = rs_copy_d2d(c, c->r_R[1 - c->r_cur], c->r_R[c->r_cur], bytes))) return r;
    c->r_fixed_valid = false;
    return MTIP_OK;
}

int mtip2d_select_best_where(mtip2d_ctx* c, const uint8_t* select) {
    if (!c) return MTIP_EINVAL;
    int r = rs_require_state(c, "select_best");
    if (r) return r;
    if (select) MTIP_HIP_CHECK(c, mtip_copy(c->stream, c->r_sel, select, (size_t)c->B));
    hipLaunchKernelGGL(k2d_rs_select, rs_grid_points(c), dim3(256), 0, c->stream, select ? (const uint8_t*)c->r_sel : (const uint8_t*)nullptr,
                       c->r_F[c->r_cur], c->r_R[c->r_cur], c->r_sup, (const double2*)c->r_bestF, (const double2*)c->r_bestR,
                       (const uint8_t*)c->r_bestsup, (long long)c->N * c->n_phi);
    rs_refresh_coefficients(c);
    MTIP_HIP_CHECK(c, hipGetLastError());
    return MTIP_OK;
}

int mtip2d_select_best(mtip2d_ctx* c) { return mtip2d_select_best_where(c, nullptr); }

/* ---- results */
static int rs_get(mtip2d_ctx* c, int batch, int which, void* out, const void* latest, const void* best, size_t elem) {
    int r = rs_require_state(c, "get");
    if (r) return r;
    if (batch < 0 || batch >= c->B || which < 0 || which > 1 || !out) C2_FAIL(c, MTIP_EINVAL, "get: batch index, which = 0 (latest) / 1 (best), buffer not null");
    const size_t G = (size_t)c->N * c->n_phi;
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, out, (const char*)(which ? best : latest) + (size_t)batch * G * elem, G * elem));
    return MTIP_OK;
}

int mtip2d_get_density(mtip2d_ctx* c, int batch, int which, mtip_cdouble* rho) {
    if (!c) return MTIP_EINVAL;
    return rs_get(c, batch, which, rho, c->r_R[c->r_cur], c->r_bestR, sizeof(double2));
}

int mtip2d_get_reciprocal_density(mtip2d_ctx* c, int batch, int which, mtip_cdouble* F) {
    if (!c) return MTIP_EINVAL;
    return rs_get(c, batch, which, F, c->r_F[c->r_cur], c->r_bestF, sizeof(double2));
}

int mtip2d_get_support(mtip2d_ctx* c, int batch, int which, uint8_t* support) {
    if (!c) return MTIP_EINVAL;
    return rs_get(c, batch, which, support, c->r_sup, c->r_bestsup, 1);
}

int mtip2d_get_unknowns(mtip2d_ctx* c, int batch, mtip_cdouble* unknowns) {
    if (!c) return MTIP_EINVAL;
    int r = rs_require_state(c, "get_unknowns");
    if (r) return r;
    if (batch < 0 || batch >= c->B || !unknowns || c->n_used == 0) C2_FAIL(c, MTIP_EINVAL, "get_unknowns: batch index / null buffer / no projection");
    MTIP_HIP_CHECK(c, mtip_copy(c->stream, unknowns, c->r_unk + (size_t)batch * c->n_used, (size_t)c->n_used * sizeof(double2)));
    return MTIP_OK;
}

int mtip2d_get_best_error(mtip2d_ctx* c, double* best_error, int64_t* n_steps_done) {
    if (!c) return MTIP_EINVAL;
    int r = rs_require_state(c, "get_best_error");
    if (r) return r;
    if (best_error) MTIP_HIP_CHECK(c, mtip_copy(c->stream, best_error, c->r_besterr, (size_t)c->B * sizeof(double)));
    if (n_steps_done) *n_steps_done = c->r_steps;
    return MTIP_OK;
}

int mtip2d_synchronize(mtip2d_ctx* c) {
    if (!c) return MTIP_EINVAL;
    (void)hipSetDevice(c->device);
    MTIP_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return MTIP_OK;
}

}  // extern "C"

// ==== the averaging worker's grid arithmetic for dimensions = 2 (mtip2d_avg_*, mtip2d_op_grid_*) ==================================
#include "k_average2d.h"

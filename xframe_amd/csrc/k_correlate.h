// correlate: polar diffraction patterns -> averaged two-point cross-correlation C(q1, q2, Delta)  (gfx950, fp64, no library FFT)
//   xframe/projects/fxs/correlate.py:401-452                        process_image after the polar resampling
//                                   347-355                        per-pattern accumulation
//                                   249-270                        normalisation, symmetrisation, Fourier coefficients
//   xframe/projects/fxs/projectLibrary/cross_correlation.py        ccf_analysis
// Included by k_extract.hip (its entry points stand beside mtip_op_cc_to_deg2).  Per batch of patterns, in chunks of COR_CHUNK:
//   k_corr_stats   one workgroup per (pattern, ring): the average_sigma pixel filter and the ring sums the pattern-wide decisions need
//                  (a handle made with filter_kind = 2 launches k_corr_stats_mad of k_ringfilter.h in its place: the median_mad filter,
//                  exact order statistics by a radix select, the same three output arrays)
//   k_corr_ring    one workgroup per (pattern, ring): fully-masked / ROI decisions, ROI normalisation, the correction factor table,
//                  waxs, and the forward real FFTs F = rfft(image), G = rfft(mask); flags and waxs stay on the device
//   k_corr_pair    a wave owns one pair (q1, q2) with its whole Delta axis: sum (f64) and count (int32) sit in its registers while it
//                  walks the chunk's patterns IN PATTERN ORDER; the global accumulators are read and written once per chunk, not
//                  once per pattern.  D = irfft(conj F[q1] F[q2]) and M = irfft(conj G[q1] G[q2]) are each one complex FFT of
//                  n_phi / 2 points (even samples in the real part, odd ones in the imaginary part) in a wave-private piece of
//                  LDS: the lanes of one wave hand data to each other there, so no workgroup barrier is inside the loop.
//   k_corr_final   ccf = sum / count (NaN where count = 0), symmetrize_ccf, fft(ccf)[..., :fc_n_max]
// These take n_phi = 16, 32, .. 1024: their three transforms are radix 2.  A handle made by mtip_correlate_create_ex with
// MTIP_CORRELATE_GENERAL_NPHI takes every even n_phi in 16 .. 2048 with no prime factor above 5 (1536, the reference's default, among
// them): k_corr_ring_g / k_corr_pair_g / k_corr_final_g are the same kernel bodies with the mixed-radix transforms of k_correlate_mr.h
// (radices 4, 2, 3, 5 by a plan made once per handle).  The pair kernel keeps its shape there: a wave per pair, sum and count in
// registers across the chunk, the transform in a wave-private piece of LDS with no workgroup barrier in the pattern loop; rows of
// 64 lanes may be partial (n_phi / 2 need not be a multiple of 64, nor even), its LDS is dynamic (49 n_phi bytes: 98 KB at 2048).
// Such a handle with a power of two up to 1024 launches the radix-2 kernels.  Still refused: odd lengths, lengths below 16 or
// above 2048, prime factors above 5.  A handle made with MTIP_CORRELATE_ANY_NPHI takes those prime factors too, every even n_phi in
// 16 .. 2048: k_corr_ring_b / k_corr_pair_b / k_corr_final_b are the same bodies again with the chirp-z (Bluestein) transform of
// k_correlate_bs.h, a circular convolution of Mc >= n_phi - 1 points (Mc the smallest 2-3-5-smooth length) by the mixed-radix stages.
// The route follows from n_phi alone: a power of two up to 1024 launches the radix-2 kernels, a 2-3-5-smooth length the _g kernels,
// anything else the _b kernels (n_phi is smooth exactly when n_phi / 2 is, so one test serves all three).  The pair kernel keeps
// its shape there as well; a wave's buffer is Mc points, its LDS 80 Mc bytes (all 160 KB of a compute unit at Mc = 2048), and the
// read-only tables a transform touches once per point (chirp, B, the fold's twiddles) are read from global memory.
//
// THE ONE DEVIATION from the reference: it tests M != 0 on a value that is an integer pair count plus FFT rounding, and so divides
// noise by noise where the true count is 0 without a whole ring being masked.  Here the test is |M| >= 0.5: masks are 0 / 1, M is an
// integer up to rounding.  A fully masked ring gives exact zeros on both sides, so wherever the reference is deterministic the two
// agree.  (Not reproduced either: process_batch tests isgood_vals[i] with the index inside a sub-batch, correlate.py:347; here a
// pattern's own flag decides.)
#pragma once
#include <cstring>

#define COR_WAVES 4                    // pairs per workgroup: one per wave
#define COR_MAX_NPHI 1024
#define COR_MIN_NPHI 16
#define COR_CHUNK 32                   // patterns per pass over the accumulators (work arrays are sized by it)
#define COR_RT 256                     // threads of the ring / final kernels
#define COR_MODE_PATTERN 0             // M from every pattern's own mask
#define COR_MODE_SHARED 1              // M read from the handle's table
#define COR_MODE_MASK_ONLY 2           // fill that table

#include "k_correlate_mr.h"
#include "k_correlate_bs.h"

#define COR_XF_R2 0                    // the transform of a kernel body: radix 2,
#define COR_XF_MR 1                    // the handle's mixed-radix plan (k_correlate_mr.h),
#define COR_XF_BS 2                    // or its chirp-z convolution (k_correlate_bs.h)

struct mtip_correlate {
    mtip_ctx* c = nullptr;
    mtip_correlate_cfg cfg{};
    int m = 0, log2n = 0;              // n_phi / 2
    bool general = false;              // the mixed-radix kernels (create_ex with MTIP_CORRELATE_GENERAL_NPHI, n_phi not 16, 32, .. 1024)
    CorPlanArgs pl_n{}, pl_m{};        // their plans for n_phi and for n_phi / 2 points
    DevBuf<uint16_t> d_perm;           // the two digit-reversal tables: n_phi entries, then n_phi / 2
    bool bluestein = false;            // the chirp-z kernels (create_ex with MTIP_CORRELATE_ANY_NPHI, n_phi / 2 has a prime factor above 5)
    CorBsArgs bs{};                    // their plan for n_phi / 2 points
    DevBuf<double2> d_bs;              // its tables: Mc twiddles, B (Mc), the chirp (n_phi / 2)
    size_t n_acc = 0;                  // n_q1 n_q2 n_phi
    DevBuf<double> d_sum;
    DevBuf<int> d_cnt;
    DevBuf<double> d_M;                // shared mask: M(q1, q2, Delta), filled by the first batch
    bool have_M = false;
    DevBuf<int> d_q1, d_q2;
    DevBuf<double> d_factor;           // (n_q, n_phi) polarisation x solid angle
    DevBuf<double2> d_tw;              // exp(-2 pi i k / n_phi), k < n_phi / 2 (general: k < n_phi)
    DevBuf<double2> d_F, d_G;          // (COR_CHUNK, n_q, m + 1)
    DevBuf<uint8_t> d_mw;              // (COR_CHUNK, n_q, n_phi) filtered masks
    DevBuf<double> d_rc, d_rs;         // (COR_CHUNK, n_q) ring mask counts / masked ring sums
    std::vector<int32_t> good;         // every pattern added or merged so far
    std::vector<double> waxs;
};

__device__ __forceinline__ int cor_brev(unsigned v, int bits) {
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    v = (v >> 16) | (v << 16);
    return (int)(v >> (32 - bits));
}

// sum over the workgroup (COR_RT threads), the same value and the same order in every thread
__device__ __forceinline__ double cor_block_sum(double v, double* s_red, int tid) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((tid & 63) == 0) s_red[tid >> 6] = v;
    __syncthreads();
    return (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}

// forward DFT (sign -) of n = 2^log2n points that sit bit-reversed in buf, by the whole workgroup; tw[k] = exp(-2 pi i k / n)
__device__ __forceinline__ void cor_block_fft(double2* buf, int n, int log2n, const double2* tw, int tid) {
    __syncthreads();
    for (int s = 0; s < log2n; ++s) {
        const int half = 1 << s;
        for (int t = tid; t < (n >> 1); t += COR_RT) {
            const int pos = t & (half - 1), i = ((t >> s) << (s + 1)) + pos, j = i + half;
            const double2 w = tw[pos << (log2n - 1 - s)];
            const double2 x = buf[i], y = cmul(buf[j], w);
            buf[i] = cadd(x, y);
            buf[j] = csub(x, y);
        }
        __syncthreads();
    }
}

struct CorRingArgs {
    const double* img;                 // (P, n_q, n_phi) this chunk's patterns; null: only the mask transform (shared mask set-up)
    const uint8_t* mask;               // (P or 1, n_q, n_phi)
    size_t mask_stride;                // n_q n_phi, or 0 for a shared mask
    uint8_t* mw;
    double *rc, *rs;
    const double* factor;
    const double2* tw;
    double2 *F, *G;
    int* good;                         // (P)
    double* waxs;                      // (P, n_q)
    int n_q, n_phi, log2n, filter, roi_lo, roi_hi, roi_filter, roi_norm, do_G;
    double filter_k, roi_min, roi_max;
};

// the average_sigma filter of one ring (correlate.py:402-413, 458-461) and the ring sums of the pattern-wide decisions
__global__ void __launch_bounds__(COR_RT) k_corr_stats(CorRingArgs a) {
    __shared__ double s_red[COR_WAVES];
    const int tid = threadIdx.x, q = blockIdx.x, p = blockIdx.y;
    const double* row = a.img + ((size_t)p * a.n_q + q) * a.n_phi;
    const uint8_t* mrow = a.mask + (size_t)p * a.mask_stride + (size_t)q * a.n_phi;
    double cnt = 0.0, sum = 0.0;
    for (int j = tid; j < a.n_phi; j += COR_RT)
        if (mrow[j]) {
            cnt += 1.0;
            sum += row[j];
        }
    cnt = cor_block_sum(cnt, s_red, tid);
    sum = cor_block_sum(sum, s_red, tid);
    if (a.filter) {
        const double mean = sum / cnt;                                  // NaN for an empty ring, as np.mean gives
        double var = 0.0;
        for (int j = tid; j < a.n_phi; j += COR_RT)
            if (mrow[j]) {
                const double d = row[j] - mean;
                var += d * d;
            }
        const double thr = a.filter_k * sqrt(cor_block_sum(var, s_red, tid) / cnt);   // np.std: ddof 0
        uint8_t* wrow = a.mw + ((size_t)p * a.n_q + q) * a.n_phi;
        cnt = sum = 0.0;
        for (int j = tid; j < a.n_phi; j += COR_RT) {
            const uint8_t keep = (mrow[j] && !(fabs(row[j] - mean) > thr)) ? 1 : 0;
            wrow[j] = keep;
            if (keep) {
                cnt += 1.0;
                sum += row[j];
            }
        }
        cnt = cor_block_sum(cnt, s_red, tid);
        sum = cor_block_sum(sum, s_red, tid);
    }
    if (tid == 0) {
        a.rc[(size_t)p * a.n_q + q] = cnt;
        a.rs[(size_t)p * a.n_q + q] = sum;
    }
}

#include "k_ringfilter.h"

// sample j of a real row of n_phi points on its way into the transform, that transform, and point k of its spectrum: radix 2 or the
// handle's mixed-radix plan (the sample at its bit- or digit-reversed place, an n_phi-point transform), or the chirp-z convolution
// (sample j is part j & 1 of point j / 2 of an n_phi / 2-point transform, whose spectrum cor_bs_unfold takes apart)
template <int XF>
__device__ __forceinline__ void cor_store_sample(const CorPlanArgs* pl, double2* buf, int j, int log2n, double v) {
    if constexpr (XF == COR_XF_BS) ((double*)buf)[j] = v;
    else if constexpr (XF == COR_XF_MR) buf[pl->perm[j]] = make_double2(v, 0.0);
    else buf[cor_brev((unsigned)j, log2n)] = make_double2(v, 0.0);
}
template <int XF>
__device__ __forceinline__ void cor_ring_fft(const CorPlanArgs* pl, const CorBsArgs* bs, double2* buf, int n, int log2n, const double2* tw,
                                             int tid) {
    if constexpr (XF == COR_XF_BS) cor_block_fft_b(buf, n >> 1, *bs, tid, COR_RT);
    else if constexpr (XF == COR_XF_MR) cor_block_fft_g(buf, pl->st, tw, tid, COR_RT);
    else cor_block_fft(buf, n, log2n, tw, tid);
}
template <int XF>
__device__ __forceinline__ double2 cor_spectrum(const double2* buf, const double2* tw, int n, int k) {
    if constexpr (XF == COR_XF_BS) return cor_bs_unfold(buf, tw, n >> 1, k);
    else return buf[k];
}

// correlate.py:416-450 for one ring of one pattern, then rfft of the image and of the mask along phi
template <int XF>
__device__ __forceinline__ void cor_ring_body(const CorRingArgs a, const CorPlanArgs* pl, const CorBsArgs* bs, double2* s_buf, double* s_red) {
    const int tid = threadIdx.x, q = blockIdx.x, p = blockIdx.y, m = a.n_phi >> 1;
    const uint8_t* mrow = a.filter ? a.mw + ((size_t)p * a.n_q + q) * a.n_phi : a.mask + (size_t)p * a.mask_stride + (size_t)q * a.n_phi;
    if (a.img != nullptr) {
        double tot = 0.0, rs = 0.0, rc = 0.0;
        for (int r = tid; r < a.n_q; r += COR_RT) {
            tot += a.rc[(size_t)p * a.n_q + r];
            if (r >= a.roi_lo && r < a.roi_hi) {
                rc += a.rc[(size_t)p * a.n_q + r];
                rs += a.rs[(size_t)p * a.n_q + r];
            }
        }
        tot = cor_block_sum(tot, s_red, tid);
        if (tot == 0.0) {                                               // a completely masked image (418-421)
            if (tid == 0) {
                a.waxs[(size_t)p * a.n_q + q] = 0.0;
                if (q == 0) a.good[p] = 0;
            }
            return;
        }
        int good = 1;
        double roi_mean = 1.0;
        if (a.roi_filter || a.roi_norm) {
            rs = cor_block_sum(rs, s_red, tid);
            rc = cor_block_sum(rc, s_red, tid);
            roi_mean = rs / rc;                                         // 425
            if (a.roi_filter && (roi_mean < a.roi_min || roi_mean > a.roi_max)) good = 0;   // 427-429
        }
        const double* row = a.img + ((size_t)p * a.n_q + q) * a.n_phi;
        const double* frow = a.factor ? a.factor + (size_t)q * a.n_phi : nullptr;
        double ws = 0.0;
        for (int j = tid; j < a.n_phi; j += COR_RT) {
            double v = row[j];
            if (a.filter && !mrow[j]) v = 0.0;                          // 413: image *= mask, only behind the filter
            if (a.roi_norm) v = v / roi_mean;                           // 431-432
            if (frow) v *= frow[j];                                     // 434-438
            if (mrow[j]) ws += v;
            cor_store_sample<XF>(pl, s_buf, j, a.log2n, v);
        }
        ws = cor_block_sum(ws, s_red, tid);
        if (tid == 0) {
            a.waxs[(size_t)p * a.n_q + q] = ws / a.rc[(size_t)p * a.n_q + q];   // 446, 466: NaN for a fully masked ring
            if (q == 0) a.good[p] = good;
        }
        if (!good) return;                                              // the pair kernel skips the pattern
        cor_ring_fft<XF>(pl, bs, s_buf, a.n_phi, a.log2n, a.tw, tid);
        double2* F = a.F + ((size_t)p * a.n_q + q) * (m + 1);
        for (int k = tid; k <= m; k += COR_RT) F[k] = cor_spectrum<XF>(s_buf, a.tw, a.n_phi, k);
        __syncthreads();
    }
    if (a.do_G) {
        for (int j = tid; j < a.n_phi; j += COR_RT) cor_store_sample<XF>(pl, s_buf, j, a.log2n, mrow[j] ? 1.0 : 0.0);
        cor_ring_fft<XF>(pl, bs, s_buf, a.n_phi, a.log2n, a.tw, tid);
        double2* G = a.G + ((size_t)p * a.n_q + q) * (m + 1);
        for (int k = tid; k <= m; k += COR_RT) G[k] = cor_spectrum<XF>(s_buf, a.tw, a.n_phi, k);
    }
}
__global__ void __launch_bounds__(COR_RT) k_corr_ring(CorRingArgs a) {
    __shared__ double2 s_buf[COR_MAX_NPHI];
    __shared__ double s_red[COR_WAVES];
    cor_ring_body<COR_XF_R2>(a, nullptr, nullptr, s_buf, s_red);
}
__global__ void __launch_bounds__(COR_RT) k_corr_ring_g(CorRingArgs a, CorPlanArgs pl) {
    __shared__ double2 s_buf[COR_G_MAX_NPHI];
    __shared__ double s_red[COR_WAVES];
    cor_ring_body<COR_XF_MR>(a, &pl, nullptr, s_buf, s_red);
}
// (s_buf: the Mc <= 2048 points of the convolution)
__global__ void __launch_bounds__(COR_RT) k_corr_ring_b(CorRingArgs a, CorBsArgs bs) {
    __shared__ double2 s_buf[COR_G_MAX_NPHI];
    __shared__ double s_red[COR_WAVES];
    cor_ring_body<COR_XF_BS>(a, nullptr, &bs, s_buf, s_red);
}

struct CorPairArgs {
    const double2 *F, *G;              // (P, n_q, m + 1)
    const double2* tw;
    const int* good;                   // (P)
    const int *q1, *q2;
    double* sum;
    int* cnt;
    double* M;                         // shared-mask table
    int n_q, n_q2, m, log2m, P, mode;
    long long npairs;
    double inv_n;
};

// x = irfft(conj(A[q1]) A[q2], n) times n, by one wave: with X the product spectrum and Xr[k] = conj(X[m - k]) the even and odd samples
// have the m-point spectra  E = (X + Xr) / 2,  O = (X - Xr) / 2 exp(+2 pi i k / n);  the inverse m-point DFT of E + i O holds x[2 j] in its
// real and x[2 j + 1] in its imaginary part.  (The factor 1 / 2 is left to the caller: out = 2 m x = n x.)
// lane l gets the samples 2 j, 2 j + 1 of j = l + 64 r in out[2 r], out[2 r + 1].
template <int NPL>
__device__ __forceinline__ void cor_wave_irfft(double2* buf, const double2* s_tw, const double2* a1, const double2* a2, int m, int log2m,
                                               int lane, double* out) {
#pragma unroll
    for (int r = 0; r < NPL; ++r) {
        const int k = lane + 64 * r;
        if (k < m) {
            const double2 x = cmulc(a2[k], a1[k]);                      // conj(a1) a2
            const double2 xr = cmulc(a1[m - k], a2[m - k]);             // conj(conj(a1) a2) at m - k
            const double2 e = cadd(x, xr), d = csub(x, xr), w = s_tw[k];
            const double2 o = make_double2(d.x * w.x + d.y * w.y, d.y * w.x - d.x * w.y);   // d conj(w)
            buf[cor_brev((unsigned)k, log2m)] = make_double2(e.x - o.y, e.y + o.x);
        }
    }
    MTIP_WAVE_LDS_SYNC();
    for (int s = 0; s < log2m; ++s) {
        const int half = 1 << s;
#pragma unroll
        for (int r = 0; r < (NPL > 1 ? NPL / 2 : 1); ++r) {
            const int t = lane + 64 * r;
            if (t < (m >> 1)) {
                const int pos = t & (half - 1), i = ((t >> s) << (s + 1)) + pos, j = i + half;
                const double2 w = s_tw[pos << (log2m - s)];             // conj below: the inverse transform
                const double2 x = buf[i], v = buf[j];
                const double2 y = make_double2(v.x * w.x + v.y * w.y, v.y * w.x - v.x * w.y);
                buf[i] = cadd(x, y);
                buf[j] = csub(x, y);
            }
        }
        MTIP_WAVE_LDS_SYNC();
    }
#pragma unroll
    for (int r = 0; r < NPL; ++r) {
        const int j = lane + 64 * r;
        const double2 z = j < m ? buf[j] : make_double2(0.0, 0.0);
        out[2 * r] = z.x;
        out[2 * r + 1] = z.y;
    }
    MTIP_WAVE_LDS_SYNC();
}

// NPL: rows of 64 lanes that hold the m points of a pair (the last one may be partial).  COR_XF_MR: s_tw has n_phi entries, s_perm the
// plan's digit reversal of m points.  COR_XF_BS: s_tw has the Mc twiddles of the convolution, a wave's buffer Mc points; the
// read-only tables that are touched once per point (a.tw, the chirp, B) stay in global memory
template <int NPL, int XF>
__device__ __forceinline__ void cor_pair_irfft(double2* buf, const double2* s_tw, const uint16_t* s_perm, const CorPlanArgs* pl,
                                               const CorBsArgs* bs, const double2* tw_n, const double2* a1, const double2* a2, int m,
                                               int log2m, int lane, double* out) {
    if constexpr (XF == COR_XF_BS) cor_wave_irfft_b<NPL>(buf, s_tw, tw_n, *bs, a1, a2, m, lane, out);
    else if constexpr (XF == COR_XF_MR) cor_wave_irfft_g<NPL>(buf, s_tw, s_perm, pl->st, a1, a2, m, lane, out);
    else cor_wave_irfft<NPL>(buf, s_tw, a1, a2, m, log2m, lane, out);
}
template <int NPL, int XF>
__device__ __forceinline__ void cor_pair_body(const CorPairArgs a, const CorPlanArgs* pl, const CorBsArgs* bs, double2* s_fft, double2* s_tw,
                                              uint16_t* s_perm) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), m = a.m;
    if constexpr (XF == COR_XF_BS) {
        for (int k = tid; k < bs->Mc; k += COR_WAVES * 64) s_tw[k] = bs->tw[k];
    } else {
        for (int k = tid; k < (XF == COR_XF_MR ? 2 * m : m); k += COR_WAVES * 64) s_tw[k] = a.tw[k];
    }
    if constexpr (XF == COR_XF_MR)
        for (int k = tid; k < m; k += COR_WAVES * 64) s_perm[k] = pl->perm[k];
    __syncthreads();
    double2* buf;
    if constexpr (XF == COR_XF_BS) buf = s_fft + wave * bs->Mc;
    else buf = s_fft + wave * m;
    const size_t row_len = (size_t)(m + 1), pat_len = (size_t)a.n_q * row_len;
    for (long long base = (long long)blockIdx.x * COR_WAVES; base < a.npairs; base += (long long)gridDim.x * COR_WAVES) {
        const long long pair = base + wave;
        if (pair >= a.npairs) continue;                                 // wave-uniform
        const int i1 = (int)(pair / a.n_q2), i2 = (int)(pair - (long long)i1 * a.n_q2);
        const size_t r1 = (size_t)a.q1[i1] * row_len, r2 = (size_t)a.q2[i2] * row_len;
        double2* gsum = (double2*)(a.sum + (size_t)pair * 2 * m);
        int2* gcnt = (int2*)(a.cnt + (size_t)pair * 2 * m);
        double2* gM = (double2*)(a.M + (size_t)pair * 2 * m);
        double sum[2 * NPL], d[2 * NPL], mm[2 * NPL];
        int cnt[2 * NPL];
        if (a.mode == COR_MODE_MASK_ONLY) {
            cor_pair_irfft<NPL, XF>(buf, s_tw, s_perm, pl, bs, a.tw, a.G + r1, a.G + r2, m, a.log2m, lane, mm);
#pragma unroll
            for (int r = 0; r < NPL; ++r) {
                const int j = lane + 64 * r;
                if (j < m) gM[j] = make_double2(mm[2 * r] * a.inv_n, mm[2 * r + 1] * a.inv_n);
            }
            continue;
        }
#pragma unroll
        for (int r = 0; r < NPL; ++r) {
            const int j = lane + 64 * r;
            const bool in = j < m;
            const double2 s = in ? gsum[j] : make_double2(0.0, 0.0);
            const int2 n = in ? gcnt[j] : make_int2(0, 0);
            sum[2 * r] = s.x;
            sum[2 * r + 1] = s.y;
            cnt[2 * r] = n.x;
            cnt[2 * r + 1] = n.y;
            if (a.mode == COR_MODE_SHARED) {
                const double2 v = in ? gM[j] : make_double2(0.0, 0.0);
                mm[2 * r] = v.x;
                mm[2 * r + 1] = v.y;
            }
        }
        for (int p = 0; p < a.P; ++p) {
            if (!a.good[p]) continue;                                   // bad patterns contribute nothing (correlate.py:347)
            const double2* Fp = a.F + (size_t)p * pat_len;
            cor_pair_irfft<NPL, XF>(buf, s_tw, s_perm, pl, bs, a.tw, Fp + r1, Fp + r2, m, a.log2m, lane, d);
            if (a.mode == COR_MODE_PATTERN) {
                const double2* Gp = a.G + (size_t)p * pat_len;
                cor_pair_irfft<NPL, XF>(buf, s_tw, s_perm, pl, bs, a.tw, Gp + r1, Gp + r2, m, a.log2m, lane, mm);
#pragma unroll
                for (int e = 0; e < 2 * NPL; ++e) mm[e] *= a.inv_n;
            }
#pragma unroll
            for (int e = 0; e < 2 * NPL; ++e)
                if (fabs(mm[e]) >= 0.5) {                               // M is an integer pair count up to rounding
                    sum[e] += (d[e] * a.inv_n) / mm[e];
                    cnt[e] += 1;
                }
        }
#pragma unroll
        for (int r = 0; r < NPL; ++r) {
            const int j = lane + 64 * r;
            if (j < m) {
                gsum[j] = make_double2(sum[2 * r], sum[2 * r + 1]);
                gcnt[j] = make_int2(cnt[2 * r], cnt[2 * r + 1]);
            }
        }
    }
}
template <int NPL>
__global__ void __launch_bounds__(COR_WAVES * 64) k_corr_pair(CorPairArgs a) {
    __shared__ double2 s_fft[COR_WAVES * (COR_MAX_NPHI / 2)];
    __shared__ double2 s_tw[COR_MAX_NPHI / 2];
    cor_pair_body<NPL, COR_XF_R2>(a, nullptr, nullptr, s_fft, s_tw, nullptr);
}
// dynamic LDS: twiddles (n_phi), COR_WAVES wave-private transforms (m each), the digit reversal (m uint16): cor_pair_lds bytes.  Four
// waves are one per SIMD, so the 16 rows of n_phi = 2048 (64 accumulator doubles and 32 counts per lane) have the whole register file.
template <int NPL>
__global__ void __launch_bounds__(COR_WAVES * 64) k_corr_pair_g(CorPairArgs a, CorPlanArgs pl) {
    HIP_DYNAMIC_SHARED(double2, sm)
    cor_pair_body<NPL, COR_XF_MR>(a, &pl, nullptr, sm + 2 * a.m, sm, (uint16_t*)(sm + (2 + COR_WAVES) * a.m));
}
static inline size_t cor_pair_lds(int m) { return (size_t)(2 + COR_WAVES) * m * sizeof(double2) + (((size_t)m * sizeof(uint16_t) + 15) & ~(size_t)15); }
// dynamic LDS: the Mc twiddles, then COR_WAVES wave-private convolutions of Mc points: cor_pair_lds_b bytes, 80 Mc (all 160 KB of a
// compute unit at Mc = 2048, n_phi = 2018 .. 2046)
template <int NPL>
__global__ void __launch_bounds__(COR_WAVES * 64) k_corr_pair_b(CorPairArgs a, CorBsArgs bs) {
    HIP_DYNAMIC_SHARED(double2, sm)
    cor_pair_body<NPL, COR_XF_BS>(a, nullptr, &bs, sm + bs.Mc, sm, nullptr);
}
static inline size_t cor_pair_lds_b(int Mc) { return (size_t)(1 + COR_WAVES) * Mc * sizeof(double2); }

__global__ void k_corr_merge(double* sum, int* cnt, const double* sum_in, const int* cnt_in, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        sum[i] += sum_in[i];
        cnt[i] += cnt_in[i];
    }
}

struct CorFinalArgs {
    const double* sum;
    const int* cnt;
    const double2* tw;
    double* ccf;                       // (pairs, n_phi) or null
    double2* fc;                       // (pairs, fc_n) or null
    int n_phi, log2n, symmetrize, pos_pi2, pos_pi, pos_3pi2, fc_n;
};

// correlate.py:258-270: sum / count with NaN where nothing was counted, symmetrize_ccf (cross_correlation.py:67-78), fft[..., :fc_n]
template <int XF>
__device__ __forceinline__ void cor_final_body(const CorFinalArgs& a, const CorPlanArgs* pl, const CorBsArgs* bs, double2* s_buf) {
    const int tid = threadIdx.x;
    const size_t row = (size_t)blockIdx.x * a.n_phi;
    for (int j = tid; j < a.n_phi; j += COR_RT) {
        int src = j;
        if (a.symmetrize) {
            if (j < a.pos_pi2) src = j + a.pos_pi;
            else if (j > a.pos_3pi2) src = j - a.pos_pi;
        }
        const int n = a.cnt[row + src];
        const double v = n != 0 ? a.sum[row + src] / (double)n : __builtin_nan("");
        if (a.ccf) a.ccf[row + j] = v;
        cor_store_sample<XF>(pl, s_buf, j, a.log2n, v);
    }
    if (a.fc == nullptr) return;
    cor_ring_fft<XF>(pl, bs, s_buf, a.n_phi, a.log2n, a.tw, tid);
    for (int k = tid; k < a.fc_n; k += COR_RT) a.fc[(size_t)blockIdx.x * a.fc_n + k] = cor_spectrum<XF>(s_buf, a.tw, a.n_phi, k);
}
__global__ void __launch_bounds__(COR_RT) k_corr_final(CorFinalArgs a) {
    __shared__ double2 s_buf[COR_MAX_NPHI];
    cor_final_body<COR_XF_R2>(a, nullptr, nullptr, s_buf);
}
__global__ void __launch_bounds__(COR_RT) k_corr_final_g(CorFinalArgs a, CorPlanArgs pl) {
    __shared__ double2 s_buf[COR_G_MAX_NPHI];
    cor_final_body<COR_XF_MR>(a, &pl, nullptr, s_buf);
}
__global__ void __launch_bounds__(COR_RT) k_corr_final_b(CorFinalArgs a, CorBsArgs bs) {
    __shared__ double2 s_buf[COR_G_MAX_NPHI];
    cor_final_body<COR_XF_BS>(a, nullptr, &bs, s_buf);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
// a copy between the caller's buffer (host or device memory) and a host vector of the handle
static inline hipError_t cor_host_copy(mtip_ctx* c, void* dst, const void* src, size_t n, const void* callers) {
#ifdef __HIPCC__
    if (mtip_is_device_pointer(callers)) return mtip_copy(c, dst, src, n, hipMemcpyDefault);
#endif
    (void)c;
    (void)callers;
    std::memcpy(dst, src, n);
    return hipSuccess;
}

extern "C" mtip_correlate* mtip_correlate_create_ex(mtip_ctx* c, const mtip_correlate_cfg* cfg, const int32_t* q1_pos,
                                                    const int32_t* q2_pos, const double* factor, uint32_t flags) {
    if (!c) return nullptr;
    char msg[400];
    if (!cfg || !q1_pos || !q2_pos || cfg->n_q < 1 || cfg->n_q1 < 1 || cfg->n_q2 < 1 || cfg->n_q > 65535 || cfg->n_q1 > 65535 ||
        cfg->n_q2 > 65535) {
        c->err = "correlate_create: null argument or a ring count outside 1 .. 65535";
        return nullptr;
    }
    if (flags & ~(uint32_t)(MTIP_CORRELATE_GENERAL_NPHI | MTIP_CORRELATE_ANY_NPHI)) {
        snprintf(msg, sizeof msg,
                 "correlate_create_ex: flags = 0x%x: only MTIP_CORRELATE_GENERAL_NPHI (bit 0) and MTIP_CORRELATE_ANY_NPHI (bit 2) are defined",
                 (unsigned)flags);
        c->err = msg;
        return nullptr;
    }
    const int n = cfg->n_phi;
    const bool radix2 = n >= COR_MIN_NPHI && n <= COR_MAX_NPHI && !(n & (n - 1));
    const bool any = (flags & MTIP_CORRELATE_ANY_NPHI) != 0;
    if (any && !cor_any_ok(n)) {
        snprintf(msg, sizeof msg, "correlate_create: n_phi = %d is not built; with MTIP_CORRELATE_ANY_NPHI: every even length %d .. %d", n,
                 COR_MIN_NPHI, COR_G_MAX_NPHI);
        c->err = msg;
        return nullptr;
    }
    const bool bluestein = any && !radix2 && !cor_general_ok(n);       // (n is smooth exactly when n / 2 is)
    if (!any && !(flags & MTIP_CORRELATE_GENERAL_NPHI) && !radix2) {
        snprintf(msg, sizeof msg, "correlate_create: n_phi = %d is not built; supported: 16, 32, 64, 128, 256, 512, 1024", n);
        c->err = msg;
        return nullptr;
    }
    if (!any && !radix2 && !cor_general_ok(n)) {
        int below, above;
        char lo[16] = "none", hi[16] = "none";
        cor_general_near(n, &below, &above);
        if (below) snprintf(lo, sizeof lo, "%d", below);
        if (above) snprintf(hi, sizeof hi, "%d", above);
        snprintf(msg, sizeof msg,
                 "correlate_create: n_phi = %d is not built; with MTIP_CORRELATE_GENERAL_NPHI: even lengths %d .. %d whose only prime "
                 "factors are 2, 3 and 5; the nearest below: %s, above: %s",
                 n, COR_MIN_NPHI, COR_G_MAX_NPHI, lo, hi);
        c->err = msg;
        return nullptr;
    }
    if (cfg->filter_kind < 0 || cfg->filter_kind > 2) {
        snprintf(msg, sizeof msg, "correlate_create: filter_kind = %d: it must be 0 (none), 1 (average_sigma) or 2 (median_mad)",
                 (int)cfg->filter_kind);
        c->err = msg;
        return nullptr;
    }
    for (int i = 0; i < cfg->n_q1 + cfg->n_q2; ++i) {
        const int q = i < cfg->n_q1 ? q1_pos[i] : q2_pos[i - cfg->n_q1];
        if (q < 0 || q >= cfg->n_q) {
            c->err = "correlate_create: a selected ring lies outside 0 .. n_q - 1";
            return nullptr;
        }
    }
    (void)hipSetDevice(c->device);
    mtip_correlate* h = new mtip_correlate;
    h->c = c;
    h->cfg = *cfg;
    h->m = n / 2;
    while ((1 << h->log2n) < n) ++h->log2n;
    h->n_acc = (size_t)cfg->n_q1 * cfg->n_q2 * n;
    const bool shared = cfg->shared_mask && !cfg->filter_kind;
    h->cfg.shared_mask = shared ? 1 : 0;
    const size_t rows = (size_t)COR_CHUNK * cfg->n_q, n_spec = rows * (h->m + 1), spec = n_spec * sizeof(double2);
    const size_t acc = h->n_acc * 12, tab = shared ? h->n_acc * 8 : 0;
    // (a mixed-radix handle's plan: twiddles of n_phi entries, digit reversals of n_phi and of n_phi / 2 points)
    // (a chirp-z handle's: twiddles of n_phi entries, and of the convolution's Mc; B; the chirp)
    const int Mc = bluestein ? cor_bs_length(h->m) : 0;
    const size_t plan = radix2      ? 0
                        : bluestein ? ((size_t)n + 2 * (size_t)Mc + h->m) * sizeof(double2)
                                    : (size_t)n * sizeof(double2) + ((size_t)n + h->m) * sizeof(uint16_t);
    const size_t work = spec * (shared ? 1 : 2) + spec / COR_CHUNK + rows * n + rows * 16 + (factor ? (size_t)cfg->n_q * n * 8 : 0) + plan;
    const size_t fr = mtip_free_memory();
    if (acc + tab + work > fr) {
        snprintf(msg, sizeof msg,
                 "correlate_create: the accumulator of %d x %d pairs x %d angles needs %.3f GB (sum f64 + count int32%s) and the work "
                 "arrays %.3f GB; %.3f GB of device memory are free",
                 cfg->n_q1, cfg->n_q2, n, (double)(acc + tab) * 1e-9, shared ? " + shared-mask table f64" : "", (double)work * 1e-9,
                 (double)fr * 1e-9);
        c->err = msg;
        delete h;
        return nullptr;
    }
    h->general = !radix2 && !bluestein;
    h->bluestein = bluestein;
    std::vector<double2> tw((size_t)(radix2 ? h->m : n));
    for (int k = 0; k < (int)tw.size(); ++k) {
        const long double ang = -2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)n;
        tw[k] = make_double2((double)cosl(ang), (double)sinl(ang));
    }
    std::vector<uint16_t> perm;
    if (h->general) {                                                   // the plan: stages and digit reversals of n and of n / 2 points
        h->pl_n.st = cor_make_stages(n, n);
        h->pl_m.st = cor_make_stages(h->m, n);
        perm.resize((size_t)n + h->m);
        cor_make_perm(h->pl_n.st, n, perm.data());
        cor_make_perm(h->pl_m.st, h->m, perm.data() + n);
    }
    std::vector<double2> bst;
    if (bluestein) {                                                    // the plan of the convolution and its tables
        h->bs.Mc = Mc;
        h->bs.st = cor_make_stages(Mc, Mc);
        bst.resize(2 * (size_t)Mc + h->m);
        cor_bs_tables(h->m, Mc, h->bs.st, bst.data(), bst.data() + Mc, bst.data() + 2 * (size_t)Mc);
    }
    hipError_t e = h->d_sum.alloc(h->n_acc);
    if (e == hipSuccess && bluestein) e = h->d_bs.alloc(bst.size());
    if (e == hipSuccess && bluestein) e = mtip_copy(c, h->d_bs, bst.data(), bst.size() * sizeof(double2), hipMemcpyHostToDevice);
    if (e == hipSuccess && bluestein) {
        h->bs.tw = h->d_bs;
        h->bs.B = h->d_bs + Mc;
        h->bs.chirp = h->d_bs + 2 * (size_t)Mc;
    }
    if (e == hipSuccess && h->general) e = h->d_perm.alloc(perm.size());
    if (e == hipSuccess && h->general) e = mtip_copy(c, h->d_perm, perm.data(), perm.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && h->general) {
        h->pl_n.perm = h->d_perm;
        h->pl_m.perm = h->d_perm + n;
    }
    if (e == hipSuccess) e = h->d_cnt.alloc(h->n_acc);
    if (e == hipSuccess && shared) e = h->d_M.alloc(h->n_acc);
    if (e == hipSuccess) e = h->d_q1.alloc((size_t)cfg->n_q1);
    if (e == hipSuccess) e = h->d_q2.alloc((size_t)cfg->n_q2);
    if (e == hipSuccess) e = h->d_tw.alloc(tw.size());
    if (e == hipSuccess) e = h->d_F.alloc(n_spec);
    if (e == hipSuccess) e = h->d_G.alloc(shared ? n_spec / COR_CHUNK : n_spec);
    if (e == hipSuccess && cfg->filter_kind) e = h->d_mw.alloc(rows * n);
    if (e == hipSuccess) e = h->d_rc.alloc(rows);
    if (e == hipSuccess) e = h->d_rs.alloc(rows);
    if (e == hipSuccess && factor) e = h->d_factor.alloc((size_t)cfg->n_q * n);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_sum, 0, h->n_acc * sizeof(double), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->d_cnt, 0, h->n_acc * sizeof(int), c->stream);
    if (e == hipSuccess) e = mtip_copy(c, h->d_q1, q1_pos, (size_t)cfg->n_q1 * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = mtip_copy(c, h->d_q2, q2_pos, (size_t)cfg->n_q2 * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = mtip_copy(c, h->d_tw, tw.data(), tw.size() * sizeof(double2), hipMemcpyHostToDevice);
    if (e == hipSuccess && factor) e = mtip_copy(c, h->d_factor, factor, (size_t)cfg->n_q * n * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        snprintf(msg, sizeof msg, "correlate_create: %s (accumulator %.3f GB)", hipGetErrorString(e), (double)(acc + tab) * 1e-9);
        c->err = msg;
        delete h;
        return nullptr;
    }
    return h;
}

extern "C" mtip_correlate* mtip_correlate_create(mtip_ctx* c, const mtip_correlate_cfg* cfg, const int32_t* q1_pos, const int32_t* q2_pos,
                                                 const double* factor) {
    return mtip_correlate_create_ex(c, cfg, q1_pos, q2_pos, factor, 0);
}

extern "C" void mtip_correlate_destroy(mtip_correlate* h) {
    if (!h) return;
    (void)hipSetDevice(h->c->device);
    (void)hipStreamSynchronize(h->c->stream);
    delete h;
}

static inline void cor_launch_ring(mtip_correlate* h, unsigned n_patterns, const CorRingArgs& r) {
    const dim3 g((unsigned)h->cfg.n_q, n_patterns), b(COR_RT);
    if (h->bluestein) hipLaunchKernelGGL(k_corr_ring_b, g, b, 0, h->c->stream, r, h->bs);
    else if (h->general) hipLaunchKernelGGL(k_corr_ring_g, g, b, 0, h->c->stream, r, h->pl_n);
    else hipLaunchKernelGGL(k_corr_ring, g, b, 0, h->c->stream, r);
}

static inline void cor_launch_pair(mtip_correlate* h, const CorPairArgs& a) {
    mtip_ctx* c = h->c;
    const unsigned grid = (unsigned)std::min<long long>(div_up(a.npairs, COR_WAVES), (long long)c->n_cu * 8);
    const dim3 g(grid), b(COR_WAVES * 64);
    if (h->bluestein) {
        const int rows = div_up(a.m, 64);
        const size_t lds = cor_pair_lds_b(h->bs.Mc);
        if (rows <= 1) hipLaunchKernelGGL(k_corr_pair_b<1>, g, b, lds, c->stream, a, h->bs);
        else if (rows <= 2) hipLaunchKernelGGL(k_corr_pair_b<2>, g, b, lds, c->stream, a, h->bs);
        else if (rows <= 4) hipLaunchKernelGGL(k_corr_pair_b<4>, g, b, lds, c->stream, a, h->bs);
        else if (rows <= 8) hipLaunchKernelGGL(k_corr_pair_b<8>, g, b, lds, c->stream, a, h->bs);
        else if (rows <= 12) hipLaunchKernelGGL(k_corr_pair_b<12>, g, b, lds, c->stream, a, h->bs);
        else hipLaunchKernelGGL(k_corr_pair_b<16>, g, b, lds, c->stream, a, h->bs);
        return;
    }
    if (h->general) {
        const int rows = div_up(a.m, 64);
        const size_t lds = cor_pair_lds(a.m);
        if (rows <= 1) hipLaunchKernelGGL(k_corr_pair_g<1>, g, b, lds, c->stream, a, h->pl_m);
        else if (rows <= 2) hipLaunchKernelGGL(k_corr_pair_g<2>, g, b, lds, c->stream, a, h->pl_m);
        else if (rows <= 4) hipLaunchKernelGGL(k_corr_pair_g<4>, g, b, lds, c->stream, a, h->pl_m);
        else if (rows <= 8) hipLaunchKernelGGL(k_corr_pair_g<8>, g, b, lds, c->stream, a, h->pl_m);
        else if (rows <= 12) hipLaunchKernelGGL(k_corr_pair_g<12>, g, b, lds, c->stream, a, h->pl_m);
        else hipLaunchKernelGGL(k_corr_pair_g<16>, g, b, lds, c->stream, a, h->pl_m);
        return;
    }
    const int npl = std::max(1, a.m / 64);
    if (npl == 1) hipLaunchKernelGGL(k_corr_pair<1>, g, b, 0, c->stream, a);
    else if (npl == 2) hipLaunchKernelGGL(k_corr_pair<2>, g, b, 0, c->stream, a);
    else if (npl == 4) hipLaunchKernelGGL(k_corr_pair<4>, g, b, 0, c->stream, a);
    else hipLaunchKernelGGL(k_corr_pair<8>, g, b, 0, c->stream, a);
}

extern "C" int mtip_correlate_add(mtip_correlate* h, int n_patterns, const double* images, const uint8_t* masks) {
    if (!h) return MTIP_EINVAL;
    mtip_ctx* c = h->c;
    if (n_patterns < 1 || !images || !masks) {
        c->err = "correlate_add: null buffer or no pattern";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    const mtip_correlate_cfg& f = h->cfg;
    const size_t ring = (size_t)f.n_q * f.n_phi;
    const bool shared = f.shared_mask != 0;
    DevView v_img(c, images, (size_t)n_patterns * ring * sizeof(double), true, false);
    DevView v_mask(c, masks, (shared ? 1 : (size_t)n_patterns) * ring, true, false);
    DevBuf<int> d_good;
    DevBuf<double> d_waxs;
    hipError_t e = v_img.err != hipSuccess ? v_img.err : v_mask.err;
    if (e == hipSuccess) e = d_good.alloc((size_t)n_patterns);
    if (e == hipSuccess) e = d_waxs.alloc((size_t)n_patterns * f.n_q);
    CorRingArgs r{};
    r.mw = h->d_mw;
    r.rc = h->d_rc;
    r.rs = h->d_rs;
    r.factor = h->d_factor;
    r.tw = h->d_tw;
    r.F = h->d_F;
    r.G = h->d_G;
    r.n_q = f.n_q;
    r.n_phi = f.n_phi;
    r.log2n = h->log2n;
    r.filter = f.filter_kind;
    r.roi_lo = f.roi_lo;
    r.roi_hi = f.roi_hi;
    r.roi_filter = f.roi_filter;
    r.roi_norm = f.roi_normalize;
    r.filter_k = f.filter_k;
    r.roi_min = f.roi_min;
    r.roi_max = f.roi_max;
    CorPairArgs a{};
    a.F = h->d_F;
    a.G = h->d_G;
    a.tw = h->d_tw;
    a.q1 = h->d_q1;
    a.q2 = h->d_q2;
    a.sum = h->d_sum;
    a.cnt = h->d_cnt;
    a.M = h->d_M;
    a.n_q = f.n_q;
    a.n_q2 = f.n_q2;
    a.m = h->m;
    a.log2m = h->log2n - 1;
    a.npairs = (long long)f.n_q1 * f.n_q2;
    a.inv_n = 1.0 / (double)f.n_phi;
    if (e == hipSuccess && shared && !h->have_M) {
        // the shared mask's M, once per handle: its transform through the ring kernel, its pair products through the pair kernel
        ProfScope ps(c, "corr_mask");
        CorRingArgs rm = r;
        rm.img = nullptr;
        rm.mask = (const uint8_t*)v_mask.dev;
        rm.mask_stride = 0;
        rm.filter = 0;
        rm.do_G = 1;
        cor_launch_ring(h, 1, rm);
        CorPairArgs am = a;
        am.mode = COR_MODE_MASK_ONLY;
        am.P = 1;
        cor_launch_pair(h, am);
        h->have_M = true;
    }
    for (int p0 = 0; e == hipSuccess && p0 < n_patterns; p0 += COR_CHUNK) {
        const int pc = std::min(COR_CHUNK, n_patterns - p0);
        r.img = (const double*)v_img.dev + (size_t)p0 * ring;
        r.mask = (const uint8_t*)v_mask.dev + (shared ? 0 : (size_t)p0 * ring);
        r.mask_stride = shared ? 0 : ring;
        r.good = d_good + p0;
        r.waxs = d_waxs + (size_t)p0 * f.n_q;
        r.do_G = shared ? 0 : 1;
        {
            ProfScope ps(c, "corr_ring");
            {
                ProfScope pt(c, "corr_stats");
                const dim3 g((unsigned)f.n_q, (unsigned)pc), b(COR_RT);
                if (f.filter_kind == 2) hipLaunchKernelGGL(k_corr_stats_mad, g, b, 0, c->stream, r, (double*)nullptr, (double*)nullptr);
                else hipLaunchKernelGGL(k_corr_stats, g, b, 0, c->stream, r);
            }
            cor_launch_ring(h, (unsigned)pc, r);
        }
        a.good = d_good + p0;
        a.P = pc;
        a.mode = shared ? COR_MODE_SHARED : COR_MODE_PATTERN;
        {
            ProfScope ps(c, "corr_pair");
            cor_launch_pair(h, a);
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) {
        const size_t old = h->good.size();
        h->good.resize(old + n_patterns);
        h->waxs.resize((old + n_patterns) * f.n_q);
        e = mtip_copy(c, h->good.data() + old, d_good, (size_t)n_patterns * sizeof(int), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = mtip_copy(c, h->waxs.data() + old * f.n_q, d_waxs, (size_t)n_patterns * f.n_q * sizeof(double), hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) {
        c->err = std::string("correlate_add: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? MTIP_ENOMEM : MTIP_EHIP;
    }
    return MTIP_OK;
}

extern "C" int mtip_correlate_num_patterns(mtip_correlate* h) { return h ? (int)h->good.size() : MTIP_EINVAL; }

extern "C" int mtip_correlate_get_partial(mtip_correlate* h, double* sum, int32_t* count, int32_t* is_good, double* waxs) {
    if (!h) return MTIP_EINVAL;
    mtip_ctx* c = h->c;
    (void)hipSetDevice(c->device);
    hipError_t e = hipSuccess;
    if (sum) e = mtip_copy(c, sum, h->d_sum, h->n_acc * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && count) e = mtip_copy(c, count, h->d_cnt, h->n_acc * sizeof(int), hipMemcpyDeviceToHost);
    if (e == hipSuccess && is_good && !h->good.empty()) e = cor_host_copy(c, is_good, h->good.data(), h->good.size() * sizeof(int32_t), is_good);
    if (e == hipSuccess && waxs && !h->waxs.empty()) e = cor_host_copy(c, waxs, h->waxs.data(), h->waxs.size() * sizeof(double), waxs);
    if (e != hipSuccess) {
        c->err = std::string("correlate_get_partial: ") + hipGetErrorString(e);
        return MTIP_EHIP;
    }
    return MTIP_OK;
}

extern "C" int mtip_correlate_merge(mtip_correlate* h, const double* sum, const int32_t* count, int n_patterns, const int32_t* is_good,
                                    const double* waxs) {
    if (!h) return MTIP_EINVAL;
    mtip_ctx* c = h->c;
    if (!sum || !count || n_patterns < 0 || (n_patterns > 0 && (!is_good || !waxs))) {
        c->err = "correlate_merge: null buffer";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    DevView v_sum(c, sum, h->n_acc * sizeof(double), true, false);
    DevView v_cnt(c, count, h->n_acc * sizeof(int), true, false);
    hipError_t e = v_sum.err != hipSuccess ? v_sum.err : v_cnt.err;
    if (e == hipSuccess) {
        const unsigned grid = (unsigned)std::min<long long>(div_up((long long)h->n_acc, 256), (long long)c->n_cu * 8);
        hipLaunchKernelGGL(k_corr_merge, dim3(grid), dim3(256), 0, c->stream, h->d_sum, h->d_cnt, (const double*)v_sum.dev, (const int*)v_cnt.dev,
                           h->n_acc);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && n_patterns > 0) {
        const size_t old = h->good.size();
        h->good.resize(old + n_patterns);
        h->waxs.resize((old + n_patterns) * h->cfg.n_q);
        e = cor_host_copy(c, h->good.data() + old, is_good, (size_t)n_patterns * sizeof(int32_t), is_good);
        if (e == hipSuccess) e = cor_host_copy(c, h->waxs.data() + old * h->cfg.n_q, waxs, (size_t)n_patterns * h->cfg.n_q * sizeof(double), waxs);
    }
    if (e != hipSuccess) {
        c->err = std::string("correlate_merge: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? MTIP_ENOMEM : MTIP_EHIP;
    }
    return MTIP_OK;
}

extern "C" int mtip_correlate_finalize(mtip_correlate* h, int symmetrize, int pos_pi2, int pos_pi, int pos_3pi2, int fc_n_max, double* ccf,
                                       mtip_cdouble* fc) {
    if (!h) return MTIP_EINVAL;
    mtip_ctx* c = h->c;
    const int n = h->cfg.n_phi;
    if ((!ccf && !fc) || (fc && (fc_n_max < 1 || fc_n_max > n))) {
        c->err = "correlate_finalize: no output buffer, or fc_n_max outside 1 .. n_phi";
        return MTIP_EINVAL;
    }
    // symmetrize_ccf copies [pos_pi, pos_pi + pos_pi2) to the front and [pos_3pi2 + 1 - pos_pi, n - pos_pi) to the back
    if (symmetrize && (pos_pi2 < 0 || pos_pi < 0 || pos_3pi2 < 0 || pos_3pi2 >= n || pos_pi + pos_pi2 > n || pos_3pi2 + 1 - pos_pi < 0)) {
        c->err = "correlate_finalize: symmetrize: the slices of symmetrize_ccf (cross_correlation.py:75-76) leave the angular axis";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    const size_t pairs = (size_t)h->cfg.n_q1 * h->cfg.n_q2;
    DevView v_ccf(c, ccf, h->n_acc * sizeof(double), false, true);
    DevView v_fc(c, fc, pairs * (size_t)(fc ? fc_n_max : 0) * sizeof(double2), false, true);
    hipError_t e = v_ccf.err != hipSuccess ? v_ccf.err : v_fc.err;
    if (e == hipSuccess) {
        CorFinalArgs a{};
        a.sum = h->d_sum;
        a.cnt = h->d_cnt;
        a.tw = h->d_tw;
        a.ccf = (double*)v_ccf.dev;
        a.fc = (double2*)v_fc.dev;
        a.n_phi = n;
        a.log2n = h->log2n;
        a.symmetrize = symmetrize ? 1 : 0;
        a.pos_pi2 = pos_pi2;
        a.pos_pi = pos_pi;
        a.pos_3pi2 = pos_3pi2;
        a.fc_n = fc ? fc_n_max : 0;
        ProfScope ps(c, "corr_final");
        if (h->bluestein) hipLaunchKernelGGL(k_corr_final_b, dim3((unsigned)pairs), dim3(COR_RT), 0, c->stream, a, h->bs);
        else if (h->general) hipLaunchKernelGGL(k_corr_final_g, dim3((unsigned)pairs), dim3(COR_RT), 0, c->stream, a, h->pl_n);
        else hipLaunchKernelGGL(k_corr_final, dim3((unsigned)pairs), dim3(COR_RT), 0, c->stream, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = v_ccf.finish();
    if (e == hipSuccess) e = v_fc.finish();
    if (e != hipSuccess) {
        c->err = std::string("correlate_finalize: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? MTIP_ENOMEM : MTIP_EHIP;
    }
    return MTIP_OK;
}

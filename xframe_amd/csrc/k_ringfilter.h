// correlate: the median_mad radial pixel filter of one ring  (gfx950, fp64, exact order statistics)
//   xframe/projects/fxs/correlate.py:405-406, 412-413               process_image: the filter
//                                   471-474                        i_median_and_mad (np.nanmedian, scipy.stats.median_abs_deviation)
// Included by k_correlate.h behind k_corr_stats, whose place it takes in a handle made with filter_kind = 2; it reads CorRingArgs and
// writes the same three arrays (mw, rc, rs), so k_corr_ring and the pair kernels do not know which filter ran.
//   k_corr_stats_mad   one workgroup of COR_RT threads per (pattern, ring), a row of n_phi <= 2048 doubles and its mask bytes.
// The statistics, over the row's valid samples (mask != 0, value not NaN; n of them), v sorted:
//   median = v[n / 2] for odd n, (v[n / 2 - 1] + v[n / 2]) / 2 for even n;  mad = the same rule on |x - median|;  NaN for n = 0.
// The filter: keep = mask && !(|x - median| > k mad): a NaN threshold (n = 0) keeps the mask, a NaN sample stays, and mad = 0 masks
// every sample that differs from the median -- all as the reference does, none guarded.
// Selection: a radix select on a 64-bit key whose unsigned order is the order of the doubles (negative: all bits flipped;
// non-negative: the sign bit flipped; the deviations are >= 0, their raw bits serve).  A thread keeps its <= 8 samples in registers.
// Eight passes of one byte from the top; the 256 bins of a pass are the 256 threads: an LDS histogram of ints filled by atomicAdd,
// an exclusive scan over the threads, and the one thread whose bin holds the wanted rank narrows the prefix and the rank.  The counts
// are integers, so nothing depends on the order in which the lanes' atomics arrive.  For even n the upper middle element comes from
// one more reduction: the count of keys <= the lower one and the least key above it.  A median is an element of the data or the
// mean of two, so the result is numpy's bit for bit (numerically: which of +0.0 / -0.0 a zero is, is not defined).
// rc and rs (count and sum of the kept samples) are accumulated in k_corr_stats's order, thread-strided and then cor_block_sum: a
// handle fed (I, M) with this filter gives the bits of an unfiltered handle fed (where(W, I, 0), W), W the filtered mask.
// CONTRACT: valid samples are finite or NaN with |x| < 1e300 (the sum of the two middle elements must not overflow).  Infinities are
// out of contract: inf - inf is a NaN deviation, which no rank is defined for.
// No global scratch, no dynamic LDS; static LDS 1.1 KB.
#pragma once

#define RF_SLOTS 8                     // samples a thread holds
#define RF_MAX_NPHI (RF_SLOTS * COR_RT)
#define RF_GRID (1 << 20)             // rows per launch of the operator entry
static_assert(RF_MAX_NPHI == 2048 && COR_RT == 256 && COR_WAVES * 64 == COR_RT, "k_corr_stats_mad: 256 threads are the 256 bins of a byte");

struct RfShared {
    int hist[COR_RT];                  // the histogram of a pass: zero between passes
    int wt[COR_WAVES];                 // wave totals of the scan / of an integer sum
    int sel[2];                        // the chosen bin and the count below it
    unsigned long long mn[COR_WAVES];
    double red[COR_WAVES];             // cor_block_sum's
};

__device__ __forceinline__ unsigned long long rf_bits(double v) { return (unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ double rf_value(unsigned long long u) { return __hiloint2double((int)(u >> 32), (int)(u & 0xffffffffull)); }
// unsigned order of the keys = order of the doubles (no NaN)
__device__ __forceinline__ unsigned long long rf_key(double v) {
    const unsigned long long u = rf_bits(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double rf_unkey(unsigned long long k) { return rf_value((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k); }

// sum over the workgroup, the same value in every thread
__device__ __forceinline__ int rf_block_sum(int v, RfShared& s, int tid) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((tid & 63) == 0) s.wt[tid >> 6] = v;
    __syncthreads();
    return (s.wt[0] + s.wt[1]) + (s.wt[2] + s.wt[3]);
}
__device__ __forceinline__ unsigned long long rf_block_min(unsigned long long v, RfShared& s, int tid) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(v, o);
        v = t < v ? t : v;
    }
    __syncthreads();
    if ((tid & 63) == 0) s.mn[tid >> 6] = v;
    __syncthreads();
    const unsigned long long a = s.mn[0] < s.mn[1] ? s.mn[0] : s.mn[1], b = s.mn[2] < s.mn[3] ? s.mn[2] : s.mn[3];
    return a < b ? a : b;
}

// the key of rank `rank` (from 0, ascending) among the workgroup's valid keys (bit r of `valid`: slot r); needs 0 <= rank < their
// number and s.hist zero, and leaves it zero.  The same value in every thread.
__device__ __forceinline__ unsigned long long rf_select(const unsigned long long (&key)[RF_SLOTS], unsigned valid, int rank, RfShared& s, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    unsigned long long want = 0;                                        // the bytes chosen so far, in place
    for (int shift = 56; shift >= 0; shift -= 8) {
#pragma unroll
        for (int r = 0; r < RF_SLOTS; ++r)
            if (((valid >> r) & 1u) && (((key[r] ^ want) >> shift) >> 8) == 0) atomicAdd(&s.hist[(int)((key[r] >> shift) & 255u)], 1);
        __syncthreads();
        const int c = s.hist[tid];
        s.hist[tid] = 0;
        int inc = c;                                                    // inclusive scan over the wave's bins
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o);
            if (lane >= o) inc += t;
        }
        if (lane == 63) s.wt[wave] = inc;
        __syncthreads();
        const int below = (wave > 0 ? s.wt[0] : 0) + (wave > 1 ? s.wt[1] : 0) + (wave > 2 ? s.wt[2] : 0) + inc - c;
        if (rank >= below && rank < below + c) {                        // one bin holds the rank
            s.sel[0] = tid;
            s.sel[1] = below;
        }
        __syncthreads();
        want |= (unsigned long long)(unsigned)s.sel[0] << shift;
        rank -= s.sel[1];
    }
    return want;
}

// the middle of the valid keys by the rule above: lo = the element of rank (n - 1) / 2, hi = that of rank n / 2 (n >= 1)
__device__ __forceinline__ void rf_middle(const unsigned long long (&key)[RF_SLOTS], unsigned valid, int n, RfShared& s, int tid,
                                          unsigned long long* lo, unsigned long long* hi) {
    const int rank = (n - 1) >> 1;
    const unsigned long long klo = rf_select(key, valid, rank, s, tid);
    *lo = *hi = klo;
    if (n & 1) return;                                                  // (n is the same in every thread)
    int le = 0;
    unsigned long long above = ~0ull;
#pragma unroll
    for (int r = 0; r < RF_SLOTS; ++r)
        if ((valid >> r) & 1u) {
            if (key[r] <= klo) ++le;
            else if (key[r] < above) above = key[r];
        }
    le = rf_block_sum(le, s, tid);
    above = rf_block_min(above, s, tid);
    if (le < rank + 2) *hi = above;                                     // no tie reaches rank n / 2: the least key above
}

// the median_mad filter of one ring and the ring sums of the pattern-wide decisions; med / mad (one value per row) may be null, and
// so may mw, rc and rs (the operator entry)
__global__ void __launch_bounds__(COR_RT) k_corr_stats_mad(CorRingArgs a, double* med_out, double* mad_out) {
    __shared__ RfShared s;
    const int tid = threadIdx.x, q = blockIdx.x, p = blockIdx.y;
    const size_t ring = (size_t)p * a.n_q + q;
    const double* row = a.img + ring * a.n_phi;
    const uint8_t* mrow = a.mask + (size_t)p * a.mask_stride + (size_t)q * a.n_phi;
    s.hist[tid] = 0;
    double x[RF_SLOTS];
    unsigned long long key[RF_SLOTS];
    unsigned in_mask = 0, valid = 0;
    int n = 0;
#pragma unroll
    for (int r = 0; r < RF_SLOTS; ++r) {
        const int j = tid + COR_RT * r;
        const bool m = j < a.n_phi && mrow[j] != 0;
        x[r] = m ? row[j] : 0.0;
        const bool v = m && x[r] == x[r];
        key[r] = rf_key(x[r]);
        in_mask |= (m ? 1u : 0u) << r;
        valid |= (v ? 1u : 0u) << r;
        n += v ? 1 : 0;
    }
    n = rf_block_sum(n, s, tid);                                        // (its barriers publish the zeroed histogram)
    double med = __builtin_nan(""), mad = __builtin_nan("");
    if (n > 0) {
        unsigned long long lo, hi;
        rf_middle(key, valid, n, s, tid, &lo, &hi);
        med = (n & 1) ? rf_unkey(lo) : (rf_unkey(lo) + rf_unkey(hi)) / 2.0;
#pragma unroll
        for (int r = 0; r < RF_SLOTS; ++r) key[r] = rf_bits(fabs(x[r] - med));
        rf_middle(key, valid, n, s, tid, &lo, &hi);
        mad = (n & 1) ? rf_value(lo) : (rf_value(lo) + rf_value(hi)) / 2.0;
    }
    const double thr = a.filter_k * mad;
    uint8_t* wrow = a.mw ? a.mw + ring * a.n_phi : nullptr;
    double cnt = 0.0, sum = 0.0;
#pragma unroll
    for (int r = 0; r < RF_SLOTS; ++r) {
        const int j = tid + COR_RT * r;
        if (j < a.n_phi) {
            const uint8_t keep = (((in_mask >> r) & 1u) && !(fabs(x[r] - med) > thr)) ? 1 : 0;
            if (wrow) wrow[j] = keep;
            if (keep) {
                cnt += 1.0;
                sum += x[r];
            }
        }
    }
    cnt = cor_block_sum(cnt, s.red, tid);
    sum = cor_block_sum(sum, s.red, tid);
    if (tid == 0) {
        if (a.rc) a.rc[ring] = cnt;
        if (a.rs) a.rs[ring] = sum;
        if (med_out) med_out[ring] = med;
        if (mad_out) mad_out[ring] = mad;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
extern "C" int mtip_op_ring_median_mad(mtip_ctx* c, int n_rows, int n_phi, const double* images, const uint8_t* masks, double k,
                                       double* median, double* mad, uint8_t* masks_out) {
    if (!c) return MTIP_EINVAL;
    if (!images || !masks) {
        c->err = "ring_median_mad: null input buffer";
        return MTIP_EINVAL;
    }
    if (n_rows < 1 || n_phi < 1 || n_phi > RF_MAX_NPHI) {
        char msg[200];
        snprintf(msg, sizeof msg, "ring_median_mad: built for n_rows >= 1 and 1 <= n_phi <= %d; got n_rows = %d, n_phi = %d", RF_MAX_NPHI,
                 n_rows, n_phi);
        c->err = msg;
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    const size_t n = (size_t)n_rows * n_phi;
    DevView v_img(c, images, n * sizeof(double), true, false);
    DevView v_mask(c, masks, n, true, false);
    DevView v_med(c, median, (size_t)n_rows * sizeof(double), false, true);
    DevView v_mad(c, mad, (size_t)n_rows * sizeof(double), false, true);
    DevView v_out(c, masks_out, n, false, true);
    hipError_t e = hipSuccess;
    for (const DevView* v : {&v_img, &v_mask, &v_med, &v_mad, &v_out})
        if (e == hipSuccess) e = v->err;
    if (e == hipSuccess) {
        CorRingArgs a{};
        a.n_phi = n_phi;
        a.filter = 2;
        a.filter_k = k;
        ProfScope ps(c, "ring_mad");
        for (int r0 = 0; r0 < n_rows; r0 += RF_GRID) {                  // rows on a flat grid: one "pattern" of up to RF_GRID rings
            const size_t off = (size_t)r0 * n_phi;
            a.n_q = std::min(RF_GRID, n_rows - r0);
            a.img = (const double*)v_img.dev + off;
            a.mask = (const uint8_t*)v_mask.dev + off;
            a.mw = masks_out ? (uint8_t*)v_out.dev + off : nullptr;
            hipLaunchKernelGGL(k_corr_stats_mad, dim3((unsigned)a.n_q), dim3(COR_RT), 0, c->stream, a,
                               median ? (double*)v_med.dev + r0 : nullptr, mad ? (double*)v_mad.dev + r0 : nullptr);
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = v_med.finish();
    if (e == hipSuccess) e = v_mad.finish();
    if (e == hipSuccess) e = v_out.finish();
    if (e != hipSuccess) {
        c->err = std::string("ring_median_mad: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? MTIP_ENOMEM : MTIP_EHIP;
    }
    return MTIP_OK;
}

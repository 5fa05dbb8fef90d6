// correlate: chirp-z (Bluestein) transforms for the angular lengths whose half has a prime factor above 5, the ones the mixed-radix plan
// of k_correlate_mr.h cannot factor (mtip_correlate_create_ex with MTIP_CORRELATE_ANY_NPHI: every even n_phi in 16 .. 2048).
// Included by k_correlate.h, whose kernels k_corr_ring_b / k_corr_pair_b / k_corr_final_b call what is here.
//
// All three kernels need one transform only, the DFT of m = n_phi / 2 complex points: the pair kernel's inverse real transform is
// the fold E + i O of cor_wave_irfft_g, which holds for every m, and the ring and final kernels pack a real row into m complex
// points (even samples real, odd ones imaginary) and unfold the spectrum (cor_bs_unfold).  With j k = (j^2 + k^2 - (k - j)^2) / 2
//   X[k] = c[k] sum_j (x[j] c[j]) conj(c[k - j]),   c[j] = exp(-+ i pi (j^2 mod 2 m) / m)
// (j^2 is reduced mod 2 m in integers, on the host, before the angle is formed): a circular convolution of any length
// Mc >= 2 m - 1.  Mc is the smallest such length with factors 2, 3, 5 only (odd ones such as 25 or 27 occur), and the convolution
// runs by the stage code of k_correlate_mr.h in one buffer of Mc points, with no digit-reversal pass at all:
//   a = x c, zero-padded to Mc, in natural order
//   forward Mc-point transform by decimation in FREQUENCY (cor_bs_dif_stage: the transposes of the plan's stages, last one first),
//     which leaves spectrum point k where the plan's digit reversal stores input point k
//   times B, stored in that order too: the Mc-point spectrum of the wrapped conjugate chirp h[j] = h[Mc - j] = conj(c[j]), j < m,
//     over Mc; summed directly in long double on the host, once per handle.  h is symmetric, so the spectrum of conj(h) is conj(B):
//     the same table serves the inverse m-point transform
//   inverse Mc-point transform by the plan's own decimation-in-time stages (cor_mr_stage<true>), natural order out; times c.
// One rendezvous per stage and per pointwise pass: of the wave alone in the pair kernel, of the workgroup in the ring and final
// kernels.  The stage bounds of CorStage::magic hold: Mc <= 2048, so t < Mc / 2 <= 2^10 and L <= 2^10.
#pragma once

struct CorBsArgs {
    const double2* tw;                 // exp(-2 pi i k / Mc), k < Mc
    const double2* B;                  // spectrum of the wrapped conjugate chirp over Mc, point k at the plan's digit reversal of k
    const double2* chirp;              // c[j] = exp(-i pi (j^2 mod 2 m) / m), j < m
    int Mc;
    CorStages st;                      // of the Mc-point transform
};

template <bool WAVE>
__device__ __forceinline__ void cor_bs_sync() {
    if constexpr (WAVE) MTIP_WAVE_LDS_SYNC();
    else __syncthreads();
}

// butterfly t of the transpose of stage g (forward): the R-point DFT first, then point c times w^(c pos)
template <int R>
__device__ __forceinline__ void cor_bs_dif_bfly(double2* buf, const double2* tw, const CorStage& g, int t) {
    const int blk = g.L == 1 ? t : (int)(((unsigned long long)(unsigned)t * g.magic) >> 32), pos = t - blk * g.L, i = blk * g.L * R + pos;
    double2 v[R];
#pragma unroll
    for (int c = 0; c < R; ++c) v[c] = buf[i + c * g.L];
    cor_dft<R, false>(v);
    buf[i] = v[0];
#pragma unroll
    for (int c = 1; c < R; ++c) buf[i + c * g.L] = cmul(v[c], tw[c * pos * g.tws]);
}
__device__ __forceinline__ void cor_bs_dif_stage(double2* buf, const double2* tw, const CorStage& g, int first, int step) {
    switch (g.r) {
        case 2:
            for (int t = first; t < g.nb; t += step) cor_bs_dif_bfly<2>(buf, tw, g, t);
            break;
        case 3:
            for (int t = first; t < g.nb; t += step) cor_bs_dif_bfly<3>(buf, tw, g, t);
            break;
        case 4:
            for (int t = first; t < g.nb; t += step) cor_bs_dif_bfly<4>(buf, tw, g, t);
            break;
        default:
            for (int t = first; t < g.nb; t += step) cor_bs_dif_bfly<5>(buf, tw, g, t);
            break;
    }
}

// buf (Mc points, natural order, written by the threads first, first + step, ..) convolved in place with the wrapped chirp behind
// B: with conj(c) for the forward m-point transform, with c (INV) for the inverse one.  Begins and ends with a rendezvous.
template <bool INV, bool WAVE>
__device__ __forceinline__ void cor_bs_convolve(double2* buf, const double2* tw, const CorBsArgs& bs, int first, int step) {
    cor_bs_sync<WAVE>();
    for (int s = bs.st.count - 1; s >= 0; --s) {
        cor_bs_dif_stage(buf, tw, bs.st.s[s], first, step);
        cor_bs_sync<WAVE>();
    }
    for (int k = first; k < bs.Mc; k += step) buf[k] = INV ? cmulc(buf[k], bs.B[k]) : cmul(buf[k], bs.B[k]);
    cor_bs_sync<WAVE>();
    for (int s = 0; s < bs.st.count; ++s) {
        cor_mr_stage<true>(buf, tw, bs.st.s[s], first, step);
        cor_bs_sync<WAVE>();
    }
}

// forward DFT of the m complex points in buf[0 .. m) by the whole workgroup (step = its thread count); tw: the Mc twiddles
__device__ __forceinline__ void cor_block_fft_b(double2* buf, int m, const CorBsArgs& bs, int tid, int step) {
    __syncthreads();
    for (int j = tid; j < bs.Mc; j += step) buf[j] = j < m ? cmul(buf[j], bs.chirp[j]) : make_double2(0.0, 0.0);
    cor_bs_convolve<false, false>(buf, bs.tw, bs, tid, step);
    for (int k = tid; k < m; k += step) buf[k] = cmul(buf[k], bs.chirp[k]);
    __syncthreads();
}

// spectrum point k < 2 m of the real row whose even samples sit in the real and whose odd ones in the imaginary parts of the m points
// z transformed above: with Z the spectrum in buf and Zr[k] = conj(Z[m - k]),  X[k] = (Z + Zr) / 2 - i w^k (Z - Zr) / 2,
// w^k = tw_n[k] = exp(-2 pi i k / n_phi); the upper half is the conjugate of the lower one
__device__ __forceinline__ double2 cor_bs_unfold(const double2* buf, const double2* tw_n, int m, int k) {
    const int kk = k > m ? 2 * m - k : k;
    const double2 z = buf[kk == m ? 0 : kk], y = buf[kk == 0 ? 0 : m - kk], w = tw_n[kk];
    const double2 e = make_double2(0.5 * (z.x + y.x), 0.5 * (z.y - y.y)), d = make_double2(0.5 * (z.x - y.x), 0.5 * (z.y + y.y));
    const double2 o = cmul(make_double2(d.y, -d.x), w);                 // -i d w
    return make_double2(e.x + o.x, k > m ? -(e.y + o.y) : e.y + o.y);
}

// cor_wave_irfft_g with the m-point inverse transform as a convolution: buf has Mc points, s_tw the Mc twiddles, tw_n[k] =
// exp(-2 pi i k / n_phi).  lane l gets the samples 2 j, 2 j + 1 of j = l + 64 r in out[2 r], out[2 r + 1] (zeros beyond m).
template <int NPL>
__device__ __forceinline__ void cor_wave_irfft_b(double2* buf, const double2* s_tw, const double2* tw_n, const CorBsArgs& bs,
                                                 const double2* a1, const double2* a2, int m, int lane, double* out) {
#pragma unroll
    for (int r = 0; r < NPL; ++r) {
        const int k = lane + 64 * r;
        if (k < m) {
            const double2 x = cmulc(a2[k], a1[k]);                      // conj(a1) a2
            const double2 xr = cmulc(a1[m - k], a2[m - k]);             // conj(conj(a1) a2) at m - k
            const double2 e = cadd(x, xr), d = csub(x, xr), w = tw_n[k];
            const double2 o = make_double2(d.x * w.x + d.y * w.y, d.y * w.x - d.x * w.y);   // d conj(w)
            buf[k] = cmulc(make_double2(e.x - o.y, e.y + o.x), bs.chirp[k]);
        }
    }
    for (int k = m + lane; k < bs.Mc; k += 64) buf[k] = make_double2(0.0, 0.0);
    cor_bs_convolve<true, true>(buf, s_tw, bs, lane, 64);
#pragma unroll
    for (int r = 0; r < NPL; ++r) {
        const int j = lane + 64 * r;
        const double2 z = j < m ? cmulc(buf[j], bs.chirp[j]) : make_double2(0.0, 0.0);
        out[2 * r] = z.x;
        out[2 * r + 1] = z.y;
    }
    MTIP_WAVE_LDS_SYNC();
}

// ---- host side: the plan -------------------------------------------------------------------------------------------------------------
static inline bool cor_any_ok(int n) { return n >= COR_MIN_NPHI && n <= COR_G_MAX_NPHI && !(n & 1); }

// the convolution length of an m-point transform: the smallest one >= 2 m - 1 with factors 2, 3, 5 only (<= 2048 for m <= 1024)
static inline int cor_bs_length(int m) {
    for (int k = 2 * m - 1;; ++k) {
        int r = k;
        for (int p : {2, 3, 5})
            while (r % p == 0) r /= p;
        if (r == 1) return k;
    }
}

// the tables of an m-point plan, in long double: tw (Mc), B over Mc in the digit-reversed order of st (Mc), chirp (m)
static inline void cor_bs_tables(int m, int Mc, const CorStages& st, double2* tw, double2* B, double2* chirp) {
    const long double pi = 3.14159265358979323846264338327950288L;
    std::vector<long double> wc((size_t)Mc), ws((size_t)Mc), hc((size_t)m), hs((size_t)m);
    for (int k = 0; k < Mc; ++k) {
        const long double ang = -2.0L * pi * (long double)k / (long double)Mc;
        wc[k] = cosl(ang);
        ws[k] = sinl(ang);
        tw[k] = make_double2((double)wc[k], (double)ws[k]);
    }
    for (int j = 0; j < m; ++j) {
        const long double ang = -pi * (long double)((long long)j * j % (2 * m)) / (long double)m;
        hc[j] = cosl(ang);
        hs[j] = -sinl(ang);                                             // h = conj(c)
        chirp[j] = make_double2((double)cosl(ang), (double)sinl(ang));
    }
    std::vector<uint16_t> perm((size_t)Mc);
    cor_make_perm(st, Mc, perm.data());
    for (int k = 0; k < Mc; ++k) {                                      // h[j] = h[Mc - j]: B[k] = h[0] + 2 sum_j h[j] cos(2 pi j k / Mc)
        long double re = hc[0], im = hs[0];
        for (int j = 1; j < m; ++j) {
            const long double c2 = 2.0L * wc[(size_t)((long long)j * k % Mc)];
            re += hc[j] * c2;
            im += hs[j] * c2;
        }
        B[perm[k]] = make_double2((double)(re / (long double)Mc), (double)(im / (long double)Mc));
    }
}

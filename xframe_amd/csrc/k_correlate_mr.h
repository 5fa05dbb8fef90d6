// correlate: mixed-radix (2, 3, 4, 5) transforms for the angular lengths the radix-2 code of k_correlate.h does not take: every even
// n_phi in 16 .. 2048 whose prime factors are 2, 3 and 5 (mtip_correlate_create_ex with MTIP_CORRELATE_GENERAL_NPHI).
// Included by k_correlate.h, whose kernels k_corr_ring_g / k_corr_pair_g / k_corr_final_g call what is here.
//
// The plan is made on the host once per handle (cor_make_stages, cor_make_perm): an in-place decimation-in-time transform whose
// input is stored through a digit-reversal table, the counterpart of the bit-reversed store of the radix-2 code.  Stage s has
// radix r_s and span L_s = r_0 .. r_(s-1); butterfly t < n / r_s takes the points i + c L_s (c < r_s) of the block of L_s r_s points
// it falls in, multiplies point c by w^(c pos) with w = exp(-+2 pi i / (L_s r_s)) and pos = t mod L_s, and writes the r_s-point DFT
// back to the same places.  No two butterflies of a stage touch the same point, so one rendezvous per stage is enough: of the
// workgroup in the ring and final kernels, of the wave alone (MTIP_WAVE_LDS_SYNC) in the pair kernel.
// One table exp(-2 pi i k / n_phi), k < n_phi, serves the n_phi-point transforms and the n_phi / 2-point one of the pair kernel
// (stride doubled): the largest index a stage asks for is (r - 1) pos n_phi / (L r) < n_phi.
#pragma once

#define COR_G_MAX_NPHI 2048
#define COR_MAX_STAGES 8               // 1458 = 2 3^6 has the most: 7

struct CorStage {
    int r, L, nb, tws;                 // radix, span, butterflies n / r, twiddle stride (table length) / (L r)
    unsigned magic;                    // ceil(2^32 / L): t / L = (t magic) >> 32 for t < 2^11, L <= 2^10 (t e < 2^32 with e = magic L - 2^32 < L)
};
struct CorStages {
    int count;
    CorStage s[COR_MAX_STAGES];
};
struct CorPlanArgs {
    const uint16_t* perm;              // where input point j is stored
    CorStages st;
};

// cos and sin of 2 pi / 3, 2 pi / 5, 4 pi / 5 (cos 2 pi / 3 = -1 / 2 exactly)
#define COR_S3 0.86602540378443864676372317075294
#define COR_C5A 0.30901699437494742410229341718282
#define COR_C5B (-0.80901699437494742410229341718282)
#define COR_S5A 0.95105651629515357211643933337938
#define COR_S5B 0.58778525229247312916870595463907

// a times the primitive fourth root of the transform's sign: -i forward, +i inverse
template <bool INV>
__device__ __forceinline__ double2 cor_rot(double2 a) {
    return INV ? make_double2(-a.y, a.x) : make_double2(a.y, -a.x);
}

// R-point DFT of v in place (sign - forward, + inverse)
template <int R, bool INV>
__device__ __forceinline__ void cor_dft(double2* v) {
    if constexpr (R == 2) {
        const double2 a = v[0], b = v[1];
        v[0] = cadd(a, b);
        v[1] = csub(a, b);
    } else if constexpr (R == 3) {
        const double2 t = cadd(v[1], v[2]), d = cor_rot<INV>(cscale(csub(v[1], v[2]), COR_S3));
        const double2 c = make_double2(v[0].x - 0.5 * t.x, v[0].y - 0.5 * t.y);
        v[0] = cadd(v[0], t);
        v[1] = cadd(c, d);
        v[2] = csub(c, d);
    } else if constexpr (R == 4) {
        const double2 s0 = cadd(v[0], v[2]), d0 = csub(v[0], v[2]), s1 = cadd(v[1], v[3]), d1 = cor_rot<INV>(csub(v[1], v[3]));
        v[0] = cadd(s0, s1);
        v[1] = cadd(d0, d1);
        v[2] = csub(s0, s1);
        v[3] = csub(d0, d1);
    } else {
        static_assert(R == 5, "radices 2, 3, 4, 5");
        const double2 p1 = cadd(v[1], v[4]), p2 = cadd(v[2], v[3]), q1 = csub(v[1], v[4]), q2 = csub(v[2], v[3]);
        const double2 a = make_double2(v[0].x + COR_C5A * p1.x + COR_C5B * p2.x, v[0].y + COR_C5A * p1.y + COR_C5B * p2.y);
        const double2 b = make_double2(v[0].x + COR_C5B * p1.x + COR_C5A * p2.x, v[0].y + COR_C5B * p1.y + COR_C5A * p2.y);
        const double2 e = cor_rot<INV>(make_double2(COR_S5A * q1.x + COR_S5B * q2.x, COR_S5A * q1.y + COR_S5B * q2.y));
        const double2 f = cor_rot<INV>(make_double2(COR_S5B * q1.x - COR_S5A * q2.x, COR_S5B * q1.y - COR_S5A * q2.y));
        v[0] = cadd(v[0], cadd(p1, p2));
        v[1] = cadd(a, e);
        v[2] = cadd(b, f);
        v[3] = csub(b, f);
        v[4] = csub(a, e);
    }
}

// butterfly t of stage g; tw[k] = exp(-2 pi i k / (table length)), conjugated for the inverse transform
template <int R, bool INV>
__device__ __forceinline__ void cor_mr_bfly(double2* buf, const double2* tw, const CorStage& g, int t) {
    const int blk = g.L == 1 ? t : (int)(((unsigned long long)(unsigned)t * g.magic) >> 32), pos = t - blk * g.L, i = blk * g.L * R + pos;
    double2 v[R];
    v[0] = buf[i];
#pragma unroll
    for (int c = 1; c < R; ++c) {
        double2 w = tw[c * pos * g.tws];
        if (INV) w.y = -w.y;
        v[c] = cmul(buf[i + c * g.L], w);
    }
    cor_dft<R, INV>(v);
#pragma unroll
    for (int c = 0; c < R; ++c) buf[i + c * g.L] = v[c];
}

// one stage by the threads first, first + step, ..: those beyond the stage's n / r butterflies idle
template <bool INV>
__device__ __forceinline__ void cor_mr_stage(double2* buf, const double2* tw, const CorStage& g, int first, int step) {
    switch (g.r) {
        case 2:
            for (int t = first; t < g.nb; t += step) cor_mr_bfly<2, INV>(buf, tw, g, t);
            break;
        case 3:
            for (int t = first; t < g.nb; t += step) cor_mr_bfly<3, INV>(buf, tw, g, t);
            break;
        case 4:
            for (int t = first; t < g.nb; t += step) cor_mr_bfly<4, INV>(buf, tw, g, t);
            break;
        default:
            for (int t = first; t < g.nb; t += step) cor_mr_bfly<5, INV>(buf, tw, g, t);
            break;
    }
}

// forward DFT of the n points that sit digit-reversed in buf, by the whole workgroup (step = its thread count)
__device__ __forceinline__ void cor_block_fft_g(double2* buf, const CorStages& st, const double2* tw, int tid, int step) {
    __syncthreads();
    for (int s = 0; s < st.count; ++s) {
        cor_mr_stage<false>(buf, tw, st.s[s], tid, step);
        __syncthreads();
    }
}

// cor_wave_irfft of k_correlate.h for any even n = 2 m: the fold E + i O holds for every m, odd ones included; a1 and a2 have m + 1
// entries.  lane l gets the samples 2 j, 2 j + 1 of j = l + 64 r in out[2 r], out[2 r + 1] (zeros beyond m: a partial last row).
template <int NPL>
__device__ __forceinline__ void cor_wave_irfft_g(double2* buf, const double2* s_tw, const uint16_t* s_perm, const CorStages& st,
                                                 const double2* a1, const double2* a2, int m, int lane, double* out) {
#pragma unroll
    for (int r = 0; r < NPL; ++r) {
        const int k = lane + 64 * r;
        if (k < m) {
            const double2 x = cmulc(a2[k], a1[k]);                      // conj(a1) a2
            const double2 xr = cmulc(a1[m - k], a2[m - k]);             // conj(conj(a1) a2) at m - k
            const double2 e = cadd(x, xr), d = csub(x, xr), w = s_tw[k];
            const double2 o = make_double2(d.x * w.x + d.y * w.y, d.y * w.x - d.x * w.y);   // d conj(w)
            buf[s_perm[k]] = make_double2(e.x - o.y, e.y + o.x);
        }
    }
    MTIP_WAVE_LDS_SYNC();
    for (int s = 0; s < st.count; ++s) {
        cor_mr_stage<true>(buf, s_tw, st.s[s], lane, 64);
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

// ---- host side: the plan -------------------------------------------------------------------------------------------------------------
static inline bool cor_general_ok(int n) {
    if (n < COR_MIN_NPHI || n > COR_G_MAX_NPHI || (n & 1)) return false;
    for (int p : {2, 3, 5})
        while (n % p == 0) n /= p;
    return n == 1;
}

// the nearest accepted lengths below and above n (0: none)
static inline void cor_general_near(int n, int* below, int* above) {
    *below = *above = 0;
    for (int k = std::min(n - 1, COR_G_MAX_NPHI); k >= COR_MIN_NPHI && !*below; --k)
        if (cor_general_ok(k)) *below = k;
    for (int k = std::max(n + 1, COR_MIN_NPHI); k <= COR_G_MAX_NPHI && !*above; ++k)
        if (cor_general_ok(k)) *above = k;
}

// stages of an n-point transform whose twiddles come from a table of n_tw entries (n divides n_tw): fours first, then 2, 3, 5
static inline CorStages cor_make_stages(int n, int n_tw) {
    CorStages st{};
    int rest = n, L = 1;
    while (rest > 1) {
        const int r = rest % 4 == 0 ? 4 : rest % 2 == 0 ? 2 : rest % 3 == 0 ? 3 : 5;
        CorStage& g = st.s[st.count++];
        g.r = r;
        g.L = L;
        g.nb = n / r;
        g.tws = n_tw / (L * r);
        g.magic = 0xffffffffu / (unsigned)L + 1u;                       // (L = 1 wraps to 0: the kernels do not divide there)
        L *= r;
        rest /= r;
    }
    return st;
}

// the digit reversal that goes with the stages: the last stage takes the points j = c mod r to block c, and so on inwards
static inline void cor_make_perm(const CorStages& st, int n, uint16_t* perm) {
    for (int j = 0; j < n; ++j) {
        int rest = j, pos = 0;
        for (int s = st.count - 1; s >= 0; --s) {
            pos += (rest % st.s[s].r) * st.s[s].L;
            rest /= st.s[s].r;
        }
        perm[j] = (uint16_t)pos;
    }
}

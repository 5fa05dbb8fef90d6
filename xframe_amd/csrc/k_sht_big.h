// Spherical-harmonic transform for band limits 64 <= L <= 128 (plan_sht: SHT_FWD_BIG / SHT_INV_BIG), included by k_sht.hip.
// The tuned tiers of k_sht_reg / k_sht_fused / k_sht_chain keep a shell's spectra and at most nine (l, m) pairs per thread on a CU;
// beyond L = 63 neither holds.  Here the two stages of the transform are separate launches with the spectra in global memory between
// them, in the layout the Legendre stage reads and writes as whole rows:
//
//     gs[mi = m + L][theta][bq = restart * Nq + shell]      (double2; c->d_g, the same size as the generic kernels' [bq][theta][mi])
//
//   forward   k_sht_big_fft_fwd   phi-FFT of the rows (theta, bq0 .. bq0 + 7) (prologue, w_theta 2 pi / n_phi), the 2L + 1 modes of the
//                                 eight shells staged in LDS and written as 128-byte runs
//             k_sht_big_leg_fwd   per order |m| and tile of 16 shells:  c[l][col] = sum_theta P_lm(theta) g[theta][col],
//                                 col = (+-m, shell, re/im)
//   inverse   k_sht_big_leg_inv   g[theta][col] = sum_l P_lm(theta) c[l][col]
//             k_sht_big_fft_inv   the inverse FFT of the rows, EPI_STORE / EPI_SCALE_SHELL / EPI_MODULUS (F' = F sqrt(I'/I): the
//                                 step's modulus stage), the output optionally through the slot table
//
// The Legendre stages are real-matrix x complex-panel products on v_mfma_f64_16x16x4_f64 (lane j: A[i = j & 15][k = j >> 4],
// B[k = j >> 4][col = j & 15], D reg r = D[(j >> 4) + 4 r][j & 15], as in k_hankel_tile).  P_lm(pi - theta) = (-1)^(l + m) P_lm(theta):
// only the northern half of the table is contracted -- the analysis folds g(theta) +- g(pi - theta) when it stages the panel and
// multiplies the even l - m with the sum, the odd with the difference; the synthesis forms the even and the odd sum and stores E + O
// north, E - O south.  So n_theta is even and at most 256 here (plan_sht: an odd or larger n_theta stays with the generic kernels), and n_phi is 256 or 512
// (n_phi > 2L).
// Why the matrix cores: a 16 x 16 x 4 step takes one A and one B double per lane from LDS and one instruction for 16 FMAs per lane; a
// 4 x 4 register tile of plain FMAs takes eight operands and sixteen instructions.  Measured (profiles/sht_bigl_timing.txt): the
// Legendre stages are a quarter of a direction's time at 512 x L128 and run at 2.0 - 2.5 TB/s of their algorithmic bytes; the FFT
// stages (radix-2 Stockham in LDS, a barrier per stage, the rows of a workgroup one after the other) are the other three quarters.
// LDS row strides are 16 doubles mod 32: the two k rows a half-wave reads fall on disjoint banks.
#pragma once

#define BL_QB 8                     // shells per workgroup of the FFT stages (128-byte runs of the spectra)
#define BL_KC 16                    // contraction chunk (4 MFMA k-steps)
#define BL_CT 32                    // doubles per column tile: 16 shells (re, im), two MFMA column tiles
#define BL_XS (BL_CT + 16)          // LDS row stride of the panels
#define BL_PS 80                    // analysis: rows l of one parity (<= 65: five row tiles)
#define BL_TS 144                   // synthesis: theta pairs (<= 128: eight row tiles) + 16
static_assert(SHT_BIG_NT_MAX / 2 == 128 && BL_TS >= SHT_BIG_NT_MAX / 2 + 16, "k_sht_big_leg_inv: eight row tiles of theta pairs");
#define BL_NM_MAX 257               // 2 L + 1

// Stockham radix-2 FFT of the R rows of a workgroup in LDS (k_fft_fwd's): T = np / 2 threads per row; x, y: the row's two buffers.
// On return the result is in x.  Every thread of the workgroup takes part in the barriers.
template <bool INV>
__device__ __forceinline__ void bigl_fft_row(double2*& x, double2*& y, const double2* __restrict__ tw, int np, int T, int i, bool active) {
    for (int p = 1; p < np; p <<= 1) {
        if (active) {
            const int k = i & (p - 1);
            const int j = ((i - k) << 1) + k;
            double2 w = tw[k * (T / p)];
            if (INV) w.y = -w.y;
            const double2 u0 = x[i];
            const double2 u1 = cmul(x[i + T], w);
            y[j] = cadd(u0, u1);
            y[j + p] = csub(u0, u1);
        }
        __syncthreads();
        double2* t = x;
        x = y;
        y = t;
    }
}

// grid (shell groups of BL_QB, n_theta), 256 threads; np in {256, 512}: two rows or one per pass
template <int PRE>
__global__ void __launch_bounds__(256) k_sht_big_fft_fwd(const double2* __restrict__ grid, double2* __restrict__ gs,
                                                         const double2* __restrict__ tw, const double* __restrict__ gw, int np, int nt,
                                                         int L, int N, int Q, double norm, const int* __restrict__ slot, int which, int B) {
    __shared__ double2 xy[2 * 512];
    __shared__ double2 S[BL_QB * BL_NM_MAX];
    const int T = np >> 1, R = 256 / T;
    const int r = threadIdx.x / T, i = threadIdx.x - r * T;
    const int t = blockIdx.y, bq0 = blockIdx.x * BL_QB, nm = 2 * L + 1;
    const double scale = gw[t] * norm;
    for (int it = 0; it < BL_QB; it += R) {
        const int j = it + r, bq = bq0 + j;
        const bool active = bq < Q;
        double2* x = xy + (size_t)r * np;
        double2* y = xy + (size_t)(R + r) * np;
        if (active) {
            long long srow = (long long)bq * nt + t;        // slot-indirect input: (3,B,G) pair array
            if (slot != nullptr) srow += (long long)slot[(bq / N) * SL_N + which] * B * N * nt;
            double2 a = grid[srow * np + i];
            double2 b = grid[srow * np + i + T];
            if (PRE == MTIP_PRE_SQUARE) {
                a = make_double2(cabs2(a), 0.0);
                b = make_double2(cabs2(b), 0.0);
            } else if (PRE == MTIP_PRE_ABS) {
                a = make_double2(sqrt(cabs2(a)), 0.0);
                b = make_double2(sqrt(cabs2(b)), 0.0);
            }
            x[i] = a;
            x[i + T] = b;
        }
        __syncthreads();
        bigl_fft_row<false>(x, y, tw, np, T, i, active);
        if (active)
            for (int mi = i; mi < nm; mi += T) {
                const int m = mi - L;
                S[j * nm + mi] = cscale(x[m < 0 ? m + np : m], scale);
            }
        __syncthreads();                                    // S complete; x free for the next pass
    }
    for (int e = threadIdx.x; e < nm * BL_QB; e += 256) {
        const int mi = e / BL_QB, j = e - mi * BL_QB;
        if (bq0 + j < Q) gs[((size_t)mi * nt + t) * Q + bq0 + j] = S[j * nm + mi];
    }
}

template <int EPI>
__global__ void __launch_bounds__(256) k_sht_big_fft_inv(const double2* __restrict__ gs, double2* __restrict__ grid,
                                                         const double2* __restrict__ tw, int np, int nt, int L, int N, int Q,
                                                         const double* __restrict__ shell_scale, const double2* __restrict__ Fin,
                                                         const int* __restrict__ slot, int which, int B) {
    __shared__ double2 xy[2 * 512];
    __shared__ double2 S[BL_QB * BL_NM_MAX];
    const int T = np >> 1, R = 256 / T;
    const int r = threadIdx.x / T, i = threadIdx.x - r * T;
    const int t = blockIdx.y, bq0 = blockIdx.x * BL_QB, nm = 2 * L + 1;
    for (int e = threadIdx.x; e < nm * BL_QB; e += 256) {
        const int mi = e / BL_QB, j = e - mi * BL_QB;
        S[j * nm + mi] = bq0 + j < Q ? gs[((size_t)mi * nt + t) * Q + bq0 + j] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    for (int it = 0; it < BL_QB; it += R) {
        const int j = it + r, bq = bq0 + j;
        const bool active = bq < Q;
        double2* x = xy + (size_t)r * np;
        double2* y = xy + (size_t)(R + r) * np;
        if (active)
            for (int e = i; e < np; e += T) {
                double2 v = make_double2(0.0, 0.0);
                if (e <= L) v = S[j * nm + e + L];
                else if (e >= np - L) v = S[j * nm + e - np + L];
                x[e] = v;
            }
        __syncthreads();
        bigl_fft_row<true>(x, y, tw, np, T, i, active);
        if (active) {
            const double sc = EPI == EPI_SCALE_SHELL ? shell_scale[bq % N] : 1.0;
            const long long o = ((long long)bq * nt + t) * np;
            long long oo = o;                               // slot-indirect output: (3,B,G) pair array; the restart per row, a block
            if (slot != nullptr) oo += (long long)slot[(bq / N) * SL_N + which] * B * N * nt * np;     // of shells may straddle two
            for (int e = i; e < np; e += T) {
                double2 v = x[e];
                if (EPI == EPI_MODULUS) {
                    // project_to_modified_intensity, fxs_Projections.py:899-909 (k_fft_inv<EPI_MODULUS>'s arithmetic); F of the
                    // row's own point straight from global memory, a coalesced row
                    const double2 Fv = Fin[o + e];
                    const double I = cabs2(Fv);
                    const bool ok = (I >= 0.0) && (v.x >= 0.0);
                    const double mult = ok ? sqrt(v.x / I) : 0.0;
                    v = cscale(Fv, mult);
                } else if (EPI == EPI_SCALE_SHELL) {
                    v = cscale(v, sc);
                }
                grid[oo + e] = v;
            }
        }
        __syncthreads();                                    // x free for the next pass
    }
}

// Legendre analysis.  grid (L + 1 orders |m|, column tiles of BL_CT doubles), 256 threads.  gs as doubles: [mi][theta][2 Q].
// Wave w: parity (w & 1) of l - |m|, sign (w >> 1) of m: up to five row tiles (l = |m| + parity + 2 j) x two column tiles.
// PT: the theta-major northern table (c->d_PT: [theta pair][npairs], order |m| at poff[|m|]).
__global__ void __launch_bounds__(256) k_sht_big_leg_fwd(const double* __restrict__ gs, double* __restrict__ coeff,
                                                         const double* __restrict__ PT, const int* __restrict__ poff, int nt, int L, int Q) {
    __shared__ double Ps[2][BL_KC][BL_PS];                  // [parity][theta pair][j]
    __shared__ double Xs[4][BL_KC][BL_XS];                  // [2 sign + (0: g(theta) + g(pi - theta), 1: difference)][theta pair][column]
    constexpr int NP = 2 * BL_KC * BL_PS / 256, NX = 2 * BL_KC * BL_CT / 256;      // table entries, folded pairs per thread and chunk
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int am = blockIdx.x, c0 = blockIdx.y * BL_CT;
    const int C2 = 2 * Q, TP = nt / 2, nrows = L + 1 - am, npairs = (L + 1) * (L + 2) / 2, nlm = (L + 1) * (L + 1);
    const double* Pm = PT + poff[am];
    const int par = wave & 1, sg = wave >> 1;
    const int nj = (nrows - par + 1) / 2, ntile = (nj + 15) / 16;
    double rp[NP], ra[NX], rb[NX];
    auto request = [&](int tp0) {
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const int e = tid + 256 * u, k = e / (2 * BL_PS), rr = e - k * (2 * BL_PS);
            rp[u] = (rr < nrows && tp0 + k < TP) ? Pm[(size_t)(tp0 + k) * npairs + rr] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < NX; ++u) {
            const int e = tid + 256 * u, col = e & (BL_CT - 1), k = (e / BL_CT) & (BL_KC - 1), s = e / (BL_CT * BL_KC);
            const int tp = tp0 + k;
            const bool ok = tp < TP && c0 + col < C2 && !(s == 1 && am == 0);
            const size_t base = (size_t)(s ? L - am : L + am) * nt;
            ra[u] = ok ? gs[(base + tp) * C2 + c0 + col] : 0.0;
            rb[u] = ok ? gs[(base + nt - 1 - tp) * C2 + c0 + col] : 0.0;
        }
    };
    auto deposit = [&]() {
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            const int e = tid + 256 * u, k = e / (2 * BL_PS), rr = e - k * (2 * BL_PS);
            Ps[rr & 1][k][rr >> 1] = rp[u];
        }
#pragma unroll
        for (int u = 0; u < NX; ++u) {
            const int e = tid + 256 * u, col = e & (BL_CT - 1), k = (e / BL_CT) & (BL_KC - 1), s = e / (BL_CT * BL_KC);
            Xs[2 * s][k][col] = ra[u] + rb[u];
            Xs[2 * s + 1][k][col] = ra[u] - rb[u];
        }
    };
    const int li = lane & 15, kk = lane >> 4;
    v4f64 acc[5][2];
#pragma unroll
    for (int rt = 0; rt < 5; ++rt) acc[rt][0] = acc[rt][1] = v4f64{0.0, 0.0, 0.0, 0.0};
    request(0);
    for (int tp0 = 0; tp0 < TP; tp0 += BL_KC) {
        __syncthreads();                                    // the previous chunk has been multiplied
        deposit();
        __syncthreads();
        if (tp0 + BL_KC < TP) request(tp0 + BL_KC);
#pragma unroll
        for (int s4 = 0; s4 < BL_KC / 4; ++s4) {
            const double b0 = Xs[2 * sg + par][4 * s4 + kk][li], b1 = Xs[2 * sg + par][4 * s4 + kk][16 + li];
#pragma unroll
            for (int rt = 0; rt < 5; ++rt)
                if (rt < ntile) {                           // wave-uniform
                    const double af = Ps[par][4 * s4 + kk][16 * rt + li];
                    acc[rt][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, b0, acc[rt][0], 0, 0, 0);
                    acc[rt][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, b1, acc[rt][1], 0, 0, 0);
                }
        }
    }
    if (sg == 1 && am == 0) return;
    const int m = sg ? -am : am;
    const bool neg = sg && (am & 1);                        // Y_l,-m = (-1)^m conj(Y_lm)
#pragma unroll
    for (int rt = 0; rt < 5; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 16 * rt + kk + 4 * r, col = c0 + 16 * ct + li;
                if (rt < ntile && j < nj && col < C2) {
                    const int l = am + par + 2 * j;
                    const double v = acc[rt][ct][r];
                    coeff[2 * ((size_t)(col >> 1) * nlm + l * (l + 1) + m) + (col & 1)] = neg ? -v : v;
                }
            }
}

// Legendre synthesis.  Same grid; n_theta / 2 <= 128 (SHT_BIG_NT_MAX, checked by the plan).  Wave w: sign (w >> 1) of m, row tiles (theta pairs) (w & 1) + 2 u, both parities (the even and the
// odd sum of a point are unfolded from the same lane).  P: the l-major table (c->d_P: row poff[|m|] + l - |m|, n_theta entries).
__global__ void __launch_bounds__(256) k_sht_big_leg_inv(const double2* __restrict__ coeff, double* __restrict__ gs,
                                                         const double* __restrict__ P, const int* __restrict__ poff, int nt, int L, int Q) {
    __shared__ double As[2][BL_KC][BL_TS];                  // [parity][j][theta pair]
    __shared__ double Cs[4][BL_KC][BL_XS];                  // [2 sign + parity][j][column]
    constexpr int NA = 2 * BL_KC * 128 / 256, NC = 4 * BL_KC * (BL_CT / 2) / 256;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int am = blockIdx.x, c0 = blockIdx.y * BL_CT;
    const int C2 = 2 * Q, TP = nt / 2, nrows = L + 1 - am, nlm = (L + 1) * (L + 1);
    const double* Pm = P + (size_t)poff[am] * nt;
    const int sg = wave >> 1, h = wave & 1;
    const int nje = (nrows + 1) / 2;                        // orders of the even parity (the odd has as many or one less)
    double ra[NA];
    double2 rc[NC];
    auto request = [&](int j0) {
#pragma unroll
        for (int u = 0; u < NA; ++u) {
            const int e = tid + 256 * u, tp = e & 127, k = (e >> 7) & (BL_KC - 1), p = e >> 11;
            const int lrel = p + 2 * (j0 + k);
            ra[u] = (lrel < nrows && tp < TP) ? Pm[(size_t)lrel * nt + tp] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            const int e = tid + 256 * u, jj = e & 15, k = (e >> 4) & (BL_KC - 1), p = (e >> 8) & 1, s = e >> 9;
            const int l = am + p + 2 * (j0 + k), bq = (c0 >> 1) + jj;
            double2 v = make_double2(0.0, 0.0);
            if (l <= L && bq < Q && !(s == 1 && am == 0)) v = coeff[(size_t)bq * nlm + l * (l + 1) + (s ? -am : am)];
            if (s && (am & 1)) v = make_double2(-v.x, -v.y);
            rc[u] = v;
        }
    };
    auto deposit = [&]() {
#pragma unroll
        for (int u = 0; u < NA; ++u) {
            const int e = tid + 256 * u, tp = e & 127, k = (e >> 7) & (BL_KC - 1), p = e >> 11;
            As[p][k][tp] = ra[u];
        }
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            const int e = tid + 256 * u, jj = e & 15, k = (e >> 4) & (BL_KC - 1), p = (e >> 8) & 1, s = e >> 9;
            Cs[2 * s + p][k][2 * jj] = rc[u].x;
            Cs[2 * s + p][k][2 * jj + 1] = rc[u].y;
        }
    };
    const int li = lane & 15, kk = lane >> 4;
    v4f64 accE[4][2], accO[4][2];
#pragma unroll
    for (int u = 0; u < 4; ++u) accE[u][0] = accE[u][1] = accO[u][0] = accO[u][1] = v4f64{0.0, 0.0, 0.0, 0.0};
    request(0);
    for (int j0 = 0; j0 < nje; j0 += BL_KC) {
        __syncthreads();                                    // the previous chunk has been multiplied
        deposit();
        __syncthreads();
        if (j0 + BL_KC < nje) request(j0 + BL_KC);
#pragma unroll
        for (int s4 = 0; s4 < BL_KC / 4; ++s4) {
            const double e0 = Cs[2 * sg][4 * s4 + kk][li], e1 = Cs[2 * sg][4 * s4 + kk][16 + li];
            const double o0 = Cs[2 * sg + 1][4 * s4 + kk][li], o1 = Cs[2 * sg + 1][4 * s4 + kk][16 + li];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (16 * (h + 2 * u) < TP) {                // wave-uniform
                    const double aE = As[0][4 * s4 + kk][16 * (h + 2 * u) + li], aO = As[1][4 * s4 + kk][16 * (h + 2 * u) + li];
                    accE[u][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(aE, e0, accE[u][0], 0, 0, 0);
                    accE[u][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(aE, e1, accE[u][1], 0, 0, 0);
                    accO[u][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(aO, o0, accO[u][0], 0, 0, 0);
                    accO[u][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(aO, o1, accO[u][1], 0, 0, 0);
                }
        }
    }
    if (sg == 1 && am == 0) return;
    const size_t base = (size_t)(sg ? L - am : L + am) * nt;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int tp = 16 * (h + 2 * u) + kk + 4 * r, col = c0 + 16 * ct + li;
                if (tp < TP && col < C2) {
                    const double E = accE[u][ct][r], O = accO[u][ct][r];
                    gs[(base + tp) * C2 + col] = E + O;
                    gs[(base + nt - 1 - tp) * C2 + col] = E - O;
                }
            }
}

static int launch_bigl_forward(mtip_ctx* c, const double2* grid, double2* coeff, int prologue, int in_slot) {
    const int Q = c->B * c->N;
    const dim3 fg((unsigned)div_up(Q, BL_QB), (unsigned)c->nt), lg((unsigned)(c->L + 1), (unsigned)div_up(2 * Q, BL_CT));
    const double norm = 2.0 * 3.14159265358979323846 / c->np;
    const int* sl = in_slot >= 0 ? (const int*)c->d_slot : nullptr;
#define BL_FWD(PRE)                                                                                                           \
    hipLaunchKernelGGL(k_sht_big_fft_fwd<PRE>, fg, dim3(256), 0, c->stream, grid, (double2*)c->d_g, (const double2*)c->d_tw,  \
                       (const double*)c->d_gw, c->np, c->nt, c->L, c->N, Q, norm, sl, in_slot, c->B)
    if (prologue == MTIP_PRE_SQUARE) BL_FWD(MTIP_PRE_SQUARE);
    else if (prologue == MTIP_PRE_ABS) BL_FWD(MTIP_PRE_ABS);
    else BL_FWD(MTIP_PRE_NONE);
#undef BL_FWD
    hipLaunchKernelGGL(k_sht_big_leg_fwd, lg, dim3(256), 0, c->stream, reinterpret_cast<const double*>((double2*)c->d_g),
                       reinterpret_cast<double*>(coeff), (const double*)c->d_PT, (const int*)c->d_poff, c->nt, c->L, Q);
    return MTIP_OK;
}

static int launch_bigl_inverse(mtip_ctx* c, const double2* coeff, double2* grid, const InvEpilogue& epi) {
    // store, shell scale and the step's modulus, each with or without the slot-indirect output; the real-space epilogue, the fixed
    // modulus and the coefficient difference on load exist in the tiers for L <= 63 only (plan_sht leaves real_update off here)
    if ((epi.mode != EPI_STORE && epi.mode != EPI_SCALE_SHELL && epi.mode != EPI_MODULUS) || epi.coeff_sub != nullptr)
        return sht_no_kernel(c, "inverse beyond L = 63", epi.mode);
    if (epi.mode == EPI_MODULUS && epi.F == nullptr) return sht_no_kernel(c, "inverse beyond L = 63 without F", epi.mode);
    const int Q = c->B * c->N;
    const dim3 fg((unsigned)div_up(Q, BL_QB), (unsigned)c->nt), lg((unsigned)(c->L + 1), (unsigned)div_up(2 * Q, BL_CT));
    hipLaunchKernelGGL(k_sht_big_leg_inv, lg, dim3(256), 0, c->stream, coeff, reinterpret_cast<double*>((double2*)c->d_g),
                       (const double*)c->d_P, (const int*)c->d_poff, c->nt, c->L, Q);
    const int* sl = epi.out_slot >= 0 ? (const int*)c->d_slot : nullptr;
#define BL_INV(EPI)                                                                                                          \
    hipLaunchKernelGGL(k_sht_big_fft_inv<EPI>, fg, dim3(256), 0, c->stream, (const double2*)c->d_g, grid,                    \
                       (const double2*)c->d_tw, c->np, c->nt, c->L, c->N, Q, epi.shell_scale, epi.F, sl, epi.out_slot, c->B)
    if (epi.mode == EPI_SCALE_SHELL) BL_INV(EPI_SCALE_SHELL);
    else if (epi.mode == EPI_MODULUS) BL_INV(EPI_MODULUS);
    else BL_INV(EPI_STORE);
#undef BL_INV
    return MTIP_OK;
}

// Spherical-harmonic transform kernels (row a4 of SURVEY section 8):
//   forward  f(theta,phi) -> f_lm :  FFT along phi (LDS Stockham), then Gauss-Legendre sum over theta
//   inverse  f_lm -> f(theta,phi) :  Legendre synthesis, then inverse FFT along phi (+ fused epilogue)
// Convention: orthonormal Y_lm with Condon-Shortley phase, index l(l+1)+m -- what the reference gets
// from shtns (xframe/externalLibraries/shtns_plugin.py:20-24, 250-261).
#include "mtip_internal.h"
#include "k_sht_common.h"
#include "k_sht_legendre.h"
#include <cmath>
#include <cstdlib>

// ------------------------------------------------------------------------------------------------
// Legendre table  P[(poff[m] + l - m) * nt + t] = Y_lm(theta_t, 0),  m >= 0   (host, one-off)
// ------------------------------------------------------------------------------------------------
void build_legendre_tables(mtip_ctx* c, const double* cos_theta) {
    const int L = c->L, nt = c->nt;
    std::vector<int> poff(L + 2);
    for (int m = 0; m <= L + 1; ++m) poff[m] = m * (L + 1) - m * (m - 1) / 2;
    const size_t rows = (size_t)(L + 1) * (L + 2) / 2;
    std::vector<double> P(rows * nt);
    // P_lm = a_lm (x P_l-1,m - b_lm P_l-2,m), l >= m + 2; in the record order of the synthesis (k_sht_legendre.h): the rows of an
    // order run to l = L + 1, and what is no step of the recurrence stays zero
    std::vector<double2> AB((size_t)legendre_n_rec(L), make_double2(0.0, 0.0));
    const double pi = 3.14159265358979323846;
    for (int t = 0; t < nt; ++t) {
        const double x = cos_theta[t];
        const double s = std::sqrt(std::fmax(0.0, 1.0 - x * x));
        double pmm = std::sqrt(1.0 / (4.0 * pi));
        for (int m = 0; m <= L; ++m) {
            if (m > 0) pmm = -std::sqrt((2.0 * m + 1.0) / (2.0 * m)) * s * pmm;
            P[(size_t)(poff[m]) * nt + t] = pmm;
            if (m < L) {
                double p2 = pmm;
                double p1 = std::sqrt(2.0 * m + 3.0) * x * pmm;
                P[(size_t)(poff[m] + 1) * nt + t] = p1;
                for (int l = m + 2; l <= L; ++l) {
                    const double a = std::sqrt((4.0 * l * l - 1.0) / ((double)l * l - (double)m * m));
                    const double b = std::sqrt((((double)l - 1.0) * (l - 1.0) - (double)m * m) / (4.0 * (l - 1.0) * (l - 1.0) - 1.0));
                    const double p = a * (x * p1 - b * p2);
                    P[(size_t)(poff[m] + l - m) * nt + t] = p;
                    AB[(size_t)legendre_rec(m, L) + l - m] = make_double2(a, b);
                    p2 = p1;
                    p1 = p;
                }
            }
        }
    }
    (void)mtip_copy(c, c->d_P, P.data(), P.size() * sizeof(double), hipMemcpyHostToDevice);
    (void)mtip_copy(c, c->d_poff, poff.data(), poff.size() * sizeof(int), hipMemcpyHostToDevice);
    if (c->d_AB != nullptr) (void)mtip_copy(c, c->d_AB, AB.data(), AB.size() * sizeof(double2), hipMemcpyHostToDevice);
    // theta-major copy of the northern half + (l,m) lookup for the fused kernels (k_sht_fused.hip)
    if (c->d_PT != nullptr) {
        const int nth = nt / 2;
        std::vector<double> PT((size_t)nth * rows);
        std::vector<int> lmtab(rows);
        for (int m = 0; m <= L; ++m)
            for (int l = m; l <= L; ++l) {
                const size_t idx = (size_t)poff[m] + l - m;
                lmtab[idx] = l | (m << 8);
                for (int t = 0; t < nth; ++t) PT[(size_t)t * rows + idx] = P[idx * nt + t];
            }
        (void)mtip_copy(c, c->d_PT, PT.data(), PT.size() * sizeof(double), hipMemcpyHostToDevice);
        (void)mtip_copy(c, c->d_lmtab, lmtab.data(), lmtab.size() * sizeof(int), hipMemcpyHostToDevice);
        // the same table in the CHUNK layout of the chained kernel's Legendre sums (k_sht_chain.hip, CHK): a thread owns up to three
        // orders l of ONE (m, parity of l - m), so the panel values G[theta][+-m] it multiplies them with are read from LDS once for
        // the three -- slot u * 256 + t = order u of chunk t (l | m << 8, or -1: no such order, table entry 0)
        c->chain_chunks = 0;
        if (c->d_PTc != nullptr) {
            std::vector<int> lmc(3 * 256, -1);
            std::vector<double> PTc((size_t)nth * 3 * 256, 0.0);
            int t = 0;
            bool fits = true;
            for (int m = 0; m <= L && fits; ++m)
                for (int par = 0; par < 2 && fits; ++par)
                    for (int l0 = m + par; l0 <= L; l0 += 6) {
                        if (t >= 256) { fits = false; break; }
                        for (int u = 0; u < 3; ++u) {
                            const int l = l0 + 2 * u;
                            if (l > L) break;
                            const size_t idx = (size_t)poff[m] + l - m;
                            lmc[u * 256 + t] = l | (m << 8);
                            for (int th = 0; th < nth; ++th) PTc[(size_t)th * 768 + u * 256 + t] = P[idx * nt + th];
                        }
                        ++t;
                    }
            if (fits) {
                c->chain_chunks = t;
                (void)mtip_copy(c, c->d_PTc, PTc.data(), PTc.size() * sizeof(double), hipMemcpyHostToDevice);
                (void)mtip_copy(c, c->d_lmc, lmc.data(), lmc.size() * sizeof(int), hipMemcpyHostToDevice);
                // and, for the L = 32 plan, by (wave, theta-pair couple, order, lane) with two neighbouring theta pairs to an entry:
                // a thread of k_sht_chain fetches its 48 values with 24 loads of 16 bytes, a wave 1 KB in a row with each
                if (c->d_PTw != nullptr && nth == 32) {
                    std::vector<double2> PTw((size_t)8 * 8 * 3 * 64);
                    for (int w = 0; w < 8; ++w)
                        for (int cp = 0; cp < 8; ++cp)
                            for (int u = 0; u < 3; ++u)
                                for (int ln = 0; ln < 64; ++ln) {
                                    const size_t th = (size_t)(w / 4) * 16 + 2 * cp, slot = (size_t)u * 256 + (w % 4) * 64 + ln;
                                    PTw[(((size_t)w * 8 + cp) * 3 + u) * 64 + ln] = make_double2(PTc[th * 768 + slot], PTc[(th + 1) * 768 + slot]);
                                }
                    (void)mtip_copy(c, c->d_PTw, PTw.data(), PTw.size() * sizeof(double2), hipMemcpyHostToDevice);
                }
            }
        }
    }
    // twiddles exp(-2 pi i j / n_phi), j < n_phi/2
    std::vector<double2> tw(c->np / 2);
    for (int j = 0; j < c->np / 2; ++j) {
        const double a = -2.0 * pi * j / c->np;
        tw[j] = make_double2(std::cos(a), std::sin(a));
    }
    (void)mtip_copy(c, c->d_tw, tw.data(), tw.size() * sizeof(double2), hipMemcpyHostToDevice);
    if (c->d_twN != nullptr) {                       // full-circle table for the register FFT kernels
        std::vector<double2> twn(c->np);
        for (int j = 0; j < c->np; ++j) {
            const double a = -2.0 * pi * j / c->np;
            twn[j] = make_double2(std::cos(a), std::sin(a));
        }
        (void)mtip_copy(c, c->d_twN, twn.data(), twn.size() * sizeof(double2), hipMemcpyHostToDevice);
    }
}

// ------------------------------------------------------------------------------------------------
// forward: FFT rows  (grid rows -> g[row][m+L] * w_theta * 2pi/n_phi)
// ------------------------------------------------------------------------------------------------
template <int PRE>
__global__ void __launch_bounds__(256) k_fft_fwd(const double2* __restrict__ grid, double2* __restrict__ g,
                                                 const double2* __restrict__ tw, const double* __restrict__ gw,
                                                 int np, int nt, int L, long long nrows, double norm,
                                                 const int* __restrict__ slot, int which, int B, long long rows_per_b) {
    HIP_DYNAMIC_SHARED(double2, sm)
    const int T = np >> 1;
    const int R = blockDim.x / T;
    const int r = threadIdx.x / T;
    const int i = threadIdx.x - r * T;
    const long long row = (long long)blockIdx.x * R + r;
    const bool active = row < nrows;
    double2* x = sm + (size_t)r * np;
    double2* y = sm + (size_t)(R + r) * np;
    if (active) {
        long long srow = row;                       // slot-indirect input: (3,B,G) pair array
        if (slot != nullptr) srow += (long long)slot[(row / rows_per_b) * SL_N + which] * B * rows_per_b;
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
    for (int p = 1; p < np; p <<= 1) {
        if (active) {
            const int k = i & (p - 1);
            const int j = ((i - k) << 1) + k;
            const double2 w = tw[k * (T / p)];
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
    if (active) {
        const int theta = (int)(row % nt);
        const double scale = gw[theta] * norm;
        const int nm = 2 * L + 1;
        for (int mi = i; mi < nm; mi += T) {
            const int m = mi - L;
            const int k = m < 0 ? m + np : m;
            g[row * nm + mi] = cscale(x[k], scale);
        }
    }
}

// forward: Legendre analysis  c[b,q,lm] = sum_theta P_lm(theta) g[b,q,theta,m]
__global__ void __launch_bounds__(256) k_leg_fwd(const double2* __restrict__ g, double2* __restrict__ coeff,
                                                 const double* __restrict__ P, const int* __restrict__ poff,
                                                 int nt, int L, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int nlm = (L + 1) * (L + 1);
    const int nm = 2 * L + 1;
    const int lm = (int)(idx % nlm);
    const long long bq = idx / nlm;
    const int l = isqrt_lm(lm);
    const int m = lm - l * (l + 1);
    const int am = m < 0 ? -m : m;
    const double* prow = P + (size_t)(poff[am] + l - am) * nt;
    const double2* gp = g + (size_t)bq * nt * nm + (m + L);
    double ar = 0.0, ai = 0.0;
    for (int t = 0; t < nt; ++t) {
        const double p = prow[t];
        const double2 v = gp[(size_t)t * nm];
        ar = fma(p, v.x, ar);
        ai = fma(p, v.y, ai);
    }
    if (m < 0 && (am & 1)) {
        ar = -ar;
        ai = -ai;
    }
    coeff[idx] = make_double2(ar, ai);
}

// ------------------------------------------------------------------------------------------------
// inverse: Legendre synthesis  g[b,q,theta,m] = sum_l P_lm(theta) c[b,q,lm]
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_leg_inv(const double2* __restrict__ coeff, double2* __restrict__ g,
                                                 const double* __restrict__ P, const int* __restrict__ poff,
                                                 int nt, int L, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int nlm = (L + 1) * (L + 1);
    const int nm = 2 * L + 1;
    const int mi = (int)(idx % nm);
    const long long rest = idx / nm;
    const int t = (int)(rest % nt);
    const long long bq = rest / nt;
    const int m = mi - L;
    const int am = m < 0 ? -m : m;
    const double* pcol = P + (size_t)poff[am] * nt + t;
    const double2* cp = coeff + (size_t)bq * nlm;
    double ar = 0.0, ai = 0.0;
    for (int l = am; l <= L; ++l) {
        const double p = pcol[(size_t)(l - am) * nt];
        const double2 v = cp[l * (l + 1) + m];
        ar = fma(p, v.x, ar);
        ai = fma(p, v.y, ai);
    }
    if (m < 0 && (am & 1)) {
        ar = -ar;
        ai = -ai;
    }
    g[idx] = make_double2(ar, ai);
}

// inverse: FFT rows with fused epilogue
template <int EPI>
__global__ void __launch_bounds__(256) k_fft_inv(const double2* __restrict__ g, double2* __restrict__ grid,
                                                 const double2* __restrict__ tw, int np, int nt, int L, int Nq,
                                                 long long nrows, const double2* __restrict__ Fin,
                                                 const double* __restrict__ shell_scale, const int* __restrict__ slot,
                                                 int which, int B) {
    HIP_DYNAMIC_SHARED(double2, sm)
    const int T = np >> 1;
    const int R = blockDim.x / T;
    const int r = threadIdx.x / T;
    const int i = threadIdx.x - r * T;
    const long long row = (long long)blockIdx.x * R + r;
    const bool active = row < nrows;
    double2* x = sm + (size_t)r * np;
    double2* y = sm + (size_t)(R + r) * np;
    const int nm = 2 * L + 1;
    if (active) {
        for (int e = i; e < np; e += T) {
            double2 v = make_double2(0.0, 0.0);
            if (e <= L) v = g[row * nm + (e + L)];
            else if (e >= np - L) v = g[row * nm + (e - np + L)];
            x[e] = v;
        }
    }
    __syncthreads();
    for (int p = 1; p < np; p <<= 1) {
        if (active) {
            const int k = i & (p - 1);
            const int j = ((i - k) << 1) + k;
            double2 w = tw[k * (T / p)];
            w.y = -w.y;                           // inverse transform: conjugate twiddle
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
    if (active) {
        const int q = (int)((row / nt) % Nq);
        for (int e = i; e < np; e += T) {
            double2 v = x[e];
            const long long o = row * np + e;
            long long oo = o;                           // slot-indirect output: (3,B,G) pair array
            if (slot != nullptr) {
                const long long rows_per_b = (long long)Nq * nt;
                oo += (long long)slot[(row / rows_per_b) * SL_N + which] * B * rows_per_b * np;
            }
            if (EPI == EPI_MODULUS) {
                // project_to_modified_intensity, fxs_Projections.py:899-909
                const double2 Fv = Fin[o];
                const double I = cabs2(Fv);
                const bool ok = (I >= 0.0) && (v.x >= 0.0);
                const double mult = ok ? sqrt(v.x / I) : 0.0;
                v = cscale(Fv, mult);
            } else if (EPI == EPI_SCALE_SHELL) {
                v = cscale(v, shell_scale[q]);
            }
            grid[oo] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
static void fft_launch_dims(const mtip_ctx* c, long long nrows, dim3* grid, dim3* block, size_t* smem) {
    const int T = c->np / 2;
    int R = 256 / T;
    if (R < 1) R = 1;
    *block = dim3((unsigned)(R * T));
    *grid = dim3((unsigned)div_up(nrows, R));
    *smem = (size_t)2 * R * c->np * sizeof(double2);
}

// ------------------------------------------------------------------------------------------------------------------------------
// The SHT plan (ShtPlan, mtip_internal.h): the only place that reads the geometry or the environment to pick an SHT kernel.
// Tier k is taken where MTIP_SHT_TIER >= k (default 5) and the geometry fits it (L > 63: k_sht_big.h or tier 0); the launchers below and in k_sht_reg.hip,
// k_sht_fused.hip, k_sht_chain.hip only read the plan.
static constexpr size_t SHT_LDS_MAX = 160 * 1024, SHT_WIDE_LDS_MAX = 158 * 1024;

// wide inverse kernel with `nsplit` workgroups per shell (see the kernel): LDS bytes, 0 if it does not fit; *rp = rows per FFT pass
static size_t wide_lds(const mtip_ctx* c, int r1, int r2, int nsplit, int* rp) {
    if (c->nt % (2 * nsplit) != 0) return 0;
    const int ntl = c->nt / nsplit;
    if (nsplit > 1 && (ntl / 2) % 32 != 0) return 0;                   // whole 32-theta chunks per workgroup
    // twiddles, spectra, cos(theta) of the workgroup's theta pairs (doubles)
    const size_t fixed = (nsplit > 1 ? 0 : (size_t)c->np) + (size_t)ntl * c->nm + (size_t)(ntl / 2 + 1) / 2;
    // the transpose buffer aliases the records of the synthesis (recurrence and shell coefficients, zero padded, with the
    // loop's read-ahead: k_sht_legendre.h): shrink the pass until both fit
    const size_t recs = (size_t)legendre_lds_entries(c->L);
    auto bytes = [&](int v) { return (fixed + std::max(recs, (size_t)v * r1 * (r2 + 1))) * sizeof(double2); };
    *rp = largest_even_divisor_le(ntl, std::min(SW_THREADS / r2, SW_THREADS / r1));
    while (*rp >= 2 && bytes(*rp) > SHT_WIDE_LDS_MAX) *rp = largest_even_divisor_le(ntl, *rp - 2);
    return *rp >= 2 ? bytes(*rp) : 0;
}

// the chained kernel (k_sht_chain.hip), instantiated for n_phi <= 128: accumulation groups of the Legendre-sum phase are the
// smallest power-of-two group whose threads hold <= 3 (l, m) pairs each and whose count divides the theta pairs
static void plan_chain(const mtip_ctx* c, int r1, int r2, ShtPlan& p) {
    if (c->np > 128) return;
    const int TP = c->nt / 2;
    for (int gsz = 64; gsz <= SW_THREADS; gsz *= 2) {
        const int maxi = div_up(c->npairs, gsz);
        if (TP % (SW_THREADS / gsz) != 0 || maxi > 3) continue;
        p.chain_gsz = gsz;
        p.chain_thg = TP / (SW_THREADS / gsz);
        // table rows in registers for the 128-point grids, else the run-time variants
        const bool reg_tab = c->np == 128 && p.chain_thg == 16 && maxi >= 2;
        p.chain_maxi = reg_tab ? maxi : (maxi == 1 ? 1 : 3);
        p.chain = !reg_tab ? SHT_CHAIN_RT
                : (p.chain_maxi == 3 && c->L == 32 && c->nt == 64 && c->chain_chunks > 0) ? SHT_CHAIN_L32 : SHT_CHAIN_REGTAB;
        break;
    }
    if (p.chain == SHT_CHAIN_OFF) return;
    // every wave owns 64 / R2 rows at a time and a transpose buffer for them; it, the panel staging and the groups' partial sums
    // at the end alias the records of the synthesis (recurrence and shell coefficients, zero padded, with the loop's read-ahead)
    const size_t tb = (size_t)(SW_THREADS / 64) * (64 / r2) * r1 * (r2 + 1);
    const size_t fixed = (size_t)c->np + (size_t)c->nt * c->nm + (size_t)(c->nt / 2 + 1) / 2;     // twiddles, spectra, cos(theta)
    p.chain_lds = (fixed + std::max(std::max((size_t)legendre_lds_entries(c->L), tb), (size_t)SW_THREADS * p.chain_maxi * 2)) * sizeof(double2);
    if (p.chain_lds > SHT_WIDE_LDS_MAX) p.chain = SHT_CHAIN_OFF;
}

void plan_sht(mtip_ctx* c) {
    int cap = 5;
    if (const char* e = std::getenv("MTIP_SHT_TIER")) cap = std::min(std::max(std::atoi(e), 0), 5);
    ShtPlan p;
    const int nt = c->nt, np = c->np;
    const size_t z = sizeof(double2);
    if (c->L > MTIP_LOOP_L_MAX) {
        // none of the tiers below whatever the cap says: they hold a shell's spectra in LDS and <= 9 (l, m) pairs per thread.
        // The two-stage kernels pair theta with pi - theta (even n_theta) and their synthesis holds at most 128 pairs; both
        // directions must fit, as for the tiers below: anything else stays with the generic kernels
        if (cap >= 1 && nt % 2 == 0 && nt <= SHT_BIG_NT_MAX) {
            p.fwd = SHT_FWD_BIG;
            p.inv = SHT_INV_BIG;
        }
        c->sht = p;
        return;
    }
    // tier 2: register FFTs, taken only where the forward AND the inverse kernel fit
    int r1 = 0, r2 = 0;
    if (cap >= 2 && nt % 2 == 0 && reg_radices(np, &r1, &r2)) {
        p.fwd_rp = largest_even_divisor_le(nt, std::min(2 * SR_THREADS / r2, SR_THREADS / r1));
        p.inv_rp = largest_even_divisor_le(nt, std::min(SR_THREADS / r2, SR_THREADS / r1));
        p.fwd_lds = ((size_t)np + (size_t)p.fwd_rp * r1 * (r2 + 1)) * z;
        p.inv_lds = ((size_t)np + c->nlm + (size_t)p.inv_rp * c->nm + (size_t)p.inv_rp * r1 * (r2 + 1)) * z;
        if (p.fwd_rp >= 2 && p.inv_rp >= 2 && p.fwd_lds <= SHT_LDS_MAX && p.inv_lds <= SHT_LDS_MAX) {
            p.fwd = SHT_FWD_REG;
            p.inv = SHT_INV_REG;
        }
    }
    if (p.fwd == SHT_FWD_REG) {
        const int per = div_up(c->npairs, SR_THREADS);
        p.fwd_maxi = per <= 3 ? 3 : per <= 5 ? 5 : 9;
        // tier 3: the paired forward kernel (half the rows per pass, theta pairs per pass 2, 4 or 8) ...
        const int th = p.fwd_rp / 4;
        if (cap >= 3 && p.fwd_rp % 4 == 0 && (th == 2 || th == 4 || th == 8) && (nt / 2) % th == 0 && per <= 5) {
            p.fwd = SHT_FWD_PAIR;
            p.fwd_th = th;
            p.fwd_lds = ((size_t)np + (size_t)(p.fwd_rp / 2) * r1 * (r2 + 1)) * z;
        }
        // ... and the wide inverse kernel, one workgroup per shell or else two
        for (int ns = 1; cap >= 3 && ns <= 2 && p.inv != SHT_INV_WIDE; ++ns) {
            int rp = 0;
            const size_t lds = wide_lds(c, r1, r2, ns, &rp);
            if (lds == 0) continue;
            p.inv = SHT_INV_WIDE;
            p.inv_rp = rp;
            p.inv_nsplit = ns;
            p.inv_lds = lds;
        }
        // tier 4: the wide kernel's real-space epilogue (and coefficient difference on load); tier 5: the chained kernel
        p.real_update = cap >= 4 && p.inv == SHT_INV_WIDE;
        p.real_update_blocks = c->N * p.inv_nsplit;
        if (cap >= 5) plan_chain(c, r1, r2, p);
    } else if (cap >= 1 && np >= 4 && np <= SF_THREADS && nt % 2 == 0) {
        // tier 1: LDS Stockham FFTs; a pass is a whole number of row pairs that tiles n_theta
        p.fwd = SHT_FWD_LDS;
        p.inv = SHT_INV_LDS;
        int rp = std::max(2, std::min(SF_THREADS / (np / 2), nt));
        while (nt % rp) --rp;
        if (rp & 1) rp = 2;
        p.fwd_rp = p.inv_rp = rp;
        const int per = div_up(c->npairs, SF_THREADS);
        p.fwd_maxi = per <= 3 ? 3 : per <= 5 ? 5 : 9;
        p.fwd_lds = ((size_t)np / 2 + 2 * (size_t)rp * np + (size_t)rp * c->nm) * z;
        const int nchunks = std::max(1, div_up((long long)(nt / 2) * ((c->L + 2) / 2), SF_THREADS));
        p.inv_jl = div_up(nt / 2, nchunks);
        p.inv_lds = ((size_t)np / 2 + c->nlm + (size_t)2 * p.inv_jl * c->nm + 2 * (size_t)rp * np) * z;
    } else {
        p = ShtPlan();                                  // tier 0: generic kernels
    }
    c->sht = p;
}

static const char* epi_name(int mode) {
    switch (mode) {
        case EPI_STORE: return "store";
        case EPI_MODULUS: return "modulus";
        case EPI_SCALE_SHELL: return "shell scale";
        case EPI_MODULUS_FIXED: return "fixed modulus";
        case EPI_REAL_UPDATE: return "real-space update";
        default: return "unknown";
    }
}

int sht_no_kernel(mtip_ctx* c, const char* what, int epi_mode) {
    c->err = std::string("SHT plan: no kernel for this case: ") + what + ", epilogue " + epi_name(epi_mode) +
             " (MTIP_SHT_TIER and the angular grid decide which kernels exist)";
    return MTIP_ESTATE;
}

#include "k_sht_big.h"

int launch_sht_forward(mtip_ctx* c, const double2* grid, double2* coeff, int prologue, int in_slot) {
    ProfScope ps(c, "sht_fwd");
    if (c->sht.fwd == SHT_FWD_BIG) return launch_bigl_forward(c, grid, coeff, prologue, in_slot);
    if (c->sht.fwd == SHT_FWD_REG || c->sht.fwd == SHT_FWD_PAIR) {
        launch_sht_forward_reg(c, grid, coeff, prologue, in_slot);
        return MTIP_OK;
    }
    if (c->sht.fwd == SHT_FWD_LDS) {
        launch_sht_forward_fused(c, grid, coeff, prologue, in_slot);
        return MTIP_OK;
    }
    const long long nrows = (long long)c->B * c->N * c->nt;
    dim3 gr, bl;
    size_t sm;
    fft_launch_dims(c, nrows, &gr, &bl, &sm);
    const double norm = 2.0 * 3.14159265358979323846 / c->np;
    const int* sl = in_slot >= 0 ? (const int*)c->d_slot : nullptr;
    if (prologue == MTIP_PRE_SQUARE)
        hipLaunchKernelGGL(k_fft_fwd<MTIP_PRE_SQUARE>, gr, bl, sm, c->stream, grid, c->d_g, c->d_tw, c->d_gw, c->np, c->nt, c->L, nrows, norm, sl, in_slot, c->B, (long long)c->N * c->nt);
    else if (prologue == MTIP_PRE_ABS)
        hipLaunchKernelGGL(k_fft_fwd<MTIP_PRE_ABS>, gr, bl, sm, c->stream, grid, c->d_g, c->d_tw, c->d_gw, c->np, c->nt, c->L, nrows, norm, sl, in_slot, c->B, (long long)c->N * c->nt);
    else
        hipLaunchKernelGGL(k_fft_fwd<MTIP_PRE_NONE>, gr, bl, sm, c->stream, grid, c->d_g, c->d_tw, c->d_gw, c->np, c->nt, c->L, nrows, norm, sl, in_slot, c->B, (long long)c->N * c->nt);
    const long long total = (long long)c->B * c->N * c->nlm;
    hipLaunchKernelGGL(k_leg_fwd, dim3((unsigned)div_up(total, 256)), dim3(256), 0, c->stream,
                       (const double2*)c->d_g, coeff, (const double*)c->d_P, (const int*)c->d_poff, c->nt, c->L, total);
    return MTIP_OK;
}

int launch_sht_inverse(mtip_ctx* c, const double2* coeff, double2* grid, const InvEpilogue& epi) {
    // the real-space epilogue and the coefficient difference on load exist in the wide kernel only
    if ((epi.mode == EPI_REAL_UPDATE || epi.coeff_sub != nullptr) && !c->sht.real_update)
        return sht_no_kernel(c, epi.coeff_sub != nullptr ? "inverse with coefficient difference" : "inverse", epi.mode);
    // timer families by epilogue: they move different amounts of data
    ProfScope ps(c, epi.mode == EPI_REAL_UPDATE ? "sht_inv_real" : (epi.mode == EPI_MODULUS || epi.mode == EPI_MODULUS_FIXED) ? "sht_inv_modulus" : "sht_inv");
    if (c->sht.inv == SHT_INV_REG || c->sht.inv == SHT_INV_WIDE) return launch_sht_inverse_reg(c, coeff, grid, epi);
    if (c->sht.inv == SHT_INV_LDS) return launch_sht_inverse_fused(c, coeff, grid, epi);
    if (c->sht.inv == SHT_INV_BIG) return launch_bigl_inverse(c, coeff, grid, epi);
    if (epi.mode != EPI_STORE && epi.mode != EPI_MODULUS && epi.mode != EPI_SCALE_SHELL) return sht_no_kernel(c, "generic inverse", epi.mode);
    const long long nrows = (long long)c->B * c->N * c->nt;
    const long long total = nrows * c->nm;
    hipLaunchKernelGGL(k_leg_inv, dim3((unsigned)div_up(total, 256)), dim3(256), 0, c->stream, coeff, c->d_g,
                       (const double*)c->d_P, (const int*)c->d_poff, c->nt, c->L, total);
    dim3 gr, bl;
    size_t sm;
    fft_launch_dims(c, nrows, &gr, &bl, &sm);
    const double2* g = c->d_g;
    const double2* tw = c->d_tw;
    const int* sl = epi.out_slot >= 0 ? (const int*)c->d_slot : nullptr;
    switch (epi.mode) {
        case EPI_MODULUS:
            hipLaunchKernelGGL(k_fft_inv<EPI_MODULUS>, gr, bl, sm, c->stream, g, grid, tw, c->np, c->nt, c->L, c->N, nrows, epi.F, epi.shell_scale, sl, epi.out_slot, c->B);
            break;
        case EPI_SCALE_SHELL:
            hipLaunchKernelGGL(k_fft_inv<EPI_SCALE_SHELL>, gr, bl, sm, c->stream, g, grid, tw, c->np, c->nt, c->L, c->N, nrows, epi.F, epi.shell_scale, sl, epi.out_slot, c->B);
            break;
        default:
            hipLaunchKernelGGL(k_fft_inv<EPI_STORE>, gr, bl, sm, c->stream, g, grid, tw, c->np, c->nt, c->L, c->N, nrows, epi.F, epi.shell_scale, sl, epi.out_slot, c->B);
            break;
    }
    return MTIP_OK;
}

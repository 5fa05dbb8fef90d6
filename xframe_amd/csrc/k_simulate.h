// Upstream step `simulate_ccd`, its back half: degree-2 invariants B_l -> cross-correlation C(q1, q2, Delta)
//   xframe/projects/fxs/projectLibrary/fxs_invariant_tools.py:941-990   deg2_invariant_to_cc_3d
//                                                             60-74     ccd_associated_legendre_matrices_single_l
//                                                             76-97, 992-1001   ccd_legendre_matrices, cc_3d_Fl_worker (mode lstsq)
//                                                             934-939   deg2_invariant_to_cc_2d
//   xframe/library/mathLibrary.py                                       circularHarmonicTransform_real_inverse (irfft(x size, size))
// the inverse of k_cc_deg2.  Included by k_extract.hip (its entry point stands beside mtip_op_cc_to_deg2).
//
// k_sim_harmonics_cc (mode back_substitution, and dimensions 2).  A workgroup owns one q1 and SIM_TQ consecutive q2, one per lane:
//   1. harmonics.  C_n(q1, q2) = sum_{l >= n} B_l(q1, q2) T_l^n(q1) T_l^n(q2) / (2l + 1), n = 0 .. L.  A lane cannot hold L + 1 complex
//      sums, so a wave takes chunks of SIM_NC harmonics: per chunk one pass over l = n0 .. L with SIM_NC sums in registers.  The lanes
//      run along q2: B_l (l, q1, q2) and the transposed table T (l (l+1)/2 + n, q) are read in runs of 64 neighbours, T(q1) and
//      1 / (2l + 1) have wave-uniform addresses (scalar loads).  The C_n go to LDS, (n, lane).  (dimensions 2: C_n = B_n, a copy.)
//   2. angles.  irfft of a real signal of length N = 2L:  C(d) = sum_n w_n (Re C_n cos(2 pi n d / N) - Im C_n sin(2 pi n d / N)),
//      w_0 = w_L = 1, w_n = 2; the sines of n = 0 and n = L are exact zeros, which drops Im C_0 and Im C_L as numpy's irfft does.
//      d and N - d share the cosine and differ in the sign of the sine: E(d) - O(d) and E(d) + O(d) from the two sums of d = 0 .. L.
//      A wave takes SIM_DB angles, the four waves of a round 32 neighbouring ones: each lane reads C_n of its pair from LDS (16 bytes
//      per lane, conflict free) and the weighted twiddles (n, d) of a host table at wave-uniform addresses; 2 SIM_DB FMAs per LDS read.
//   3. the lanes hold columns of the output (q1, q2, d) at stride N: the 64 x 32 tile of a round goes through LDS (columns XOR-swizzled
//      by the row, both directions conflict free) and leaves as runs of 32 consecutive d per pair, once for d and once for N - d.
// N is not a power of two in general; the sums are plain table contractions, (L + 1)^2 FMA pairs per pair of shells.
//
// k_sim_legendre_cc (mode lstsq).  C(q1, q2, Delta) = sum_l B_l / (4 pi) P_l(cos t1 cos t2 + sin t1 sin t2 cos Delta) for the samples
// Delta <= pi, the samples above as the mirror [1:-1][::-1] (971): sample j also goes to n_delta - j.  A wave owns a pair, its lanes
// run along Delta (consecutive lanes write consecutive complex samples); P_l by the three-term recurrence in registers, B_l(q1, q2) and
// the recurrence coefficients at wave-uniform addresses.  The argument is rounded as numpy rounds it (no fused multiply-add): dP_l/dx
// reaches l (l + 1) / 2.

#define SIM_TQ 64                      // q2 per workgroup: one per lane
#define SIM_WAVES 4
#define SIM_NC 8                       // harmonics per register chunk of the contraction
#define SIM_DB 8                       // angles per wave and round
#define SIM_RD (SIM_WAVES * SIM_DB)    // angles per round: the width of the staging tile
#define SIM_MAX_NQ 4096
#define SIM_MAX_L 128
#define SIM_MAX_ND 4096

// bl (L + 1, nq, nq); legt ((L + 1)(L + 2) / 2, nq): T_l^n(q) at row l (l + 1) / 2 + n; inv (L + 1): 1 / (2l + 1); tw (L + 1, ndp):
// w_n (cos, sin)(2 pi n d / N), zeros for d > L; out (nq, nq, 2L).  The inputs are __restrict__ and read only: loads at wave-uniform
// addresses become scalar loads.
__global__ void __launch_bounds__(SIM_WAVES * 64) k_sim_harmonics_cc(const double2* __restrict__ bl, const double* __restrict__ legt,
                                                                     const double* __restrict__ inv, const double2* __restrict__ tw,
                                                                     double* __restrict__ out, int nq, int L, int ndp, int contract) {
    HIP_DYNAMIC_SHARED(double2, s_c)                                       // (L + 1, SIM_TQ) harmonics, then (SIM_TQ, SIM_RD) doubles
    double* s_st = reinterpret_cast<double*>(s_c + (size_t)(L + 1) * SIM_TQ);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q1 = blockIdx.y, q2base = blockIdx.x * SIM_TQ;
    const int q2 = min(q2base + lane, nq - 1);                             // (lanes past the last shell compute a copy and write nothing)
    const size_t nqq = (size_t)nq * nq;
    const double2* b = bl + (size_t)q1 * nq + q2;
    if (!contract) {
        for (int n = wave; n <= L; n += SIM_WAVES) s_c[n * SIM_TQ + lane] = b[(size_t)n * nqq];
    } else {
        const int nchunks = (L + SIM_NC) / SIM_NC;
        for (int ci = wave; ci < nchunks; ci += SIM_WAVES) {
            const int n0 = ci * SIM_NC;
            double2 acc[SIM_NC];
#pragma unroll
            for (int k = 0; k < SIM_NC; ++k) acc[k] = make_double2(0.0, 0.0);
#pragma unroll 2
            for (int l = n0; l <= L; ++l) {
                const double2 bs = cscale(b[(size_t)l * nqq], inv[l]);
                const size_t row0 = (size_t)(l * (l + 1) / 2);
                double w[SIM_NC];
                // the harmonics n > l of the chunk's first orders read row l again and enter with weight 0: no branch, all loads in flight
#pragma unroll
                for (int k = 0; k < SIM_NC; ++k) {
                    const double* t = legt + (row0 + min(n0 + k, l)) * nq;
                    w[k] = t[q1] * t[q2];
                }
#pragma unroll
                for (int k = 0; k < SIM_NC; ++k) {
                    const double wk = n0 + k <= l ? w[k] : 0.0;
                    acc[k].x = fma(bs.x, wk, acc[k].x);
                    acc[k].y = fma(bs.y, wk, acc[k].y);
                }
            }
#pragma unroll
            for (int k = 0; k < SIM_NC; ++k)
                if (n0 + k <= L) s_c[(n0 + k) * SIM_TQ + lane] = acc[k];
        }
    }
    __syncthreads();
    const int N = 2 * L;
    for (int d_round = 0; d_round < ndp; d_round += SIM_RD) {
        const int d0 = d_round + wave * SIM_DB;
        double E[SIM_DB], O[SIM_DB];
#pragma unroll
        for (int k = 0; k < SIM_DB; ++k) E[k] = O[k] = 0.0;
        for (int n = 0; n <= L; ++n) {
            const double2 c = s_c[n * SIM_TQ + lane];
            const double2* w = tw + (size_t)n * ndp + d0;
#pragma unroll
            for (int k = 0; k < SIM_DB; ++k) {
                E[k] = fma(c.x, w[k].x, E[k]);
                O[k] = fma(c.y, w[k].y, O[k]);
            }
        }
        for (int side = 0; side < 2; ++side) {                             // d, then N - d
            __syncthreads();
#pragma unroll
            for (int k = 0; k < SIM_DB; ++k)
                s_st[lane * SIM_RD + ((wave * SIM_DB + k) ^ (lane & (SIM_RD - 1)))] = side ? E[k] + O[k] : E[k] - O[k];
            __syncthreads();
            const int col = tid & (SIM_RD - 1), d = d_round + col;
            const bool d_ok = side ? (d >= 1 && d < L) : (d <= L);
            const int pos = side ? N - d : d;
            for (int p = tid / SIM_RD; p < SIM_TQ; p += SIM_WAVES * 64 / SIM_RD)
                if (d_ok && q2base + p < nq)
                    out[((size_t)q1 * nq + q2base + p) * N + pos] = s_st[p * SIM_RD + (col ^ (p & (SIM_RD - 1)))];
        }
    }
}

// bl (L + 1, nq, nq); cst (2, nq): cos, sin of theta_q; cosd (nh): cos Delta of the samples Delta <= pi; rec (L + 1):
// ((2l + 1) / (l + 1), l / (l + 1)); out (nq, nq, nd)
__global__ void __launch_bounds__(SIM_WAVES * 64) k_sim_legendre_cc(const double2* __restrict__ bl, const double* __restrict__ cst,
                                                                    const double* __restrict__ cosd, const double2* __restrict__ rec,
                                                                    double2* __restrict__ out, int nq, int L, int nd, int nh) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q1 = blockIdx.y, q2 = blockIdx.x * SIM_WAVES + wave;
    if (q2 >= nq) return;                                                  // (a whole wave: the kernel has no barrier)
    const size_t nqq = (size_t)nq * nq;
    const double c12 = cst[q1] * cst[q2], s12 = cst[nq + q1] * cst[nq + q2];
    const double2* b = bl + (size_t)q1 * nq + q2;
    double2* row = out + ((size_t)q1 * nq + q2) * nd;
    const double inv4pi = 1.0 / (4.0 * 3.14159265358979323846);
    for (int j = lane; j < nh; j += 64) {
        double x;
        {
#pragma clang fp contract(off)
            const double sc = s12 * cosd[j];                               // numpy's rounding of c1 c2 + s1 s2 cos(Delta) (95)
            x = c12 + sc;
        }
        double p0 = 1.0, p1 = x;
        double2 acc = b[0];
        acc.x = fma(b[nqq].x, x, acc.x);
        acc.y = fma(b[nqq].y, x, acc.y);
        for (int l = 1; l < L; ++l) {
            const double2 r = rec[l], bv = b[(size_t)(l + 1) * nqq];
            const double pn = fma(r.x * x, p1, -(r.y * p0));               // P_{l+1} = ((2l + 1) x P_l - l P_{l-1}) / (l + 1)
            p0 = p1;
            p1 = pn;
            acc.x = fma(bv.x, pn, acc.x);
            acc.y = fma(bv.y, pn, acc.y);
        }
        acc = cscale(acc, inv4pi);
        row[j] = acc;
        if (j >= 1 && j <= nh - 2) row[nd - j] = acc;
    }
}

// the staging copy of a caller's host array lives in device memory: true where the array is host memory (the CPU build of the tests
// has no such distinction and counts every array, against the fixed budget of mtip_free_memory)
static inline bool sim_needs_scratch(const void* p) {
#ifdef __HIPCC__
    return !mtip_is_device_pointer(p);
#else
    return p != nullptr;
#endif
}

extern "C" int mtip_op_deg2_to_cc(mtip_ctx* c, int n_q, int max_order, int n_delta, int dimensions, int mode, const mtip_cdouble* bl,
                                  const double* legendre_t, const double* cos_sin_theta, const double* cos_delta, void* cc_out) {
    if (!c) return MTIP_EINVAL;
    char msg[400];
    const bool lsq = mode == MTIP_SIM_LSTSQ;
    if (!bl || !cc_out || (dimensions != 2 && dimensions != 3) || (mode != MTIP_SIM_BACK_SUBSTITUTION && !lsq) || (lsq && dimensions != 3)) {
        c->err = "deg2_to_cc: null buffer, dimensions not 2 or 3, or a mode other than back_substitution (0) and lstsq (1, dimensions 3)";
        return MTIP_EINVAL;
    }
    if (n_q < 1 || n_q > SIM_MAX_NQ || max_order < 1 || max_order > SIM_MAX_L || n_delta < 2 || n_delta > SIM_MAX_ND) {
        snprintf(msg, sizeof msg,
                 "deg2_to_cc: built for 1 <= n_q <= %d, 1 <= max_order <= %d and 2 <= n_delta <= %d; got n_q = %d, max_order = %d, "
                 "n_delta = %d",
                 SIM_MAX_NQ, SIM_MAX_L, SIM_MAX_ND, n_q, max_order, n_delta);
        c->err = msg;
        return MTIP_EINVAL;
    }
    if (!lsq && n_delta != 2 * max_order) {
        snprintf(msg, sizeof msg, "deg2_to_cc: the inverse harmonic transform gives n_delta = 2 max_order = %d angles, got n_delta = %d",
                 2 * max_order, n_delta);
        c->err = msg;
        return MTIP_EINVAL;
    }
    if (lsq && (n_delta & 1)) {
        snprintf(msg, sizeof msg, "deg2_to_cc: lstsq mirrors the samples below pi onto those above (fxs_invariant_tools.py:971), which needs "
                                  "an even n_delta with pi on the grid; got n_delta = %d", n_delta);
        c->err = msg;
        return MTIP_EINVAL;
    }
    if ((lsq && (!cos_sin_theta || !cos_delta)) || (!lsq && dimensions == 3 && !legendre_t)) {
        c->err = "deg2_to_cc: a table the mode asks for is null (legendre_t: back_substitution in 3 dimensions; cos_sin_theta, cos_delta: lstsq)";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    const int L = max_order, nh = n_delta / 2 + 1;
    const size_t nqq = (size_t)n_q * n_q, ntri = (size_t)(L + 1) * (L + 2) / 2;
    const size_t out_bytes = nqq * n_delta * (lsq ? sizeof(double2) : sizeof(double)), bl_bytes = nqq * (L + 1) * sizeof(double2);
    {
        const size_t need = (sim_needs_scratch(cc_out) ? out_bytes : 0) + (sim_needs_scratch(bl) ? bl_bytes : 0);
        const size_t fr = mtip_free_memory();
        if (need > fr) {
            snprintf(msg, sizeof msg,
                     "deg2_to_cc: the cross-correlation of %d x %d pairs x %d angles needs %.3f GB (%s) and B_l %.3f GB; the copies of the "
                     "host arrays among them need %.3f GB of device memory, %.3f GB are free",
                     n_q, n_q, n_delta, (double)out_bytes * 1e-9, lsq ? "complex128" : "float64", (double)bl_bytes * 1e-9, (double)need * 1e-9,
                     (double)fr * 1e-9);
            c->err = msg;
            return MTIP_ENOMEM;
        }
    }
    const long double pi = 3.14159265358979323846264338327950288L;
    std::vector<double2> tab;                                                      // tw (harmonics) or rec (lstsq)
    std::vector<double> inv;
    const int ndp = div_up(L + 1, SIM_RD) * SIM_RD;
    if (lsq) {
        tab.resize((size_t)L + 1);
        for (int l = 0; l <= L; ++l) tab[l] = make_double2((double)(2 * l + 1) / (double)(l + 1), (double)l / (double)(l + 1));
    } else {
        const int N = 2 * L;
        tab.assign((size_t)(L + 1) * ndp, make_double2(0.0, 0.0));
        inv.resize((size_t)L + 1);
        for (int l = 0; l <= L; ++l) inv[l] = 1.0 / (double)(2 * l + 1);
        for (int n = 0; n <= L; ++n)
            for (int d = 0; d <= L; ++d) {
                const int k = (int)(((long long)n * d) % N);
                const double w = (n == 0 || n == L) ? 1.0 : 2.0;
                double cs, sn;
                if (k == 0) { cs = 1.0; sn = 0.0; }                                // the exact points of the circle: the sines of
                else if (2 * k == N) { cs = -1.0; sn = 0.0; }                      // n = 0 and n = L are exact zeros
                else if (4 * k == N) { cs = 0.0; sn = 1.0; }
                else if (4 * k == 3 * N) { cs = 0.0; sn = -1.0; }
                else {
                    const long double ang = 2.0L * pi * (long double)k / (long double)N;
                    cs = (double)cosl(ang);
                    sn = (double)sinl(ang);
                }
                tab[(size_t)n * ndp + d] = make_double2(w * cs, w * sn);
            }
    }
    const bool contract = !lsq && dimensions == 3;
    DevView v_bl(c, bl, bl_bytes, true, false);
    DevView v_leg(c, contract ? legendre_t : nullptr, ntri * n_q * sizeof(double), true, false);
    DevView v_cst(c, lsq ? cos_sin_theta : nullptr, (size_t)2 * n_q * sizeof(double), true, false);
    DevView v_cd(c, lsq ? cos_delta : nullptr, (size_t)nh * sizeof(double), true, false);
    DevView v_tab(c, tab.data(), tab.size() * sizeof(double2), true, false);
    DevView v_inv(c, inv.empty() ? nullptr : inv.data(), inv.size() * sizeof(double), true, false);
    DevView v_out(c, cc_out, out_bytes, false, true);
    for (DevView* v : {&v_bl, &v_leg, &v_cst, &v_cd, &v_tab, &v_inv, &v_out})
        if (v->err != hipSuccess) {
            snprintf(msg, sizeof msg, "deg2_to_cc: %s (cross-correlation %.3f GB, B_l %.3f GB)", hipGetErrorString(v->err),
                     (double)out_bytes * 1e-9, (double)bl_bytes * 1e-9);
            c->err = msg;
            return v->err == hipErrorOutOfMemory ? MTIP_ENOMEM : MTIP_EHIP;
        }
    {
        ProfScope ps(c, "deg2_cc");
        if (lsq) {
            hipLaunchKernelGGL(k_sim_legendre_cc, dim3((unsigned)div_up(n_q, SIM_WAVES), (unsigned)n_q), dim3(SIM_WAVES * 64), 0, c->stream,
                               (const double2*)v_bl.dev, (const double*)v_cst.dev, (const double*)v_cd.dev, (const double2*)v_tab.dev,
                               (double2*)v_out.dev, n_q, L, n_delta, nh);
        } else {
            const size_t lds = (size_t)(L + 1) * SIM_TQ * sizeof(double2) + (size_t)SIM_TQ * SIM_RD * sizeof(double);
            hipLaunchKernelGGL(k_sim_harmonics_cc, dim3((unsigned)div_up(n_q, SIM_TQ), (unsigned)n_q), dim3(SIM_WAVES * 64), lds, c->stream,
                               (const double2*)v_bl.dev, (const double*)v_leg.dev, (const double*)v_inv.dev, (const double2*)v_tab.dev,
                               (double*)v_out.dev, n_q, L, ndp, contract ? 1 : 0);
        }
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = v_out.finish();
    if (e != hipSuccess) {
        c->err = std::string("deg2_to_cc: ") + hipGetErrorString(e);
        return MTIP_EHIP;
    }
    return MTIP_OK;
}

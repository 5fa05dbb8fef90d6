// extract: the conditioning stages of modify_cross_correlation that stand in front of (low pass, harmonic filter) and behind
// (binned mean) the switches of k_cc_prepare
//   xframe/projects/fxs/projectLibrary/fxs_invariant_tools.py:245-247   subtract_average_intensity (first, whatever else runs)
//                                                             248-252   low_pass_order_in_q: scipy sosfilt along q1, then q2
//                                                             253-263   enforce_max_order / enforce_zero_odd_harmonics
//                                                             281-283   apply_binned_mean, 308-332 binned_mean
//   xframe/library/mathLibrary.py:484-496                               circularHarmonicTransform_real_forward / _inverse
// Included by k_extract.hip behind k_extract_lsq.h.  Three whole-array passes over C(q1, q2, Delta); each takes the average
// intensity as an option and subtracts I(q1) I(q2) while it reads, so that the first stage that runs does the subtraction.
//
// k_cc_lowpass          one lane per (fixed q, Delta): the recurrence of ONE second-order section (direct form II transposed, zero
//                       initial state, scipy's operation order without contraction) walks the other q axis.  Lanes lie along Delta:
//                       every step of the walk is one coalesced row access; the loads of the next four steps are issued before
//                       the four of this one are filtered, since the addresses do not depend on the recurrence.  Two launches:
//                       axis 0 (cc -> out), axis 1 (out -> out in place: a lane reads a sample before it writes it).
// k_cc_harmonic_filter  one workgroup per pair: the row and a table of the n twiddles (made on the host in extended precision,
//                       indexed by (m d) mod n, the index kept by addition) sit in LDS; a wave owns a kept harmonic at a time, its
//                       lanes split the angles and a butterfly adds them up; then one lane per angle sums the kept harmonics:
//                         y[d] = sum_m w_m (a_m cos(2 pi m d / n) + b_m sin(2 pi m d / n)),  a_m - i b_m = rfft(x)[m] / n,
//                       w_m = 1 for m = 0 and (even n) m = n / 2, else 2: numpy's irfft, which drops the imaginary parts of those two.
// k_cc_half_shift       enforce_zero_odd_harmonics alone at even n: y[d] = (x[d] + x[d + n/2]) / 2 keeps exactly the even harmonics.
// k_cc_binned_mean      one workgroup per pair: the rolled row goes to LDS with masked samples as zeros (line 322), then one lane per
//                       bin adds its run of samples in index order and divides by the count of valid ones; the runs come from the
//                       host, which forms them with the reference's own floor division (the kernel never recomputes a bin edge).
#pragma once

struct ClArgs {
    const double* in;                  // (nq, nq, nd)
    const double* avg;                 // (nq) or null
    double* out;
    int nq, nd, axis;
    double b0, b1, b2, a1, a2;
};

#define CL_DEPTH 4

__global__ void __launch_bounds__(256) k_cc_lowpass(ClArgs a) {
    // scipy's _sosfilt keeps  y = b0 x + z0,  z0 = b1 x - a1 y + z1,  z1 = b2 x - a2 y  as separate products and sums
#pragma clang fp contract(off)
    const int d = blockIdx.x * 256 + threadIdx.x, fixed = blockIdx.y;
    if (d >= a.nd) return;
    const size_t row = (size_t)a.nd, plane = (size_t)a.nq * a.nd;
    const size_t base = (a.axis == 0 ? (size_t)fixed * row : (size_t)fixed * plane) + d;
    const size_t step = a.axis == 0 ? plane : row;
    const double af = a.avg ? a.avg[fixed] : 0.0;
    auto load = [&](int q) { return q < a.nq ? a.in[base + (size_t)q * step] - (a.avg ? a.avg[q] * af : 0.0) : 0.0; };
    double z0 = 0.0, z1 = 0.0, x[CL_DEPTH], xn[CL_DEPTH];
#pragma unroll
    for (int u = 0; u < CL_DEPTH; ++u) x[u] = load(u);
    for (int q0 = 0; q0 < a.nq; q0 += CL_DEPTH) {
#pragma unroll
        for (int u = 0; u < CL_DEPTH; ++u) xn[u] = load(q0 + CL_DEPTH + u);
#pragma unroll
        for (int u = 0; u < CL_DEPTH; ++u) {
            if (q0 + u < a.nq) {
                const double y = a.b0 * x[u] + z0;
                z0 = a.b1 * x[u] - a.a1 * y + z1;
                z1 = a.b2 * x[u] - a.a2 * y;
                a.out[base + (size_t)(q0 + u) * step] = y;
            }
            x[u] = xn[u];
        }
    }
}

struct ChArgs {
    const double* in;                  // (nq, nq, nd)
    const double* avg;                 // (nq) or null
    const double2* tw;                 // (nd) (cos, sin)(2 pi k / nd)
    double* out;
    int nq, nd, n_keep, m_step;        // kept harmonics m = j m_step, j < n_keep
    double inv_n;
};

__global__ void __launch_bounds__(256) k_cc_harmonic_filter(ChArgs a) {
    HIP_DYNAMIC_SHARED(double2, ch_lds)                               // twiddles (16-byte entries first), row, coefficients
    double2* s_tw = ch_lds;
    double* s_row = reinterpret_cast<double*>(ch_lds + a.nd);
    double* s_coef = s_row + a.nd;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q1 = blockIdx.x / a.nq, q2 = blockIdx.x - q1 * a.nq;
    const size_t row = (size_t)blockIdx.x * a.nd;
    const double sub = a.avg ? a.avg[q1] * a.avg[q2] : 0.0;
    for (int d = tid; d < a.nd; d += 256) {
        s_row[d] = a.in[row + d] - sub;
        s_tw[d] = a.tw[d];
    }
    __syncthreads();
    for (int j = wave; j < a.n_keep; j += 4) {                        // (wave-uniform: the butterfly below has every lane)
        const int m = j * a.m_step;
        int k = (m * lane) % a.nd;
        const int kstep = (m * 64) % a.nd;
        double re = 0.0, im = 0.0;
        for (int d = lane; d < a.nd; d += 64) {
            const double x = s_row[d];
            const double2 t = s_tw[k];
            re = fma(x, t.x, re);
            im = fma(x, t.y, im);
            k += kstep;
            if (k >= a.nd) k -= a.nd;
        }
        for (int o = 32; o > 0; o >>= 1) {
            re += __shfl_xor(re, o);
            im += __shfl_xor(im, o);
        }
        if (lane == 0) {
            const double w = (m == 0 || 2 * m == a.nd) ? a.inv_n : 2.0 * a.inv_n;
            s_coef[2 * j] = re * w;
            s_coef[2 * j + 1] = im * w;
        }
    }
    __syncthreads();
    for (int d = tid; d < a.nd; d += 256) {
        const int kstep = (a.m_step * d) % a.nd;
        int k = 0;
        double y = 0.0;
        for (int j = 0; j < a.n_keep; ++j) {
            const double2 t = s_tw[k];
            y = fma(s_coef[2 * j], t.x, y);
            y = fma(s_coef[2 * j + 1], t.y, y);
            k += kstep;
            if (k >= a.nd) k -= a.nd;
        }
        a.out[row + d] = y;
    }
}

__global__ void __launch_bounds__(256) k_cc_half_shift(ChArgs a) {
    const int d = blockIdx.y * 256 + threadIdx.x;                     // (pairs along x: there can be 4096^2 of them)
    if (d >= a.nd) return;
    const int q1 = blockIdx.x / a.nq, q2 = blockIdx.x - q1 * a.nq, h = a.nd >> 1;
    const size_t row = (size_t)blockIdx.x * a.nd;
    const double sub = a.avg ? a.avg[q1] * a.avg[q2] : 0.0;
    a.out[row + d] = ((a.in[row + d] - sub) + (a.in[row + (d >= h ? d - h : d + h)] - sub)) / 2;
}

struct CbArgs {
    const double* cc;                  // (nq, nq, nd)
    const uint8_t* mask;               // (nq, nq, nd) 1 = keep
    const double* avg;                 // (nq) or null
    const int* start;                  // (n_bins + 1) first rolled sample of every bin, start[n_bins] = nd
    double* cc_out;                    // (nq, nq, n_bins)
    uint8_t* mask_out;
    int nq, nd, n_bins, roll;
};

__global__ void __launch_bounds__(256) k_cc_binned_mean(CbArgs a) {
    HIP_DYNAMIC_SHARED(double, cb_lds)                                // the rolled row, masked samples as zeros; its mask behind it
    uint8_t* s_m = reinterpret_cast<uint8_t*>(cb_lds + a.nd);
    const int tid = threadIdx.x;
    const int q1 = blockIdx.x / a.nq, q2 = blockIdx.x - q1 * a.nq;
    const size_t row = (size_t)blockIdx.x * a.nd;
    const double sub = a.avg ? a.avg[q1] * a.avg[q2] : 0.0;
    for (int r = tid; r < a.nd; r += 256) {
        const int s = r >= a.roll ? r - a.roll : r - a.roll + a.nd;    // numpy.roll(x, n)[r] = x[r - n]
        const bool m = a.mask[row + s] != 0;
        cb_lds[r] = m ? a.cc[row + s] - sub : 0.0;
        s_m[r] = m ? 1 : 0;
    }
    __syncthreads();
    for (int b = tid; b < a.n_bins; b += 256) {
        double sum = 0.0;
        int cnt = 0;
        for (int r = a.start[b]; r < a.start[b + 1]; ++r) {
            sum += cb_lds[r];
            cnt += s_m[r];
        }
        a.cc_out[(size_t)blockIdx.x * a.n_bins + b] = cnt ? sum / (double)cnt : sum;              // 329: a bin without a sample keeps 0
        a.mask_out[(size_t)blockIdx.x * a.n_bins + b] = cnt ? 1 : 0;
    }
}

// the checks the three operators share; `what` names the operator in the message
static int cc_cond_check_sizes(mtip_ctx* c, const char* what, int n_q, int n_delta, int min_delta) {
    char msg[320];
    if (n_q < 1 || n_delta < min_delta) {
        snprintf(msg, sizeof msg, "%s: n_q >= 1 and n_delta >= %d are needed; got n_q = %d, n_delta = %d", what, min_delta, n_q, n_delta);
        c->err = msg;
        return MTIP_EINVAL;
    }
    if (n_q > CX_MAX_NQ || n_delta > CX_MAX_ND) {
        snprintf(msg, sizeof msg, "%s: built for n_q <= %d and n_delta <= %d; got n_q = %d, n_delta = %d", what, CX_MAX_NQ, CX_MAX_ND, n_q,
                 n_delta);
        c->err = msg;
        return MTIP_EINVAL;
    }
    return MTIP_OK;
}

static int cc_cond_finish(mtip_ctx* c, const char* what, hipError_t e, std::initializer_list<DevView*> outputs) {
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    for (DevView* v : outputs)
        if (e == hipSuccess) e = v->finish();
    if (e != hipSuccess) {
        c->err = std::string(what) + ": " + hipGetErrorString(e);
        return MTIP_EHIP;
    }
    return MTIP_OK;
}

extern "C" int mtip_op_cc_lowpass_q(mtip_ctx* c, int n_q, int n_delta, const double* sos, const double* cc, const double* average_intensity,
                                    double* cc_out) {
    if (!c) return MTIP_EINVAL;
    if (!sos || !cc || !cc_out || cc == cc_out) {
        c->err = "cc_lowpass_q: null buffer, or output aliasing its input";
        return MTIP_EINVAL;
    }
    int rc = cc_cond_check_sizes(c, "cc_lowpass_q", n_q, n_delta, 1);
    if (rc != MTIP_OK) return rc;
    (void)hipSetDevice(c->device);
    double s[6];
    hipError_t e = mtip_copy(c, s, sos, sizeof s, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        c->err = std::string("cc_lowpass_q: ") + hipGetErrorString(e);
        return MTIP_EHIP;
    }
    bool finite = true;
    for (double v : s) finite = finite && std::isfinite(v);
    if (!finite || s[3] != 1.0) {
        c->err = "cc_lowpass_q: sos must be six finite numbers b0 b1 b2 1 a1 a2 (scipy's sosfilt asks for a0 = 1)";
        return MTIP_EINVAL;
    }
    const size_t n = (size_t)n_q * n_q * n_delta;
    DevView v_cc(c, cc, n * sizeof(double), true, false);
    DevView v_avg(c, average_intensity, (size_t)n_q * sizeof(double), true, false);
    DevView v_out(c, cc_out, n * sizeof(double), false, true);
    rc = cc_masked_view_error(c, "cc_lowpass_q", {&v_cc, &v_avg, &v_out});
    if (rc != MTIP_OK) return rc;
    ClArgs a{};
    a.in = (const double*)v_cc.dev;
    a.avg = (const double*)v_avg.dev;
    a.out = (double*)v_out.dev;
    a.nq = n_q;
    a.nd = n_delta;
    a.b0 = s[0];
    a.b1 = s[1];
    a.b2 = s[2];
    a.a1 = s[4];
    a.a2 = s[5];
    {
        ProfScope ps(c, "cc_lowpass");
        const dim3 grid((unsigned)div_up(n_delta, 256), (unsigned)n_q);
        a.axis = 0;
        hipLaunchKernelGGL(k_cc_lowpass, grid, dim3(256), 0, c->stream, a);
        a.in = a.out;                                                // the second pass works in place, and subtracts nothing
        a.avg = nullptr;
        a.axis = 1;
        hipLaunchKernelGGL(k_cc_lowpass, grid, dim3(256), 0, c->stream, a);
    }
    return cc_cond_finish(c, "cc_lowpass_q", hipSuccess, {&v_out});
}

extern "C" int mtip_op_cc_harmonic_filter(mtip_ctx* c, int n_q, int n_delta, int max_order, int zero_odd, const double* cc,
                                          const double* average_intensity, double* cc_out) {
    if (!c) return MTIP_EINVAL;
    if (!cc || !cc_out || cc == cc_out || (max_order < 0 && !zero_odd)) {
        c->err = "cc_harmonic_filter: null buffer, output aliasing its input, or neither a max_order >= 0 nor zero_odd";
        return MTIP_EINVAL;
    }
    int rc = cc_cond_check_sizes(c, "cc_harmonic_filter", n_q, n_delta, 2);
    if (rc != MTIP_OK) return rc;
    (void)hipSetDevice(c->device);
    const size_t n = (size_t)n_q * n_q * n_delta;
    const int top = max_order < 0 ? n_delta / 2 : std::min(max_order, n_delta / 2);     // rfft has the harmonics 0 .. n / 2
    ChArgs a{};
    a.nq = n_q;
    a.nd = n_delta;
    a.m_step = zero_odd ? 2 : 1;
    a.n_keep = top / a.m_step + 1;
    a.inv_n = 1.0 / (double)n_delta;
    const bool half_shift = zero_odd && max_order < 0 && (n_delta & 1) == 0;
    std::vector<double2> tw(half_shift ? 0 : (size_t)n_delta);
    for (size_t k = 0; k < tw.size(); ++k) {
        const long double ang = 2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)n_delta;
        tw[k] = make_double2((double)cosl(ang), (double)sinl(ang));
    }
    DevView v_cc(c, cc, n * sizeof(double), true, false);
    DevView v_avg(c, average_intensity, (size_t)n_q * sizeof(double), true, false);
    DevView v_tw(c, half_shift ? nullptr : tw.data(), tw.size() * sizeof(double2), true, false);
    DevView v_out(c, cc_out, n * sizeof(double), false, true);
    rc = cc_masked_view_error(c, "cc_harmonic_filter", {&v_cc, &v_avg, &v_tw, &v_out});
    if (rc != MTIP_OK) return rc;
    a.in = (const double*)v_cc.dev;
    a.avg = (const double*)v_avg.dev;
    a.tw = (const double2*)v_tw.dev;
    a.out = (double*)v_out.dev;
    {
        ProfScope ps(c, "cc_harmonic");
        if (half_shift) {
            hipLaunchKernelGGL(k_cc_half_shift, dim3((unsigned)(n_q * n_q), (unsigned)div_up(n_delta, 256)), dim3(256), 0, c->stream, a);
        } else {
            const size_t lds = (size_t)n_delta * sizeof(double2) + ((size_t)n_delta + 2 * (size_t)a.n_keep) * sizeof(double);
            hipLaunchKernelGGL(k_cc_harmonic_filter, dim3((unsigned)(n_q * n_q)), dim3(256), lds, c->stream, a);
        }
    }
    return cc_cond_finish(c, "cc_harmonic_filter", hipSuccess, {&v_out});
}

extern "C" int mtip_op_cc_binned_mean(mtip_ctx* c, int n_q, int n_delta, int n_bins, const int32_t* bin_start, int n_roll, const double* cc,
                                      const uint8_t* cc_mask, const double* average_intensity, double* cc_out, uint8_t* mask_out) {
    if (!c) return MTIP_EINVAL;
    char msg[320];
    if (!bin_start || !cc || !cc_mask || !cc_out || !mask_out || cc == cc_out || cc_mask == mask_out) {
        c->err = "cc_binned_mean: null buffer, or output aliasing its input";
        return MTIP_EINVAL;
    }
    int rc = cc_cond_check_sizes(c, "cc_binned_mean", n_q, n_delta, 1);
    if (rc != MTIP_OK) return rc;
    if (n_bins < 1 || n_bins > n_delta || n_roll < 0 || n_roll >= n_delta) {
        snprintf(msg, sizeof msg, "cc_binned_mean: 1 <= n_bins <= n_delta and 0 <= n_roll < n_delta are needed; got n_bins = %d, n_roll = %d, "
                 "n_delta = %d", n_bins, n_roll, n_delta);
        c->err = msg;
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    std::vector<int32_t> start((size_t)n_bins + 1);
    hipError_t e = mtip_copy(c, start.data(), bin_start, start.size() * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        c->err = std::string("cc_binned_mean: ") + hipGetErrorString(e);
        return MTIP_EHIP;
    }
    for (int b = 0; b <= n_bins; ++b)
        if ((b == 0 && start[0] != 0) || (b > 0 && start[b] <= start[b - 1]) || (b == n_bins && start[b] != n_delta)) {
            snprintf(msg, sizeof msg, "cc_binned_mean: bin_start must rise strictly from 0 to n_delta = %d (every bin holds a sample); "
                     "bin_start[%d] = %d", n_delta, b, start[b]);
            c->err = msg;
            return MTIP_EINVAL;
        }
    const size_t nqq = (size_t)n_q * n_q, n = nqq * n_delta;
    DevView v_start(c, start.data(), start.size() * sizeof(int32_t), true, false);
    DevView v_cc(c, cc, n * sizeof(double), true, false);
    DevView v_mask(c, cc_mask, n, true, false);
    DevView v_avg(c, average_intensity, (size_t)n_q * sizeof(double), true, false);
    DevView v_out(c, cc_out, nqq * n_bins * sizeof(double), false, true);
    DevView v_mout(c, mask_out, nqq * n_bins, false, true);
    rc = cc_masked_view_error(c, "cc_binned_mean", {&v_start, &v_cc, &v_mask, &v_avg, &v_out, &v_mout});
    if (rc != MTIP_OK) return rc;
    CbArgs a{};
    a.start = (const int*)v_start.dev;
    a.cc = (const double*)v_cc.dev;
    a.mask = (const uint8_t*)v_mask.dev;
    a.avg = (const double*)v_avg.dev;
    a.cc_out = (double*)v_out.dev;
    a.mask_out = (uint8_t*)v_mout.dev;
    a.nq = n_q;
    a.nd = n_delta;
    a.n_bins = n_bins;
    a.roll = n_roll;
    {
        ProfScope ps(c, "cc_binned_mean");
        const size_t lds = (size_t)n_delta * sizeof(double) + (((size_t)n_delta + 7) & ~(size_t)7);
        hipLaunchKernelGGL(k_cc_binned_mean, dim3((unsigned)nqq), dim3(256), lds, c->stream, a);
    }
    return cc_cond_finish(c, "cc_binned_mean", hipSuccess, {&v_out, &v_mout});
}

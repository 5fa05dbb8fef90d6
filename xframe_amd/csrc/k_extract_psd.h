// The back-substitution modes of ccd_to_deg2_invariant_3d beside `back_substitution` (included by k_extract.hip):
//   xframe/projects/fxs/projectLibrary/fxs_invariant_tools.py:519-576   back_substitution_memory_hungry
//                                                             646-694   back_substitution_qqsym
//                                                             710-761   back_substitution_psd
//   xframe/library/mathLibrary.py:872-892                               nearest_positive_semidefinite_matrix (limit = 0)
//                                 1499-1517                             psd_back_substitution, back_substitution
// on harmonic coefficients C_m(q1, q2) that are already on the device (what k_cc_deg2 writes with dimensions = 2, stride 1).
//
// nearest PSD matrix of a stack, three launches, nothing per matrix through the host:
//   k_psd_prep     H = (A + A^+) / 2 as the column-major work matrix of k_herm_eig, sigma = |H|_F           (one workgroup per matrix)
//   k_herm_eig     one-sided Jacobi on H + sigma 1 (k_extract.hip, unchanged), eigenvalues minus sigma      (one workgroup per matrix)
//   k_psd_rebuild  out = sum_k lambda_k^+ v_k v_k^+, n_clipped = #{lambda_k < 0}                             (tiles of (q1, q2))
// The shift is taken on the FIRST pass: H + |H|_F 1 is positive semi-definite, so the one-sided Jacobi (which returns singular values)
// meets no +x / -x eigenvalue pair, whose singular vectors only span the joint space; mtip_op_hermitian_eig finds such a matrix by
// its residual and repeats it through host memory.  The eigenvalues come out to eps |H|_F absolute -- what LAPACK gives, and all a
// projection onto the positive cone needs (an eigenvalue that small contributes that little to the rebuild either way).
//
// psd back-substitution, from the highest order down, two launches per order and no host round trip between them:
//   k_herm_eig     of the prepared H_l = Herm(C_l / c_l^l), shift sigma_l
//   k_psd_step     rebuilds B_l = sum_k lambda_k^+ v_k v_k^+ for its tile, writes it (where the order stride picks l), subtracts
//                  B_l c_l^m from C_m for every m < l while B_l sits in registers, and leaves H_{l-1}, its norm and its shift for
//                  the next k_herm_eig: the tiles write partial sums of |H_{l-1}|^2 and the last tile to finish adds them in tile
//                  order (the same bits whatever the order of arrival)
// A thread owns the element pair (q1, q2), (q2, q1) with q1 <= q2: B_l is Hermitian by construction (the mirrored element is the
// conjugate, the diagonal real), C_m need not be (a qq_mask may zero one of the two), and the Hermitian part of the next input
// needs both.  c_l^m = P_l^m(q1) P_l^m(q2) / (2 l + 1) is symmetric in the pair.
// The rebuild loads only the eigenvectors with lambda > 0 (the others enter the products as zeros).  It runs on the matrix cores:
// measured at 128 x 128 against a plain FMA tile (one element per thread, eigenvectors staged through LDS), k_psd_step took 34.8 us
// against 41.2 us on average over the steps of L = 32 and 64 (profiles/ccmodes_timing.txt); either is 0.3 % of a step, which waits
// for the single-workgroup Jacobi (13 ms at 128 x 128).

#define PS_T 16                        // tile edge: PS_T x PS_T threads, one element pair each
#define PS_MAX_N 1024
#define PS_MAX_ORDER 128
#define PS_PLAIN_MAX_NQ 4096

// tile pair (ti <= tj) of the upper triangle from the linear block index
__device__ __forceinline__ void ps_tile(int b, int nt, int& ti, int& tj) {
    ti = 0;
    while (b >= nt - ti) {
        b -= nt - ti;
        ++ti;
    }
    tj = ti + b;
}

// A (n_mat, n, n) row major; leg != null: element (i, j) divided by P(i) P(j) / norm first (P at leg[q * ntri + dg]).
// W (n_mat, n, n): column c of H at W + c * n (the layout k_herm_eig rotates); shift (n_mat) = |H|_F
__global__ void __launch_bounds__(256) k_psd_prep(const double2* __restrict__ A_all, double2* __restrict__ W_all, double* __restrict__ shift, int n,
                                                  const double* __restrict__ leg, int ntri, int dg, double norm) {
    __shared__ double s_red[256];
    const double2* A = A_all + (size_t)blockIdx.x * n * n;
    double2* W = W_all + (size_t)blockIdx.x * n * n;
    const int tid = threadIdx.x;
    double f2 = 0.0;
    for (int e = tid; e < n * n; e += 256) {
        const int i = e / n, j = e - i * n;
        double2 x = A[(size_t)i * n + j], y = A[(size_t)j * n + i];
        if (leg) {
            const double cd = leg[(size_t)i * ntri + dg] * leg[(size_t)j * ntri + dg] / norm;
            x = make_double2(x.x / cd, x.y / cd);
            y = make_double2(y.x / cd, y.y / cd);
        }
        const double2 h = make_double2((x.x + y.x) / 2, i == j ? 0.0 : (x.y - y.y) / 2);
        W[(size_t)j * n + i] = h;                                  // column j, row i
        f2 += cabs2(h);
    }
    s_red[tid] = f2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_red[tid] += s_red[tid + o];
        __syncthreads();
    }
    if (tid == 0) shift[blockIdx.x] = sqrt(s_red[0]);
}

// B(i, j) = sum_k lambda_k^+ v_k(i) conj(v_k(j)) for this thread's pair (i = i0 + ty <= j = j0 + tx); V: eigenvector k at V + k * n.
// Through v_mfma_f64_16x16x4: the four waves of the workgroup take the eigenvectors k = 4 w .. 4 w + 3 (mod 16), each
// with the complex product as four real ones (lane: A[i = lane & 15][k = lane >> 4] = lambda^+ v_k(i0 + i), B[k][j = lane & 15] =
// v_k(j0 + j); D reg r = D[(lane >> 4) + 4 r][lane & 15]); the partial tiles meet in LDS and are added in wave order.
__device__ __forceinline__ double2 ps_rebuild_mfma(const double2* __restrict__ V, const double* __restrict__ lam, int n, int i0, int j0, int tx,
                                                   int ty, double2 (*s_part)[PS_T * PS_T]) {
    const int tid = ty * PS_T + tx, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, kq = lane >> 4;
    const int ri = i0 + r16, rj = j0 + r16;
    v4f64 ax = {0.0, 0.0, 0.0, 0.0}, ay = {0.0, 0.0, 0.0, 0.0};
    for (int k0 = wave * 4; k0 < n; k0 += 16) {
        const int k = k0 + kq;
        const double l = k < n ? fmax(lam[k], 0.0) : 0.0;
        double2 a = make_double2(0.0, 0.0), b = make_double2(0.0, 0.0);
        if (l > 0.0) {
            if (ri < n) a = V[(size_t)k * n + ri];
            if (rj < n) b = V[(size_t)k * n + rj];
        }
        a = make_double2(l * a.x, l * a.y);
        ax = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, ax, 0, 0, 0);       // Re a conj(b) = a.x b.x + a.y b.y
        ax = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.y, ax, 0, 0, 0);
        ay = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.x, ay, 0, 0, 0);       // Im a conj(b) = a.y b.x - a.x b.y
        ay = __builtin_amdgcn_mfma_f64_16x16x4f64(-a.x, b.y, ay, 0, 0, 0);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) s_part[wave][(kq + 4 * r) * PS_T + r16] = make_double2(ax[r], ay[r]);
    __syncthreads();
    double2 s = s_part[0][tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) s = make_double2(s.x + s_part[w][tid].x, s.y + s_part[w][tid].y);
    return s;
}

// out (n_mat, n, n) = nearest PSD matrix from the eigenpairs of k_herm_eig; qq_mask (n, n) uint8 or null: pairs with 0 are zeroed
// (fxs_invariant_tools.py:759); n_clipped (n_mat) or null.  grid (tile pairs, n_mat)
__global__ void __launch_bounds__(PS_T * PS_T) k_psd_rebuild(const double2* __restrict__ V_all, const double* __restrict__ lam_all, int n,
                                                             const uint8_t* __restrict__ qq_mask, double2* __restrict__ out_all,
                                                             int* __restrict__ n_clipped) {
    const int tx = threadIdx.x, ty = threadIdx.y, nt = (n + PS_T - 1) / PS_T;
    int ti, tj;
    ps_tile(blockIdx.x, nt, ti, tj);
    const double2* V = V_all + (size_t)blockIdx.y * n * n;
    const double* lam = lam_all + (size_t)blockIdx.y * n;
    double2* out = out_all + (size_t)blockIdx.y * n * n;
    __shared__ double2 s_part[4][PS_T * PS_T];
    const double2 b = ps_rebuild_mfma(V, lam, n, ti * PS_T, tj * PS_T, tx, ty, s_part);
    const int i = ti * PS_T + ty, j = tj * PS_T + tx;
    if (i < n && j < n && i <= j) {
        const bool mij = !qq_mask || qq_mask[(size_t)i * n + j], mji = !qq_mask || qq_mask[(size_t)j * n + i];
        const double2 zero = make_double2(0.0, 0.0);
        if (i == j) {
            out[(size_t)i * n + i] = mij ? make_double2(b.x, 0.0) : zero;
        } else {
            out[(size_t)i * n + j] = mij ? b : zero;
            out[(size_t)j * n + i] = mji ? make_double2(b.x, -b.y) : zero;
        }
    }
    if (n_clipped && blockIdx.x == 0 && tx == 0 && ty == 0) {
        int cnt = 0;
        for (int k = 0; k < n; ++k) cnt += lam[k] < 0.0 ? 1 : 0;
        n_clipped[blockIdx.y] = cnt;
    }
}

struct PsStep {
    const double2* V;                  // (n, n) eigenvectors of H_l, eigenvector k at V + k * n
    const double* lam;                 // (n)
    double2* C;                        // (l_max + 1, n, n) the harmonics, updated in place
    double2* b_out;                    // (l_max + 1, n, n)
    double2* W;                        // (n, n) next work matrix, column major
    double* shift;                     // next shift
    double* partial;                   // (tile pairs) partial sums of |H_{l-1}|^2
    int* counter;                      // tiles finished (left at 0)
    int* info;                         // (l_max + 1) eigenvalues clipped per step
    const double* leg;                 // (n, ntri) stride-1 table
    int n, ntri, l, write;
};

__global__ void __launch_bounds__(PS_T * PS_T) k_psd_step(PsStep a) {
    __shared__ double2 s_part[4][PS_T * PS_T];
    __shared__ double s_red[PS_T * PS_T];
    __shared__ int s_last;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * PS_T + tx, n = a.n, l = a.l;
    const int nt = (n + PS_T - 1) / PS_T;
    int ti, tj;
    ps_tile(blockIdx.x, nt, ti, tj);
    double2 b = ps_rebuild_mfma(a.V, a.lam, n, ti * PS_T, tj * PS_T, tx, ty, s_part);
    const int i = ti * PS_T + ty, j = tj * PS_T + tx;
    const bool act = i < n && j < n && i <= j;
    const size_t nn = (size_t)n * n, eij = (size_t)i * n + j, eji = (size_t)j * n + i;
    double f2 = 0.0;
    if (act) {
        if (i == j) b.y = 0.0;
        if (a.write) {
            a.b_out[(size_t)l * nn + eij] = b;
            if (i != j) a.b_out[(size_t)l * nn + eji] = make_double2(b.x, -b.y);
        }
        // C_m -= B_l c_l^m, m < l (mathLibrary.py:1505); the last one, m = l - 1, becomes the next input
        const double* pi = a.leg + (size_t)i * a.ntri + (size_t)l * (l + 1) / 2;
        const double* pj = a.leg + (size_t)j * a.ntri + (size_t)l * (l + 1) / 2;
        const double norm = (double)(2 * l + 1);
        for (int m = 0; m < l; ++m) {
            const double cm = pi[m] * pj[m] / norm;
            double2 x = a.C[(size_t)m * nn + eij];
            x = make_double2(x.x - b.x * cm, x.y - b.y * cm);
            a.C[(size_t)m * nn + eij] = x;
            double2 y = x;
            if (i != j) {
                y = a.C[(size_t)m * nn + eji];
                y = make_double2(y.x - b.x * cm, y.y + b.y * cm);
                a.C[(size_t)m * nn + eji] = y;
            }
            if (m == l - 1) {                                      // H_{l-1} = Herm(C_{l-1} / c_{l-1}^{l-1}) (1504, 878)
                const int dg = m * (m + 1) / 2 + m;
                const double cd = a.leg[(size_t)i * a.ntri + dg] * a.leg[(size_t)j * a.ntri + dg] / (double)(2 * m + 1);
                x = make_double2(x.x / cd, x.y / cd);
                y = make_double2(y.x / cd, y.y / cd);
                const double2 h = make_double2((x.x + y.x) / 2, i == j ? 0.0 : (x.y - y.y) / 2);
                a.W[eji] = h;                                      // column j, row i
                f2 = cabs2(h);
                if (i != j) {
                    a.W[eij] = make_double2(h.x, -h.y);
                    f2 *= 2;
                }
            }
        }
    }
    if (blockIdx.x == 0 && tid == 0) {
        int cnt = 0;
        for (int k = 0; k < n; ++k) cnt += a.lam[k] < 0.0 ? 1 : 0;
        a.info[l] = cnt;
    }
    if (l == 0) return;
    s_red[tid] = f2;
    __syncthreads();
    for (int o = PS_T * PS_T / 2; o > 0; o >>= 1) {
        if (tid < o) s_red[tid] += s_red[tid + o];
        __syncthreads();
    }
    // hand-off between workgroups inside the launch: the partial sum goes out as an agent-scope (write-through) store, released
    // by the fence before the counter's atomic; the last arriver acquires at agent scope and reads with agent-scope loads
    if (tid == 0) {
        __hip_atomic_store(a.partial + blockIdx.x, s_red[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        s_last = atomicAdd(a.counter, 1) == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (s_last && tid == 0) {
        __threadfence();
        double s = 0.0;
        for (unsigned t = 0; t < gridDim.x; ++t) s += __hip_atomic_load(a.partial + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.shift[0] = sqrt(s);
        *a.counter = 0;
    }
}

// plain elimination (mathLibrary.py:1509-1517) of one element pair per thread: b_out[li stride] = (C_{li stride} - sum_{lj > li}
// B_lj c_lj^li) / c_li^li, subtracted from the highest order down as the reference subtracts them.  hermitian: C_m is the mean of
// C_m and C_m^+ first (fxs_invariant_tools.py:688); masked pairs are zeroed before the elimination (687, 690 / 560)
struct BsPlain {
    const double2* cm;                 // (n_out, n, n)
    const double* leg;                 // (n, ntri) at `stride`
    const uint8_t* qq_mask;
    double2* b_out;                    // (n_out, n, n)
    int n, ntri, stride, n_m, n_out, hermitian;
};

__global__ void __launch_bounds__(256) k_bs_plain(BsPlain a) {
    const int n = a.n;
    const int j = blockIdx.x * 16 + (threadIdx.x & 15), i = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (i >= n || j >= n) return;
    const size_t nn = (size_t)n * n, e = (size_t)i * n + j, et = (size_t)j * n + i;
    const bool keep = !a.qq_mask || a.qq_mask[e];
    const double* pi = a.leg + (size_t)i * a.ntri;
    const double* pj = a.leg + (size_t)j * a.ntri;
    for (int li = a.n_m - 1; li >= 0; --li) {
        double2 acc = make_double2(0.0, 0.0);
        if (keep) {
            acc = a.cm[(size_t)li * a.stride * nn + e];
            if (a.hermitian) {
                const double2 t = a.cm[(size_t)li * a.stride * nn + et];
                acc = make_double2((acc.x + t.x) / 2, (acc.y - t.y) / 2);
            }
        }
        for (int lj = a.n_m - 1; lj > li; --lj) {
            const int tri = lj * (lj + 1) / 2 + li;
            const double c = pi[tri] * pj[tri] / (double)(2 * lj * a.stride + 1);
            const double2 b = a.b_out[(size_t)lj * a.stride * nn + e];
            acc = make_double2(acc.x - b.x * c, acc.y - b.y * c);
        }
        const int dg = li * (li + 1) / 2 + li;
        const double cd = pi[dg] * pj[dg] / (double)(2 * li * a.stride + 1);
        a.b_out[(size_t)li * a.stride * nn + e] = make_double2(acc.x / cd, acc.y / cd);
    }
    for (int l = 0; l < a.n_out; ++l)                              // the orders that are not extracted: zeros (417-419)
        if (l % a.stride != 0 || l / a.stride >= a.n_m) a.b_out[(size_t)l * nn + e] = make_double2(0.0, 0.0);
}

static void ps_launch_eig(mtip_ctx* c, int n, int n_mat, double2* dW, double2* dV, double* dl, const double* dshift, double* dres) {
    // 8 lanes per column pair; the pairs of a round are disjoint, so the rotations and their bits do not depend on how many groups
    // share them: a power of two of threads (the kernel's reductions halve) that covers the pairs, at most the 512 of the entry point
    int threads = 64;
    while (threads < 512 && threads < ((n + 1) / 2) * HE_TG) threads *= 2;
    hipLaunchKernelGGL(k_herm_eig, dim3((unsigned)n_mat), dim3((unsigned)threads), 0, c->stream, dW, dV, dl, n, dshift, dres);
}

static int ps_view_error(mtip_ctx* c, const char* op, std::initializer_list<DevView*> views) {
    for (DevView* v : views)
        if (v->err != hipSuccess) {
            c->err = std::string(op) + ": " + hipGetErrorString(v->err);
            return v->err == hipErrorOutOfMemory ? MTIP_ENOMEM : MTIP_EHIP;
        }
    return MTIP_OK;
}

extern "C" int mtip_op_nearest_psd(mtip_ctx* c, int n, int n_mat, const mtip_cdouble* A, mtip_cdouble* out, int32_t* n_clipped) {
    if (!c) return MTIP_EINVAL;
    char msg[240];
    if (!A || !out || !n_clipped || n_mat < 1 || (const void*)A == (const void*)out) {
        c->err = "nearest_psd: null buffer, output aliasing its input, or n_mat < 1";
        return MTIP_EINVAL;
    }
    if (n < 1 || n > PS_MAX_N) {
        snprintf(msg, sizeof msg, "nearest_psd: built for 1 <= n <= %d; got n = %d", PS_MAX_N, n);
        c->err = msg;
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    const size_t nn = (size_t)n_mat * n * n;
    DevView v_a(c, A, nn * sizeof(double2), true, false);
    DevView v_out(c, out, nn * sizeof(double2), false, true);
    DevView v_clip(c, n_clipped, (size_t)n_mat * sizeof(int32_t), false, true);
    int rc = ps_view_error(c, "nearest_psd", {&v_a, &v_out, &v_clip});
    if (rc != MTIP_OK) return rc;
    DevBuf<double2> dW, dV;
    DevBuf<double> dl, dshift, dres;
    if (dW.alloc(nn) != hipSuccess || dV.alloc(nn) != hipSuccess || dl.alloc((size_t)n_mat * n) != hipSuccess ||
        dshift.alloc((size_t)n_mat) != hipSuccess || dres.alloc((size_t)n_mat) != hipSuccess) {
        c->err = "nearest_psd: out of device memory";
        return MTIP_ENOMEM;
    }
    const int nt = div_up(n, PS_T);
    {
        ProfScope ps(c, "nearest_psd");
        hipLaunchKernelGGL(k_psd_prep, dim3((unsigned)n_mat), dim3(256), 0, c->stream, (const double2*)v_a.dev, (double2*)dW, (double*)dshift, n,
                           (const double*)nullptr, 0, 0, 1.0);
        ps_launch_eig(c, n, n_mat, dW, dV, dl, dshift, dres);
        hipLaunchKernelGGL(k_psd_rebuild, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)n_mat), dim3(PS_T, PS_T), 0, c->stream,
                           (const double2*)dV, (const double*)dl, n, (const uint8_t*)nullptr, (double2*)v_out.dev, (int*)v_clip.dev);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    for (DevView* v : {&v_out, &v_clip})
        if (e == hipSuccess) e = v->finish();
    if (e != hipSuccess) {
        c->err = std::string("nearest_psd: ") + hipGetErrorString(e);
        return MTIP_EHIP;
    }
    return MTIP_OK;
}

extern "C" int mtip_op_cm_backsub(mtip_ctx* c, int n_q, int max_order, int order_stride, int mode, uint32_t flags, const mtip_cdouble* cm,
                                  const double* legendre, const uint8_t* qq_mask, mtip_cdouble* b_out, int32_t* info) {
    if (!c) return MTIP_EINVAL;
    char msg[320];
    const int s = order_stride;
    if (!cm || !legendre || !b_out || (const void*)cm == (const void*)b_out || (mode != MTIP_BS_PLAIN && mode != MTIP_BS_PSD) ||
        (s != 1 && s != 2) || max_order < 0 || n_q < 1 || (flags & ~(uint32_t)MTIP_BS_HERMITIAN_MEAN) ||
        (mode == MTIP_BS_PSD && (flags || !info))) {
        c->err = "cm_backsub: null buffer, output aliasing its input, unknown mode or flag (the Hermitian mean belongs to MTIP_BS_PLAIN), "
                 "or order stride not 1 or 2";
        return MTIP_EINVAL;
    }
    const int nq_max = mode == MTIP_BS_PSD ? PS_MAX_N : PS_PLAIN_MAX_NQ;
    if (n_q > nq_max || max_order > PS_MAX_ORDER) {
        snprintf(msg, sizeof msg, "cm_backsub: mode %s is built for n_q <= %d and max_order <= %d; got n_q = %d, max_order = %d",
                 mode == MTIP_BS_PSD ? "psd" : "plain", nq_max, PS_MAX_ORDER, n_q, max_order);
        c->err = msg;
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    const int n = n_q, L = max_order, n_m = mode == MTIP_BS_PSD ? L + 1 : L / s + 1, ntri = n_m * (n_m + 1) / 2;
    const size_t mat = (size_t)n * n, nn = mat * (L + 1);
    DevView v_cm(c, cm, nn * sizeof(double2), true, false);
    DevView v_leg(c, legendre, (size_t)n * ntri * sizeof(double), true, false);
    DevView v_mask(c, qq_mask, mat, true, false);
    DevView v_out(c, b_out, nn * sizeof(double2), false, true);
    DevView v_info(c, mode == MTIP_BS_PSD ? info : nullptr, (size_t)(L + 1) * sizeof(int32_t), false, true);
    int rc = ps_view_error(c, "cm_backsub", {&v_cm, &v_leg, &v_mask, &v_out, &v_info});
    if (rc != MTIP_OK) return rc;
    hipError_t e = hipSuccess;
    if (mode == MTIP_BS_PLAIN) {
        BsPlain a{};
        a.cm = (const double2*)v_cm.dev;
        a.leg = (const double*)v_leg.dev;
        a.qq_mask = (const uint8_t*)v_mask.dev;
        a.b_out = (double2*)v_out.dev;
        a.n = n;
        a.ntri = ntri;
        a.stride = s;
        a.n_m = n_m;
        a.n_out = L + 1;
        a.hermitian = (flags & MTIP_BS_HERMITIAN_MEAN) ? 1 : 0;
        ProfScope ps(c, "cm_backsub");
        hipLaunchKernelGGL(k_bs_plain, dim3((unsigned)div_up(n, 16), (unsigned)div_up(n, 16)), dim3(256), 0, c->stream, a);
    } else {
        const int nt = div_up(n, PS_T), tiles = nt * (nt + 1) / 2;
        DevBuf<double2> dC, dW, dV;
        DevBuf<double> dl, dshift, dres, dpart;
        DevBuf<int> dcount;
        if (dC.alloc(nn) != hipSuccess || dW.alloc(nn) != hipSuccess || dV.alloc(nn) != hipSuccess || dl.alloc((size_t)(L + 1) * n) != hipSuccess ||
            dshift.alloc((size_t)L + 1) != hipSuccess || dres.alloc((size_t)L + 1) != hipSuccess || dpart.alloc((size_t)tiles) != hipSuccess ||
            dcount.alloc(1) != hipSuccess) {
            snprintf(msg, sizeof msg, "cm_backsub: out of device memory (three work arrays of %.2f GB)", (double)nn * sizeof(double2) / 1e9);
            c->err = msg;
            return MTIP_ENOMEM;
        }
        ProfScope ps(c, "cm_backsub");
        e = hipMemsetAsync(dcount, 0, sizeof(int), c->stream);
        if (e == hipSuccess && s == 2) e = hipMemsetAsync(v_out.dev, 0, nn * sizeof(double2), c->stream);   // the orders not picked (760)
        // every C_m -> its nearest PSD matrix, masked pairs zeroed (755-759): the L + 1 matrices side by side
        hipLaunchKernelGGL(k_psd_prep, dim3((unsigned)(L + 1)), dim3(256), 0, c->stream, (const double2*)v_cm.dev, (double2*)dW, (double*)dshift, n,
                           (const double*)nullptr, 0, 0, 1.0);
        ps_launch_eig(c, n, L + 1, dW, dV, dl, dshift, dres);
        hipLaunchKernelGGL(k_psd_rebuild, dim3((unsigned)tiles, (unsigned)(L + 1)), dim3(PS_T, PS_T), 0, c->stream, (const double2*)dV,
                           (const double*)dl, n, (const uint8_t*)v_mask.dev, (double2*)dC, (int*)nullptr);
        // the loop of mathLibrary.py:1503-1506; the first input by the prepare kernel, every later one by the step before it
        hipLaunchKernelGGL(k_psd_prep, dim3(1), dim3(256), 0, c->stream, (const double2*)(dC + (size_t)L * mat), (double2*)dW, (double*)dshift, n,
                           (const double*)v_leg.dev, ntri, L * (L + 1) / 2 + L, (double)(2 * L + 1));
        PsStep a{};
        a.V = dV;
        a.lam = dl;
        a.C = dC;
        a.b_out = (double2*)v_out.dev;
        a.W = dW;
        a.shift = dshift;
        a.partial = dpart;
        a.counter = dcount;
        a.info = (int*)v_info.dev;
        a.leg = (const double*)v_leg.dev;
        a.n = n;
        a.ntri = ntri;
        for (int l = L; l >= 0 && e == hipSuccess; --l) {
            ps_launch_eig(c, n, 1, dW, dV, dl, dshift, dres);
            a.l = l;
            a.write = (l % s) == 0;
            hipLaunchKernelGGL(k_psd_step, dim3((unsigned)tiles), dim3(PS_T, PS_T), 0, c->stream, a);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);       // the work arrays go when this scope ends
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    for (DevView* v : {&v_out, &v_info})
        if (e == hipSuccess) e = v->finish();
    if (e != hipSuccess) {
        c->err = std::string("cm_backsub: ") + hipGetErrorString(e);
        return MTIP_EHIP;
    }
    return MTIP_OK;
}

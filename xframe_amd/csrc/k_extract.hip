// Upstream step `extract`: B_l -> projection matrices V_l, i.e. the eigen-decomposition of the
// Hermitian degree-2 invariants  xframe/projects/fxs/projectLibrary/fxs_invariant_tools.py:1079-1131 (deg2_invariant_eigenvalues:
// numpy eigh), 1171-1207 (top min(2l+1, Nq) eigenpairs, negative eigenvalues clipped, V_l = eigvecs sqrt(eigvals)).
// One workgroup per matrix: one-sided (Hestenes) Jacobi on the columns of A = B_l with accumulation of the rotations,
//   A V = W (orthogonal columns),  eigenvector i = column i of V,  eigenvalue_i = sign(Re v_i^+ w_i) |w_i|
// (for a Hermitian matrix the right singular vectors are eigenvectors and the singular values |eigenvalues|).  Two eigenvalues
// +x and -x share a singular value, and their singular vectors are then only a basis of the joint space: the kernel
// reports the eigen-residual max_i |w_i - lambda_i v_i| / max|lambda| per matrix, and the host repeats a matrix that
// fails it with the shift A + |A|_F 1 (positive semi-definite, no such pairs; eigenvalues to |A| eps as LAPACK's).
// Semi-definite B_l -- the use the reference makes of it -- pass the first time and keep the relative accuracy of
// their small eigenvalues.
// A one-off setup computation (L+1 matrices of Nq x Nq): matrices stay in global memory (L2 resident), 8 lanes per pair.
#include "mtip_internal.h"
#include <cmath>

#define HE_TG 8
#define HE_MAX_SWEEPS 60
#define HE_TOL 1e-15

__global__ void __launch_bounds__(512) k_herm_eig(double2* __restrict__ Wall, double2* __restrict__ Vall, double* __restrict__ lam_all,
                                                  int n, const double* __restrict__ shift, double* __restrict__ resid_out) {
    __shared__ int s_rotated;
    __shared__ double s_red[512];
    double2* W = Wall + (size_t)blockIdx.x * n * n;           // column c at W + c * n
    double2* V = Vall + (size_t)blockIdx.x * n * n;
    double* lam = lam_all + (size_t)blockIdx.x * n;
    const int tid = threadIdx.x;
    const double sigma = shift ? shift[blockIdx.x] : 0.0;
    for (int e = tid; e < n * n; e += blockDim.x) {
        const bool diag = (e / n) == (e % n);
        V[e] = make_double2(diag ? 1.0 : 0.0, 0.0);
        if (diag) W[e].x += sigma;
    }
    __syncthreads();
    const int Cp = n + (n & 1), rounds = Cp - 1, pairs = Cp / 2;
    const int ngroups = blockDim.x / HE_TG, group = tid / HE_TG, t = tid - group * HE_TG;
    const int per_group = (pairs + ngroups - 1) / ngroups;
    int sweep = 0;
    for (; sweep < HE_MAX_SWEEPS && n > 1; ++sweep) {
        if (tid == 0) s_rotated = 0;
        __syncthreads();
        for (int r = 0; r < rounds; ++r) {
            for (int it = 0; it < per_group; ++it) {
                const int pi = group + it * ngroups;
                int ci = 0, cj = 0;
                bool valid = pi < pairs;
                if (valid) {
                    const int M = Cp - 1;                            // tournament pairing: player M stays, the others rotate
                    if (pi == 0) { ci = r; cj = M; }
                    else { ci = (r + pi) % M; cj = (r - pi + M) % M; }
                    valid = (ci < n) && (cj < n);
                }
                double2* wi = W + (size_t)ci * n;
                double2* wj = W + (size_t)cj * n;
                double alpha = 0.0, beta = 0.0, gr = 0.0, gi = 0.0;
                if (valid)
                    for (int row = t; row < n; row += HE_TG) {
                        const double2 a = wi[row], c = wj[row];
                        alpha += cabs2(a);
                        beta += cabs2(c);
                        gr += a.x * c.x + a.y * c.y;                 // conj(a) * c
                        gi += a.x * c.y - a.y * c.x;
                    }
                for (int o = HE_TG / 2; o > 0; o >>= 1) {
                    alpha += __shfl_xor(alpha, o, HE_TG);
                    beta += __shfl_xor(beta, o, HE_TG);
                    gr += __shfl_xor(gr, o, HE_TG);
                    gi += __shfl_xor(gi, o, HE_TG);
                }
                const double g2 = gr * gr + gi * gi;
                if (valid && g2 > (HE_TOL * HE_TOL) * alpha * beta && g2 > 0.0) {
                    const double gabs = sqrt(g2);
                    const double zeta = (beta - alpha) / (2.0 * gabs);
                    const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
                    const double2 em = make_double2(gr / gabs, -gi / gabs);          // conj(gamma) / |gamma|
                    double2* vi = V + (size_t)ci * n;
                    double2* vj = V + (size_t)cj * n;
                    for (int row = t; row < n; row += HE_TG) {
                        const double2 a = wi[row], bj = cmul(em, wj[row]);
                        wi[row] = make_double2(cs * a.x - sn * bj.x, cs * a.y - sn * bj.y);
                        wj[row] = make_double2(sn * a.x + cs * bj.x, sn * a.y + cs * bj.y);
                        const double2 va = vi[row], vb = cmul(em, vj[row]);
                        vi[row] = make_double2(cs * va.x - sn * vb.x, cs * va.y - sn * vb.y);
                        vj[row] = make_double2(sn * va.x + cs * vb.x, sn * va.y + cs * vb.y);
                    }
                    if (t == 0) s_rotated = 1;
                }
            }
            __syncthreads();
        }
        const int rotated = s_rotated;
        __syncthreads();
        if (!rotated) break;
    }
    // eigenvalue_i = (v_i^+ w_i) (real for a Hermitian matrix): magnitude |w_i|, sign from the inner product
    double res = 0.0, top = 0.0;
    for (int c = tid; c < n; c += blockDim.x) {
        double s2 = 0.0, ip = 0.0;
        for (int row = 0; row < n; ++row) {
            const double2 w = W[(size_t)c * n + row], v = V[(size_t)c * n + row];
            s2 += cabs2(w);
            ip += v.x * w.x + v.y * w.y;
        }
        const double mu = (ip >= 0.0 ? 1.0 : -1.0) * sqrt(s2);                     // eigenvalue of the shifted matrix
        double r2 = 0.0;
        for (int row = 0; row < n; ++row) {
            const double2 w = W[(size_t)c * n + row], v = V[(size_t)c * n + row];
            const double dx = w.x - mu * v.x, dy = w.y - mu * v.y;
            r2 += dx * dx + dy * dy;
        }
        res = fmax(res, sqrt(r2));
        top = fmax(top, fabs(mu));
        lam[c] = mu - sigma;
    }
    s_red[tid] = res;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
        if (tid < o) s_red[tid] = fmax(s_red[tid], s_red[tid + o]);
        __syncthreads();
    }
    res = s_red[0];
    __syncthreads();
    s_red[tid] = top;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
        if (tid < o) s_red[tid] = fmax(s_red[tid], s_red[tid + o]);
        __syncthreads();
    }
    if (tid == 0 && resid_out) resid_out[blockIdx.x] = s_red[0] > 0.0 ? res / s_red[0] : 0.0;
}

#define HE_RESID_TOL 1e-13

static hipError_t herm_eig_pass(mtip_ctx* c, int n, int n_mat, const mtip_cdouble* A, const double* shift_host, double2* dW, double2* dV,
                                double* dl, double* dshift, double* dres, double* eigvals, mtip_cdouble* eigvecs, double* resid) {
    const size_t nn = (size_t)n_mat * n * n;
    hipError_t e = mtip_copy(c, dW, A, nn * sizeof(double2), hipMemcpyHostToDevice);
    if (e == hipSuccess && shift_host) e = mtip_copy(c, dshift, shift_host, (size_t)n_mat * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_herm_eig, dim3((unsigned)n_mat), dim3(512), 0, c->stream, dW, dV, dl, n, shift_host ? dshift : (const double*)nullptr,
                       dres);
    e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = mtip_copy(c, eigvals, dl, (size_t)n_mat * n * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = mtip_copy(c, eigvecs, dV, nn * sizeof(double2), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = mtip_copy(c, resid, dres, (size_t)n_mat * sizeof(double), hipMemcpyDeviceToHost);
    return e;
}

extern "C" int mtip_op_hermitian_eig(mtip_ctx* c, int n, int n_mat, const mtip_cdouble* A, double* eigvals, mtip_cdouble* eigvecs) {
    if (!c) return MTIP_EINVAL;
    if (n < 1 || n > 1024 || n_mat < 1 || !A || !eigvals || !eigvecs) {
        c->err = "hermitian_eig: bad sizes or null buffer";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    DevBuf<double2> dW, dV;
    DevBuf<double> dl, dshift, dres;
    const size_t nn = (size_t)n_mat * n * n, mat = (size_t)n * n;
    if (dW.alloc(nn) != hipSuccess || dV.alloc(nn) != hipSuccess || dl.alloc((size_t)n_mat * n) != hipSuccess ||
        dshift.alloc((size_t)n_mat) != hipSuccess || dres.alloc((size_t)n_mat) != hipSuccess) {
        c->err = "hermitian_eig: out of device memory";
        return MTIP_ENOMEM;
    }
    std::vector<double> resid(n_mat, 0.0);
    hipError_t e = herm_eig_pass(c, n, n_mat, A, nullptr, dW, dV, dl, dshift, dres, eigvals, eigvecs, resid.data());
    std::vector<int> again;
    for (int k = 0; k < n_mat && e == hipSuccess; ++k)
        if (!(resid[k] <= HE_RESID_TOL * n)) again.push_back(k);
    if (e == hipSuccess && !again.empty()) {                                           // +x / -x eigenvalue pairs: shifted repeat
        const int m = (int)again.size();
        std::vector<mtip_cdouble> sub((size_t)m * mat), vec((size_t)m * mat);
        std::vector<double> shift(m), val((size_t)m * n), res2(m);
        for (int i = 0; i < m; ++i) {
            const mtip_cdouble* src = A + (size_t)again[i] * mat;
            double f2 = 0.0;
            for (size_t q = 0; q < mat; ++q) f2 += src[q].re * src[q].re + src[q].im * src[q].im;
            shift[i] = sqrt(f2);
            std::copy(src, src + mat, sub.begin() + (size_t)i * mat);
        }
        e = herm_eig_pass(c, n, m, sub.data(), shift.data(), dW, dV, dl, dshift, dres, val.data(), vec.data(), res2.data());
        for (int i = 0; i < m && e == hipSuccess; ++i) {
            std::copy(val.begin() + (size_t)i * n, val.begin() + (size_t)(i + 1) * n, eigvals + (size_t)again[i] * n);
            std::copy(vec.begin() + (size_t)i * mat, vec.begin() + (size_t)(i + 1) * mat, eigvecs + (size_t)again[i] * mat);
        }
    }
    if (e != hipSuccess) {
        c->err = std::string("hermitian_eig: ") + hipGetErrorString(e);
        return MTIP_EHIP;
    }
    return MTIP_OK;
}

// ---- real symmetric matrices up to 128 x 128: LDS-resident one-sided Jacobi (round 3) ---------------------------------------
// B_l of a real intensity is real (the reference types it complex; its imaginary part is zero from cross-correlation data,
// rounding residue on the `density` route of extract.py:288); the host takes this solver for matrices without imaginary part
// (the rules of fxs_invariant_tools.py:1114-1131 on top).  The matrix is shifted to A' = A + s 1, s = |A|_F: positive definite with condition <= 2, so the
// one-sided Jacobi on its columns  A' V = W  has no +x / -x singular pairs, no numerical null space, and converges in a few
// sweeps; the eigenvectors are the normalised columns of W (left = right singular vectors of a definite matrix, V is never
// formed), the eigenvalues |W_i| - s -- accurate to eps |A|, as LAPACK's.  W lives in LDS for the whole solve (128 x 129 doubles =
// 132 KB; the global-memory kernel above moved 390 x the matrix bytes through HBM), 16 lanes per column pair in the resident-
// column ordering of k_proj.hip (its schedule is read from L2 one round ahead), HBM traffic = the matrix in, the vectors out.
#include "k_jacobi.h"

#define SE_MAX_N 128
#define SE_MAX_SWEEPS 40
// the sweeps go on until one stays below this relative off-diagonal: the shifted matrix has most of its eigenvalues in one cluster
// (those of a rank 2l+1 matrix: all but 2l+1 equal the shift), where the convergence is not quadratic -- measured 7e-5 -> 1e-7 ->
// 1e-11 per sweep -- so the projection kernels' early exit (JL_EARLY) would leave 1e-8
#define SE_EARLY 1e-12

template <int NR>
__device__ __forceinline__ void se_sweep(double* Ws, int ns, int t, int group, const int* __restrict__ tab, int n_rounds, int ps,
                                         bool l_ok, bool& big) {
    double rx[NR];
#pragma unroll
    for (int u = 0; u < NR; ++u) rx[u] = 0.0;
    int cur = -1;
    bool dirty = false;
    int e_next = (group < ps && n_rounds > 0) ? tab[group] : 0;
    for (int r = 0; r < n_rounds; ++r) {
        const int e = e_next;
        if (r + 1 < n_rounds && group < ps) e_next = tab[(size_t)(r + 1) * ps + group];
        const bool act = (e & JS_ACTIVE) != 0;
        const int res = act ? (e & 255) : 0, mov = act ? ((e >> 8) & 255) : 0;
        double* xh = Ws + (size_t)res * ns + t;
        double* xm = Ws + (size_t)mov * ns + t;
        double mx[NR];
#pragma unroll
        for (int u = 0; u < NR; ++u) mx[u] = 0.0;
        if (act) {
#pragma unroll
            for (int u = 0; u < NR; ++u) mx[u] = xm[u * 16];
            if (res != cur) {
#pragma unroll
                for (int u = 0; u < NR; ++u) rx[u] = xh[u * 16];
                if (!l_ok) rx[NR - 1] = 0.0;
                cur = res;
                dirty = false;
            }
            if (!l_ok) mx[NR - 1] = 0.0;
        }
        double alpha = 0.0, beta = 0.0, g = 0.0, zero = 0.0;
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            alpha = fma(rx[u], rx[u], alpha);
            beta = fma(mx[u], mx[u], beta);
            g = fma(rx[u], mx[u], g);
        }
        group_sum4<16>(alpha, beta, g, zero);                     // (every group: uniform control flow around DPP)
        const double g2 = g * g, ab = alpha * beta;
        if (act && g2 > (JAC_TOL * JAC_TOL) * ab && g2 > 0.0) {
            big = big || (g2 > (SE_EARLY * SE_EARLY) * ab);
            const double d = 0.5 * (beta - alpha);
            const double ih = fast_rsqrt(fma(d, d, g2));
            const double c2 = fma(0.5 * fabs(d), ih, 0.5);
            const double rc = fast_rsqrt(c2);
            const double cs = c2 * rc, w = ((d >= 0.0 ? 0.5 : -0.5) * ih * rc) * g;
#pragma unroll
            for (int u = 0; u < NR; ++u) {
                const double a = rx[u], bq = mx[u];
                rx[u] = fma(-w, bq, cs * a);
                if (u < NR - 1 || l_ok) xm[u * 16] = fma(w, a, cs * bq);
            }
            dirty = true;
        }
        if (act && (e & JS_WB)) {
            if (dirty) {
#pragma unroll
                for (int u = 0; u < NR; ++u)
                    if (u < NR - 1 || l_ok) xh[u * 16] = rx[u];
            }
            cur = -1;
        }
        __syncthreads();
    }
}

// one workgroup per matrix; A (n_mat, n, n) real symmetric (either triangle order: it is symmetric), U (n_mat, n, n) eigenvector i
// in U[i][:], lam (n_mat, n)
__global__ void __launch_bounds__(1024) k_sym_eig(const double* __restrict__ A_all, double* __restrict__ U_all, double* __restrict__ lam_all,
                                                  int n, const int* __restrict__ sched, const int* __restrict__ sched_off,
                                                  const int* __restrict__ sched_rounds, int sched_ps, int* __restrict__ sweeps_out) {
    HIP_DYNAMIC_SHARED(double, Ws)
    __shared__ double s_red[16];
    __shared__ double s_gmax[64];
    __shared__ int s_cont;
    const double* A = A_all + (size_t)blockIdx.x * n * n;
    double* U = U_all + (size_t)blockIdx.x * n * n;
    double* lam = lam_all + (size_t)blockIdx.x * n;
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int ns = n | 1, nr = (n + 15) >> 4;
    // |A|_F
    double f2 = 0.0;
    for (int e = tid; e < n * n; e += nthreads) f2 = fma(A[e], A[e], f2);
    for (int o = 32; o > 0; o >>= 1) f2 += __shfl_xor(f2, o, 64);
    if ((tid & 63) == 0) s_red[tid >> 6] = f2;
    __syncthreads();
    double s = 0.0;
    for (int wv = 0; wv < (nthreads >> 6); ++wv) s += s_red[wv];
    s = sqrt(s);
    if (!(s > 0.0)) s = 1.0;                                       // the zero matrix: eigenvalues 0, vectors e_i
    for (int e = tid; e < n * n; e += nthreads) {
        const int cc = e / n, r = e - cc * n;
        Ws[(size_t)cc * ns + r] = A[e] + (cc == r ? s : 0.0);     // column cc of the symmetric matrix = its row cc
    }
    __syncthreads();
    const int ngroups = nthreads >> 4, group = tid >> 4, t = tid & 15;
    const bool l_ok = t + (nr - 1) * 16 < n;
    int sweep = 0;
    if (n > 1) {
        const int* tab = sched + sched_off[n];
        const int nrd = sched_rounds[n];
        for (; sweep < SE_MAX_SWEEPS; ++sweep) {
            bool big = false;
            switch (nr) {
            case 1: se_sweep<1>(Ws, ns, t, group, tab, nrd, sched_ps, l_ok, big); break;
            case 2: se_sweep<2>(Ws, ns, t, group, tab, nrd, sched_ps, l_ok, big); break;
            case 3: se_sweep<3>(Ws, ns, t, group, tab, nrd, sched_ps, l_ok, big); break;
            case 4: se_sweep<4>(Ws, ns, t, group, tab, nrd, sched_ps, l_ok, big); break;
            case 5: se_sweep<5>(Ws, ns, t, group, tab, nrd, sched_ps, l_ok, big); break;
            case 6: se_sweep<6>(Ws, ns, t, group, tab, nrd, sched_ps, l_ok, big); break;
            case 7: se_sweep<7>(Ws, ns, t, group, tab, nrd, sched_ps, l_ok, big); break;
            default: se_sweep<8>(Ws, ns, t, group, tab, nrd, sched_ps, l_ok, big); break;
            }
            if (t == 0) s_gmax[group] = big ? 1.0 : 0.0;
            __syncthreads();
            if (tid == 0) {
                double m = 0.0;
                for (int gq = 0; gq < ngroups; ++gq) m = fmax(m, s_gmax[gq]);
                s_cont = m > 0.0 ? 1 : 0;
            }
            __syncthreads();
            const int cont = s_cont;
            __syncthreads();
            if (!cont) {
                ++sweep;
                break;
            }
        }
    }
    if (tid == 0 && sweeps_out) sweeps_out[blockIdx.x] = sweep;
    // eigenvector i = W_i / |W_i|, eigenvalue |W_i| - s
    for (int cc0 = 0; cc0 < n; cc0 += ngroups) {                   // uniform trip count: DPP sums need the whole group
        const int cc = cc0 + group;
        double s2 = 0.0;
        if (cc < n)
            for (int u = 0; u < nr; ++u)
                if (t + u * 16 < n) {
                    const double x = Ws[(size_t)cc * ns + t + u * 16];
                    s2 = fma(x, x, s2);
                }
        s2 = group_sum<16>(s2);
        const double sig = sqrt(s2), inv = sig > 0.0 ? 1.0 / sig : 0.0;
        if (cc < n) {
            if (t == 0) lam[cc] = sig - s;
            for (int u = 0; u < nr; ++u)
                if (t + u * 16 < n) U[(size_t)cc * n + t + u * 16] = Ws[(size_t)cc * ns + t + u * 16] * inv;
        }
    }
}

// ---- 128 < n <= 288: the same one-sided Jacobi, blocked over workgroups -----------------------------------------------------
// The matrix no longer fits one CU's LDS (256 x 257 doubles = 514 KB).  Its columns are cut into blocks of SB_BW = 32; a workgroup
// takes a PAIR of blocks (64 columns x n rows <= 148 KB of LDS), runs one full sweep of the resident-column ordering over those 64
// columns (se_sweep, rows zero padded to whole 16-lane chunks) and writes them back; the block pairs of an outer round (round-robin
// tournament over the blocks: every two blocks meet once per outer sweep) are disjoint, so one launch does n_mat x blocks/2 of them
// side by side, and the launch boundary is the global synchronisation.  49 matrices of 256 x 256 (config 5): 196 workgroups per
// launch, 7 launches per outer sweep.  HBM traffic per launch: every matrix once in, once out.
#define SB_BW 32
#define SB_MAX_N 288
#define SB_MAX_OUTER 30

__global__ void __launch_bounds__(1024) k_sym_eig_shift(const double* __restrict__ A_all, double* __restrict__ W_all, double* __restrict__ shift,
                                                        int n) {
    __shared__ double s_red[16];
    const double* A = A_all + (size_t)blockIdx.x * n * n;
    double* W = W_all + (size_t)blockIdx.x * n * n;
    const int tid = threadIdx.x, nthreads = blockDim.x;
    double f2 = 0.0;
    for (int e = tid; e < n * n; e += nthreads) f2 = fma(A[e], A[e], f2);
    for (int o = 32; o > 0; o >>= 1) f2 += __shfl_xor(f2, o, 64);
    if ((tid & 63) == 0) s_red[tid >> 6] = f2;
    __syncthreads();
    double s = 0.0;
    for (int wv = 0; wv < (nthreads >> 6); ++wv) s += s_red[wv];
    s = sqrt(s);
    if (!(s > 0.0)) s = 1.0;
    if (tid == 0) shift[blockIdx.x] = s;
    for (int e = tid; e < n * n; e += nthreads) {
        const int cc = e / n, r = e - cc * n;
        W[e] = A[e] + (cc == r ? s : 0.0);                          // column cc of the symmetric matrix = its row cc
    }
}

// one workgroup per (matrix, block pair of this outer round); W (n_mat, n columns, n rows); 2 SB_BW groups of 16 lanes
template <int NR>
__global__ void __launch_bounds__(SB_BW * 16) k_sym_eig_block(double* __restrict__ W_all, int n, const int2* __restrict__ pairs, int n_pairs,
                                                              const int* __restrict__ tab, int nrd, int sched_ps, int* __restrict__ flags) {
    HIP_DYNAMIC_SHARED(double, Ws)
    constexpr int ns = NR * 16 + 1;
    const int mat = blockIdx.x / n_pairs;
    const int2 pr = pairs[blockIdx.x - mat * n_pairs];
    double* W = W_all + (size_t)mat * n * n;
    const int tid = threadIdx.x, group = tid >> 4, t = tid & 15;
    // columns of the two blocks -> LDS (a block beyond the matrix, or the columns past n of the last one: zero columns, which no
    // rotation touches -- the Gram element with a zero column is 0)
    for (int lc = group; lc < 2 * SB_BW; lc += SB_BW) {
        const int gc = (lc < SB_BW ? pr.x : pr.y) * SB_BW + (lc & (SB_BW - 1));
        const bool have = gc < n && (lc < SB_BW ? pr.x : pr.y) >= 0;
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            const int r = t + u * 16;
            Ws[(size_t)lc * ns + r] = (have && r < n) ? W[(size_t)gc * n + r] : 0.0;
        }
    }
    __syncthreads();
    bool big = false;
    se_sweep<NR>(Ws, ns, t, group, tab, nrd, sched_ps, true, big);
    if (big && t == 0) atomicAdd(flags + mat, 1);
    for (int lc = group; lc < 2 * SB_BW; lc += SB_BW) {
        const int gc = (lc < SB_BW ? pr.x : pr.y) * SB_BW + (lc & (SB_BW - 1));
        if (gc < n && (lc < SB_BW ? pr.x : pr.y) >= 0) {
#pragma unroll
            for (int u = 0; u < NR; ++u) {
                const int r = t + u * 16;
                if (r < n) W[(size_t)gc * n + r] = Ws[(size_t)lc * ns + r];
            }
        }
    }
}

// eigenvector i = W_i / |W_i|, eigenvalue |W_i| - s; one workgroup per matrix, 16 lanes per column
__global__ void __launch_bounds__(1024) k_sym_eig_finish(const double* __restrict__ W_all, const double* __restrict__ shift,
                                                         double* __restrict__ U_all, double* __restrict__ lam_all, int n) {
    const double* W = W_all + (size_t)blockIdx.x * n * n;
    double* U = U_all + (size_t)blockIdx.x * n * n;
    const double s = shift[blockIdx.x];
    const int ngroups = blockDim.x >> 4, group = threadIdx.x >> 4, t = threadIdx.x & 15;
    for (int cc0 = 0; cc0 < n; cc0 += ngroups) {                   // uniform trip count: DPP sums need the whole group
        const int cc = cc0 + group;
        double s2 = 0.0;
        if (cc < n)
            for (int r = t; r < n; r += 16) s2 = fma(W[(size_t)cc * n + r], W[(size_t)cc * n + r], s2);
        s2 = group_sum<16>(s2);
        const double sig = sqrt(s2), inv = sig > 0.0 ? 1.0 / sig : 0.0;
        if (cc < n) {
            if (t == 0) lam_all[(size_t)blockIdx.x * n + cc] = sig - s;
            for (int r = t; r < n; r += 16) U[(size_t)cc * n + r] = W[(size_t)cc * n + r] * inv;
        }
    }
}

template <int NR>
static void launch_sym_eig_block(mtip_ctx* c, double* dW, int n, const int2* d_pairs, int n_pairs, int n_mat, int* d_flags) {
    const size_t lds = (size_t)2 * SB_BW * (NR * 16 + 1) * sizeof(double);
    hipLaunchKernelGGL((k_sym_eig_block<NR>), dim3((unsigned)(n_mat * n_pairs)), dim3(SB_BW * 16), lds, c->stream, dW, n, d_pairs, n_pairs,
                       (const int*)(c->js.d_tab) + c->js.off[2 * SB_BW], c->js.nrd[2 * SB_BW], c->js.ps, d_flags);
}

// n in (128, 288]: blocked solve; dA, dU, dl device buffers as in mtip_op_symmetric_eig.  Returns the outer sweeps done (< 0: error).
static int sym_eig_blocked(mtip_ctx* c, int n, int n_mat, const double* dA, double* dU, double* dl) {
    const int nb = (n + SB_BW - 1) / SB_BW, nbe = nb + (nb & 1);                 // blocks, padded to an even count (-1 = empty block)
    const int n_pairs = nbe / 2, n_rounds = nbe - 1;
    std::vector<int2> pairs;
    for (int r = 0; r < n_rounds; ++r) {                                          // circle method: block nbe-1 stays, the others rotate
        pairs.push_back(make_int2(nbe - 1 < nb ? nbe - 1 : -1, r));
        for (int k = 1; k < n_pairs; ++k) pairs.push_back(make_int2((r + k) % (nbe - 1), (r - k + nbe - 1) % (nbe - 1)));
    }
    {   // every two blocks meet exactly once per outer sweep
        std::vector<char> met((size_t)nbe * nbe, 0);
        for (size_t i = 0; i < pairs.size(); ++i) {
            const int x = pairs[i].x < 0 ? nbe - 1 : pairs[i].x, y = pairs[i].y;
            if (x == y || met[(size_t)x * nbe + y]) return -1;
            met[(size_t)x * nbe + y] = met[(size_t)y * nbe + x] = 1;
        }
        if ((int)pairs.size() != n_rounds * n_pairs) return -1;
    }
    for (auto& pr : pairs)                                                        // the kept (first) block in .x must exist
        if (pr.x < 0) std::swap(pr.x, pr.y);
    DevBuf<int2> d_pairs;
    DevBuf<int> d_flags;
    DevBuf<double> dW, d_shift;
    if (d_pairs.alloc(pairs.size()) != hipSuccess || d_flags.alloc((size_t)n_mat) != hipSuccess ||
        dW.alloc((size_t)n_mat * n * n) != hipSuccess || d_shift.alloc((size_t)n_mat) != hipSuccess)
        return -2;
    if (mtip_copy(c, d_pairs, pairs.data(), pairs.size() * sizeof(int2), hipMemcpyHostToDevice) != hipSuccess) return -3;
    hipLaunchKernelGGL(k_sym_eig_shift, dim3((unsigned)n_mat), dim3(1024), 0, c->stream, dA, dW, d_shift, n);
    const int nr = (n + 15) / 16;
    std::vector<int> flags(n_mat);
    int rc = 0, outer = 0;
    for (; outer < SB_MAX_OUTER; ++outer) {
        (void)hipMemsetAsync(d_flags, 0, (size_t)n_mat * sizeof(int), c->stream);
        for (int r = 0; r < n_rounds; ++r) {
            const int2* pp = d_pairs + (size_t)r * n_pairs;
            if (nr <= 10) launch_sym_eig_block<10>(c, dW, n, pp, n_pairs, n_mat, d_flags);
            else if (nr <= 12) launch_sym_eig_block<12>(c, dW, n, pp, n_pairs, n_mat, d_flags);
            else if (nr <= 14) launch_sym_eig_block<14>(c, dW, n, pp, n_pairs, n_mat, d_flags);
            else if (nr <= 16) launch_sym_eig_block<16>(c, dW, n, pp, n_pairs, n_mat, d_flags);
            else launch_sym_eig_block<18>(c, dW, n, pp, n_pairs, n_mat, d_flags);
        }
        if (mtip_copy(c, flags.data(), d_flags, (size_t)n_mat * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) {
            rc = -3;
            break;
        }
        bool any = false;
        for (int f : flags) any = any || f != 0;
        if (!any) {
            ++outer;
            break;
        }
    }
    if (rc == 0) {
        hipLaunchKernelGGL(k_sym_eig_finish, dim3((unsigned)n_mat), dim3(1024), 0, c->stream, (const double*)dW, (const double*)d_shift, dU, dl, n);
        rc = outer;
    }
    (void)hipStreamSynchronize(c->stream);                                        // the work arrays go when this returns
    return rc;
}

// eigvals (n_mat, n) unsorted, eigvecs (n_mat, n, n): eigenvector i of matrix k in eigvecs[k][i][:]
extern "C" int mtip_op_symmetric_eig(mtip_ctx* c, int n, int n_mat, const double* A, double* eigvals, double* eigvecs) {
    if (!c) return MTIP_EINVAL;
    if (n < 1 || n > SB_MAX_N || n_mat < 1 || !A || !eigvals || !eigvecs) {
        c->err = "symmetric_eig: n must be in [1, 288], n_mat >= 1, buffers not null";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    if (n >= 2 && build_jacobi_schedule(c, n > SE_MAX_N ? 2 * SB_BW : n) != MTIP_OK) {
        c->err = "symmetric_eig: pairing schedule";
        return MTIP_ENOMEM;
    }
    DevBuf<double> dA, dU, dl;
    const size_t nn = (size_t)n_mat * n * n;
    if (dA.alloc(nn) != hipSuccess || dU.alloc(nn) != hipSuccess || dl.alloc((size_t)n_mat * n) != hipSuccess) {
        c->err = "symmetric_eig: out of device memory";
        return MTIP_ENOMEM;
    }
    int rc = MTIP_OK;
    hipError_t e = mtip_copy(c, dA, A, nn * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && n > SE_MAX_N) {
        ProfScope ps(c, "sym_eig");
        const int outer = sym_eig_blocked(c, n, n_mat, dA, dU, dl);
        if (outer < 0) {
            c->err = "symmetric_eig: blocked solve failed (device memory or block schedule)";
            rc = MTIP_EHIP;
        } else if (c->d_sweeps != nullptr) {
            (void)mtip_copy(c, c->d_sweeps, &outer, sizeof(int), hipMemcpyHostToDevice);
        }
    } else if (e == hipSuccess) {
        // all pairs of a round in one workgroup: floor(n / 2) groups of 16 lanes (the schedule's group count for n columns)
        const int groups = std::max(n / 2, 1);
        const int threads = std::min(1024, std::max(64, (groups * 16 + 63) / 64 * 64));
        const size_t lds = ((size_t)n * (n | 1) + 128) * sizeof(double);
        ProfScope ps(c, "sym_eig");
        hipLaunchKernelGGL(k_sym_eig, dim3((unsigned)n_mat), dim3((unsigned)threads), lds, c->stream, (const double*)dA, dU, dl, n,
                           (const int*)c->js.d_tab, (const int*)c->js.d_off, (const int*)c->js.d_rounds, c->js.ps,
                           n_mat <= c->B * (c->L + 1) ? c->d_sweeps : (int*)nullptr);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && rc == MTIP_OK) e = mtip_copy(c, eigvals, dl, (size_t)n_mat * n * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = mtip_copy(c, eigvecs, dU, nn * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        c->err = std::string("symmetric_eig: ") + hipGetErrorString(e);
        rc = MTIP_EHIP;
    }
    return rc;
}

// ---- cross-correlation -> B_l -----------------------------------------------------------------------------------------------
// The part of `extract` in front of the eigen-decompositions above: cross-correlation C(q1, q2, Delta) -> degree-2 invariants
//   xframe/projects/fxs/projectLibrary/fxs_invariant_tools.py:578-645   ccd_to_deg2_invariant_3d_back_substitution
//                                                             60-74     ccd_associated_legendre_matrices_single_l
//                                                             813-839   ccd_to_deg2_invariant_2d
//                                                             235-289   modify_cross_correlation (subtract_average_intensity,
//                                                                       pi_periodicity, q1q2_symmetric; unmasked data)
//   xframe/library/mathLibrary.py:484-490                               circularHarmonicTransform_real_forward (rfft / n)
// One kernel.  A workgroup owns CX_TP pairs (q1, q2 .. q2 + CX_TP - 1): their rows are one contiguous piece of C; each of its waves
// owns CX_PW of them.  The rows are read once, in chunks of CX_DC folded samples that sit in the registers of the wave (sample
// c0 + lane in lane `lane`, the next chunk loading while this one is summed); lane mi accumulates the harmonic m = mi * stride of the
// CX_PW pairs, reading the samples lane by lane (v_readlane: no LDS traffic); the triangular system  C_m = sum_l B_l c_l^m  is then
// solved inside the wave from the highest order down (the value of lane li goes to all lanes, lanes below it subtract); B_l leaves
// through LDS so that consecutive lanes write consecutive q2.  Nothing of the size of C is written.
//
// Folding (the sum is a table contraction, n_Delta is arbitrary):
//   * stride 2 and even n_Delta: the samples Delta and Delta + n/2 share the twiddle of every even m:  y[d] = x[d] + x[d + n/2],
//     n' = n / 2, m' = m / 2; otherwise y = x, n' = n, m' = m
//   * d and n' - d share the cosine and differ in the sign of the sine:  E[d] = y[d] + y[n'-d], O[d] = y[d] - y[n'-d] for
//     0 < d < n'/2, E = y, O = 0 at d = 0 and d = n'/2
//   C_m = (1/n) (sum_d E[d] cos(2 pi m' d / n') - i sum_d O[d] sin(2 pi m' d / n')),  d = 0 .. floor(n'/2)
// The twiddles come from a table of n' entries made on the host in extended precision, indexed by (m' d) mod n' (kept by
// addition); it sits in LDS up to CX_TW_LDS entries and in global memory (L2) beyond.
//
// More than 64 harmonics (k_cc_deg2<HM>, HM = 1, 2, 3 slots per lane): lane j owns the harmonic indices j, j + 64, j + 128, each with
// its own sums, twiddle index and 1 / c_l^l; one v_readlane of a sample feeds all HM slots.  Order index li lives in slot li >> 6,
// lane li & 63.  The back-substitution walks the slots from the highest down (the slot is wave-uniform and unrolled at compile time:
// no register is indexed dynamically); when order li is solved every lane of the slots below and the lanes below li & 63 of its own
// slot subtract, reading the Legendre row at m = slot * 64 + lane (consecutive lanes, consecutive addresses).  HM = 1 is the kernel
// as it was before the slots; mtip_op_cc_to_deg2 launches only that one, mtip_op_cc_to_deg2_wide picks HM from the number of orders.

#define CX_WAVES 4
#define CX_PW 4                        // pairs per wave (register block)
#define CX_TP (CX_WAVES * CX_PW)       // pairs per workgroup
#define CX_DC 64                       // folded samples per register chunk: one per lane
#define CX_TW_LDS 1024                 // twiddle entries held in LDS
#define CX_MAX_M 64                    // harmonics per pair and slot: one lane each
#define CX_MAX_HM 3                    // slots per lane of the widest instantiation
#define CX_WIDE_MAX_ORDER 128          // mtip_op_cc_to_deg2_wide: the limit of its inverse mtip_op_deg2_to_cc
#define CX_WIDE_MAX_M (CX_WIDE_MAX_ORDER + 1)
#define CX_MAX_NQ 4096
#define CX_MAX_ND 4096

struct CcArgs {
    const double* cc;                  // (nq, nq, nd)
    const double* avg;                 // (nq) average intensity (MTIP_CC_SUBTRACT_AVERAGE)
    const uint8_t* bad;                // (nd) angles zeroed by MTIP_CC_PI_PERIODICITY
    const double* leg;                 // (nq, ntri) P_l^m(cos theta_q), l = li stride, m = mi stride, at li (li + 1) / 2 + mi
    const double2* tw;                 // (np) (cos, sin)(2 pi k / np)
    double2* out;                      // (n_out, nq, nq)
    int nq, nd, np, half, nfold, stride, mstep, n_m, n_out, backsub, flags, ntri;
    double inv_n;
};

// one sample after subtract_average_intensity and pi_periodicity (fxs_invariant_tools.py:245-247, 264-269)
__device__ __forceinline__ double cx_val(const CcArgs& a, int q1, int q2, int d) {
    const double* row = a.cc + ((size_t)q1 * a.nq + q2) * a.nd;
    const double sub = (a.flags & MTIP_CC_SUBTRACT_AVERAGE) ? a.avg[q1] * a.avg[q2] : 0.0;
    double v = row[d] - sub;
    if (a.flags & MTIP_CC_PI_PERIODICITY) {
        const int h = a.nd >> 1, d2 = d >= h ? d - h : d + h;          // the copy rolled by n / 2
        const double w = row[d2] - sub;
        v = (a.bad[d] ? 0.0 : v) + (a.bad[d2] ? 0.0 : w);
    }
    return v;
}
// ... after q1q2_symmetric (271-279): the mean with C(q2, q1, -Delta), index 0 kept
__device__ __forceinline__ double cx_sample(const CcArgs& a, int q1, int q2, int d) {
    double v = cx_val(a, q1, q2, d);
    if (a.flags & MTIP_CC_Q1Q2_SYMMETRIC) v = (cx_val(a, q2, q1, d == 0 ? 0 : a.nd - d) + v) / 2;
    return v;
}
__device__ __forceinline__ double cx_y(const CcArgs& a, int q1, int q2, int d) {
    double v = cx_sample(a, q1, q2, d);
    if (a.half) v += cx_sample(a, q1, q2, d + a.np);
    return v;
}

// the (E, O) pair of folded sample d of one pair of shells (zeros beyond the folded range or the last shell)
__device__ __forceinline__ void cx_load(const CcArgs& a, int q1, int q2, int d, double& E, double& O) {
    E = O = 0.0;
    if (d < a.nfold && q2 < a.nq) {
        const double y = cx_y(a, q1, q2, d);
        if (d == 0 || 2 * d == a.np) {
            E = y;
        } else {
            const double z = cx_y(a, q1, q2, a.np - d);
            E = y + z;
            O = y - z;
        }
    }
}
// how many samples of y the entry E[d] holds
__device__ __forceinline__ double cx_weight(const CcArgs& a, int d) { return d >= a.nfold ? 0.0 : (d == 0 || 2 * d == a.np) ? 1.0 : 2.0; }
// the value lane `src` (wave-uniform) holds, for every lane
__device__ __forceinline__ double cx_lane(double v, int src) {
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    const int lo = __builtin_amdgcn_readlane((int)__double_as_longlong(v), src);
    return __hiloint2double(hi, lo);
}

template <int HM>
__global__ void __launch_bounds__(CX_WAVES * 64) k_cc_deg2(CcArgs a) {
    HIP_DYNAMIC_SHARED(double2, s_buf)                 // HM * CX_MAX_M * CX_TP: B of (order index, pair) on its way out
    __shared__ double2 s_tw[CX_TW_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q1 = blockIdx.y, q2base = blockIdx.x * CX_TP, q2w = q2base + wave * CX_PW;
    const bool tw_lds = a.np <= CX_TW_LDS;
    if (tw_lds)
        for (int k = tid; k < a.np; k += CX_WAVES * 64) s_tw[k] = a.tw[k];
    __syncthreads();
    int mp[HM], k[HM];                                 // m' of this lane's slots, and (m' d) mod n'
#pragma unroll
    for (int s = 0; s < HM; ++s) {
        const int mi = s * CX_MAX_M + lane;
        mp[s] = mi < a.n_m ? mi * a.mstep : 0;
        k[s] = 0;
    }
    // A chunk of 64 folded samples lives in the registers of the wave, sample c0 + lane in lane `lane`; the sums read it lane by lane.
    double E[CX_PW], O[CX_PW], En[CX_PW], On[CX_PW], re[HM][CX_PW], im[HM][CX_PW], shift[CX_PW];
#pragma unroll
    for (int p = 0; p < CX_PW; ++p) cx_load(a, q1, q2w + p, lane, E[p], O[p]);
    // A constant taken off the samples leaves every harmonic m != 0 unchanged (the twiddles of a full period sum to zero) and m = 0
    // gets it back below.  With the mean of the first chunk as that constant the sums no longer carry the large angle-independent
    // part of a cross-correlation through their rounding: the weak high harmonics keep their digits.
    {
        const double w0 = cx_weight(a, lane);
#pragma unroll
        for (int p = 0; p < CX_PW; ++p) {
            double se = E[p], sw = w0;
            for (int o = 32; o > 0; o >>= 1) {
                se += __shfl_xor(se, o);
                sw += __shfl_xor(sw, o);
            }
            shift[p] = se / sw;
#pragma unroll
            for (int s = 0; s < HM; ++s) re[s][p] = im[s][p] = 0.0;
        }
    }
    for (int c0 = 0; c0 < a.nfold; c0 += CX_DC) {
        const bool more = c0 + CX_DC < a.nfold;
        if (more)
#pragma unroll
            for (int p = 0; p < CX_PW; ++p) cx_load(a, q1, q2w + p, c0 + CX_DC + lane, En[p], On[p]);
        const double wd = cx_weight(a, c0 + lane);
#pragma unroll
        for (int p = 0; p < CX_PW; ++p) E[p] -= wd * shift[p];
        const int lim = min(CX_DC, a.nfold - c0);
        for (int dd = 0; dd < lim; ++dd) {
            double2 t[HM];
#pragma unroll
            for (int s = 0; s < HM; ++s) {
                t[s] = tw_lds ? s_tw[k[s]] : a.tw[k[s]];
                k[s] += mp[s];
                if (k[s] >= a.np) k[s] -= a.np;
            }
#pragma unroll
            for (int p = 0; p < CX_PW; ++p) {
                const double e = cx_lane(E[p], dd), o = cx_lane(O[p], dd);     // one broadcast feeds every slot
#pragma unroll
                for (int s = 0; s < HM; ++s) {
                    re[s][p] += e * t[s].x;
                    im[s][p] -= o * t[s].y;
                }
            }
        }
        if (more)
#pragma unroll
            for (int p = 0; p < CX_PW; ++p) {
                E[p] = En[p];
                O[p] = On[p];
            }
    }
#pragma unroll
    for (int p = 0; p < CX_PW; ++p) {
        if (lane == 0) re[0][p] += shift[p] * (double)a.np;                     // m = 0: slot 0, lane 0
#pragma unroll
        for (int s = 0; s < HM; ++s) {
            re[s][p] *= a.inv_n;
            im[s][p] *= a.inv_n;
        }
    }
    if (a.backsub) {
        // B_l = C_l / c_l^l,  C_m -= B_l c_l^m (m < l),  c_l^m = P_l^m(q1) P_l^m(q2) / (2 l + 1)   (fxs_invariant_tools.py:629-632)
        // lane li prepares 1 / c_l^l of its own orders once: one division per pair instead of one per pair and order
        const double* leg1 = a.leg + (size_t)q1 * a.ntri;
        double rdiag[HM][CX_PW];
#pragma unroll
        for (int s = 0; s < HM; ++s) {
            const int mi = s * CX_MAX_M + lane;
            const int dg = mi * (mi + 1) / 2 + mi;
            const bool act = mi < a.n_m;
            const double p1 = act ? leg1[dg] : 1.0;
#pragma unroll
            for (int p = 0; p < CX_PW; ++p) {
                const int q2 = min(q2w + p, a.nq - 1);
                const double p2 = act ? a.leg[(size_t)q2 * a.ntri + dg] : 1.0;
                rdiag[s][p] = 1.0 / (p1 * p2 / (double)(2 * mi * a.stride + 1));
            }
        }
        // the slots from the highest down; `so` is a compile-time constant in every copy of the body
#pragma unroll
        for (int so = HM - 1; so >= 0; --so) {
            for (int li = min(a.n_m, (so + 1) * CX_MAX_M) - 1; li >= so * CX_MAX_M; --li) {
                const int ll = li - so * CX_MAX_M;                                  // the owner's lane (wave-uniform)
                const int tri = li * (li + 1) / 2;
                const double inv_norm = 1.0 / (double)(2 * li * a.stride + 1);
                // every lane of the slots below subtracts; in the owner's slot the lanes below ll
                double p1[HM];
#pragma unroll
                for (int s = 0; s < HM; ++s)
                    if (s <= so) p1[s] = (s < so || lane < ll) ? leg1[tri + s * CX_MAX_M + lane] * inv_norm : 0.0;
#pragma unroll
                for (int p = 0; p < CX_PW; ++p) {
                    const int q2 = min(q2w + p, a.nq - 1);
                    const double r = cx_lane(rdiag[so][p], ll);
                    const double br = cx_lane(re[so][p], ll) * r, bi = cx_lane(im[so][p], ll) * r;
#pragma unroll
                    for (int s = 0; s < HM; ++s)
                        if (s <= so) {
                            const bool act = s < so || lane < ll;
                            const double cm = act ? p1[s] * a.leg[(size_t)q2 * a.ntri + tri + s * CX_MAX_M + lane] : 0.0;
                            if (act) {
                                re[s][p] -= br * cm;
                                im[s][p] -= bi * cm;
                            } else if (s == so && lane == ll) {
                                re[s][p] = br;
                                im[s][p] = bi;
                            }
                        }
                }
            }
        }
    }
#pragma unroll
    for (int s = 0; s < HM; ++s) {
        const int mi = s * CX_MAX_M + lane;
        if (mi < a.n_m)
#pragma unroll
            for (int p = 0; p < CX_PW; ++p) s_buf[mi * CX_TP + wave * CX_PW + p] = make_double2(re[s][p], im[s][p]);
    }
    __syncthreads();
    // every order 0 .. n_out - 1 is written: the ones that were not extracted as zeros (fxs_invariant_tools.py:417-419)
    for (int idx = tid; idx < a.n_out * CX_TP; idx += CX_WAVES * 64) {
        const int l = idx / CX_TP, p = idx - l * CX_TP, q2 = q2base + p;
        if (q2 >= a.nq) continue;
        const int li = l / a.stride;
        const bool have = (l - li * a.stride) == 0 && li < a.n_m;
        a.out[((size_t)l * a.nq + q1) * a.nq + q2] = have ? s_buf[li * CX_TP + p] : make_double2(0.0, 0.0);
    }
}

template <int HM>
static void launch_cc_deg2(mtip_ctx* c, const CcArgs& a) {
    const size_t lds = (size_t)HM * CX_MAX_M * CX_TP * sizeof(double2);
    hipLaunchKernelGGL((k_cc_deg2<HM>), dim3((unsigned)div_up(a.nq, CX_TP), (unsigned)a.nq), dim3(CX_WAVES * 64), lds, c->stream, a);
}

// the body of both entry points: `wide` only moves the limit on the extracted orders (and names the entry in the messages)
static int cc_to_deg2_entry(mtip_ctx* c, bool wide, int n_q, int n_delta, int max_order, int order_stride, int dimensions, uint32_t flags,
                            const double* cc, const double* average_intensity, const uint8_t* bad_angles, const double* legendre,
                            mtip_cdouble* b_out) {
    if (!c) return MTIP_EINVAL;
    char msg[400];
    const std::string name = wide ? "cc_to_deg2_wide: " : "cc_to_deg2: ";
    const int s = order_stride;
    const int n_m = (s == 1 || s == 2) && max_order >= 0 ? max_order / s + 1 : 0;
    if (!cc || !b_out || (dimensions != 2 && dimensions != 3) || (s != 1 && s != 2) || max_order < 0 || n_q < 1 || n_delta < 2 ||
        (flags & ~(uint32_t)(MTIP_CC_SUBTRACT_AVERAGE | MTIP_CC_PI_PERIODICITY | MTIP_CC_Q1Q2_SYMMETRIC))) {
        c->err = name + "null buffer, dimensions not 2 or 3, order stride not 1 or 2, or unknown flag";
        return MTIP_EINVAL;
    }
    if (!wide && (n_q > CX_MAX_NQ || n_delta > CX_MAX_ND || n_m > CX_MAX_M || n_delta < 2 * max_order)) {
        snprintf(msg, sizeof msg,
                 "cc_to_deg2: built for n_q <= %d, 2 max_order <= n_delta <= %d and at most %d extracted orders (max_order <= %d at "
                 "stride 2, <= %d at stride 1); got n_q = %d, n_delta = %d, max_order = %d, stride = %d",
                 CX_MAX_NQ, CX_MAX_ND, CX_MAX_M, 2 * CX_MAX_M - 1, CX_MAX_M - 1, n_q, n_delta, max_order, s);
        c->err = msg;
        return MTIP_EINVAL;
    }
    if (wide && (n_q > CX_MAX_NQ || n_delta > CX_MAX_ND || max_order > CX_WIDE_MAX_ORDER || n_m > CX_WIDE_MAX_M || n_delta < 2 * max_order)) {
        snprintf(msg, sizeof msg,
                 "cc_to_deg2_wide: built for n_q <= %d, 2 max_order <= n_delta <= %d, max_order <= %d and at most %d extracted orders; "
                 "got n_q = %d, n_delta = %d, max_order = %d, stride = %d (%d extracted orders)",
                 CX_MAX_NQ, CX_MAX_ND, CX_WIDE_MAX_ORDER, CX_WIDE_MAX_M, n_q, n_delta, max_order, s, n_m);
        c->err = msg;
        return MTIP_EINVAL;
    }
    if (((flags & MTIP_CC_SUBTRACT_AVERAGE) && !average_intensity) || ((flags & MTIP_CC_PI_PERIODICITY) && !bad_angles) ||
        (dimensions == 3 && !legendre)) {
        c->err = name + "a table the flags / dimensions ask for is null (average_intensity, bad_angles, legendre)";
        return MTIP_EINVAL;
    }
    if ((flags & MTIP_CC_PI_PERIODICITY) && (n_delta & 1)) {
        c->err = name + "pi_periodicity needs an even number of angles (fxs_invariant_tools.py:265)";
        return MTIP_EINVAL;
    }
    (void)hipSetDevice(c->device);
    CcArgs a{};
    a.nq = n_q;
    a.nd = n_delta;
    a.half = (s == 2 && (n_delta & 1) == 0) ? 1 : 0;
    a.np = a.half ? n_delta / 2 : n_delta;
    a.mstep = a.half ? 1 : s;
    a.nfold = a.np / 2 + 1;
    a.stride = s;
    a.n_m = n_m;
    a.n_out = max_order + 1;
    a.backsub = dimensions == 3;
    a.flags = (int)flags;
    a.ntri = n_m * (n_m + 1) / 2;
    a.inv_n = 1.0 / (double)n_delta;
    std::vector<double2> tw((size_t)a.np);
    for (int k = 0; k < a.np; ++k) {
        const long double ang = 2.0L * 3.14159265358979323846264338327950288L * (long double)k / (long double)a.np;
        tw[k] = make_double2((double)cosl(ang), (double)sinl(ang));
    }
    const size_t nqq = (size_t)n_q * n_q;
    DevView v_cc(c, cc, nqq * n_delta * sizeof(double), true, false);
    DevView v_avg(c, (flags & MTIP_CC_SUBTRACT_AVERAGE) ? average_intensity : nullptr, (size_t)n_q * sizeof(double), true, false);
    DevView v_bad(c, (flags & MTIP_CC_PI_PERIODICITY) ? bad_angles : nullptr, (size_t)n_delta, true, false);
    DevView v_leg(c, a.backsub ? legendre : nullptr, (size_t)n_q * a.ntri * sizeof(double), true, false);
    DevView v_tw(c, tw.data(), tw.size() * sizeof(double2), true, false);
    DevView v_out(c, b_out, nqq * a.n_out * sizeof(double2), false, true);
    for (DevView* v : {&v_cc, &v_avg, &v_bad, &v_leg, &v_tw, &v_out})
        if (v->err != hipSuccess) {
            c->err = name + hipGetErrorString(v->err);
            return v->err == hipErrorOutOfMemory ? MTIP_ENOMEM : MTIP_EHIP;
        }
    a.cc = (const double*)v_cc.dev;
    a.avg = (const double*)v_avg.dev;
    a.bad = (const uint8_t*)v_bad.dev;
    a.leg = (const double*)v_leg.dev;
    a.tw = (const double2*)v_tw.dev;
    a.out = (double2*)v_out.dev;
    {
        ProfScope ps(c, "cc_deg2");
        static_assert(CX_WIDE_MAX_M <= CX_MAX_HM * CX_MAX_M, "the widest instantiation holds every order of the wide entry");
        if (n_m <= CX_MAX_M) launch_cc_deg2<1>(c, a);                 // (the checks above leave the narrow entry nothing else)
        else if (n_m <= 2 * CX_MAX_M) launch_cc_deg2<2>(c, a);
        else launch_cc_deg2<3>(c, a);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = v_out.finish();
    if (e != hipSuccess) {
        c->err = name + hipGetErrorString(e);
        return MTIP_EHIP;
    }
    return MTIP_OK;
}

extern "C" int mtip_op_cc_to_deg2(mtip_ctx* c, int n_q, int n_delta, int max_order, int order_stride, int dimensions, uint32_t flags,
                                  const double* cc, const double* average_intensity, const uint8_t* bad_angles, const double* legendre,
                                  mtip_cdouble* b_out) {
    return cc_to_deg2_entry(c, false, n_q, n_delta, max_order, order_stride, dimensions, flags, cc, average_intensity, bad_angles, legendre,
                            b_out);
}

extern "C" int mtip_op_cc_to_deg2_wide(mtip_ctx* c, int n_q, int n_delta, int max_order, int order_stride, int dimensions, uint32_t flags,
                                       const double* cc, const double* average_intensity, const uint8_t* bad_angles,
                                       const double* legendre, mtip_cdouble* b_out) {
    return cc_to_deg2_entry(c, true, n_q, n_delta, max_order, order_stride, dimensions, flags, cc, average_intensity, bad_angles, legendre,
                            b_out);
}

// ---- masked cross-correlation data: modify_cross_correlation with a mask, and B_l by least squares ----------------------
#include "k_extract_lsq.h"
// ---- the rest of modify_cross_correlation: low pass in q, harmonic filter, binned mean -------------------------------------
#include "k_extract_cond.h"
// ---- the other back-substitution modes (psd, qqsym, memory_hungry) on harmonics that are on the device; nearest PSD matrix ----
#include "k_extract_psd.h"
// ---- patterns -> cross-correlation (the stage in front of the one above) -----------------------------------------------
#include "k_correlate.h"
// ---- B_l -> cross-correlation (simulate_ccd: the inverse of mtip_op_cc_to_deg2) ------------------------------------------
#include "k_simulate.h"
// ---- detector frames -> patterns (the stage in front of that one) ------------------------------------------------------
#include "k_resample.h"

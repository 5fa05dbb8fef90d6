// Radial Hankel step (rows a1-a3 of SURVEY section 8): the reference's only live GPU kernel,
// OpenCL `apply_weights` (xframe/projects/fxs/projectLibrary/hankel_transforms.py:702-731 midpoint,
// 671-700 trapz):   out[k, lm] = c_l * sum_p W[l(lm)][p][k] * in[p (+1), lm]
// W is the *real* raw weight array (hankel_transforms.py:399-410); the complex prefactor
// c_l = (-/+ i)^l * scale of assemble_weights_mid (426-452) is applied once in the epilogue, so the
// contraction is real-matrix x complex-panel.
#include "mtip_internal.h"
#include <vector>

void launch_hankel_mfma(mtip_ctx* c, const double2* in, double2* out, int inverse);

void launch_hankel(mtip_ctx* c, const double2* in, double2* out, int inverse) {
    ProfScope ps(c, "hankel");
    launch_hankel_mfma(c, in, out, inverse);
}

// out = a - b for shells > 0, out = a for shell 0   (ft_stab add-back folded into coefficient space,
// misk.py:326-329 add_above_zero_index; used by the fused step only)
__global__ void __launch_bounds__(256) k_coeff_diff(const double2* __restrict__ a, const double2* __restrict__ b,
                                                    double2* __restrict__ out, int N, int nlm, long long total) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int q = (int)((idx / nlm) % N);
    double2 v = a[idx];
    if (q > 0) v = csub(v, b[idx]);
    out[idx] = v;
}

void launch_coeff_diff(mtip_ctx* c, const double2* a, const double2* b, double2* out) {
    const long long total = (long long)c->B * c->N * c->nlm;
    hipLaunchKernelGGL(k_coeff_diff, dim3((unsigned)div_up(total, 256)), dim3(256), 0, c->stream, a, b, out, c->N,
                       c->nlm, total);
}

// ------------------------------------------------------------------------------------------------------
// Per order l the contraction is a real GEMM  D[k][col] = sum_p W_l[p][k] * X[p][col] with the (batch, m, re/im) axes
// flattened into columns (B (4l+2) of them).  v_mfma_f64_16x16x4_f64: lane j holds A[i = j&15][kk = j>>4] = W_l[p0+kk][k0+i],
// B[kk = j>>4][col = j&15] = X[p0+kk][col0+col], D reg r = D[(j>>4) + 4r][j&15].  The (-/+ i)^l * scale prefactor is applied in
// the epilogue: multiplying by +-i swaps the re/im columns, i.e. neighbouring lanes (shfl_xor 1).
// ---- one-pass workgroup tile -----------------------------------------------------------------------------------
// A 512-thread workgroup owns 16 CT columns x 128 output shells of one order; wave w owns row tile w.  Per stage of
// ST input shells (32; 64 at CT = 1) a wave requests its own 16 columns of W_l, ST / 4 doubles per lane, from the
// fragment-ordered copy d_Wf (below) in 16-byte loads and keeps them in registers: W never enters LDS.  The
// workgroup requests the stage's panel ST x 16 CT as 16-byte (re, im) pairs (SUB: the subtracted panel too; the
// difference is taken at the deposit), deposits it once into one of two LDS buffers and meets at ONE barrier; behind
// it the stage's k-steps run A from registers and B fragments from LDS, with no global access, no wait for one and no
// barrier, while the next stage's operands are in flight in a second register set.  Every accumulator sees the k-steps
// in ascending p, four shells each, and in SUB wave 0's masked row-0 MFMA directly behind the main one of its k-step:
// the MFMA sequence of the chunked kernel this replaced, the same bits.  The LDS row stride is 16 doubles mod 32, so
// the two input shells a half-wave reads land on disjoint banks.  (One stage of 128 shells with everything requested at
// entry, and operands two stages ahead, were measured and are slower at CT >= 2: profiles/hankel_onepass_timing.txt.)
#define HT_CT_MAX 5                 // 16-column MFMA tiles per workgroup: template parameter CT in {1, 2, 3, 5}
#define HT_ROWS 128                 // output shells per workgroup (8 row tiles = 8 waves)
#define HT_THREADS 512
#define HT_PPAD 64                  // d_Wf pads the input shells of an order to a multiple of this: a whole number of stages

struct HankelTile32 { int l, cflat0; };

// d_Wf: W in MFMA-fragment order.  Block (l, row block rb, wave w, k-step pair j) is 64 lanes x 2 doubles: lane (i = lane & 15,
// kk = lane >> 4) finds W_l[8j + kk][k] and W_l[8j + 4 + kk][k], k = 128 rb + 16 w + i, next to each other -- its A values
// of k-steps 2j and 2j + 1; a wave load is 1 KiB contiguous.  Entries with p >= Np or k >= N are zero, so the kernel needs no
// predicate on this side; j runs to hankel_wf_pairs(Np), a whole number of stages.
static inline int hankel_wf_pairs(int Np) { return div_up(Np, HT_PPAD) * (HT_PPAD / 8); }

size_t hankel_wf_doubles(const mtip_ctx* c) {
    return (size_t)(c->L + 1) * div_up(c->N, HT_ROWS) * (HT_ROWS / 16) * hankel_wf_pairs(c->Np) * 128;
}

int upload_hankel_fragments(mtip_ctx* c, const double* w_raw) {
    const int N = c->N, Np = c->Np, nrb = div_up(N, HT_ROWS), nj = hankel_wf_pairs(Np);
    std::vector<double> wf(hankel_wf_doubles(c), 0.0);
    size_t o = 0;
    for (int l = 0; l <= c->L; ++l)
        for (int rb = 0; rb < nrb; ++rb)
            for (int w = 0; w < HT_ROWS / 16; ++w)
                for (int j = 0; j < nj; ++j)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int h = 0; h < 2; ++h, ++o) {
                            const int p = 8 * j + 4 * h + (lane >> 4), k = HT_ROWS * rb + 16 * w + (lane & 15);
                            if (p < Np && k < N) wf[o] = w_raw[((size_t)l * Np + p) * N + k];
                        }
    return mtip_copy(c, c->d_Wf, wf.data(), wf.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess ? MTIP_OK : MTIP_EHIP;
}

// SUB: out = H(in - in_sub) on output shells > 0 and H(in) on shell 0 in ONE pass (the ft_stab step needs
// IFT(F') - IFT(F) above shell 0 and IFT(F') on it, misk.py:326-329): the staged panel is the difference, and the wave
// that owns output row 0 adds H(in_sub)[0] back with a second MFMA chain whose A fragment is W_l masked to row 0.
template <int HT_CT, bool SUB>
__global__ void __launch_bounds__(HT_THREADS) k_hankel_tile(const double* __restrict__ in, double* __restrict__ out,
                                                            const double* __restrict__ Wf,
                                                            const HankelTile32* __restrict__ tiles, int N, int Np, int L,
                                                            int B, int poffs, double scale, int sign,
                                                            const double* __restrict__ in_sub, const uint8_t* __restrict__ sub_mask) {
    // input shells per stage: 32, and 64 at CT = 1, where 32 rows of 8 pairs would leave half the waves without a deposit
    // (and so without the wait for their own W fragments in front of the barrier)
    constexpr int HT_ST = HT_CT == 1 ? 64 : 32;
    constexpr int HT_COLS = 16 * HT_CT;
    constexpr int HT_XS = (HT_CT & 1) ? HT_COLS : HT_COLS + 16; // 16, 48, 48, 80: 16 mod 32
    constexpr int HT_PW = HT_COLS / 2;                          // (re, im) pairs per panel row
    constexpr int HT_RP = HT_THREADS / HT_PW;                   // panel rows per pass of the workgroup
    constexpr int HT_NX = (HT_ST + HT_RP - 1) / HT_RP;          // passes = pairs per thread and stage
    constexpr int HT_NA = HT_ST / 8;                            // A pairs per lane and stage
    static_assert(HT_PPAD % HT_ST == 0 && HT_ST % 8 == 0 && HT_XS % 32 == 16, "stage and stride rules");
    __shared__ double Xs[2][HT_ST][HT_XS] __attribute__((aligned(16)));
    __shared__ double Ss[SUB ? 2 : 1][SUB ? HT_ST : 1][HT_XS] __attribute__((aligned(16)));   // the subtracted panel itself (row-0 correction)
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const HankelTile32 tinfo = tiles[blockIdx.x];
    const int l = tinfo.l;
    const int k_base = blockIdx.y * HT_ROWS;                      // row block (Nq > 128)
    const int ncl = 4 * l + 2;                                    // doubles per (batch, shell) of this order
    const int nlm2 = 2 * (L + 1) * (L + 1);                       // doubles per (batch, shell)
    const double2* Wa = reinterpret_cast<const double2*>(Wf) +
                        (((size_t)l * gridDim.y + blockIdx.y) * (HT_ROWS / 16) + wave) * ((Np + HT_PPAD - 1) / HT_PPAD * (HT_PPAD / 8)) * 64 + lane;
    // ---- staging role: pair tid % HT_PW of the panel rows tid / HT_PW + j HT_RP.  2 l^2, the column within the order and
    //      cflat0 are even, so a pair is 16-byte aligned and never straddles two restarts
    const int prow = tid / HT_PW, pc = tid - prow * HT_PW;
    const int cflat_x = tinfo.cflat0 + 2 * pc;
    const bool xok = prow < HT_RP && cflat_x < B * ncl;
    const int xb = xok ? cflat_x / ncl : 0;
    const size_t xoff = (size_t)xb * N * nlm2 + 2 * (size_t)l * l + (xok ? cflat_x - xb * ncl : 0);
    const bool xsub = SUB && (sub_mask == nullptr || sub_mask[xb] != 0);   // this column's restart takes the subtraction (per-restart ft_stab; all without a mask)
    // ---- MFMA roles: wave = row tile, all HT_CT column tiles
    const int li = lane & 15, kk = lane >> 4;
    v4f64 acc[HT_CT];
#pragma unroll
    for (int t = 0; t < HT_CT; ++t) acc[t] = v4f64{0.0, 0.0, 0.0, 0.0};
    // two register sets: the operands of the NEXT stage are in flight while this one is multiplied; the difference is taken at
    // the deposit, so that nothing waits for a load before the stage that needs it
    double2 a0[HT_NA], a1[HT_NA], rx0[HT_NX], rx1[HT_NX], rs0[SUB ? HT_NX : 1], rs1[SUB ? HT_NX : 1];
    auto request = [&](int p0, double2 (&a)[HT_NA], double2 (&rx)[HT_NX], double2 (&rs)[SUB ? HT_NX : 1]) {
        const double2* wa = Wa + (size_t)(p0 / 8) * 64;
#pragma unroll
        for (int j = 0; j < HT_NA; ++j) a[j] = wa[(size_t)j * 64];
#pragma unroll
        for (int j = 0; j < HT_NX; ++j) {
            const int row = prow + j * HT_RP;
            const bool ok = xok && ((j + 1) * HT_RP <= HT_ST || row < HT_ST) && p0 + row < Np;
            const size_t o = xoff + (size_t)(p0 + row + poffs) * nlm2;
            rx[j] = ok ? *reinterpret_cast<const double2*>(in + o) : make_double2(0.0, 0.0);
            if (SUB) rs[j] = (ok && xsub) ? *reinterpret_cast<const double2*>(in_sub + o) : make_double2(0.0, 0.0);
        }
    };
    auto deposit = [&](int buf, const double2 (&rx)[HT_NX], const double2 (&rs)[SUB ? HT_NX : 1]) {
#pragma unroll
        for (int j = 0; j < HT_NX; ++j) {
            const int row = prow + j * HT_RP;
            if ((HT_RP * HT_PW == HT_THREADS || prow < HT_RP) && ((j + 1) * HT_RP <= HT_ST || row < HT_ST)) {
                double2 d = rx[j];
                if (SUB) {
                    d.x -= rs[j].x;
                    d.y -= rs[j].y;
                    *reinterpret_cast<double2*>(&Ss[buf][row][2 * pc]) = rs[j];
                }
                *reinterpret_cast<double2*>(&Xs[buf][row][2 * pc]) = d;
            }
        }
    };
    auto multiply = [&](int buf, const double2 (&a)[HT_NA]) {
#pragma unroll
        for (int s = 0; s < HT_ST / 4; ++s) {                      // k-steps past the last shell multiply zeros
            const double af = (s & 1) ? a[s >> 1].y : a[s >> 1].x;
#pragma unroll
            for (int t = 0; t < HT_CT; ++t) {
                const double bf = Xs[buf][4 * s + kk][16 * t + li];
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf, acc[t], 0, 0, 0);
            }
            if (SUB && wave == 0 && k_base == 0) {               // wave-uniform: output row 0 lives here
                const double a0m = li == 0 ? af : 0.0;
#pragma unroll
                for (int t = 0; t < HT_CT; ++t) {
                    const double sf = Ss[buf][4 * s + kk][16 * t + li];
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0m, sf, acc[t], 0, 0, 0);
                }
            }
        }
    };
    // a buffer is written again two stages after it was read: every wave has passed the barrier of the stage in between
    request(0, a0, rx0, rs0);
#pragma unroll 1
    for (int p0 = 0; p0 < Np; p0 += 2 * HT_ST) {
        deposit(0, rx0, rs0);
        if (p0 + HT_ST < Np) request(p0 + HT_ST, a1, rx1, rs1);
        __syncthreads();
        multiply(0, a0);
        if (p0 + HT_ST >= Np) break;
        deposit(1, rx1, rs1);
        if (p0 + 2 * HT_ST < Np) request(p0 + 2 * HT_ST, a0, rx0, rs0);
        __syncthreads();
        multiply(1, a1);
    }
    // epilogue: * scale * (-/+ i)^l, store
    int r = l & 3;
    if (sign < 0) r = (4 - r) & 3;
    const bool is_im = (li & 1) != 0;
#pragma unroll
    for (int t = 0; t < HT_CT; ++t) {
        const int cflat = tinfo.cflat0 + 16 * t + li;
        const bool col_ok = cflat < B * ncl;
        const int b = col_ok ? cflat / ncl : 0;
        const int within = col_ok ? cflat - b * ncl : 0;
        const size_t col_off = (size_t)b * N * nlm2 + 2 * (size_t)l * l + within;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            double v = acc[t][j] * scale;
            const double partner = __shfl_xor(v, 1, 64);
            double o;
            if (r == 0) o = v;
            else if (r == 2) o = -v;
            else if (r == 1) o = is_im ? partner : -partner;       // * i : (a+bi) i = -b + a i
            else o = is_im ? -partner : partner;                   // * -i: (a+bi)(-i) = b - a i
            const int k = k_base + wave * 16 + kk + 4 * j;
            if (col_ok && k < N) out[col_off + (size_t)k * nlm2] = o;
        }
    }
}

bool hankel_has_difference(const mtip_ctx* c) { return c->d_htiles32 != nullptr; }

int hankel_row_blocks(const mtip_ctx* c) { return div_up(c->N, HT_ROWS); }

// out = H(in - in_sub) above output shell 0, H(in) on it (in_sub == nullptr: plain transform)
void launch_hankel_mfma_sub(mtip_ctx* c, const double2* in, const double2* in_sub, double2* out, int inverse, const uint8_t* sub_mask) {
    const dim3 grid((unsigned)c->n_htiles32, (unsigned)hankel_row_blocks(c));
#define HT_LAUNCH(CT, SUBF)                                                                                                  \
    hipLaunchKernelGGL((k_hankel_tile<CT, SUBF>), grid, dim3(HT_THREADS), 0, c->stream, reinterpret_cast<const double*>(in), \
                       reinterpret_cast<double*>(out), (const double*)c->d_Wf, (const HankelTile32*)c->d_htiles32, c->N,      \
                       c->Np, c->L, c->B, c->cfg.hankel_trapz ? 1 : 0, inverse ? c->inv_scale : c->fwd_scale,                \
                       inverse ? +1 : -1, reinterpret_cast<const double*>(in_sub), sub_mask)
    if (in_sub != nullptr) {
        switch (c->htile_ct) {
            case 1: HT_LAUNCH(1, true); break;
            case 2: HT_LAUNCH(2, true); break;
            case 3: HT_LAUNCH(3, true); break;
            default: HT_LAUNCH(5, true); break;
        }
    } else {
        switch (c->htile_ct) {
            case 1: HT_LAUNCH(1, false); break;
            case 2: HT_LAUNCH(2, false); break;
            case 3: HT_LAUNCH(3, false); break;
            default: HT_LAUNCH(5, false); break;
        }
    }
#undef HT_LAUNCH
}

void launch_hankel_mfma(mtip_ctx* c, const double2* in, double2* out, int inverse) {
    launch_hankel_mfma_sub(c, in, nullptr, out, inverse);
}

int build_hankel_tiles(mtip_ctx* c) {
    // widest workgroup tile that still gives (about) one workgroup per CU: W_l is re-read once per tile
    std::vector<HankelTile32> t32;
    const int cts[4] = {5, 3, 2, 1};
    for (int ci = 0; ci < 4; ++ci) {
        t32.clear();
        c->htile_ct = cts[ci];
        for (int l = c->L; l >= 0; --l) {                   // heavy orders first
            const int ncols = c->B * (4 * l + 2);
            for (int c0 = 0; c0 < ncols; c0 += 16 * cts[ci]) t32.push_back(HankelTile32{l, c0});
        }
        if (c->htile_force > 0 ? cts[ci] == c->htile_force : (int)t32.size() * hankel_row_blocks(c) * 5 >= c->n_cu * 4) break;
    }
    {
        // XCD-aware order: consecutive workgroup ids go round-robin to the 8 XCDs (one L2 each), so the tiles of one order
        // are dealt to ONE residue class mod 8 and W_l is fetched into one L2 instead of up to eight.  Orders go to the
        // least loaded XCD, heaviest first; a queue that runs dry takes tiles from the tail of the longest one.
        const int X = 8;
        std::vector<std::vector<HankelTile32>> q(X);
        size_t i0 = 0;
        while (i0 < t32.size()) {
            size_t i1 = i0;
            while (i1 < t32.size() && t32[i1].l == t32[i0].l) ++i1;
            int best = 0;
            for (int x = 1; x < X; ++x)
                if (q[x].size() < q[best].size()) best = x;
            q[best].insert(q[best].end(), t32.begin() + i0, t32.begin() + i1);
            i0 = i1;
        }
        std::vector<size_t> head(X, 0);
        std::vector<HankelTile32> order;
        while (order.size() < t32.size())
            for (int x = 0; x < X && order.size() < t32.size(); ++x) {
                if (head[x] < q[x].size()) { order.push_back(q[x][head[x]++]); continue; }
                int longest = 0;
                for (int y = 1; y < X; ++y)
                    if (q[y].size() - head[y] > q[longest].size() - head[longest]) longest = y;
                order.push_back(q[longest].back());
                q[longest].pop_back();
            }
        t32.swap(order);
    }
    c->n_htiles32 = (int)t32.size();
    if (c->d_htiles32.alloc(t32.size()) != hipSuccess) return MTIP_ENOMEM;
    (void)mtip_copy(c, c->d_htiles32, t32.data(), t32.size() * sizeof(HankelTile32), hipMemcpyHostToDevice);
    return MTIP_OK;
}

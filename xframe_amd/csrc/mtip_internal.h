// Internal declarations of libmtip_hip.so (gfx950 only).  Public ABI: include/mtip_hip.h
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include "../../include/mtip_hip.h"

// Scheduling fence for values in vector registers: the (empty) statement reads and writes its operands, so loads that
// produce them stay above it and are waited for here, not where the compiler would fold them to.
#ifndef MTIP_PIN_VGPRS4
#define MTIP_PIN_VGPRS4(a, b, c, d) asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
#endif
// all LDS operations of this wave have completed (diagnostic timers: separates the store drain from the barrier wait)
#ifndef MTIP_WAIT_LDS
#define MTIP_WAIT_LDS() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#endif


// LDS data handed from some lanes of a wave to others of the SAME wave: LDS operations of one wave complete in the order they were
// issued, so only the compiler has to keep them in order (the emulation runs the lanes one after the other and needs a real
// rendezvous: tests/emul defines its own)
#ifndef MTIP_WAVE_LDS_SYNC
#define MTIP_WAVE_LDS_SYNC()                        \
    do {                                            \
        asm volatile("" ::: "memory");              \
        __builtin_amdgcn_wave_barrier();            \
        asm volatile("" ::: "memory");              \
    } while (0)
#endif

typedef double v4f64 __attribute__((vector_size(32)));   // accumulator of v_mfma_f64_16x16x4_f64

// ---- complex helpers (complex128 = double2, interleaved like numpy) ----------------------------
__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 cmulc(double2 a, double2 b) {   // a * conj(b)
    return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cscale(double2 a, double s) { return make_double2(a.x * s, a.y * s); }
__device__ __forceinline__ double cabs2(double2 a) { return a.x * a.x + a.y * a.y; }
__device__ __forceinline__ int isqrt_lm(int lm) {   // l of index l(l+1)+m, exact integer version
    int l = (int)sqrt((double)lm);
    while (l * l > lm) --l;
    while ((l + 1) * (l + 1) <= lm) ++l;
    return l;
}
// multiply by (-i)^l (sign=-1) or (+i)^l (sign=+1)
__device__ __forceinline__ double2 cmul_ipow(double2 a, int l, int sign) {
    int r = l & 3;
    if (sign < 0) r = (4 - r) & 3;              // (-i)^l = i^(-l)
    switch (r) {
        case 0: return a;
        case 1: return make_double2(-a.y, a.x);   // * i
        case 2: return make_double2(-a.x, -a.y);
        default: return make_double2(a.y, -a.x);  // * -i
    }
}

#define MTIP_CHAIN_DBG_SLOTS 18
#define MTIP_POLAR_DBG_SLOTS MTIP_POLAR_TIMING_SLOTS   // int64 per (restart, order) of the k_rproj timers (include/mtip_hip.h)
// ---- per-restart slot table (device ints), see DESIGN.md "state" ---------------------------------
// SL_HIST: the pair the reference's stale local `hist` ends with (reconstruct.py:859, 913): the input pair of the most
// recent step, or the latest pair when no step has run in the current sub-loop call; read by SW_center (893) and by the
// fixed amplitudes of the *_non_FXS variants (901)
enum { SL_CUR = 0, SL_OUT = 1, SL_BEST = 2, SL_SUP = 3, SL_SUP_BEST = 4, SL_ENFORCE = 5, SL_HAS_ERR = 6, SL_HIST = 7, SL_N = 8 };

// the metrics a main error can list (mtip_set_main_error_ex), and what k_finish_step is handed to read them
enum { MAIN_ITEM_REAL_L2 = 0, MAIN_ITEM_DEG2 = 1, MAIN_ITEM_RECIPROCAL_L2 = 2, MAIN_ITEM_II = 3, MAIN_ITEM_CCD = 4, MAIN_ITEM_DEG2_RANKED = 5 };
#define MAIN_ITEMS_MAX 8
struct MainItems {
    int n, ranked_col;              // n < 0: a listed metric has no value yet; ranked_col: column of the deg2 row (item 5)
    int items[MAIN_ITEMS_MAX];
    const double* rl2;              // (B) row of d_rl2_hist
    const double* im;               // (B, 2 + Nq) row of d_im_hist: II (B) | ccd (B) | fqc
    const double* deg2;             // (B, L+1) row of d_deg2_hist
};

// real-space constraint flags (mtip_set_real_constraints)
enum { RC_SUPPORT = 1, RC_VALUE_LO = 2, RC_VALUE_HI = 4, RC_LIMIT_IMAG = 8 };

struct RealParams {
    uint32_t flags, hio_flags;
    double lo, hi, imag_thr;
};

// One grid point of the real-space stage: P = real_projection(w) (support, value bounds, imaginary-part limit;
// fxs_Projections.py:72-130), new density = P (error reduction) or prev - beta (w - P) where a constraint counted
// by the HIO mask was violated (fxs_IO_methods.py:40-64).  Returns the new density, P through P_out.
__device__ __forceinline__ double2 real_update_point(const RealParams& rp, int method, double beta, double2 w, double2 pv,
                                                     bool S, double2& P_out) {
    double2 P = w;
    uint32_t viol = 0;
    if (rp.flags & RC_SUPPORT) {
        if (!S) {
            P = make_double2(0.0, 0.0);
            viol |= RC_SUPPORT;
        }
    }
    if ((rp.flags & RC_VALUE_LO) && (rp.flags & RC_VALUE_HI)) {
        if (P.x < rp.lo) { P.x = rp.lo; viol |= RC_VALUE_LO; }
        if (P.x > rp.hi) { P.x = rp.hi; viol |= RC_VALUE_LO; }
    } else if (rp.flags & RC_VALUE_LO) {
        if (P.x < rp.lo) { P.x = rp.lo; viol |= RC_VALUE_LO; }
    } else if (rp.flags & RC_VALUE_HI) {
        if (P.x > rp.hi) { P.x = rp.hi; viol |= RC_VALUE_LO; }
    }
    if (rp.flags & RC_LIMIT_IMAG) {
        if (fabs(P.y) >= rp.imag_thr) { P.y = 0.0; viol |= RC_LIMIT_IMAG; }
    }
    double2 nw = P;
    if (method == MTIP_HIO || method == MTIP_HIO_NON_FXS) {
        uint32_t hm = rp.hio_flags;
        if (hm & (RC_VALUE_LO | RC_VALUE_HI)) hm |= RC_VALUE_LO;      // both bounds share one mask
        if (viol & hm) {
            nw.x = pv.x - beta * (w.x - P.x);
            nw.y = pv.y - beta * (w.y - P.y);
        }
    }
    P_out = P;
    return nw;
}

// The same point update with the settings decoded once (uniform booleans) and no short-circuit logic: in the chained kernel the
// flag tests of real_update_point became scalar branches around every grid point (157 branches in the kernel, eight points per
// lane and row group).  Bit-identical results: the same comparisons and the same arithmetic in the same order.
struct RealFlags {
    bool support, lo, hi, both, imag, hio, h_support, h_value, h_imag;
};
__device__ __forceinline__ RealFlags real_flags(const RealParams& rp, int method) {
    RealFlags f;
    f.support = (rp.flags & RC_SUPPORT) != 0;
    f.lo = (rp.flags & RC_VALUE_LO) != 0;
    f.hi = (rp.flags & RC_VALUE_HI) != 0;
    f.both = f.lo && f.hi;
    f.imag = (rp.flags & RC_LIMIT_IMAG) != 0;
    f.hio = method == MTIP_HIO || method == MTIP_HIO_NON_FXS;
    uint32_t hm = rp.hio_flags;
    if (hm & (RC_VALUE_LO | RC_VALUE_HI)) hm |= RC_VALUE_LO;          // both bounds share one mask
    f.h_support = (hm & RC_SUPPORT) != 0;
    f.h_value = (hm & RC_VALUE_LO) != 0;
    f.h_imag = (hm & RC_LIMIT_IMAG) != 0;
    return f;
}
__device__ __forceinline__ double2 real_update_point_flat(const RealParams& rp, const RealFlags& f, double beta, double2 w, double2 pv,
                                                          bool S, double2& P_out) {
    double2 P = w;
    const bool v_s = f.support & !S;
    P.x = v_s ? 0.0 : P.x;
    P.y = v_s ? 0.0 : P.y;
    // (with both bounds the upper one is tested on the value the lower one may have replaced, as in real_update_point)
    const bool c_lo = f.lo & (P.x < rp.lo);
    P.x = c_lo ? rp.lo : P.x;
    const bool c_hi = f.hi & (P.x > rp.hi);
    P.x = c_hi ? rp.hi : P.x;
    const bool v_i = f.imag & (fabs(P.y) >= rp.imag_thr);
    P.y = v_i ? 0.0 : P.y;
    const bool take = f.hio & ((f.h_support & v_s) | (f.h_value & (c_lo | c_hi)) | (f.h_imag & v_i));
    double2 nw;
    nw.x = take ? pv.x - beta * (w.x - P.x) : P.x;
    nw.y = take ? pv.y - beta * (w.y - P.y) : P.y;
    P_out = P;
    return nw;
}

// real-space stage fused into the last inverse SHT of a step (EPI_REAL_UPDATE): w = iSHT value (+ previous density on
// shells > 0: the ft_stab add-back), densities and support read / written through the slot table, error partial
// sums per shell
struct RealEpi {
    const double2* prev = nullptr;     // slot base (3,B,G)
    double2* out = nullptr;            // slot base (3,B,G)
    const uint8_t* sup = nullptr;      // support slot base (3,B,G)
    const uint8_t* S0 = nullptr;       // (G)
    const double* wr = nullptr;        // (Nq) radial error weights
    const double* wt = nullptr;        // (nt) polar error weights
    double* partial = nullptr;         // (B, Nq, 2)
    RealParams rp{};
    int method = 0, err_use_mask = 0, add_prev = 0;
    const uint8_t* add_mask = nullptr; // (B) per-restart ft_stab (the add-back only where set), or nullptr: every restart
    double beta = 0.0;
};

// epilogues of the inverse SHT (grid-side fused elementwise stages)
enum { EPI_STORE = 0, EPI_MODULUS = 1, EPI_SCALE_SHELL = 2, EPI_MODULUS_FIXED = 3, EPI_REAL_UPDATE = 4 };

struct ProfEntry { double ms = 0; long long n = 0; };

// Which SHT kernels run, decided once per context from the geometry (plan_sht, k_sht.hip).  Tier k is taken where the cap
// MTIP_SHT_TIER (default 5) is >= k and the geometry fits it:  5 the chained inverse -> forward kernel (k_sht_chain), 4 the wide
// inverse with the real-space epilogue, 3 the wide inverse (k_sht_inv_wide) and the paired forward (k_sht_fwd_pair), 2 the
// pass-wise register-FFT kernels (k_sht_fwd_reg / k_sht_inv_reg: both directions must fit), 1 the LDS Stockham kernels
// (k_sht_fused.hip), 0 the generic FFT + Legendre kernels (k_sht.hip).  Tiers 1-5 are sized for L <= MTIP_LOOP_L_MAX; a context
// beyond it takes the two-stage kernels of k_sht_big.h (cap >= 1, even n_theta <= SHT_BIG_NT_MAX) or the generic ones, without chain or real_update.
#define MTIP_LOOP_L_MAX 63              // band limit of the tuned SHT tiers and, unless cfg.reserved has MTIP_CFG_LOOP_BIG_L, of the projection and the phasing loop
#define SHT_BIG_NT_MAX 256              // k_sht_big.h: the synthesis holds the <= 128 theta pairs of a chunk in eight row tiles
enum { SHT_FWD_GENERIC = 0, SHT_FWD_LDS, SHT_FWD_REG, SHT_FWD_PAIR, SHT_FWD_BIG };
enum { SHT_INV_GENERIC = 0, SHT_INV_LDS, SHT_INV_REG, SHT_INV_WIDE, SHT_INV_BIG };
// k_sht_chain instantiations: run-time tables (THG = 0), table rows in registers (THG = 16, n_phi = 128), and the latter with
// L = 32 at compile time and the chunk layout of the Legendre sums
enum { SHT_CHAIN_OFF = 0, SHT_CHAIN_RT, SHT_CHAIN_REGTAB, SHT_CHAIN_L32 };
struct ShtPlan {
    int fwd = SHT_FWD_GENERIC;
    int fwd_rp = 0;                    // rows per pass (register / LDS kernels)
    int fwd_th = 0;                    // theta pairs per pass (paired kernel)
    int fwd_maxi = 0;                  // (l, m) pairs per thread: the kernel's MAXI
    size_t fwd_lds = 0;
    int inv = SHT_INV_GENERIC;
    int inv_rp = 0;                    // rows per FFT pass
    int inv_nsplit = 1;                // workgroups per shell (wide)
    int inv_jl = 0;                    // theta pairs per Legendre chunk (LDS kernel)
    size_t inv_lds = 0;
    bool real_update = false;          // the inverse takes EPI_REAL_UPDATE and coeff_sub (wide kernel, tier 4)
    int real_update_blocks = 0;        // error partial sums per restart that epilogue writes
    int chain = SHT_CHAIN_OFF;
    int chain_gsz = 0, chain_thg = 0, chain_maxi = 0;   // accumulation group size, theta pairs per group, MAXI
    size_t chain_lds = 0;
};

// ---- device memory ----------------------------------------------------------------------------------
// Move-only owner of one device allocation.  It converts to the raw pointer, so kernel arguments, pointer arithmetic and
// null tests read as they do with a plain pointer; what it does not allow is a second owner of the same block.
template <typename T>
struct DevBuf {
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            swap(o);
        }
        return *this;
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }
    // releases what it held; at least one element, so that an empty table still has an address.  Null on failure.
    hipError_t alloc(size_t count) {
        reset();
        const hipError_t e = hipMalloc((void**)&p_, std::max<size_t>(count, 1) * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
    void swap(DevBuf& o) noexcept { std::swap(p_, o.p_); }
    operator T*() const { return p_; }

private:
    T* p_ = nullptr;
};
static_assert(!std::is_copy_constructible_v<DevBuf<double>>);

// Pairing schedule of the one-sided Jacobi kernels (build_jacobi_schedule, k_proj.hip), shared by the projection and extract's
// eigensolver: it depends on a column count only and grows when a caller asks for more columns
struct JacobiSchedule {
    DevBuf<int> d_tab, d_off, d_rounds;               // entries, offset of every column count's table, rounds of a sweep per column count
    int kmax = 0, ps = 0;                             // column count it was built for, row length (pair-groups) of every table
    std::vector<int> nrd, off;                        // host copies of d_rounds and d_off
};
struct ProjSwitches {                                 // the projection's switches, read once (read_proj_switches, at mtip_create)
    bool fuse = true;                                 // MTIP_PROJ_FUSE=0: four separate projection products instead of the two fused pairs
    bool jac_resident = true;                         // MTIP_JAC_RESIDENT=0: round-robin ordering, both columns via LDS
    int jac_tg = 16;                                  // MTIP_JAC_TG=8|16: lanes per Jacobi column pair
    bool real = true;                                 // MTIP_PROJ_REAL=0: never take the real form of the projection (k_projr.hip)
    double polar_abs_tol = 0.0;                       // MTIP_POLAR_ABS_TOL: 0 = purely relative Jacobi criterion
    bool rp_corr = true;                              // MTIP_RP_CORR=0: k_rproj closes its sweeps with the classic confirming sweep
    double rp_early = 3e-2, rp_corr2_max = 1.5e-4;    // MTIP_RP_EARLY, MTIP_RP_CORR2_MAX: thresholds of the closing step (k_projr.hip)
};
struct RpGeom {                                       // threads and dynamic LDS of a k_rproj launch (plan_rproj, k_projr.hip)
    int tg = 16, threads = 256, acc = 0;              // lanes per column pair; 16 x 16 tiles a wave holds in the in-place products
    int tab_ints = 0, tab2_entries = 0;               // ints reserved for the raw pairing table, entries of its per-sweep translation
    bool big = false;                                 // some order has the tight layout (k_rproj<768, ...>)
    size_t lds = 0;
};

// How the reciprocal projection runs, decided once per set of V_l (plan_projection, k_proj.hip: on the first projection after
// invalidate_projection, which every mtip_set_projection_matrix calls).  A call with real_intensity takes the one real kernel
// (k_rproj) where `real_ok`: the switch `real`, every used V_l without imaginary part, every solved order square (k_l = 2l+1) with
// at most 111 columns, and a geometry `rg` within k_rproj's instantiations (768 threads, 160 KiB LDS, the tiles a wave can hold).
// Every other call takes the complex kernels: the polar factors in LDS (k_polar_jacobi_lds<jac_inst>) where X_l and V_r of the
// largest order fit a CU (`lds_path`), else in global memory, between the fused product pairs (`fuse`) or the four products.
// The plan owns the tables made from V_l, k_l, used and active; each route's are built when that route first runs.  `rg`,
// `use_sched` and `threads` depend on the pairing schedule's row length and round counts (c->js.ps, c->js.nrd), which grow when
// build_jacobi_schedule is asked for more columns: it clears `planned` and the next projection decides again (tables and V_r stay).
enum { PROJ_JAC_5x16 = 0, PROJ_JAC_9x8, PROJ_JAC_16x8 };   // k_polar_jacobi_lds<MAXR, TG, ...>
struct ProjPlan {
    bool planned = false, real_ok = false;
    RpGeom rg;
    int kmax = 1, nmax = 1, kmax_used = 1;            // largest k_l and 2l+1 over the active orders, largest k_l the apply product touches
    bool fuse = false, lds_path = false, use_sched = false;
    int tg = 16, pad = 0, threads = 64, jac_inst = PROJ_JAC_5x16;
    size_t lds_use = 0, xw_lds = 0, ua_lds = 0;       // dynamic LDS of the polar-factor kernel, of k_proj_xw and of k_proj_ua
    DevBuf<int> d_jorder;                             // active orders, heaviest first (grid of the polar-factor kernel)
    DevBuf<int> d_pg_tiles[6];                        // (order, tile) lists of the projection GEMMs (4, 5: fused pairs)
    int n_jorder = 0, n_pg_tiles[6] = {0, 0, 0, 0, 0, 0}, rp_n_slots = 0, rp_slot_len = 0;
    DevBuf<double> d_rp_DV, d_rp_Vt;                  // q^2 V_l (N x k) and V_l^T (k x N), real, at voff[l]
    DevBuf<int> d_rp_slots;                           // (rp_n_slots, rp_slot_len) order | kind << 8 lists of the k_rproj workgroups
};
enum { VR_NONE = 0, VR_COMPLEX, VR_REAL };            // what d_Vr carries from the previous projection: a route warm-starts only from its own kind

struct HankelTile32;                                  // k_hankel.hip

struct mtip_ctx {
    mtip_cfg cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    int N = 0, L = 0, nt = 0, np = 0, B = 0, nlm = 0, nm = 0, Np = 0;
    size_t G = 0, C = 0;
    // tables
    DevBuf<double> d_cost, d_gw, d_P, d_r, d_q;
    DevBuf<int> d_poff;
    DevBuf<double2> d_AB;                          // (npairs + L + 1) three-term recurrence coefficients (a_lm, b_lm) in record order (k_sht_legendre.h)
    DevBuf<double> d_PT;                           // (nt/2, npairs) theta-major Legendre table (fused SHT)
    DevBuf<double> d_PTc;                          // (nt/2, 768) the same table in the chunk layout of k_sht_chain's Legendre sums
    DevBuf<int> d_lmc;                             // (768) l | m << 8 of slot u * 256 + t, -1: none
    DevBuf<double2> d_PTw;                         // (8, 8, 3, 64) d_PTc of the L = 32 plan (n_theta 64) by (wave, theta-pair couple, order u, lane): entry =
                                                   // theta pairs 16 g + 2 c, 2 c + 1 of slot u * 256 + t, wave = 4 g + t / 64, lane = t % 64; null elsewhere
    DevBuf<uint8_t> d_ftmask;                      // (B) per-restart ft_stab of the next runs (mtip_set_ft_stab_mask)
    bool ftmask_mixed = false;                        // the mask has both values: steps with ft_stab take it per restart
    hipEvent_t turn_ev = nullptr;                     // mtip_run_group_async: end of this context's latest transform block
    int chain_chunks = 0;                             // chunks (threads of an accumulation group with work) in that layout; 0: it does not fit 256
    DevBuf<int> d_lmtab;                           // (npairs) l | m << 8
    int npairs = 0;
    ShtPlan sht;                                      // SHT kernel choice (plan_sht, at mtip_set_angular_grid)
    DevBuf<double2> d_twN;                         // exp(-2 pi i j / n_phi), j < n_phi
    DevBuf<double2> d_tw;
    DevBuf<double> d_W;
    DevBuf<double> d_Wf;                              // d_W again in MFMA-fragment order, zero padded (k_hankel.hip): what k_hankel_tile reads
    int n_cu = 256;                                   // compute units of the device (persistent-grid sizing)
    JacobiSchedule js;                                // resident-column pairing schedule
    // non-default reciprocal metrics (k_metrics.hip): flags 1 II_error | 2 ccd_diff | 4 fqc_error, their constant tables, history rows
    uint32_t im_which = 0;
    DevBuf<uint8_t> d_im_zmask;
    DevBuf<double2> d_im_IIref, d_im_ccdref;
    DevBuf<double> d_rl2_wr, d_rl2_wt, d_rl2_part, d_rl2_hist;   // reciprocal l2_projection_diff (k_metrics.hip)
    DevBuf<double> d_im_fq;                         // (B, Nq, Nq) fqc values of a step (k_metric_fqc -> k_metric_fqc_fold)
    DevBuf<double2> d_im_part;                      // (B, IM_BLOCKS, 4) partial sums of II_error / ccd_diff
    DevBuf<double> d_im_qq, d_im_ccdT, d_im_P, d_im_refavg, d_im_refw, d_im_hist;
    double im_ccd_inv_norm = 0.0;
    int so_order = -1;                                // SO_freedom: order whose unknown [4][2] is made real after every projection (-1: off)
    DevBuf<long long> d_polar_dbg;                 // (B, L+1, MTIP_POLAR_DBG_SLOTS) phase / round timers of k_rproj, allocated by mtip_debug_polar_timing
    DevBuf<double2> d_c0n;                         // (B, C) SHT of the current density, written by the chained last kernel of a step
    DevBuf<long long> d_chain_dbg;                 // (3 kinds, B * Nq, MTIP_CHAIN_DBG_SLOTS) phase stamps of k_sht_chain, allocated by mtip_debug_chain_timing
    bool c0n_valid = false;                           // d_c0n holds SHT(rho[SL_CUR]) of every restart
    DevBuf<HankelTile32> d_htiles32;                       // workgroup tiles (order, first column) of k_hankel_tile
    int htile_force = 0;                              // env MTIP_HANKEL_CT=1|2|3|5: tile width of k_hankel_tile instead of the occupancy rule (A/B)
    int n_htiles32 = 0, htile_ct = 5;                 // 16-column MFMA tiles per workgroup
    double fwd_scale = 0, inv_scale = 0;
    bool have_angular = false, have_radial = false, have_weights = false, have_support = false, have_errw = false;
    // projection data
    ProjSwitches psw;
    ProjPlan pp;                                      // route, geometry and V_l tables of the projection (plan_projection)
    std::vector<int> kl, used, active, voff, xoff, uoff;     // host copies (active = used and V_l != 0)
    DevBuf<int> d_active;
    DevBuf<int> d_sweeps;                          // (B, L+1) Jacobi sweeps of the last projection (diagnostic)
    std::vector<char> v_real;                         // per order: V_l has no imaginary part
    std::vector<double2> h_V;                         // host copy of the concatenated V_l (tables of the real projection)
    int vr = VR_NONE;                                 // what d_Vr holds (VR_*)
    long long proj_calls = 0;                         // every 64th call starts cold: bounds the rounding drift of the carried V_r
    DevBuf<int> d_kl, d_used, d_voff, d_xoff, d_uoff;
    int vtot = 0, xtot = 0, utot = 0;                 // per-restart element counts
    DevBuf<double2> d_V;                           // concatenated V_l, (Nq, k_l) row-major each
    DevBuf<uint8_t> d_rmask;                       // (L+1, Nq)
    std::vector<char> have_V;
    double n_particles = 1.0;
    // deg2 metric
    int deg2_enable = 0;
    DevBuf<double2> d_Bref;                        // (L+1, Nq, Nq) masked reference B_l
    DevBuf<double> d_Bnorm;                        // (L+1)
    DevBuf<double> d_deg2_part;                    // (B, L+1, (Nq/16)^2) per-tile partial sums of the B_l metric
    bool deg2_simple = false;                         // env MTIP_DEG2_SIMPLE=1: one thread per B_l element instead of MFMA tiles
    bool bref_dirty = true;
    // real-space constraints and error metric
    RealParams rp{RC_SUPPORT | RC_VALUE_LO, RC_SUPPORT | RC_VALUE_LO, 0.0, 0.0, 0.0};
    DevBuf<uint8_t> d_S0, d_sup;        // (G), (3, B, G)
    DevBuf<uint16_t> d_mk;                         // (3, B, Nq, nt, R2) the same masks packed for k_sht_chain: bit n1 = support, bit 8 + n1 = S0 of point R2 n1 + n2 of the row
    DevBuf<double> d_err_wr, d_err_wt;
    int err_use_mask = 1;
    // state
    DevBuf<double2> d_rho, d_Fp;        // (3, B, G) each
    DevBuf<int> d_slot;                            // (B, SL_N)
    DevBuf<double> d_best_err, d_last_err;   // (B)
    DevBuf<double> d_op_err;                       // (B) error of the single-operator entry point (never the loop's)
    DevBuf<double> d_gq;                           // (Nq) shrink-wrap Gaussian G_sigma(q)
    DevBuf<double> d_err_hist;                     // (cap, B) real l2 metric per step
    DevBuf<double> d_main_hist;                    // (cap, B) main error per step when it is not the real metric (main_mode 1, 2)
    // mtip_set_main_error_ex: main_mode 0 = items [0], 1 = items [1] (the per-order vector), 2 = any other list of scalar items
    int main_mode = 0, main_type = 0;
    int main_n = 1, main_items[MAIN_ITEMS_MAX] = {0, 0, 0, 0, 0, 0, 0, 0}, main_ranked_col = 0;
    long long last_fxs_step = -1;                     // last FXS step of this reconstruction: the rows its reciprocal metrics were recorded in
    DevBuf<double> d_deg2_hist;                    // (cap, B, L+1)
    long long err_cap = 0, n_steps_done = 0;
    bool state_ready = false, fixed_valid = false;
    // work buffers
    DevBuf<double2> d_F, d_T1, d_T2;   // grids (B, G)
    DevBuf<double> d_fixed;                        // real grid (B, G)
    DevBuf<double2> d_g;                           // (B, Nq, nt, 2L+1)
    DevBuf<double2> d_c[6];   // coefficient arrays (B, C)
    DevBuf<double2> d_X, d_Vr, d_U;   // projection workspaces
    DevBuf<double> d_partial;                      // (B, nblk, 2) error partial sums
    int n_partial_blocks = 0;
    DevBuf<double> d_minmax;                       // (B, nblk, 2)
    DevBuf<double2> d_Bl;                          // (B, L+1, Nq, Nq) scratch (lazy)
    // rotational alignment (k_align.hip): Wigner table d^l_mn(beta_b), DFT twiddles, work arrays
    DevBuf<double> d_so3_d;
    DevBuf<double2> d_so3_tw, d_so3_T, d_so3_S, d_so3_P, d_so3_D;
    DevBuf<double> d_so3_C;
    int so3_bw = 0;
    // profiling
    int prof = 0;
    std::map<std::string, ProfEntry> prof_data;
    // asynchronous family timers: event pairs recorded on the ctx stream, resolved when the numbers are read
    std::vector<hipEvent_t> prof_events;
    std::vector<std::pair<const char*, int>> prof_pending;   // (family, index of the first event of the pair)
    int prof_next = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
};

// ---- launchers (defined next to their kernels) ------------------------------------------------------
// SHT: the kernels of c->sht; MTIP_OK, or MTIP_ESTATE (c->err set) for an epilogue / prologue the planned kernel does not have
void plan_sht(mtip_ctx* c);                          // after build_legendre_tables
// in_slot >= 0: grid is a (3,B,G) slot array read through slot[b][in_slot]
int launch_sht_forward(mtip_ctx* c, const double2* grid, double2* coeff, int prologue, int in_slot = -1);
struct InvEpilogue {
    int mode = EPI_STORE;
    const double2* F = nullptr;        // EPI_MODULUS*: reciprocal density to rescale
    const double* fixed = nullptr;     // EPI_MODULUS_FIXED
    const double* shell_scale = nullptr;   // EPI_SCALE_SHELL (Nq)
    const double2* coeff_sub = nullptr;    // coefficients to subtract on shells > 0 before the synthesis (ft_stab)
    RealEpi real;                          // EPI_REAL_UPDATE
    int out_slot = -1;                 // >= 0: grid is a (3,B,G) slot array written through slot[b][out_slot]
};
int launch_sht_inverse(mtip_ctx* c, const double2* coeff, double2* grid, const InvEpilogue& epi);
void build_legendre_tables(mtip_ctx* c, const double* cos_theta);
int sht_no_kernel(mtip_ctx* c, const char* what, int epi_mode);   // k_sht.hip: sets c->err, returns MTIP_ESTATE
void launch_sht_forward_fused(mtip_ctx* c, const double2* grid, double2* coeff, int prologue, int in_slot);
int launch_sht_inverse_fused(mtip_ctx* c, const double2* coeff, double2* grid, const InvEpilogue& epi);
void launch_sht_forward_reg(mtip_ctx* c, const double2* grid, double2* coeff, int prologue, int in_slot);
int launch_sht_inverse_reg(mtip_ctx* c, const double2* coeff, double2* grid, const InvEpilogue& epi);
// k_sht_chain.hip: grid = epilogue(iSHT(coeff)) and coeff_out = SHT(prologue(grid)) in one kernel (EPI_STORE with
// MTIP_PRE_NONE / MTIP_PRE_SQUARE, EPI_MODULUS, EPI_REAL_UPDATE without coeff_sub), where c->sht.chain is set
int launch_sht_chain(mtip_ctx* c, const double2* coeff, double2* grid, const InvEpilogue& epi, int prologue, double2* coeff_out);
// Hankel
void launch_hankel(mtip_ctx* c, const double2* in, double2* out, int inverse);
bool hankel_has_difference(const mtip_ctx* c);       // launch_hankel_mfma_sub is available (workgroup-tiled kernel)
void launch_hankel_mfma_sub(mtip_ctx* c, const double2* in, const double2* in_sub, double2* out, int inverse, const uint8_t* sub_mask = nullptr);
int build_jacobi_schedule(mtip_ctx* c, int kmax);    // k_proj.hip: resident-column pairing schedule, verified on the host
int jacobi_groups(int k);                            // pair-groups a round of that schedule keeps busy for k columns (<= js.ps: the table's row length)
int build_hankel_tiles(mtip_ctx* c);
size_t hankel_wf_doubles(const mtip_ctx* c);          // length of d_Wf
int upload_hankel_fragments(mtip_ctx* c, const double* w_raw);   // d_Wf from the host table of mtip_set_hankel_weights
int hankel_row_blocks(const mtip_ctx* c);            // row blocks (128 output shells each) of k_hankel_tile: the grid's y extent
int launch_invariant_metrics(mtip_ctx* c, const double2* Ilm, long long step);
int launch_reciprocal_l2_metric(mtip_ctx* c, const double2* F, const double2* Fp, long long step);
void launch_deg2(mtip_ctx* c, const double2* Ilm, double2* Bl);
void launch_coeff_diff(mtip_ctx* c, const double2* a, const double2* b, double2* out);
// reciprocal projection
// real_intensity: the caller guarantees I_{l,-m} = (-1)^m conj(I_{l,m}) (coefficients of a real grid, as in the phasing
// loop): with real V_l the projection then takes its real form (k_projr.hip)
int launch_project_coefficients(mtip_ctx* c, const double2* Ilm, double2* out, bool real_intensity = false);   // MTIP_OK or an error code (c->err set)
int require_projection_columns(mtip_ctx* c, const char* what);   // k_proj.hip: MTIP_ESTATE (c->err set) where an active order has more than 128 columns
void plan_projection(mtip_ctx* c);                    // k_proj.hip: decides c->pp where it is not planned
void plan_rproj(mtip_ctx* c);                         // k_projr.hip: real_ok and rg of c->pp
void invalidate_projection(mtip_ctx* c);              // k_proj.hip: V_l, k_l, used or active change: drops the plan, its tables and the carried V_r
int launch_rproj(mtip_ctx* c, double2* coef);         // in place
int launch_apply_unknowns(mtip_ctx* c, const double2* Ilm, double2* out);
void launch_deg2_metric(mtip_ctx* c, const double2* Ilm, double* out /*(B, L+1)*/);
// elementwise / reductions
// rho_p = IFT(F') (B,G); prev/out: slot arrays (3,B,G) when use_slots else plain (B,G); rho_rt may be null
void launch_real_update(mtip_ctx* c, const double2* rho_p, const double2* prev, const double2* rho_rt, double2* out,
                        int method, double beta, int use_slots);
// step_index >= 0: loop step (history, best tracking, slot rotation); < 0: only the error, written to c->d_op_err
void launch_finish_step(mtip_ctx* c, long long step_index, int nblk = 0);   // nblk partial sums per restart (0: grid blocks)
void launch_abs_to_fixed(mtip_ctx* c);
void launch_modulus_plain(mtip_ctx* c, const double2* F, const double2* Inew, double2* out);
void launch_modulus_fixed_slots(mtip_ctx* c, const double2* F);
void launch_copy_to_slot(mtip_ctx* c, const double2* src, double2* dst_slots, int which);
void launch_sw_clamp(mtip_ctx* c, const double2* conv, double* tmp_real);
void launch_sw_threshold(mtip_ctx* c, const double* tmp_real, double threshold, double error_limit);
void launch_pack_masks(mtip_ctx* c);                  // d_sup, d_S0 -> d_mk (all slots; after every writer of the two)
void launch_apply_matrix(mtip_ctx* c, const double* M, const double* x, double* y, int nr, int nc, int nv);

// ---- small utilities ---------------------------------------------------------------------------------
#define MTIP_HIP_CHECK(c, call)                                                              \
    do {                                                                                     \
        hipError_t e__ = (call);                                                             \
        if (e__ != hipSuccess) {                                                             \
            (c)->err = std::string(#call) + ": " + hipGetErrorString(e__);                   \
            return MTIP_EHIP;                                                                \
        }                                                                                    \
    } while (0)

void prof_flush(mtip_ctx* c);       // mtip_api.hip: synchronise the stream and fold the pending event pairs into prof_data

// hipEvent bracket of one kernel family launch.  Nothing waits here: the pair is resolved by prof_flush (called when
// the numbers are read, or when 4096 pairs are pending), so the brackets can stay on during a timed run.
struct ProfScope {
    mtip_ctx* c;
    const char* name;
    int idx = -1;
    ProfScope(mtip_ctx* c_, const char* n) : c(c_), name(n) {
        if (!c->prof) return;
        if (c->prof_next + 2 > 8192) prof_flush(c);
        while ((int)c->prof_events.size() < c->prof_next + 2) {
            hipEvent_t e;
            // no system-scope fence at the record: a default event releases to the host (cache write-back) every time it is
            // recorded -- eighteen of those made a bracketed step twice as long; the timestamps do not need it
            if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return;
            c->prof_events.push_back(e);
        }
        idx = c->prof_next;
        c->prof_next += 2;
        (void)hipEventRecord(c->prof_events[idx], c->stream);
    }
    ~ProfScope() {
        if (idx < 0) return;
        (void)hipEventRecord(c->prof_events[idx + 1], c->stream);
        c->prof_pending.emplace_back(name, idx);
    }
};

// The context's stream is created hipStreamNonBlocking: it does not synchronise with the null stream, so a blocking copy of one
// engine no longer stalls the kernels of the other engines of the process (measured in the worker: -20 % loop time).  The price:
// nothing orders a null-stream copy against the stream's kernels any more -- every blocking copy therefore first waits for the
// stream (free when it is idle, as in all setters), and memsets / device-to-device copies are enqueued ON the stream.
// The caller's side of a copy (`kind` names the direction the ABI documents) may itself be device memory -- the averaging keeps
// its batch in HBM between operator calls -- so the direction is left to the runtime (unified addressing); a device-to-device
// hipMemcpy is ordered on the null stream, which this context's stream does not wait for: wait for it here.
static inline hipError_t mtip_copy(hipStream_t stream, void* dst, const void* src, size_t n) {
    hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    e = hipMemcpy(dst, src, n, hipMemcpyDefault);
    return e != hipSuccess ? e : hipStreamSynchronize(nullptr);
}
static inline hipError_t mtip_copy(mtip_ctx* c, void* dst, const void* src, size_t n, hipMemcpyKind kind) {
    (void)kind;
    return mtip_copy(c->stream, dst, src, n);
}

static inline bool mtip_is_device_pointer(const void* p) {
    hipPointerAttribute_t at;
    const bool is_dev = hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice;
    (void)hipGetLastError();                        // (an unregistered host pointer sets the sticky error on some runtimes)
    return is_dev;
}

// free device memory in bytes (handles that size their work arrays to what is left)
static inline size_t mtip_free_memory() {
#ifdef __HIPCC__
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) return fr;
#endif
    return (size_t)8 << 30;            // (the CPU build of the tests: a fixed budget)
}

// a caller's array as device memory: itself when it is device memory, else a temporary that is filled / copied back
struct DevView {
    mtip_ctx* c = nullptr;
    void* dev = nullptr;
    void* host = nullptr;
    size_t bytes = 0;
    bool writeback = false;
    hipError_t err = hipSuccess;
    DevBuf<char> temp;
    DevView(mtip_ctx* c_, const void* p, size_t n, bool read, bool write) : c(c_), bytes(n), writeback(write) {
        if (p == nullptr || n == 0) return;
        if (mtip_is_device_pointer(p)) {
            dev = const_cast<void*>(p);
            return;
        }
        host = const_cast<void*>(p);
        err = temp.alloc(n);
        dev = temp;
        if (err == hipSuccess && read) err = mtip_copy(c, dev, p, n, hipMemcpyHostToDevice);
    }
    hipError_t finish() {                           // after the stream has been synchronised
        if (temp && writeback && err == hipSuccess) err = mtip_copy(c, host, dev, bytes, hipMemcpyDeviceToHost);
        return err;
    }
};

static inline int div_up(long long a, long long b) { return (int)((a + b - 1) / b); }

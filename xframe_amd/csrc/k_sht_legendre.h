// Legendre synthesis of the rows of a shell into LDS spectra by the in-register three-term recurrence -- the first half of
// the inverse spherical-harmonic transform (sh.inverse_d, shtns_plugin.py:250-261), shared by k_sht_inv_wide (k_sht_reg.hip)
// and k_sht_chain (k_sht_chain.hip).
//
// The wave is the unit of work: an item = (pair of orders m = 2p, 2p + 1; chunk of 32 thetas).  Lanes 0-31 run the recurrence
// P_lm = a_lm (x P_l-1,m - b_lm P_l-2,m) of m = 2p for their theta, lanes 32-63 that of m = 2p + 1, and every lane accumulates
// the rows of +m AND -m (P_lm is the same for both).  Even and odd l - m accumulate separately (north = E + O, south = E - O).
// Items are dealt to the waves in snake order of decreasing length.
//
// Everything the recurrence reads sits in LDS as RECORDS: record (m, l), l = m .. L + 1, holds (a_lm, b_lm), c_l,+m and c_l,-m,
// three double2, order-major (legendre_rec).  A lane walks the records of its order with one running address; a double step
// (l, l + 1) reads six consecutive entries.  The records l = L + 1 are zero: with them every lane of a wave runs the trip
// count of the wave's smaller order and the same closing step, and what a lane does beyond its own l = L is fma(0, 0, acc),
// which leaves a finite accumulator as it is -- no clamp, no EXEC-mask region in the loop.  The loop requests its operands two
// double steps ahead and so reads up to LEG_AHEAD entries past the last record; the block is allocated that much longer.
//
// Between the barrier behind legendre_stage and the caller's barrier behind legendre_synthesis_rows no global memory is
// touched where the wave's items fit the start-value queue (REFILL = false): the start values P_mm, P_m+1,m of the wave's
// first NQ items and cos(theta) of the lane are requested at kernel entry (legendre_prefetch), in front of the staging loads,
// so the wait in front of the staging stores covers them.  With REFILL the queue is topped up NQ items ahead.
#pragma once
#include "mtip_internal.h"

constexpr int LEG_AHEAD = 12;           // entries the loop may request behind the last record: two operand sets

// first record (l = m) of order m; number of records; LDS entries (double2) of the record block
__host__ __device__ inline int legendre_rec(int m, int L) { return m * (L + 2) - m * (m - 1) / 2; }
__host__ __device__ inline int legendre_n_rec(int L) { return (L + 1) * (L + 2) / 2 + L + 1; }
__host__ __device__ inline int legendre_lds_entries(int L) { return 3 * legendre_n_rec(L) + LEG_AHEAD; }

template <int NQ>
struct LegendreStart {
    double pmm[NQ], pm1[NQ];            // start values of the wave's next NQ items
    double x = 0.0;                     // cos(theta) of the lane (one theta chunk per workgroup)
};

// item index of round kk for this wave (snake order)
__device__ __forceinline__ int legendre_item(int kk, int nw, int wave) { return kk * nw + ((kk & 1) ? nw - 1 - wave : wave); }

// branch-free (clamped addresses): the loads of all slots leave together
__device__ __forceinline__ void legendre_load_start(double& pmm, double& pm1, const double* __restrict__ P, int nt, int L, int nth,
                                                    int j0, int n_chunks, int item, int lane) {
    const int jj = lane & 31, half_id = lane >> 5;
    const int mp = n_chunks == 1 ? item : item / n_chunks, ch = item - mp * n_chunks;
    const int m = min(2 * mp + half_id, L);
    const int j = ch * 32 + jj;
    const int jc = j0 + (j < nth ? j : nth - 1);
    const double* pcol = P + (size_t)(m * (L + 1) - m * (m - 1) / 2) * nt + jc;
    pmm = pcol[0];
    const double v = pcol[m < L ? nt : 0];
    pm1 = m < L ? v : 0.0;
}

// start values of the wave's first NQ items and cos(theta): issued before the tables are staged
// (nth theta pairs of this workgroup, the first one j0)
template <int NQ, bool ONECH>
__device__ __forceinline__ void legendre_prefetch(LegendreStart<NQ>& s, const double* __restrict__ P, const double* __restrict__ cost,
                                                  int nt, int L, int nth, int j0, int wave, int nw, int lane) {
    const int n_chunks = ONECH ? 1 : (nth + 31) >> 5;
    const int n_items = ((L + 2) >> 1) * n_chunks;
#pragma unroll
    for (int u = 0; u < NQ; ++u)
        legendre_load_start(s.pmm[u], s.pm1[u], P, nt, L, nth, j0, n_chunks, min(legendre_item(u, nw, wave), n_items - 1), lane);
    if (ONECH) s.x = cost[j0 + min(lane & 31, nth - 1)];
}

// Staging of everything the workgroup keeps in LDS through the synthesis: twiddles (n_tw entries, 0: none), cos(theta) of the
// workgroup's n_cos theta pairs (0: none), the records from the padded table ABp (legendre_n_rec entries, record order) and the
// shell's coefficients csrc (minus ssrc where SUB).  A thread requests ALL its loads of a chunk -- one twiddle, one cosine, two
// recurrence entries, four coefficients -- before it stores the first: one global round trip per chunk, and one chunk where L
// and nthr are compile-time constants of the benchmark's size.  `younger` runs between the loads of the first chunk and its
// stores: loads the caller wants in flight as well but not waited for here (vmcnt counts in order).  The caller synchronises.
template <bool SUB, class Younger>
__device__ __forceinline__ void legendre_stage(double2* __restrict__ tw_s, const double2* __restrict__ tw_g, int n_tw,
                                               double* __restrict__ cos_s, const double* __restrict__ cost, int n_cos,
                                               double2* __restrict__ rec, const double2* __restrict__ ABp,
                                               const double2* __restrict__ csrc, const double2* __restrict__ ssrc, int L, int tid, int nthr,
                                               Younger&& younger) {
    constexpr int NA = 2, NC = 4;
    const int n_rec = legendre_n_rec(L), nlm = (L + 1) * (L + 1), n_co = (L + 2) * (L + 2);
    const int n_ch = max(max((n_tw + nthr - 1) / nthr, (n_cos + nthr - 1) / nthr),
                         max((n_rec + NA * nthr - 1) / (NA * nthr), (n_co + NC * nthr - 1) / (NC * nthr)));
    for (int c = 0; c < n_ch; ++c) {
        const int e1 = c * nthr + tid;
        double2 vt = tw_g[max(min(e1, n_tw - 1), 0)];
        double vx = cost[max(min(e1, n_cos - 1), 0)];
        double2 va[NA], vc[NC], vs[SUB ? NC : 1];
#pragma unroll
        for (int u = 0; u < NA; ++u) va[u] = ABp[min((c * NA + u) * nthr + tid, n_rec - 1)];
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            const int e = min((c * NC + u) * nthr + tid, nlm - 1);
            vc[u] = csrc[e];
            if (SUB) vs[u] = ssrc[e];
        }
        asm volatile("" ::: "memory");                   // the younger loads stay younger
        if (c == 0) younger();
        // (pinned: left alone the compiler moves each load into the conditional block of its store, a round trip per block)
        double pz = 0.0;
        MTIP_PIN_VGPRS4(vt.x, vt.y, vx, pz)
#pragma unroll
        for (int u = 0; u < NA; u += 2) { MTIP_PIN_VGPRS4(va[u].x, va[u].y, va[u + 1].x, va[u + 1].y) }
#pragma unroll
        for (int u = 0; u < NC; u += 2) { MTIP_PIN_VGPRS4(vc[u].x, vc[u].y, vc[u + 1].x, vc[u + 1].y) }
        if (SUB) {
#pragma unroll
            for (int u = 0; u < NC; u += 2) { MTIP_PIN_VGPRS4(vs[u].x, vs[u].y, vs[SUB ? u + 1 : 0].x, vs[SUB ? u + 1 : 0].y) }
        }
        if (e1 < n_tw) tw_s[e1] = vt;
        if (e1 < n_cos) cos_s[e1] = vx;
#pragma unroll
        for (int u = 0; u < NA; ++u) {
            const int e = (c * NA + u) * nthr + tid;
            if (e < n_rec) rec[3 * e] = va[u];
        }
#pragma unroll
        for (int u = 0; u < NC; ++u) {
            // entry e = l (l + 1) + m of the coefficients padded to l = L + 1; |m| = L + 1 has no record
            const int e = (c * NC + u) * nthr + tid;
            const int l = (int)sqrtf((float)e + 0.5f);
            const int mq = e - l * (l + 1), ma = mq < 0 ? -mq : mq;
            if (e < n_co && ma <= L) {
                double2 v = SUB ? csub(vc[u], vs[u]) : vc[u];
                if (e >= nlm) v = make_double2(0.0, 0.0);
                double2* r = rec + 3 * (legendre_rec(ma, L) + l - ma);
                if (mq >= 0) r[1] = v;
                if (mq <= 0) r[2] = v;
            }
        }
    }
}

// Gs: spectra, row 2j = theta_(j0+j), row 2j+1 = its mirror, 2L+1 entries per row (m = -L..L); rec: the records; cos_s:
// cos(theta_(j0+j)) in LDS (read where !ONECH).  All of Gs that belongs to the workgroup's rows is written; the caller
// synchronises afterwards.
template <int NQ, bool REFILL, bool ONECH>
__device__ __forceinline__ void legendre_synthesis_rows(LegendreStart<NQ>& s, double2* __restrict__ Gs, const double2* __restrict__ rec,
                                                        const double* __restrict__ cos_s, const double* __restrict__ P,
                                                        int nt, int L, int nth, int j0, int wave, int nw, int lane) {
    const int nm = 2 * L + 1;
    const int jj = lane & 31, half_id = lane >> 5;
    const int n_chunks = ONECH ? 1 : (nth + 31) >> 5;
    const int n_items = ((L + 2) >> 1) * n_chunks;
    for (int kk = 0;; ++kk) {
        const int i = legendre_item(kk, nw, wave);
        if (i >= n_items) break;
        const int mp = ONECH ? i : i / n_chunks, ch = i - mp * n_chunks;
        const int m_a = 2 * mp;                                  // the smaller order of the pair: sets the trip count of the wave
        const bool m_ok = m_a + half_id <= L;
        const int m = min(m_a + half_id, L);                     // this lane's order (clamped: an odd L + 1 has no partner)
        const int j = ch * 32 + jj;
        const bool act = (j < nth) && m_ok;
        const double x = ONECH ? s.x : cos_s[j < nth ? j : nth - 1];
        double p2 = s.pmm[0], p1 = s.pm1[0];
#pragma unroll
        for (int u = 0; u + 1 < NQ; ++u) {
            s.pmm[u] = s.pmm[u + 1];
            s.pm1[u] = s.pm1[u + 1];
        }
        if (REFILL) {   // the start values of the item NQ rounds ahead
            const int i2 = legendre_item(kk + NQ, nw, wave);
            if (i2 < n_items) legendre_load_start(s.pmm[NQ - 1], s.pm1[NQ - 1], P, nt, L, nth, j0, n_chunks, i2, lane);
        }
        const double2* r = rec + 3 * legendre_rec(m, L);         // records l = m, m + 1: the start values times their coefficients
        double2 Ep, Em, Op, Om;
        {
            const double2 a = r[1], b = r[2], c = r[4], d = r[5];
            Ep = make_double2(p2 * a.x, p2 * a.y);
            Em = make_double2(p2 * b.x, p2 * b.y);
            Op = make_double2(p1 * c.x, p1 * c.y);               // (m = L: p1 = 0 times the zero record)
            Om = make_double2(p1 * d.x, p1 * d.y);
        }
        r += 6;
        // The recurrence is a dependent chain and there are only two waves per SIMD: with the operands read at the top of
        // each iteration an LDS round trip per iteration was most of the loop.  Two operand sets, A and B, alternate in fixed
        // registers; a set is requested as soon as its registers are free, two double steps before it is used, and waited for
        // by count (the other set's requests are younger and stay in flight).  All lanes run the double steps of the wave's smaller
        // order and its closing single step (the zero records make that harmless for the lane whose l has run out).
        const int n_it = m_a + 2 <= L ? (L - m_a - 1) >> 1 : 0;  // double steps of the wave (uniform)
        const bool tail = m_a + 2 <= L && ((L - m_a) & 1) == 0;  // and a single one at l = L of the smaller order (uniform)
        double2 Aab0, Aab1, Acp, Aop, Acm, Aom, Bab0, Bab1, Bcp, Bop, Bcm, Bom;
#define LEG_LOAD(S, q_)                                              \
        {                                                            \
            S##ab0 = (q_)[0];                                        \
            S##cp = (q_)[1];                                         \
            S##cm = (q_)[2];                                         \
            S##ab1 = (q_)[3];                                        \
            S##op = (q_)[4];                                         \
            S##om = (q_)[5];                                         \
        }
#define LEG_STEP(S)                                                         \
        {                                                                   \
            const double pa = S##ab0.x * (x * p1 - S##ab0.y * p2);          \
            const double pb = S##ab1.x * (x * pa - S##ab1.y * p1);          \
            Ep.x = fma(pa, S##cp.x, Ep.x); Ep.y = fma(pa, S##cp.y, Ep.y);   \
            Op.x = fma(pb, S##op.x, Op.x); Op.y = fma(pb, S##op.y, Op.y);   \
            Em.x = fma(pa, S##cm.x, Em.x); Em.y = fma(pa, S##cm.y, Em.y);   \
            Om.x = fma(pb, S##om.x, Om.x); Om.y = fma(pb, S##om.y, Om.y);   \
            p2 = pa;                                                        \
            p1 = pb;                                                        \
        }
        // (the fence keeps a request where it is written: left alone the compiler moves it down to the step that uses it)
#define LEG_PIN(S)                                                  \
        MTIP_PIN_VGPRS4(S##ab0.x, S##ab0.y, S##ab1.x, S##ab1.y)     \
        MTIP_PIN_VGPRS4(S##cp.x, S##cp.y, S##op.x, S##op.y)         \
        MTIP_PIN_VGPRS4(S##cm.x, S##cm.y, S##om.x, S##om.y)         \
        asm volatile("" ::: "memory");
        LEG_LOAD(A, r)
        LEG_LOAD(B, r + 6)
        int it = n_it;
        if (it >= 2) {
            do {                                                 // (one block, the test at its end: no copies on the back edge)
                LEG_PIN(A)                                       // waits for A alone: B is younger
                LEG_STEP(A)
                LEG_LOAD(A, r + 12)
                LEG_PIN(B)
                LEG_STEP(B)
                LEG_LOAD(B, r + 18)
                r += 12;
                it -= 2;
            } while (it >= 2);
        }
        LEG_PIN(A)
        if (it) {
            LEG_STEP(A)
            LEG_PIN(B)
            Aab0 = Bab0;
            Acp = Bcp;
            Acm = Bcm;
        }
#undef LEG_LOAD
#undef LEG_STEP
#undef LEG_PIN
        if (tail) {
            const double pa = Aab0.x * (x * p1 - Aab0.y * p2);
            Ep.x = fma(pa, Acp.x, Ep.x); Ep.y = fma(pa, Acp.y, Ep.y);
            Em.x = fma(pa, Acm.x, Em.x); Em.y = fma(pa, Acm.y, Em.y);
        }
        if (act) {
            double2* g_p = Gs + (size_t)(2 * j) * nm + L + m;
            g_p[0] = make_double2(Ep.x + Op.x, Ep.y + Op.y);
            g_p[nm] = make_double2(Ep.x - Op.x, Ep.y - Op.y);
            if (m > 0) {
                const double sg = (m & 1) ? -1.0 : 1.0;            // Y_l,-m = (-1)^m conj(Y_lm)
                double2* g_m = Gs + (size_t)(2 * j) * nm + L - m;
                g_m[0] = make_double2(sg * (Em.x + Om.x), sg * (Em.y + Om.y));
                g_m[nm] = make_double2(sg * (Em.x - Om.x), sg * (Em.y - Om.y));
            }
        }
    }
}

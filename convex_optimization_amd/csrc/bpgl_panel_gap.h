// Panel duality-gap certificate.  Included by bpgl_panel_abi.hip only.
// Checkpoint operations, not per-iteration ones.
//
// The certificate describes the STORED x (the solver's fp32 iterate), not the solver's carried
// state.  bf16 A widens to fp64 exactly; everything after that is fp64:
//   Rf[k][i]     = sum_j A[i][j] x_k[j] - B[k][i]          over all feature blocks   (product 1)
//   G[blk][k][j] = sum_i A[i][blk w + j] Rf[k][i]          from Rf only              (product 2)
// and per right-hand side k, with mu_k and d_j = ||a_j||^2 (the context's diag), the formulas of
// bpgl_gap.h:
//   primal, dual, gap, scale, ||g||_inf;  keep[k][j] = !(score_j < mu_k);  n_keep
//   drift_k = max_i |R_solver[k][i] - Rf[k][i]|
//
//   k_pgap_prod<NT, PROD>   a 256-thread block owns 64 outputs x all 16 NT right-hand sides over one
//                           chunk of the reduction; wave w owns 16 outputs x NT tiles of
//                           v_mfma_f64_16x16x4_f64.  A travels global -> registers (16-byte pieces
//                           along its contiguous dimension) -> LDS as fp64, the k-wide operand
//                           (x, fp32, or Rf, fp64) likewise; the next stage's pieces are in
//                           registers while this stage's MFMAs run.  Writes its chunk's partial.
//   k_pgap_fold<PROD>       out = the chunks' partials added in chunk order (- B for product 1)
//   k_pgap_partials         per (block, RHS): [sum r^2, sum r.b, sum |x|, max |g|, max |R - r|]
//   k_pgap_final            one block per RHS: folds them in block order -> res[k][0..4], res[k][6]
//   k_pgap_screen           keep[k][j] and per-block counts
//   k_pgap_count            one block per RHS: res[k][5] = n_keep
// With a row mask w (bpgl_panel_set_row_mask; B is then stored as w o B):
//   k_pgap_fold<1, true>    Rf[k][i] = w_ki (a_i . x_k - b_ki), and per 256-thread block (one RHS: m is a
//                           multiple of 256) the held-out sum of (1 - w_ki)(a_i . x_k - b_ki)^2 from Bh
//   k_pgap_holdout          one block per RHS: res[k][7] = those block sums added in block order
// Product 2 and everything after it then describe the masked problem; the screen keeps the full diag.
// With the intercept (bpgl_panel_set_intercept; B is then stored as P_w B with its
// in-row mean in bmean, and a mask is always installed):
//   k_pgap_fold<1, true, true>   Rf[k][i] = a_i . x_k - (in ? (P_w b)_ki : b_ki) at EVERY row -- the uncentred
//                           e, shifted by bmean_k at the in-rows -- and per block the in-row sum of it
//   k_pgap_icpt_mean        one block per RHS: those sums in block order -> c' = sum / n_w, beta0 = bmean - c'
//   k_pgap_centre           Rf = in ? Rf - c' : 0, i.e. P_w(A x - b); the held-out (e - c)^2 = (a.x + beta0 - b)^2,
//                           squared directly, to the per-block partials that k_pgap_holdout consumes
// Product 2 and everything after it read the centred Rf: the certificate of the profiled problem.
// With the non-negative constraint (bpgl_panel_set_positive; the POS variants, which only
// bpgl_panel_pos.hip instantiates):
//   k_pgap_partials         max |g| becomes max_j (-g_j)+, so scale = min(1, mu / that) makes scale r feasible for the
//                           one-sided dual constraint -a_j . theta <= mu; primal, dual and gap keep their formulas
//   k_pgap_screen           score_j = scale (-g_j) + sqrt(d_j) sqrt(2 max(gap, 0))
// With penalty factors p (bpgl_panel_set_penalty; k_pgap_partials_pf and k_pgap_screen_pf,
// the same bodies with one more argument, which only bpgl_panel_pen.hip instantiates):
//   k_pgap_partials_pf      sum |x| becomes sum p_j |x_j| and max |g| becomes max_j |g_j| / p_j (max_j (-g_j)+ / p_j
//                           with POS), so scale = min(1, mu / that) gives |a_j . (scale r)| <= mu p_j; k_pgap_final is
//                           unchanged
//   k_pgap_screen_pf        keep_j = not (score_j < mu p_j), the score as above
// With observation weights w in [0, 1] (bpgl_panel_set_row_weights; B is then stored as w o B, the
// full B in Bh; the kernels of bpgl_panel_wt.hip):
//   k_pgap_fold_wt          E[k][i] = e = a_i . x_k - b_ki at every row, Rf = w o e, and per block the scoring partial
//                           sum h e^2 that k_pgap_holdout consumes; with the intercept the uncentred e and per block
//                           sum w e for k_pgap_icpt_mean (unchanged: n_w is then sum w), and
//   k_pgap_centre_wt        E = e - ebar_w, Rf = w o E, the scoring partials from a_i . x + beta0 - b_i
//   k_pgap_partials_wt      sum w e^2 = sum Rf E and sum w e b = sum E B instead of sum r^2 and sum r b (pgap_partials_body's
//                           WT flag), in the same walk; with POS and / or PF as their variants have it
// Every reduction walks its dimension in a fixed order (within a chunk: 32-deep stages in index
// order, 4 at a time through the MFMA; then the chunks; then wave_sum / wave_max, the waves, the
// blocks in index order).  No floating-point atomics: two calls on the same state return the same
// bits.
// bpgl_panel_reset_x0 runs product 1 on X0 into the solver's R: with one feature
// block through k_pgap_fold<1> as above, with more through
//   k_pgap_fold_ax          Ax[b] = block b's chunks (the chunks aligned to the blocks), R = sum_b Ax[b] - B
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bpgl_panel.h"

// (The kernels that are not templates sit under BPGL_PANEL_TEMPLATES_ONLY guards: see bpgl_panel.h.)
namespace bpgl {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int kPgTile = 64;               // outputs per block
constexpr int kPgK = 32;                  // reduction depth per stage
// LDS row strides in doubles.  An MFMA operand read takes, per half-wave, rows i = 0..15 at depths
// j, j + 1: [row][depth] images want stride = 2 (mod 32) and the [depth][row] image 16 (mod 32) for
// 32 distinct 8-byte banks.
constexpr int kPgLdV = kPgK + 2;          // k-wide operand  [rhs][depth]
constexpr int kPgLdA1 = kPgK + 2;         // product 1's A   [output row][depth]
constexpr int kPgLdA2 = kPgTile + 16;     // product 2's A   [depth][output column]
constexpr int kPgBlocksTarget = 512;      // the reduction is split until a product has about this many blocks
constexpr int kPgRes = 8;                 // res[k]: primal, dual, gap, scale, ||g||_inf, n_keep, drift, held-out SSE (0 without a mask)
constexpr int kPgPart = 5;                // partials per (block, RHS)
constexpr int kPgPartBlocks = kThreads;   // at most one partial per thread of k_pgap_final

struct PanelGapArgs {
    const __bf16* A;      // [m][lda]
    long long lda, m, n, w;
    int nblock, k;
    const float* X;       // [nblock][k][w]   the solver's iterate
    const double* B;      // [k][m]
    const double* R;      // [k][m]           the solver's residual (drift only)
    const double* diag;   // [n]
    const double* mu;     // [k]
    double* Rf;           // [k][m]           caller's
    double* G;            // [nblock][k][w]   caller's
    double* part;         // [spl][k][len]    a product's chunk partials
    int spl;              // chunks of the product being run
    long long chunk;      // stages per chunk
    // row mask (null without one): the masked fold of product 1 only
    const unsigned char* W;   // [k][m]
    const double* Bh;     // [k][m]           (1 - w) o B
    double* hpart;        // [k m / 256]      held-out partial of each fold block
    // intercept (null / unread without it): the centring of product 1
    double* ipart;        // [k m / 256]      in-row sum of each fold block
    double* icp;          // [2][k]           c' = the in-row mean of what the fold left; beta0
    const double* nw;     // [k]              rows in each RHS's objective
    const double* bmean;  // [k]              the in-row mean of b that the stored P_w B had subtracted
    // observation weights (null / unread without them): the weighted fold of product 1 and the weighted partials
    const double* Wt;     // [k][m]           w in [0, 1]
    const double* Hd;     // [k][m]           the scoring weights h >= 0 of res[k][7]
    double* E;            // [k][m]           e = a_i . x - b_i (centred with the intercept), unweighted
};

// bf16 e of 8 in a 16-byte piece -> fp64 (exact)
__device__ __forceinline__ double pg_widen(const u32x4& v, int e) {
    const unsigned word = v[e >> 1];
    return (double)__uint_as_float((e & 1) ? (word & 0xffff0000u) : (word << 16));
}

// PROD 1: outputs = rows of A, depth = columns (A contiguous along the depth);
// PROD 2: outputs = columns of A, depth = rows (A contiguous along the outputs).
// grid = tiles * spl; block b: tile b % tiles, chunk b / tiles
template <int NT, int PROD>
__global__ __launch_bounds__(kThreads) void k_pgap_prod(PanelGapArgs a) {
    constexpr int K = 16 * NT;
    constexpr int NV = PROD == 1 ? (NT + 1) / 2 : NT;   // 16-byte pieces of the k-wide operand per thread and stage
    constexpr int VP = PROD == 1 ? 8 : 16;              // ... per right-hand side
    __shared__ __attribute__((aligned(16))) double As[PROD == 1 ? kPgTile * kPgLdA1 : kPgK * kPgLdA2];
    __shared__ __attribute__((aligned(16))) double Vs[K * kPgLdV];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long len = PROD == 1 ? a.m : a.n;
    const long long tiles = len / kPgTile;
    const long long tile = blockIdx.x % tiles;
    const long long c = blockIdx.x / tiles;
    const long long o0 = tile * kPgTile;
    const long long s0 = c * a.chunk, s1 = s0 + a.chunk;

    u32x4 ra, rv[NV];
    auto fetch = [&](long long s) {
        const long long d0 = s * kPgK;
        if (PROD == 1) {
            ra = *reinterpret_cast<const u32x4*>(a.A + (o0 + (tid >> 2)) * a.lda + d0 + (tid & 3) * 8);
            const long long blk = d0 / a.w, jj = d0 % a.w;
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const int p = tid + kThreads * q;
                if (p < K * VP)
                    rv[q] = *reinterpret_cast<const u32x4*>(a.X + (blk * K + (p >> 3)) * a.w + jj + (p & 7) * 4);
            }
        } else {
            ra = *reinterpret_cast<const u32x4*>(a.A + (d0 + (tid >> 3)) * a.lda + o0 + (tid & 7) * 8);
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const int p = tid + kThreads * q;
                rv[q] = *reinterpret_cast<const u32x4*>(a.Rf + (long long)(p >> 4) * a.m + d0 + (p & 15) * 2);
            }
        }
    };
    auto stash = [&]() {
        double* ad = PROD == 1 ? As + (tid >> 2) * kPgLdA1 + (tid & 3) * 8 : As + (tid >> 3) * kPgLdA2 + (tid & 7) * 8;
#pragma unroll
        for (int e = 0; e < 8; e += 2) {
            f64x2 v;
            v[0] = pg_widen(ra, e);
            v[1] = pg_widen(ra, e + 1);
            *reinterpret_cast<f64x2*>(ad + e) = v;
        }
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const int p = tid + kThreads * q;
            if (PROD == 1) {
                if (p < K * VP) {
                    double* vd = Vs + (p >> 3) * kPgLdV + (p & 7) * 4;
                    f64x2 lo, hi;
                    lo[0] = (double)__uint_as_float(rv[q][0]);
                    lo[1] = (double)__uint_as_float(rv[q][1]);
                    hi[0] = (double)__uint_as_float(rv[q][2]);
                    hi[1] = (double)__uint_as_float(rv[q][3]);
                    *reinterpret_cast<f64x2*>(vd) = lo;
                    *reinterpret_cast<f64x2*>(vd + 2) = hi;
                }
            } else {
                union { u32x4 q; f64x2 d; } u;
                u.q = rv[q];
                *reinterpret_cast<f64x2*>(Vs + (p >> 4) * kPgLdV + (p & 15) * 2) = u.d;
            }
        }
    };

    f64x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int li = lane & 15, lj = lane >> 4;
    fetch(s0);
    for (long long s = s0; s < s1; ++s) {
        __syncthreads();          // the previous stage's reads are done
        stash();
        __syncthreads();
        if (s + 1 < s1) fetch(s + 1);
#pragma unroll
        for (int d = 0; d < kPgK; d += 4) {
            // the MFMA's "A" operand is the k-wide one (its rows = right-hand sides) and its "B" operand
            // the matrix (its columns = outputs): D[row = rhs][col = output], so a lane's results sit
            // at one output and 16 lanes store 128 contiguous bytes
            const double bv = PROD == 1 ? As[(16 * wave + li) * kPgLdA1 + d + lj]
                                        : As[(d + lj) * kPgLdA2 + 16 * wave + li];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const double av = Vs[(16 * t + li) * kPgLdV + d + lj];
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[t], 0, 0, 0);
            }
        }
    }
    // C/D of v_mfma_f64_16x16x4_f64: col = lane & 15, row = (lane >> 4) + 4 reg
    double* dst = a.part + (c * K) * len + o0 + 16 * wave + li;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[(long long)(16 * t + lj + 4 * r) * len] = acc[t][r];
}

// one thread per (rhs, output): the chunks in index order; product 1 subtracts B and writes Rf[k][i],
// product 2 writes G[blk][k][j].  MK (product 1 with a row mask; a.B holds w o B): Rf = 0 at the
// held-out rows, whose squared errors against Bh go to one partial per block (lanes, waves in order)
template <int PROD, bool MK = false, bool IC = false>
__global__ __launch_bounds__(kThreads) void k_pgap_fold(PanelGapArgs a) {
    static_assert(!MK || PROD == 1, "the mask enters product 1 only");
    static_assert(!IC || MK, "the intercept runs on the masked fold");
    const long long len = PROD == 1 ? a.m : a.n;
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if constexpr (MK) {
        // k m is a multiple of kThreads (m is one of 256), so no thread of a block is out of range
        double v = a.part[e];
        for (int c = 1; c < a.spl; ++c) v += a.part[(long long)c * a.k * len + e];
        const bool in = a.W[e] != 0;
        if constexpr (IC) {
            const double ev = v - (in ? a.B[e] : a.Bh[e]);
            a.Rf[e] = ev;
            const double es = wave_sum(in ? ev : 0.0);
            __shared__ double red[kWaves];
            const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
            if (lane == 0) red[wave] = es;
            __syncthreads();
            if (threadIdx.x == 0) a.ipart[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
            return;
        }
        a.Rf[e] = in ? v - a.B[e] : 0.0;
        const double h = in ? 0.0 : v - a.Bh[e];
        const double hh = wave_sum(h * h);
        __shared__ double red[kWaves];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) red[wave] = hh;
        __syncthreads();
        if (threadIdx.x == 0) a.hpart[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    } else {
        if (e >= (long long)a.k * len) return;
        const long long k = e / len, o = e % len;
        double v = a.part[e];
        for (int c = 1; c < a.spl; ++c) v += a.part[(long long)c * a.k * len + e];
        if (PROD == 1) a.Rf[e] = v - a.B[e];
        else a.G[((o / a.w) * a.k + k) * a.w + o % a.w] = v;
    }
}

#ifndef BPGL_PANEL_TEMPLATES_ONLY
// intercept, one block per RHS: the nb fold blocks' in-row sums added in block order (loaded kThreads at a
// time, thread 0 adding them in index order) -> icp[0][k] = c' = sum / n_w (0 for an all-zero mask column),
// icp[1][k] = beta0 = bmean - c' = -mean_in(a_i . x - b_i)
__global__ __launch_bounds__(kThreads) void k_pgap_icpt_mean(PanelGapArgs a, long long nb) {
    const int k = blockIdx.x;
    __shared__ double buf[kThreads];
    double tot = 0.0;
    for (long long q0 = 0; q0 < nb; q0 += kThreads) {
        const long long q = q0 + threadIdx.x;
        if (q < nb) buf[threadIdx.x] = a.ipart[(long long)k * nb + q];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < kThreads && q0 + i < nb; ++i) tot += buf[i];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double n = a.nw[k];
    const double c = n > 0.0 ? tot / n : 0.0;
    a.icp[k] = c;
    a.icp[a.k + k] = n > 0.0 ? a.bmean[k] - c : 0.0;
}

// intercept, one thread per (rhs, row) (k m is a multiple of kThreads and a block lies in one RHS, as in the
// masked fold): Rf = e' - c' at the in-rows, 0 at the others; the held-out rows' e - c = e' - c' + bmean
// squared directly (no expanded square) into the block's partial, lanes then waves in order
__global__ __launch_bounds__(kThreads) void k_pgap_centre(PanelGapArgs a) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long k = e / a.m;
    const double c = a.icp[k], bm = a.bmean[k];
    const bool in = a.W[e] != 0;
    const double ev = a.Rf[e];
    a.Rf[e] = in ? ev - c : 0.0;
    const double h = in ? 0.0 : (ev - c) + bm;
    const double hh = wave_sum(h * h);
    __shared__ double red[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = hh;
    __syncthreads();
    if (threadIdx.x == 0) a.hpart[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}
#endif  // BPGL_PANEL_TEMPLATES_ONLY

// bpgl_panel_reset_x0 with more than one feature block: product 1 ran with its
// chunks aligned to the feature blocks (a.spl = nblock x spb, chunk c inside block c / spb).  One thread
// per (rhs, row): Ax[b] = block b's chunks added in chunk order, R = sum_b Ax[b] - B with b in index
// order, as k_panel_update sums them.  MK (a.B holds w o B): Ax[b] and R are 0 at the held-out rows,
// by select -- the solver's Ax is the sum of masked S, so it is masked too.
template <bool MK>
__global__ __launch_bounds__(kThreads) void k_pgap_fold_ax(PanelGapArgs a, int spb, double* __restrict__ Ax,
                                                           double* __restrict__ R) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long km = (long long)a.k * a.m;
    if (e >= km) return;
    bool in = true;
    if constexpr (MK) in = a.W[e] != 0;
    double acc = 0.0;
    for (int b = 0; b < a.nblock; ++b) {
        const double* part = a.part + (long long)b * spb * km + e;
        double v = part[0];
        for (int c = 1; c < spb; ++c) v += part[(long long)c * km];
        v = in ? v : 0.0;
        Ax[(long long)b * km + e] = v;
        acc = b == 0 ? v : acc + v;
    }
    R[e] = in ? acc - a.B[e] : 0.0;
}

#ifndef BPGL_PANEL_TEMPLATES_ONLY
// one block per RHS: res[k][7] = the held-out partials of its nb fold blocks, thread q taking blocks
// q, q + kThreads, ... in order and thread 0 adding the threads' sums in thread order
__global__ __launch_bounds__(kThreads) void k_pgap_holdout(const double* __restrict__ hpart, long long nb,
                                                           double* __restrict__ res_all) {
    const int k = blockIdx.x;
    double s = 0.0;
    for (long long q = threadIdx.x; q < nb; q += kThreads) s += hpart[(long long)k * nb + q];
    __shared__ double red[kThreads];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double tot = 0.0;
    for (int q = 0; q < kThreads; ++q) tot += red[q];
    res_all[(long long)k * kPgRes + 7] = tot;
}
#endif  // BPGL_PANEL_TEMPLATES_ONLY

// grid (nparts, k); parts[k][nparts][kPgPart].  POS: the dual constraint is one-sided, -a_j . theta <= mu, and
// the fourth partial is max (-g)+ instead of max |g|
// WT (observation weights; the variants of bpgl_panel_wt.hip): Rf is w o e and the stored B is w o b (both centred with
// the intercept), so r^2 and r b would carry w twice.  The first two partials are sum w e^2 = sum Rf e and
// sum w e b = sum e B instead, with e read from a.E, where the weighted fold left it -- never Rf / w.  Same walk, same
// order: with w in {0, 1} they are the sums of the masked certificate term for term.
template <bool POS, bool PF, bool WT = false>
__device__ __forceinline__ void pgap_partials_body(const PanelGapArgs& a, double* __restrict__ parts,
                                                   const double* __restrict__ pen) {
    const int k = blockIdx.y;
    const long long tid = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long stride = (long long)gridDim.x * kThreads;
    double rr = 0.0, rb = 0.0, ax = 0.0, gm = 0.0, dr = 0.0;
    const double* __restrict__ rf = a.Rf + (long long)k * a.m;
    const double* __restrict__ b = a.B + (long long)k * a.m;
    const double* __restrict__ rs = a.R + (long long)k * a.m;
    for (long long i = tid; i < a.m; i += stride) {
        const double r = rf[i];
        if constexpr (WT) {
            const double ev = a.E[(long long)k * a.m + i];
            rr = fma(r, ev, rr);
            rb = fma(ev, b[i], rb);
        } else {
        rr = fma(r, r, rr);
        rb = fma(r, b[i], rb);
        }
        dr = nan_max(dr, fabs(rs[i] - r));
    }
    for (long long j = tid; j < a.n; j += stride) {
        const long long e = ((j / a.w) * a.k + k) * a.w + j % a.w;
        if constexpr (PF) {   // the weighted l1 norm and the weighted dual norm (p_j > 0 and finite: set_penalty)
            const double pj = pen[j], gv = a.G[e];
            ax += pj * fabs((double)a.X[e]);
            gm = nan_max(gm, (POS ? (gv > 0.0 ? 0.0 : -gv) : fabs(gv)) / pj);
        } else {
        ax += fabs((double)a.X[e]);
        if constexpr (POS) {
            const double gv = a.G[e];
            gm = nan_max(gm, gv > 0.0 ? 0.0 : -gv);   // (a NaN stays a NaN)
        } else {
            gm = nan_max(gm, fabs(a.G[e]));
        }
        }
    }
    rr = wave_sum(rr);
    rb = wave_sum(rb);
    ax = wave_sum(ax);
    gm = wave_max(gm);
    dr = wave_max(dr);
    __shared__ double red[kPgPart][kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[0][wave] = rr; red[1][wave] = rb; red[2][wave] = ax; red[3][wave] = gm; red[4][wave] = dr; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* dst = parts + ((long long)k * gridDim.x + blockIdx.x) * kPgPart;
        for (int q = 0; q < 3; ++q) dst[q] = ((red[q][0] + red[q][1]) + red[q][2]) + red[q][3];
        for (int q = 3; q < 5; ++q)
            dst[q] = nan_max(nan_max(nan_max(red[q][0], red[q][1]), red[q][2]), red[q][3]);
    }
}
template <bool POS = false>
__global__ __launch_bounds__(kThreads) void k_pgap_partials(PanelGapArgs a, double* __restrict__ parts) {
    pgap_partials_body<POS, false>(a, parts, nullptr);
}
// ... with the penalty factors pen [n], global column order
template <bool POS>
__global__ __launch_bounds__(kThreads) void k_pgap_partials_pf(PanelGapArgs a, double* __restrict__ parts,
                                                               const double* __restrict__ pen) {
    pgap_partials_body<POS, true>(a, parts, pen);
}
// ... with observation weights (a.E, beside a.Rf and the stored w o b); pen is read with PF only
template <bool POS, bool PF>
__global__ __launch_bounds__(kThreads) void k_pgap_partials_wt(PanelGapArgs a, double* __restrict__ parts,
                                                               const double* __restrict__ pen) {
    pgap_partials_body<POS, PF, true>(a, parts, pen);
}

#ifndef BPGL_PANEL_TEMPLATES_ONLY
// one block per RHS; thread q holds partial q (nparts <= kPgPartBlocks = kThreads).  The formulas and
// the NaN behaviour of k_gap_final.
__global__ __launch_bounds__(kThreads) void k_pgap_final(const double* __restrict__ parts, int nparts,
                                                         const double* __restrict__ mu_all,
                                                         double* __restrict__ res_all) {
    const int k = blockIdx.x, q = threadIdx.x;
    const bool ok = q < nparts;
    const double* src = parts + ((long long)k * nparts + q) * kPgPart;
    double rr = ok ? src[0] : 0.0;
    double rb = ok ? src[1] : 0.0;
    double ax = ok ? src[2] : 0.0;
    double gm = ok ? src[3] : 0.0;
    double dr = ok ? src[4] : 0.0;
    rr = wave_sum(rr);
    rb = wave_sum(rb);
    ax = wave_sum(ax);
    gm = wave_max(gm);
    dr = wave_max(dr);
    __shared__ double red[kPgPart][kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[0][wave] = rr; red[1][wave] = rb; red[2][wave] = ax; red[3][wave] = gm; red[4][wave] = dr; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    rr = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    rb = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    ax = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
    gm = nan_max(nan_max(nan_max(red[3][0], red[3][1]), red[3][2]), red[3][3]);
    dr = nan_max(nan_max(nan_max(red[4][0], red[4][1]), red[4][2]), red[4][3]);
    const double mu = mu_all[k];
    const double primal = 0.5 * rr + mu * ax;
    double s = 1.0;                       // also for g = 0 and for a NaN
    if (gm > 0.0) { s = mu / gm; s = s < 1.0 ? s : 1.0; }
    const double dual = -0.5 * s * s * rr - s * rb;
    double* res = res_all + (long long)k * kPgRes;
    res[0] = primal;
    res[1] = dual;
    res[2] = primal - dual;
    res[3] = s;
    res[4] = gm;
    res[5] = 0.0;
    res[6] = dr;
    res[7] = 0.0;
}
#endif  // BPGL_PANEL_TEMPLATES_ONLY

// grid (ceil(n / kThreads), k): keep[k][j] for the global column j; counts[k][block] = columns kept.
// POS: score_j = scale (-g_j) + ...
// (the body's pointers carry no __restrict__: the kernels' own qualifiers say it already, and a second set changed
// the instruction schedule of the instantiations that existed)
template <bool POS, bool PF>
__device__ __forceinline__ void pgap_screen_body(const PanelGapArgs& a, const double* res_all, unsigned char* keep,
                                                 int* counts, const double* pen) {
    const int k = blockIdx.y;
    const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
    bool kp = false;
    if (j < a.n) {
        const double* res = res_all + (long long)k * kPgRes;
        const double gap = res[2], s = res[3];
        const double gp = gap < 0.0 ? 0.0 : gap;   // a NaN stays a NaN
        const double g = a.G[((j / a.w) * a.k + k) * a.w + j % a.w];
        const double score = s * (POS ? -g : fabs(g)) + sqrt(a.diag[j]) * sqrt(2.0 * gp);
        if constexpr (PF) kp = !(score < a.mu[k] * pen[j]);
        else kp = !(score < a.mu[k]);
        keep[(long long)k * a.n + j] = kp ? 1 : 0;
    }
    const int cnt = __popcll(__ballot(kp));
    __shared__ int red[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) counts[(long long)k * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}
template <bool POS = false>
__global__ __launch_bounds__(kThreads) void k_pgap_screen(PanelGapArgs a, const double* __restrict__ res_all,
                                                          unsigned char* __restrict__ keep,
                                                          int* __restrict__ counts) {
    pgap_screen_body<POS, false>(a, res_all, keep, counts, nullptr);
}
template <bool POS>
__global__ __launch_bounds__(kThreads) void k_pgap_screen_pf(PanelGapArgs a, const double* __restrict__ res_all,
                                                             unsigned char* __restrict__ keep,
                                                             int* __restrict__ counts,
                                                             const double* __restrict__ pen) {
    pgap_screen_body<POS, true>(a, res_all, keep, counts, pen);
}

#ifndef BPGL_PANEL_TEMPLATES_ONLY
// one block per RHS: res[k][5] = sum of its per-block counts (integers: exact in any order)
__global__ __launch_bounds__(kThreads) void k_pgap_count(const int* __restrict__ counts, long long nblocks,
                                                         double* __restrict__ res_all) {
    const int k = blockIdx.x;
    long long s = 0;
    for (long long q = threadIdx.x; q < nblocks; q += kThreads) s += counts[(long long)k * nblocks + q];
    __shared__ long long red[kThreads];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    long long tot = 0;
    for (int q = 0; q < kThreads; ++q) tot += red[q];
    res_all[(long long)k * kPgRes + 5] = (double)tot;
}
#endif  // BPGL_PANEL_TEMPLATES_ONLY

}  // namespace bpgl

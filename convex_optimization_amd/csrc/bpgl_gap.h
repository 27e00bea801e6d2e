// Duality-gap certificate, gap-safe column screening and the column gather (DESIGN.md
// section 9).  Included by bpgl.hip only.  Checkpoint operations, not per-iteration ones.
//
// With r = A x - b (the solver's residual), g = A^T r over ALL feature blocks (exact: a fresh
// k_colpass + k_colreduce per block, never the one-pass path's carried G) and d_j = ||a_j||^2
// (the context's diag):
//   primal P = 1/2 ||r||^2 + mu ||x||_1
//   scale  s = min(1, mu / ||g||_inf)   (1 when ||g||_inf = 0): theta = s r is dual feasible
//   dual   D = -1/2 s^2 ||r||^2 - s r.b
//   gap      = P - D >= P(x) - P*;  D is 1-strongly concave, so ||theta - theta*|| <= sqrt(2 gap)
//   score_j  = s |g_j| + sqrt(d_j) sqrt(2 max(gap, 0));  score_j < mu  =>  x*_j = 0
//
//   k_gap_partials  per-block fp64 partials [sum r^2, sum r.b, sum |x|, max |g|]
//   k_gap_final     one block: folds them in block order -> [primal, dual, gap, scale, ||g||_inf]
//   k_gap_screen    one thread per column: keep[b w_pad + j] = !(score_j < mu), per-block counts
//   k_gap_count     one block: n_keep = sum of the counts
//   k_gather_cols   A_out[i][c] = A(i, cols[c]) for 2-, 4- and 8-byte elements (bpgl_gather.h)
// Every reduction is a fixed-order one (wave_sum / wave_max, then the waves, then the blocks in
// index order): two calls on the same state return the same bits.  No floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bpgl_gather.h"
#include "bpgl_kernels.h"

namespace bpgl {

constexpr int kGapBlocks = kThreads;   // at most one partial per thread of k_gap_final

// res: [0] primal, [1] dual, [2] gap, [3] scale, [4] ||g||_inf, [5] n_keep
constexpr int kGapRes = 8;

// grid <= kGapBlocks blocks of kThreads; grid-stride over the m rows and the nblock * w_pad
// column slots (padding slots j >= w take no part)
__global__ __launch_bounds__(kThreads) void k_gap_partials(Params p, const double* __restrict__ g_all,
                                                           double* __restrict__ parts) {
    const long long tid = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long stride = (long long)gridDim.x * kThreads;
    double rr = 0.0, rb = 0.0, ax = 0.0, gm = 0.0;
    for (long long i = tid; i < p.m; i += stride) {
        const double r = p.r[i];
        rr = fma(r, r, rr);
        rb = fma(r, p.b[i], rb);
    }
    const long long n = (long long)p.nblock * p.wp;
    for (long long k = tid; k < n; k += stride) {
        if (k % p.wp < p.w) {
            ax += fabs(p.x[k]);
            gm = nan_max(gm, fabs(g_all[k]));
        }
    }
    rr = wave_sum(rr);
    rb = wave_sum(rb);
    ax = wave_sum(ax);
    gm = wave_max(gm);
    __shared__ double red[4][kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[0][wave] = rr; red[1][wave] = rb; red[2][wave] = ax; red[3][wave] = gm; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* dst = parts + 4ll * blockIdx.x;
        dst[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        dst[1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        dst[2] = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
        dst[3] = nan_max(nan_max(nan_max(red[3][0], red[3][1]), red[3][2]), red[3][3]);
    }
}

// one block; thread k holds partial k (nparts <= kGapBlocks = kThreads)
__global__ __launch_bounds__(kThreads) void k_gap_final(const double* __restrict__ parts, int nparts, double mu,
                                                        double* __restrict__ res) {
    const int k = threadIdx.x;
    const bool ok = k < nparts;
    double rr = ok ? parts[4ll * k] : 0.0;
    double rb = ok ? parts[4ll * k + 1] : 0.0;
    double ax = ok ? parts[4ll * k + 2] : 0.0;
    double gm = ok ? parts[4ll * k + 3] : 0.0;
    rr = wave_sum(rr);
    rb = wave_sum(rb);
    ax = wave_sum(ax);
    gm = wave_max(gm);
    __shared__ double red[4][kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[0][wave] = rr; red[1][wave] = rb; red[2][wave] = ax; red[3][wave] = gm; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    rr = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    rb = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    ax = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
    gm = nan_max(nan_max(nan_max(red[3][0], red[3][1]), red[3][2]), red[3][3]);
    const double primal = 0.5 * rr + mu * ax;
    double s = 1.0;                       // also for g = 0 and for a NaN
    if (gm > 0.0) { s = mu / gm; s = s < 1.0 ? s : 1.0; }
    const double dual = -0.5 * s * s * rr - s * rb;
    res[0] = primal;
    res[1] = dual;
    res[2] = primal - dual;
    res[3] = s;
    res[4] = gm;
    res[5] = 0.0;
}

// one thread per column slot k = b w_pad + j; counts[block] = columns kept by this block
__global__ __launch_bounds__(kThreads) void k_gap_screen(Params p, const double* __restrict__ g_all,
                                                         const double* __restrict__ res,
                                                         unsigned char* __restrict__ keep,
                                                         int* __restrict__ counts) {
    const long long k = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long n = (long long)p.nblock * p.wp;
    bool kp = false;
    if (k < n) {
        if (k % p.wp < p.w) {
            const double gap = res[2], s = res[3];
            const double gp = gap < 0.0 ? 0.0 : gap;   // a NaN stays a NaN
            const double score = s * fabs(g_all[k]) + sqrt(p.diag[k]) * sqrt(2.0 * gp);
            kp = !(score < p.mu);
        }
        keep[k] = kp ? 1 : 0;
    }
    const int cnt = __popcll(__ballot(kp));
    __shared__ int red[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// one block: res[5] = sum of the per-block counts (integers: exact in any order)
__global__ __launch_bounds__(kThreads) void k_gap_count(const int* __restrict__ counts, long long nblocks,
                                                        double* __restrict__ res) {
    long long s = 0;
    for (long long k = threadIdx.x; k < nblocks; k += kThreads) s += counts[k];
    __shared__ long long red[kThreads];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    long long tot = 0;
    for (int k = 0; k < kThreads; ++k) tot += red[k];
    res[5] = (double)tot;
}

}  // namespace bpgl

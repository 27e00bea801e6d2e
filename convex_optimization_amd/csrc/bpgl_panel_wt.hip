// The observation weights' kernels (bpgl_panel_set_row_weights) as a code object of their own:
// the WT instantiations of k_panel_reduce, k_panel_reduce_upd, k_panel_update1 and k_pgap_partials_wt, and the kernels
// only the weights need -- the validation, the weighted resets, the weight sum and the certificate's weighted product-1
// fold and centring.  As with bpgl_panel_pos.hip and bpgl_panel_pen.hip, bpgl_panel_abi.hip instantiates none of them:
// the code object it compiles to holds what it held before these existed.  The host side hands out kernel addresses
// only (bpgl_panel_wt.h).
//
// The kernel headers are included for their templates and types alone: their kernels that are not templates stay
// defined in bpgl_panel_abi.hip only.
#define BPGL_PANEL_TEMPLATES_ONLY 1
#include <hip/hip_runtime.h>

#include "bpgl_host.h"
#include "bpgl_panel_wt.h"

using namespace bpgl;
using namespace bpgl_host;

namespace {
// bpgl_panel_set_row_weights' validation: every weight finite and in [0, 1], every scoring weight finite and >= 0 (a
// NaN fails both comparisons).  One flag, set with an ordinary store by every thread that finds a bad entry (they all
// store the same value).
__global__ __launch_bounds__(kThreads) void k_panel_check_weights(const double* __restrict__ wt,
                                                                  const double* __restrict__ hold, long long n,
                                                                  int* __restrict__ bad) {
    bool b = false;
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < n; e += (long long)gridDim.x * kThreads) {
        const double v = wt[e];
        if (!(v >= 0.0) || !(v <= 1.0)) b = true;
        if (hold) {
            const double h = hold[e];
            if (!(h >= 0.0) || !(h < __builtin_inf())) b = true;
        }
    }
    if (b) *bad = 1;
}

// the scoring weights when the caller gives none: 1 where the weight is 0, else 0 (the row mask's rule)
__global__ __launch_bounds__(kThreads) void k_panel_default_hold(const double* __restrict__ wt, long long n,
                                                                 double* __restrict__ hold) {
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < n; e += (long long)gridDim.x * kThreads)
        hold[e] = wt[e] == 0.0 ? 1.0 : 0.0;
}

// per RHS (one block each): n_w = sum_i w_i in fp64 and a fixed order -- a thread's rows in index order, wave sums, the
// 4 waves in order.  (0/1 weights: an integer count, exact in any order, so it is k_panel_count_rows' value.)
__global__ __launch_bounds__(kThreads) void k_panel_sum_weights(const double* __restrict__ Wt, long long m,
                                                                double* __restrict__ nw) {
    const long long k0 = (long long)blockIdx.x * m;
    double s = 0.0;
    for (long long i = threadIdx.x; i < m; i += kThreads) s += Wt[k0 + i];
    s = wave_sum(s);
    __shared__ double red[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) nw[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// reset with weights: the caller's full B [k][m] -> Bw = w o B (where the solver and the certificate read B, so
// R0 = -w o B is exactly 0 at the zero-weight rows -- by select, so that not even the sign of that 0 depends on b) and
// Bh = B, every entry (a row can carry a weight and a scoring weight at once, so the certificate forms e against the
// full b at every row)
__global__ __launch_bounds__(kThreads) void k_panel_weight_b(const double* __restrict__ B,
                                                             const double* __restrict__ Wt, long long n,
                                                             double* __restrict__ Bw, double* __restrict__ Bh) {
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < n; e += (long long)gridDim.x * kThreads) {
        const double v = B[e];
        const double w = Wt[e];
        Bw[e] = w != 0.0 ? w * v : 0.0;
        Bh[e] = v;
    }
}

// reset with weights and the intercept (one block per RHS): bmean = sum w b / n_w (k_panel_centre_b's order), then
// Bw = w o (b - bmean) (so R0 = -w o (b - bmean), whose sum over the rows is 0) and Bh = B
__global__ __launch_bounds__(kThreads) void k_panel_centre_b_wt(const double* __restrict__ B,
                                                                const double* __restrict__ Wt, long long m,
                                                                const double* __restrict__ nw, double* __restrict__ Bw,
                                                                double* __restrict__ Bh, double* __restrict__ bmean) {
    const long long k0 = (long long)blockIdx.x * m;
    double s = 0.0;
    for (long long i = threadIdx.x; i < m; i += kThreads) s += Wt[k0 + i] * B[k0 + i];
    s = wave_sum(s);
    __shared__ double red[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const double n = nw[blockIdx.x];
    const double mean = n > 0.0 ? (((red[0] + red[1]) + red[2]) + red[3]) / n : 0.0;
    if (threadIdx.x == 0) bmean[blockIdx.x] = mean;
    for (long long i = threadIdx.x; i < m; i += kThreads) {
        const double v = B[k0 + i];
        const double d = v - mean;
        const double w = Wt[k0 + i];
        Bw[k0 + i] = w != 0.0 ? w * d : 0.0;
        Bh[k0 + i] = v;
    }
}

// the block's sum of one value per thread -> dst[blockIdx.x]: lanes, then the 4 waves in order
__device__ __forceinline__ void block_partial(double v, double* __restrict__ dst) {
    v = wave_sum(v);
    __shared__ double red[kWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) dst[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// product 1's weighted fold, one thread per (rhs, row) (k m is a multiple of kThreads and a block lies in one RHS, as
// in the masked fold): the chunks in index order, e = a_i . x - b_i against the full b (a.Bh), then
//   without the intercept: E = e, Rf = w e, and the block's scoring partial sum h e^2;
//   IC: Rf = e', the uncentred error shifted by bmean at the rows with a weight (e' = a_i . x - (b_i - bmean), the
//       stored difference of the reset, as the masked intercept fold forms it) and e itself at the zero-weight rows,
//       and the block's sum of w e' for k_pgap_icpt_mean; k_pgap_centre_wt finishes.
template <bool IC>
__global__ __launch_bounds__(kThreads) void k_pgap_fold_wt(PanelGapArgs a) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    double v = a.part[e];
    for (int c = 1; c < a.spl; ++c) v += a.part[(long long)c * a.k * a.m + e];
    const double w = a.Wt[e], bf = a.Bh[e];
    if constexpr (IC) {
        const double bm = a.bmean[e / a.m];
        const double ev = w != 0.0 ? v - (bf - bm) : v - bf;
        a.Rf[e] = ev;
        block_partial(w * ev, a.ipart);
    } else {
        const double ev = v - bf;
        a.E[e] = ev;
        a.Rf[e] = w != 0.0 ? w * ev : 0.0;   // (a +0 whatever e's sign: b at a zero-weight row reaches the score only)
        // (h e) e, not h (e e): the first add of the wave sum contracts the product into an fma, and with h in {0, 1}
        // fma(h e, e, .) is the masked fold's fma(e, e, .) -- the same bits
        block_partial((a.Hd[e] * ev) * ev, a.hpart);
    }
}

// intercept with weights, one thread per (rhs, row): with c' = sum w e' / n_w (k_pgap_icpt_mean) the centred error
// e - ebar_w = e' - c' at the rows with a weight: E = e' - c', Rf = w E.  The scored error a_i . x + beta0 - b_i is that
// same value there and (e - c') + bmean at the zero-weight rows (whose e' carries no bmean), squared directly and
// weighted by h into the block's partial.
__global__ __launch_bounds__(kThreads) void k_pgap_centre_wt(PanelGapArgs a) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long k = e / a.m;
    const double c = a.icp[k], bm = a.bmean[k];
    const double w = a.Wt[e];
    const double ec = a.Rf[e] - c;
    a.E[e] = ec;
    a.Rf[e] = w != 0.0 ? w * ec : 0.0;
    const double err = w != 0.0 ? ec : ec + bm;
    block_partial((a.Hd[e] * err) * err, a.hpart);   // (h e) e: see k_pgap_fold_wt
}
}  // namespace

namespace bpgl_wt {

ReduceFn reduce(bool icpt) { return icpt ? &k_panel_reduce<false, true, true> : &k_panel_reduce<false, false, true>; }
FusedFn fused(int U, bool icpt) {
    return dispatch<1, 2, 4>(U, [&](auto u) -> FusedFn {
        return icpt ? &k_panel_reduce_upd<decltype(u)::value, false, true, true>
                    : &k_panel_reduce_upd<decltype(u)::value, false, false, true>;
    });
}
Update1Fn update1_icpt() { return &k_panel_update1<true, true>; }
CheckFn check() { return &k_panel_check_weights; }
HoldFn default_hold() { return &k_panel_default_hold; }
SumFn sum_weights() { return &k_panel_sum_weights; }
WeightBFn weight_b() { return &k_panel_weight_b; }
CentreBFn centre_b() { return &k_panel_centre_b_wt; }
GapFn gap_fold(bool icpt) { return icpt ? &k_pgap_fold_wt<true> : &k_pgap_fold_wt<false>; }
GapFn gap_centre() { return &k_pgap_centre_wt; }
GapPartialsFn gap_partials(bool pos, bool pf) {
    if (pos) return pf ? &k_pgap_partials_wt<true, true> : &k_pgap_partials_wt<true, false>;
    return pf ? &k_pgap_partials_wt<false, true> : &k_pgap_partials_wt<false, false>;
}

}  // namespace bpgl_wt

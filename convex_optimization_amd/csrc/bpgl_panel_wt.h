// Kernel addresses of bpgl_panel_wt.hip (the observation weights' code object, bpgl_panel_set_row_weights, DESIGN.md
// section 16) for bpgl_panel_abi.hip, which launches them as it launches its own kernels.
#pragma once
#include "bpgl_panel.h"
#include "bpgl_panel_gap.h"

namespace bpgl_wt {
using ReduceFn = void (*)(bpgl::PanelParams, double*, int);                  // k_panel_reduce<false, IC, true>
using FusedFn = void (*)(bpgl::PanelParams, int, int);                       // k_panel_reduce_upd<U, false, IC, true>
using Update1Fn = void (*)(bpgl::PanelParams, int);                          // k_panel_update1<true, true>
using CheckFn = void (*)(const double*, const double*, long long, int*);     // k_panel_check_weights
using HoldFn = void (*)(const double*, long long, double*);                  // k_panel_default_hold
using SumFn = void (*)(const double*, long long, double*);                   // k_panel_sum_weights
using WeightBFn = void (*)(const double*, const double*, long long, double*, double*);   // k_panel_weight_b
using CentreBFn = void (*)(const double*, const double*, long long, const double*, double*, double*, double*);
using GapFn = void (*)(bpgl::PanelGapArgs);                                  // k_pgap_fold_wt<IC>, k_pgap_centre_wt
using GapPartialsFn = void (*)(bpgl::PanelGapArgs, double*, const double*);  // k_pgap_partials_wt<POS, PF>

// the solver's weighted fold: the two-kernel form's reduce, the fused reduce + update of U groups per block, and the
// intercept's weighted update (without the intercept the stored s^ goes through k_panel_update1<false>)
__attribute__((visibility("hidden"))) ReduceFn reduce(bool icpt);
__attribute__((visibility("hidden"))) FusedFn fused(int U, bool icpt);
__attribute__((visibility("hidden"))) Update1Fn update1_icpt();
// *bad |= 1 when an entry of wt [n] is not finite or outside [0, 1], or (hold non-null) an entry of hold [n] is not
// finite or < 0; kThreads threads per block, grid-stride
__attribute__((visibility("hidden"))) CheckFn check();
// hold [n] = 1 where wt is 0, else 0: the row mask's rule
__attribute__((visibility("hidden"))) HoldFn default_hold();
// per RHS (one block each): nw = sum_i w_i, a thread's rows in index order, wave sums, the 4 waves in order
__attribute__((visibility("hidden"))) SumFn sum_weights();
// the resets: Bw = w o B (and Bh = B, the full right-hand sides, for the certificate); with the intercept (one block per
// RHS) Bw = w o (b - bmean), bmean = sum w b / nw
__attribute__((visibility("hidden"))) WeightBFn weight_b();
__attribute__((visibility("hidden"))) CentreBFn centre_b();
// the certificate's product-1 fold, the intercept's centring (its mean is k_pgap_icpt_mean's, which reads no mask) and
// the scalar partials
__attribute__((visibility("hidden"))) GapFn gap_fold(bool icpt);
__attribute__((visibility("hidden"))) GapFn gap_centre();
__attribute__((visibility("hidden"))) GapPartialsFn gap_partials(bool pos, bool pf);
}  // namespace bpgl_wt

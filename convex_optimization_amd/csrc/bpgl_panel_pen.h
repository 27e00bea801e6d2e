// Kernel addresses of bpgl_panel_pen.hip and bpgl_panel_penpos.hip (the penalty factors' code objects, without and
// with the non-negative constraint) for bpgl_panel_abi.hip, which launches them as it launches its own kernels.
#pragma once
#include "bpgl_panel.h"
#include "bpgl_panel_gap.h"

namespace bpgl_pen {
// k_panel_pass1<..., POS, PF = true>: the third argument is the factors p [nblock][w]
using Pass1Fn = void (*)(bpgl::PanelParams, int, double*);
using GapPartialsFn = void (*)(bpgl::PanelGapArgs, double*, const double*);                             // k_pgap_partials_pf
using GapScreenFn = void (*)(bpgl::PanelGapArgs, const double*, unsigned char*, int*, const double*);   // k_pgap_screen_pf
using CheckFn = void (*)(const double*, long long, int*);                                               // k_panel_check_pen

// the fused-shrink pass 1 with the factors: k right-hand sides, mainloop form ilv, ns direction pieces, gm the
// carried-gradient form (0 plain, 1 exact + store G, 2 carried); the _pos forms add the constraint x >= 0
__attribute__((visibility("hidden"))) Pass1Fn pass1(int k, int ilv, int ns, int gm);
__attribute__((visibility("hidden"))) Pass1Fn pass1_pos(int k, int ilv, int ns, int gm);
__attribute__((visibility("hidden"))) GapPartialsFn gap_partials();
__attribute__((visibility("hidden"))) GapPartialsFn gap_partials_pos();
__attribute__((visibility("hidden"))) GapScreenFn gap_screen();
__attribute__((visibility("hidden"))) GapScreenFn gap_screen_pos();
// *bad |= 1 when an entry of pen [n] is not finite or not > 0; kThreads threads per block, grid-stride
__attribute__((visibility("hidden"))) CheckFn check();
}  // namespace bpgl_pen

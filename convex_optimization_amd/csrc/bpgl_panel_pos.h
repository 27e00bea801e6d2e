// Kernel addresses of bpgl_panel_pos.hip (the non-negative lasso's code object) for bpgl_panel_abi.hip, which
// launches them as it launches its own kernels.
#pragma once
#include "bpgl_panel.h"
#include "bpgl_panel_gap.h"

namespace bpgl_pos {
using Pass1Fn = void (*)(bpgl::PanelParams, int, double*);                                  // k_panel_pass1<..., POS = true>
using GapPartialsFn = void (*)(bpgl::PanelGapArgs, double*);                                // k_pgap_partials<true>
using GapScreenFn = void (*)(bpgl::PanelGapArgs, const double*, unsigned char*, int*);      // k_pgap_screen<true>
using ProjectFn = void (*)(float*, long long);                                              // k_panel_project_x

// the fused-shrink pass 1 with the constraint: k right-hand sides, mainloop form ilv, ns direction pieces, gm the
// carried-gradient form (0 plain, 1 exact + store G, 2 carried)
__attribute__((visibility("hidden"))) Pass1Fn pass1(int k, int ilv, int ns, int gm);
__attribute__((visibility("hidden"))) GapPartialsFn gap_partials();
__attribute__((visibility("hidden"))) GapScreenFn gap_screen();
__attribute__((visibility("hidden"))) ProjectFn project_x();   // kThreads threads per block, grid-stride
}  // namespace bpgl_pos

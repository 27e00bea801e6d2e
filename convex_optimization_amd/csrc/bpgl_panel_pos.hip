// The non-negative lasso's kernels (bpgl_panel_set_positive) as a code object of their
// own: the POS instantiations of k_panel_pass1, k_pgap_partials and k_pgap_screen, and k_panel_project_x.
// bpgl_panel_abi.hip instantiates none of them, so the code object it compiles to -- every kernel the solver
// runs with the constraint off -- holds what it held before these existed, and this one is built beside it
// (in parallel: `make -j`).  The host side hands out kernel addresses only (bpgl_panel_pos.h);
// bpgl_panel_abi.hip launches them as it launches its own.
//
// The kernel headers are included for their templates and types alone: their kernels that are not templates
// stay defined in bpgl_panel_abi.hip only.
#define BPGL_PANEL_TEMPLATES_ONLY 1
#include <hip/hip_runtime.h>

#include "bpgl_host.h"
#include "bpgl_panel_pos.h"

using namespace bpgl;
using namespace bpgl_host;

namespace {
// X <- max(X, 0) in place (n elements): bpgl_panel_reset_x0 with the constraint on, before the residual is formed
// from X.  A positive entry keeps its bits, -0 and the negatives become +0, a NaN stays.
__global__ __launch_bounds__(kThreads) void k_panel_project_x(float* __restrict__ X, long long n) {
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < n; e += (long long)gridDim.x * kThreads) {
        const float v = X[e];
        if (v < 0.0f || v == 0.0f) X[e] = 0.0f;
    }
}
}  // namespace

namespace bpgl_pos {

Pass1Fn pass1(int k, int ilv, int ns, int gm) {
    return dispatch<1, 2, 4, 8>(k / 16, [&](auto ntc) {
        return dispatch<0, 1, 2>(ilv, [&](auto ilvc) {
            return dispatch<1, 2>(ns, [&](auto nsc) {
                return dispatch<1, 2, 0>(gm, [](auto gmc) -> Pass1Fn {
                    return &k_panel_pass1<decltype(ntc)::value, 1, decltype(ilvc)::value, decltype(nsc)::value,
                                          decltype(gmc)::value, true>;
                });
            });
        });
    });
}
GapPartialsFn gap_partials() { return &k_pgap_partials<true>; }
GapScreenFn gap_screen() { return &k_pgap_screen<true>; }
ProjectFn project_x() { return &k_panel_project_x; }

}  // namespace bpgl_pos

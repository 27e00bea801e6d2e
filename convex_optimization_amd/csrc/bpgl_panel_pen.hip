// The penalty factors' kernels (bpgl_panel_set_penalty) as a code object of their own: the
// PF instantiations of k_panel_pass1, k_pgap_partials_pf and k_pgap_screen_pf without the non-negative constraint,
// and k_panel_check_pen.  (Those with the constraint are in bpgl_panel_penpos.hip, so that the two build in
// parallel.)  As with bpgl_panel_pos.hip, bpgl_panel_abi.hip instantiates none of them: the code object it
// compiles to holds what it held before these existed.  The host side hands out kernel addresses only
// (bpgl_panel_pen.h).
//
// The kernel headers are included for their templates and types alone: their kernels that are not templates
// stay defined in bpgl_panel_abi.hip only.
#define BPGL_PANEL_TEMPLATES_ONLY 1
#include <hip/hip_runtime.h>

#include "bpgl_host.h"
#include "bpgl_panel_pen.h"

using namespace bpgl;
using namespace bpgl_host;

namespace {
// bpgl_panel_set_penalty's validation: every entry finite and > 0 (a NaN fails `> 0`).  One flag, set with an
// ordinary store by every thread that finds a bad entry (they all store the same value).
__global__ __launch_bounds__(kThreads) void k_panel_check_pen(const double* __restrict__ pen, long long n,
                                                              int* __restrict__ bad) {
    bool b = false;
    for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < n; e += (long long)gridDim.x * kThreads) {
        const double v = pen[e];
        if (!(v > 0.0) || !(v < __builtin_inf())) b = true;
    }
    if (b) *bad = 1;
}
}  // namespace

namespace bpgl_pen {

Pass1Fn pass1(int k, int ilv, int ns, int gm) {
    return dispatch<1, 2, 4, 8>(k / 16, [&](auto ntc) {
        return dispatch<0, 1, 2>(ilv, [&](auto ilvc) {
            return dispatch<1, 2>(ns, [&](auto nsc) {
                return dispatch<1, 2, 0>(gm, [](auto gmc) -> Pass1Fn {
                    return &k_panel_pass1<decltype(ntc)::value, 1, decltype(ilvc)::value, decltype(nsc)::value,
                                          decltype(gmc)::value, false, true>;
                });
            });
        });
    });
}
GapPartialsFn gap_partials() { return &k_pgap_partials_pf<false>; }
GapScreenFn gap_screen() { return &k_pgap_screen_pf<false>; }
CheckFn check() { return &k_panel_check_pen; }

}  // namespace bpgl_pen

// The penalty factors' kernels with the non-negative constraint (bpgl_panel_set_penalty together with
// bpgl_panel_set_positive): the PF + POS instantiations of k_panel_pass1, k_pgap_partials_pf
// and k_pgap_screen_pf, a code object of their own beside bpgl_panel_pen.hip (see there).
#define BPGL_PANEL_TEMPLATES_ONLY 1
#include <hip/hip_runtime.h>

#include "bpgl_host.h"
#include "bpgl_panel_pen.h"

using namespace bpgl;
using namespace bpgl_host;

namespace bpgl_pen {

Pass1Fn pass1_pos(int k, int ilv, int ns, int gm) {
    return dispatch<1, 2, 4, 8>(k / 16, [&](auto ntc) {
        return dispatch<0, 1, 2>(ilv, [&](auto ilvc) {
            return dispatch<1, 2>(ns, [&](auto nsc) {
                return dispatch<1, 2, 0>(gm, [](auto gmc) -> Pass1Fn {
                    return &k_panel_pass1<decltype(ntc)::value, 1, decltype(ilvc)::value, decltype(nsc)::value,
                                          decltype(gmc)::value, true, true>;
                });
            });
        });
    });
}
GapPartialsFn gap_partials_pos() { return &k_pgap_partials_pf<true>; }
GapScreenFn gap_screen_pos() { return &k_pgap_screen_pf<true>; }

}  // namespace bpgl_pen

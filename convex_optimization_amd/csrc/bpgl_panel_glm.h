// Kernel addresses of bpgl_panel_glm.hip (the logistic model between two inner solves: bpgl_panel_glm_model and
// bpgl_panel_glm_dual) for bpgl_panel_abi.hip, which launches them as it launches its own kernels.
// The kernels take their own argument struct: PanelParams and PanelGapArgs do not grow, so no existing kernel's
// kernargs move.
#pragma once
#include <stdint.h>

namespace bpgl_glm {

constexpr int kGlmRes = 8;    // res[k]: sum om l, sum h l, sum h [miss], sum om, sum p |x|, |phi|, Newton steps, flag
constexpr int kGlmPart = 4;   // block partials of the model kernel: the first four of them
constexpr int kGlmNewtonMax = 40;

struct GlmArgs {
    long long m, n;
    int k;
    int icpt;             // the context's intercept switch: beta0 is solved for (else 0)
    const float* X;       // [k][n]           the solver's stored iterate (one feature block)
    const double* pen;    // [n]              the penalty factors, null: all ones
    const double* part;   // [spl][k][m]      product 1's chunk partials
    int spl;
    double* AX;           // [k][m]           A x, the chunks folded in chunk order
    const double* Y;      // [k][m]           labels in [0, 1]
    const double* Om;     // [k][m]           prior weights in [0, 1]
    const double* Hd;     // [k][m]           scoring weights >= 0, null: none (both scoring sums are 0)
    const int32_t* curv;  // [k]              0: Newton curvature floored at 1e-5, 1: Boehning's 1/4; null: all 0
    double* beta0;        // [k]              in: the Newton start; out: the root
    double* W;            // [k][m]           4 om v
    double* Z;            // [k][m]           eta + (y - p) / v
    double* P;            // [k][m]           sigma(eta); bpgl_panel_glm_dual reads it
    double* bpart;        // [kGlmPart][k m / 256]
    double* res;          // [k][kGlmRes]
    const double* scale;  // [k]              bpgl_panel_glm_dual: the dual scaling s
    double* dual;         // [k]              ... and D = -sum om Nh(s p + (1 - s) y)
};

using GlmFn = void (*)(GlmArgs);

// AX = the chunk partials added in chunk order (nothing subtracted); one thread per (rhs, row)
__attribute__((visibility("hidden"))) GlmFn fold();
// one block per RHS: beta0 by the safeguarded Newton iteration (a.icpt; else beta0 = 0), res[k][5..7]
__attribute__((visibility("hidden"))) GlmFn newton();
// one thread per (rhs, row): P, W, Z and the block partials
__attribute__((visibility("hidden"))) GlmFn model();
// one block per RHS: sum p |x| and the block partials folded in block order -> res[k][0..4]
__attribute__((visibility("hidden"))) GlmFn l1_final();
// one block per RHS: dual[k]
__attribute__((visibility("hidden"))) GlmFn dual_sum();

}  // namespace bpgl_glm

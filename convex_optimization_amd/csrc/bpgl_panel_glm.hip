// The logistic model's kernels (bpgl_panel_glm_model, bpgl_panel_glm_dual) as a code object of
// their own: what runs between two inner solves of the IRLS loop -- the fold of product 1 into A x, the intercept's
// Newton iteration, the link function with the working weights and response, the scalars, and the dual sum of the
// logistic certificate.  No iteration kernel has a variant here: the inner solve is the weighted lasso as it stands.
// As with bpgl_panel_wt.hip, bpgl_panel_abi.hip instantiates none of these and the host side hands out kernel
// addresses only (bpgl_panel_glm.h).
//
// All of it is fp64 on the stored fp32 x and the bf16 A widened exactly (product 1 is the certificate's).  Every sum
// has a fixed order: a thread's rows in index order, the lanes by wave_sum, the 4 waves in order, blocks in block
// order.  No floating-point atomics: two calls on the same state return the same bits.
#include <hip/hip_runtime.h>

#include "bpgl_device.h"
#include "bpgl_panel_glm.h"

using namespace bpgl;
using bpgl_glm::GlmArgs;

namespace {
constexpr double kGlmFloor = 1e-5;      // glmnet's floor of p (1 - p)
constexpr double kGlmPhiTol = 1e-14;    // Newton stops at |phi| <= this x sum om (the sums' own rounding is below it)

// sigma(eta) and l(eta; y) = log(1 + e^eta) - y eta in their overflow-safe forms
__device__ __forceinline__ double glm_sigma(double eta) {
    const double t = exp(-fabs(eta));
    return eta >= 0.0 ? 1.0 / (1.0 + t) : t / (1.0 + t);
}
__device__ __forceinline__ double glm_loss(double eta, double y) {
    return (eta > 0.0 ? eta : 0.0) + log1p(exp(-fabs(eta))) - y * eta;
}

// the block's sum of one value per thread, on every thread: lanes, then the 4 waves in order.  `red` is reused by the
// next call, hence the second barrier.
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    const double s = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return s;
}
__device__ __forceinline__ double block_max(double v, double* red) {
    v = wave_max(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    const double s = nan_max(nan_max(nan_max(red[0], red[1]), red[2]), red[3]);
    __syncthreads();
    return s;
}

// one thread per (rhs, row); k m is a multiple of kThreads (m is one of 256), so no thread is out of range
__global__ __launch_bounds__(kThreads) void k_glm_fold(GlmArgs a) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long km = (long long)a.k * a.m;
    double v = a.part[e];
    for (int c = 1; c < a.spl; ++c) v += a.part[(long long)c * km + e];
    a.AX[e] = v;
}

// One block per RHS.  phi(beta) = sum_i om_i (sigma(AX_i + beta) - y_i) is increasing in beta; with ybar = sum om y /
// sum om its root lies in [logit(ybar) - max AX, logit(ybar) - min AX] (the extremes over the rows with a weight): at
// the lower end every sigma is <= ybar, at the upper end >= ybar.  From the caller's beta0 (the bracket's midpoint
// when it lies outside) a Newton step that leaves the bracket becomes the midpoint; at most kGlmNewtonMax steps.
// Every thread holds the same beta (block_sum returns the same bits on all of them), so the branches are uniform.
// res[k][5] = the final |phi|, [6] = the steps taken, [7] = 1 when there is no finite root (sum om y = 0 or = sum om;
// beta0 is then left as it was).  Without the intercept beta0 = 0, no steps.
__global__ __launch_bounds__(kThreads) void k_glm_newton(GlmArgs a) {
    __shared__ double red[kWaves];
    const int k = blockIdx.x;
    const long long k0 = (long long)k * a.m;
    const double* __restrict__ ax = a.AX + k0;
    const double* __restrict__ om = a.Om + k0;
    const double* __restrict__ y = a.Y + k0;
    double* res = a.res + (long long)k * bpgl_glm::kGlmRes;

    double sw = 0.0, sy = 0.0, lo = -__builtin_inf(), hi = -__builtin_inf();
    for (long long i = threadIdx.x; i < a.m; i += kThreads) {
        const double w = om[i];
        sw += w;
        sy += w * y[i];
        if (w > 0.0) {
            lo = nan_max(lo, ax[i]);     // max AX
            hi = nan_max(hi, -ax[i]);    // -min AX
        }
    }
    sw = block_sum(sw, red);
    sy = block_sum(sy, red);
    lo = block_max(lo, red);
    hi = block_max(hi, red);

    // f = phi(beta), d = phi'(beta)
    auto eval = [&](double beta, double& f, double& d) {
        double fs = 0.0, ds = 0.0;
        for (long long i = threadIdx.x; i < a.m; i += kThreads) {
            const double p = glm_sigma(ax[i] + beta);
            fs += om[i] * (p - y[i]);
            ds += om[i] * (p * (1.0 - p));
        }
        f = block_sum(fs, red);
        d = block_sum(ds, red);
    };

    double beta = a.icpt ? a.beta0[k] : 0.0, f, d;
    const bool root = sy > 0.0 && sy < sw;
    int steps = 0;
    if (a.icpt && root) {
        const double lg = log(sy / (sw - sy));
        lo = lg - lo;
        hi = lg + hi;
        if (!(beta >= lo && beta <= hi)) beta = 0.5 * (lo + hi);
        for (;;) {
            eval(beta, f, d);
            if (fabs(f) <= kGlmPhiTol * sw || steps == bpgl_glm::kGlmNewtonMax) break;
            if (f > 0.0) hi = beta;
            else lo = beta;
            double nb = d > 0.0 ? beta - f / d : lo;
            if (!(nb > lo && nb < hi)) nb = 0.5 * (lo + hi);
            beta = nb;
            ++steps;
        }
    } else {
        eval(beta, f, d);
    }
    if (threadIdx.x == 0) {
        if (!a.icpt || root) a.beta0[k] = beta;
        res[5] = fabs(f);
        res[6] = (double)steps;
        res[7] = a.icpt && !root ? 1.0 : 0.0;
    }
}

// one value per thread -> dst[blockIdx.x]
__device__ __forceinline__ void block_partial(double v, double* red, double* __restrict__ dst) {
    const double s = block_sum(v, red);
    if (threadIdx.x == 0) dst[blockIdx.x] = s;
}

// one thread per (rhs, row); a block lies in one RHS.  eta = AX + beta0, p = sigma(eta), v = max(p (1 - p), 1e-5) or
// 1/4 (curv), W = 4 om v, Z = eta + (y - p) / v; the block's partials of om l, h l, h [(p > 1/2) != (y > 1/2)], om.
__global__ __launch_bounds__(kThreads) void k_glm_model(GlmArgs a) {
    __shared__ double red[kWaves];
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int k = (int)(e / a.m);
    const double eta = a.AX[e] + a.beta0[k];
    const double y = a.Y[e], om = a.Om[e];
    const double h = a.Hd ? a.Hd[e] : 0.0;
    const double p = glm_sigma(eta);
    const bool bound = a.curv && a.curv[k] != 0;
    const double pq = p * (1.0 - p);
    const double v = bound ? 0.25 : (pq > kGlmFloor ? pq : kGlmFloor);
    a.P[e] = p;
    a.W[e] = (4.0 * om) * v;
    a.Z[e] = eta + (y - p) / v;
    const double l = glm_loss(eta, y);
    const long long nb = (long long)gridDim.x;
    block_partial(om * l, red, a.bpart);
    block_partial(h * l, red, a.bpart + nb);
    block_partial(((p > 0.5) != (y > 0.5)) ? h : 0.0, red, a.bpart + 2 * nb);
    block_partial(om, red, a.bpart + 3 * nb);
}

// one block per RHS: sum_j p_j |x_j| (a thread's columns in index order, lanes, waves), and the model's block
// partials added in block order by thread 0 -> res[k][0..4]
__global__ __launch_bounds__(kThreads) void k_glm_l1_final(GlmArgs a) {
    __shared__ double red[kWaves];
    const int k = blockIdx.x;
    const float* __restrict__ x = a.X + (long long)k * a.n;
    double s = 0.0;
    for (long long j = threadIdx.x; j < a.n; j += kThreads)
        s += a.pen ? a.pen[j] * fabs((double)x[j]) : fabs((double)x[j]);
    s = block_sum(s, red);
    if (threadIdx.x != 0) return;
    const long long nbr = a.m / kThreads, nb = nbr * a.k;
    double* res = a.res + (long long)k * bpgl_glm::kGlmRes;
    for (int q = 0; q < bpgl_glm::kGlmPart; ++q) {
        const double* src = a.bpart + q * nb + (long long)k * nbr;
        double t = 0.0;
        for (long long b = 0; b < nbr; ++b) t += src[b];
        res[q] = t;
    }
    res[4] = s;
}

// one block per RHS: D = -sum_i om_i Nh(s p_i + (1 - s) y_i), Nh(t) = t log t + (1 - t) log(1 - t) with 0 log 0 = 0
__global__ __launch_bounds__(kThreads) void k_glm_dual(GlmArgs a) {
    __shared__ double red[kWaves];
    const int k = blockIdx.x;
    const long long k0 = (long long)k * a.m;
    const double s = a.scale[k];
    double acc = 0.0;
    for (long long i = threadIdx.x; i < a.m; i += kThreads) {
        const double t = s * a.P[k0 + i] + (1.0 - s) * a.Y[k0 + i];
        const double u = 1.0 - t;
        const double nh = (t > 0.0 ? t * log(t) : 0.0) + (u > 0.0 ? u * log(u) : 0.0);
        acc += a.Om[k0 + i] * nh;
    }
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) a.dual[k] = -acc;
}
}  // namespace

namespace bpgl_glm {
GlmFn fold() { return &k_glm_fold; }
GlmFn newton() { return &k_glm_newton; }
GlmFn model() { return &k_glm_model; }
GlmFn l1_final() { return &k_glm_l1_final; }
GlmFn dual_sum() { return &k_glm_dual; }
}  // namespace bpgl_glm

// bpgl panel ABI -- k right-hand sides on bf16 A (BASELINE configs[4]): the
// bpgl_panel_* entry points of include/bpgl.h over the MFMA kernels of
// bpgl_panel.h.  Same conventions as bpgl.hip: caller-owned device memory,
// validated shapes, negative codes + bpgl_last_error() on failure.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/bpgl.h"
#include "bpgl_gather.h"
#include "bpgl_host.h"
#include "bpgl_panel.h"
#include "bpgl_panel_gap.h"
#include "bpgl_panel_pos.h"
#include "bpgl_panel_pen.h"
#include "bpgl_panel_wt.h"
#include "bpgl_panel_glm.h"

using namespace bpgl;
using namespace bpgl_host;

// ===========================================================================
// panel path (k right-hand sides, bf16 A, MFMA): BASELINE configs[4]
// ===========================================================================
constexpr int kPanelKinds = 5;   // pass1, pass2, reduce, step, update

// byte offsets of the scratch regions (panel_layout), in the order they are laid out
struct PanelLayout {
    int64_t st, Rh, Rl, Dh, Dl, X, Ax, B, R, diag, rec, Sslab, S, norms, lsp, mu, gamma, err_rhs, cnt, ready, lsdone, Gc,
        Sh, Ec, At, A1t, gpart, gparts, gcounts, gres, W, Bh, ghold, lss, cshift, nw, bmean, gipart, gicp, pen, Wt, Hd, gE,
        glmAX, glmpart, glmres, glmsd, total;
};

struct bpgl_panel {
    int device = 0;
    int64_t m = 0, n = 0, w = 0;
    int32_t nblock = 1, k = 0, kchunks = 1;
    hipStream_t stream = nullptr;
    bool own_stream = false, bound = false, have_diag = false, solver = false;
    PanelParams p{};
    hipGraphExec_t gexec = nullptr;
    KernelTimes<kPanelKinds> tm;   // step: folded into reduce, never recorded
    int interleave[2] = {2, -1};  // mainloop variant per pass (tuning knobs; -1: the measured default, panel_ilv)
    int dsplit = 1;               // bf16 pieces of the solver's direction (d_split knob; 1 since round 4)
    int defer_x = 1;              // one block: x += gamma D' in the next pass-1 epilogue ("defer_x" knob; round 4 default)
    int carry_g = 1;              // carried gradient, one feature block ("carry_g" knob; ignored for nblock > 1)
    int64_t g_period = 64;        // exact gradient every g_period iterations ("g_refresh" knob)
    int gm_cur = 0;               // pass-1 form of the launch being enqueued: 0 plain, 1 exact + store G, 2 carried
    hipGraphExec_t gexec_ref = nullptr;   // carry_g: a graph whose first iteration is the exact-gradient one
    int fuse_update = 1;          // one block, x deferred: reduce + line search + R update in one launch ("fuse_update")
    int fuse_ok = 0;              // ... and the shape and occupancy admit it (panel_fused_geo, set at bind)
    int fuse_cus = 0;             // the CUs that check counted (the stream's CU mask, or the device)
    int fuse_grid = 1024;         // its grid: at most this many blocks, k x G ("fuse_grid": 256, 512 or 1024;
                                  // 1024 measured best with 512, +0.4 % over 256: profiles/r05/panel_fused)
    int64_t t_host = 0;           // iterations enqueued since the last reset
    int64_t n_exact = 0;          // carried gradient: exact-gradient iterations since the last reset
    hipEvent_t gap_ev[3] = {};    // bpgl_panel_gap: before product 1, between the products, after product 2
    int64_t gap_ns[2] = {};       // the last call's two products (each with its fold), stats "gap_prod1_ns" / "gap_prod2_ns"
    bool masked = false;          // a mask is installed (the caller's, or the intercept's all-ones one): the MK kernel variants run
    bool user_mask = false;       // ... and it is the caller's (bpgl_panel_set_row_mask)
    bool icpt = false;            // bpgl_panel_set_intercept: the intercept (IC) kernel variants run (always with `masked`)
    bool positive = false;        // bpgl_panel_set_positive: x >= 0 (the POS pass-1 variants, the one-sided certificate)
    bool penalty = false;         // bpgl_panel_set_penalty: per-column l1 weights (the PF pass-1 variants, the weighted certificate)
    bool weighted = false;        // bpgl_panel_set_row_weights: observation weights (the WT fold variants; never with `user_mask`,
                                  // and `masked` is then false: the weights stand where the mask would)
    bool icpt_valid = false;      // a bpgl_panel_gap has run since the last reset: icpt_host is its beta0
    std::vector<double> icpt_host;
    bool have_x = false;          // a reset has run since bind: X is an iterate (bpgl_panel_glm_model needs one)
    char* scratch = nullptr;      // the caller's scratch and its layout (bpgl_panel_bind)
    PanelLayout L{};
    template <typename T>
    T* at(int64_t off) const { return reinterpret_cast<T*>(scratch + off); }   // the region at L.<name>
    int64_t ldr() const { return m; }
    int64_t ldd() const { return w; }
};

namespace {

// NT, the 16-wide RHS tiles of the k right-hand sides (16, 32, 64 or 128: bpgl_panel_create)
template <typename F>
auto dispatch_nt(int k, F&& f) { return dispatch<1, 2, 4, 8>(k / 16, f); }

// bpgl_panel_gap: the chunks of a product's reduction (`stages` 32-deep stages, `tiles` 64-output
// tiles) -- doubled while the product has fewer than kPgBlocksTarget blocks and a chunk keeps two
// stages.  A function of the shape alone.
int pgap_split(int64_t tiles, int64_t stages) {
    int spl = 1;
    while (tiles * spl < kPgBlocksTarget && stages % (2 * spl) == 0 && stages / (2 * spl) >= 2) spl *= 2;
    return spl;
}
int pgap_nparts(const bpgl_panel* c) {
    return (int)std::min<int64_t>(cdiv(std::max<int64_t>(c->m, c->n), 4 * kThreads), kPgPartBlocks);
}
template <int PROD>
int pgap_prod(bpgl_panel* c, const PanelGapArgs& a, dim3 grid) {
    const dim3 blk(kThreads);
    const auto prod = dispatch_nt(c->k, [](auto nt) { return &k_pgap_prod<decltype(nt)::value, PROD>; });
    hipLaunchKernelGGL(prod, grid, blk, 0, c->stream, a);
    LAUNCH_CHECK("k_pgap_prod");
    const dim3 fgrid((unsigned)cdiv((int64_t)c->k * (PROD == 1 ? c->m : c->n), kThreads));
    if (PROD == 1 && c->weighted) hipLaunchKernelGGL(bpgl_wt::gap_fold(c->icpt), fgrid, blk, 0, c->stream, a);
    else if (PROD == 1 && c->icpt) hipLaunchKernelGGL((k_pgap_fold<1, true, true>), fgrid, blk, 0, c->stream, a);
    else if (PROD == 1 && c->masked) hipLaunchKernelGGL((k_pgap_fold<1, true>), fgrid, blk, 0, c->stream, a);
    else hipLaunchKernelGGL((k_pgap_fold<PROD, false>), fgrid, blk, 0, c->stream, a);
    LAUNCH_CHECK("k_pgap_fold");
    if (PROD == 1 && c->icpt) {   // the fold left the uncentred e: its in-row mean per RHS, then P_w e and the held-out squares
        hipLaunchKernelGGL(k_pgap_icpt_mean, dim3((unsigned)c->k), blk, 0, c->stream, a, (long long)(c->m / kThreads));
        LAUNCH_CHECK("k_pgap_icpt_mean");
        if (c->weighted) hipLaunchKernelGGL(bpgl_wt::gap_centre(), fgrid, blk, 0, c->stream, a);
        else hipLaunchKernelGGL(k_pgap_centre, fgrid, blk, 0, c->stream, a);
        LAUNCH_CHECK("k_pgap_centre");
    }
    return 0;
}
PanelLayout panel_layout(const bpgl_panel* c) {
    Carve k;
    PanelLayout L;
    const int64_t km = (int64_t)c->k * c->m, kw = (int64_t)c->k * c->w;
    L.st = k.take(sizeof(PanelState));
    L.Rh = k.take(2 * (int64_t)c->k * c->ldr());
    L.Rl = k.take(2 * (int64_t)c->k * c->ldr());
    L.Dh = k.take(2 * (int64_t)c->k * c->ldd());
    L.Dl = k.take(2 * (int64_t)c->k * c->ldd());
    L.X = k.take(4 * kw * c->nblock);
    L.Ax = k.take(8 * km * c->nblock);
    L.B = k.take(8 * km);
    L.R = k.take(8 * km);
    L.diag = k.take(8 * c->n);
    L.rec = k.take(8 * c->n);
    L.Sslab = k.take(4 * km * c->kchunks);
    L.S = k.take(8 * km);
    L.norms = k.take(8 * 4 * (c->w / kPanelRows) * c->k);
    L.lsp = k.take(8 * 2 * cdiv(c->m, kLspRows) * c->k);
    L.mu = k.take(8 * c->k);
    L.gamma = k.take(8 * c->k);
    L.err_rhs = k.take(8 * c->k);
    L.cnt = k.take(8 * (int64_t)c->k);
    L.ready = k.take(8 * (int64_t)c->k);
    L.lsdone = k.take(8);
    // the carried gradient's state (one feature block only; ADVICE r04: not reserved otherwise)
    const bool carry = c->nblock == 1;
    L.Gc = k.take(carry ? 4 * kw : 0);                           // the carried gradient (fp32)
    L.Sh = k.take(carry ? 2 * (int64_t)c->k * c->ldr() : 0);     // the carried product's bf16 operand
    L.Ec = k.take(carry ? 4 * km : 0);                           // its rounding error, fed into the next one (fp32)
    L.At = k.take(2 * c->m * c->n);                              // pass 2's tiled copy of A (bf16)
    L.A1t = k.take(2 * c->m * c->n);                             // pass 1's tiled copy of A (bf16)
    // bpgl_panel_gap (bpgl_panel_gap.h): the two products' chunk partials (one buffer, the larger), the
    // per-RHS partials, the screen's per-block counts and the results.  Laid out last: nothing before
    // them moves.
    const int64_t sp1 = pgap_split(c->m / kPgTile, c->n / kPgK), sp2 = pgap_split(c->n / kPgTile, c->m / kPgK);
    // bpgl_panel_reset_x0 with nblock > 1 runs product 1 with nblock x pgap_split(m / 64, w / 32)
    // block-aligned chunks into the same buffer: it grows only where that exceeds the certificate's need
    const int64_t spw = c->nblock > 1 ? (int64_t)c->nblock * pgap_split(c->m / kPgTile, c->w / kPgK) : 0;
    L.gpart = k.take(8 * (int64_t)c->k * std::max(std::max(sp1 * c->m, sp2 * c->n), spw * c->m));
    L.gparts = k.take(8 * (int64_t)kPgPart * pgap_nparts(c) * c->k);
    L.gcounts = k.take(4 * (int64_t)c->k * cdiv(c->n, kThreads));
    L.gres = k.take(8 * (int64_t)kPgRes * c->k);
    // the row mask (bpgl_panel_set_row_mask), the held-out part of B and the certificate's held-out
    // partials (one per 256-thread fold block).  Laid out after everything else, as the pieces above were.
    L.W = k.take(km);
    L.Bh = k.take(8 * km);
    L.ghold = k.take(8 * (km / kThreads));
    // the intercept (bpgl_panel_set_intercept): the line search's sum-s partials and c, the in-row counts, the
    // in-row means of b, and the certificate's in-row partials and its c' / beta0.  Again after everything else.
    L.lss = k.take(8 * cdiv(c->m, kLspRows) * c->k);
    L.cshift = k.take(8 * (int64_t)c->k);
    L.nw = k.take(8 * (int64_t)c->k);
    L.bmean = k.take(8 * (int64_t)c->k);
    L.gipart = k.take(8 * (km / kThreads));
    L.gicp = k.take(8 * 2 * (int64_t)c->k);
    // the penalty factors (bpgl_panel_set_penalty): p [n] fp64 and, behind them, the validation kernel's flag.
    // After everything else once more.
    L.pen = k.take(8 * c->n + 256);
    // the observation weights (bpgl_panel_set_row_weights): w and the scoring weights h [k][m] fp64, the validation
    // kernel's flag behind them, and the certificate's unweighted e.  After everything else once more.
    L.Wt = k.take(8 * km);
    L.Hd = k.take(8 * km + 256);
    L.gE = k.take(8 * km);
    // the logistic model (bpgl_panel_glm_model / _dual): A x, the model kernel's block partials, the scalars, and the
    // dual call's scale and result.  After everything else once more.
    L.glmAX = k.take(8 * km);
    L.glmpart = k.take(8 * (int64_t)bpgl_glm::kGlmPart * (km / kThreads));
    L.glmres = k.take(8 * (int64_t)bpgl_glm::kGlmRes * c->k);
    L.glmsd = k.take(8 * 2 * (int64_t)c->k);
    L.total = k.off;
    return L;
}

// ns: bf16 pieces of the direction (pass 1's epilogue writes it, pass 2 reads it): the
// solver's d_split knob, 2 for the API products (bpgl_panel_mtm / _mm)
// the mainloop variant of a pass: the knob, or the measured default -- pass 1: 2 (software-pipelined);
// pass 2: 2 with the bf16 direction alone at k >= 64 (+0.7 % at k = 64 and 128), else 1 (k = 32 and the
// hi + lo direction; profiles/r04/ilv)
int panel_ilv(const bpgl_panel* c, int which, int ns) {
    const int v = c->interleave[which];
    if (v >= 0) return v;
    return which == 0 ? 2 : (ns == 1 && c->k >= 64 ? 2 : 1);
}
// pass 1 (which 0; mode 0: G to `out`, the API product; mode 1: the fused shrink in the form gm_cur names:
// 0 plain, 1 exact + store G, 2 carried) or pass 2 (which 1) of block `fixed_block` (-1: the solver's)
int panel_launch(bpgl_panel* c, int which, int fixed_block, double* out, int mode, int ns) {
    return dispatch_nt(c->k, [&](auto ntc) {
        return dispatch<0, 1, 2>(panel_ilv(c, which, ns), [&](auto ilvc) {
            return dispatch<1, 2>(ns, [&](auto nsc) {
                constexpr int NT = decltype(ntc)::value, ILV = decltype(ilvc)::value, NS = decltype(nsc)::value;
                if (which == 0) {
                    void (*pass1)(PanelParams, int, double*) = &k_panel_pass1<NT, 0, ILV, 2>;
                    if (mode)
                        pass1 = dispatch<1, 2, 0>(c->gm_cur, [](auto gm) {
                            return &k_panel_pass1<NT, 1, ILV, NS, decltype(gm)::value>;
                        });
                    if (mode && c->positive)   // the POS variant of the same form, from its own code object
                        pass1 = bpgl_pos::pass1(c->k, ILV, NS, c->gm_cur);
                    double* arg3 = out;
                    if (mode && c->penalty) {   // the PF variants: the factors travel where the API product's G does
                        pass1 = c->positive ? bpgl_pen::pass1_pos(c->k, ILV, NS, c->gm_cur)
                                            : bpgl_pen::pass1(c->k, ILV, NS, c->gm_cur);
                        arg3 = c->at<double>(c->L.pen);
                    }
                    hipLaunchKernelGGL(pass1, dim3((unsigned)(c->w / kPanelRows)), dim3(PanelGeo<NT, 2>::T), 0,
                                       c->stream, c->p, fixed_block, arg3);
                    LAUNCH_CHECK("k_panel_pass1");
                } else {
                    hipLaunchKernelGGL((k_panel_pass2<NT, ILV, NS>), dim3((unsigned)((c->m / kPanelRows) * c->kchunks)),
                                       dim3(PanelGeo<NT, NS>::T), 0, c->stream, c->p, fixed_block);
                    LAUNCH_CHECK("k_panel_pass2");
                }
                return 0;
            });
        });
    });
}
bool panel_carry(const bpgl_panel* c) { return c->carry_g && c->nblock == 1; }
int panel_pass(bpgl_panel* c, int which) { return panel_launch(c, which, -1, nullptr, 1, c->dsplit); }
// k_panel_reduce_upd's geometry: G blocks per RHS of U 1024-row groups each (k x G <= fuse_grid
// blocks); false when the shape does not admit it (m a multiple of 1024, U in {1, 2, 4})
bool panel_fused_geo(const bpgl_panel* c, int* G, int* U) {
    if (c->m % kLspRows) return false;
    const int64_t groups = c->m / kLspRows;
    const int64_t g = std::min<int64_t>(std::max<int64_t>(1, c->fuse_grid / c->k), groups);
    if (groups % g) return false;
    const int64_t u = groups / g;
    if (u != 1 && u != 2 && u != 4) return false;
    *G = (int)g;
    *U = (int)u;
    return true;
}
// the k_panel_reduce_upd variant of a geometry: what panel_fuse_check asks the occupancy of is what
// panel_reduce_upd launches
using PanelFusedFn = void (*)(PanelParams, int, int);
PanelFusedFn panel_fused_fn(int U, bool masked, bool icpt, bool weighted) {
    if (weighted) return bpgl_wt::fused(U, icpt);   // the WT variants, from their own code object
    return dispatch<1, 2, 4>(U, [&](auto u) -> PanelFusedFn {
        if (icpt) return &k_panel_reduce_upd<decltype(u)::value, true, true>;
        return masked ? &k_panel_reduce_upd<decltype(u)::value, true> : &k_panel_reduce_upd<decltype(u)::value, false>;
    });
}
int panel_reduce_upd(bpgl_panel* c, int cflag) {
    int G = 0, U = 0;
    (void)panel_fused_geo(c, &G, &U);
    hipLaunchKernelGGL(panel_fused_fn(U, c->masked, c->icpt, c->weighted), dim3((unsigned)(c->k * G)), dim3(kThreads), 0, c->stream, c->p,
                       cflag, G);
    LAUNCH_CHECK("k_panel_reduce_upd");
    return 0;
}
// the fused reduce + update needs its k x G blocks resident together: on the CUs the stream may use
// (a CU-masked stream from bpgl_stream_create gets fewer), else the two-kernel form runs.  The
// occupancy is that of the variant that will run (masked, weighted or neither, with the intercept or not), so
// bpgl_panel_set_row_mask, bpgl_panel_set_row_weights and bpgl_panel_set_intercept repeat it.
void panel_fuse_check(bpgl_panel* c) {
    int G = 0, U = 0, nb = 0;
    c->fuse_ok = 0;
    c->fuse_cus = 0;
    if (!panel_fused_geo(c, &G, &U)) return;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)panel_fused_fn(U, c->masked, c->icpt, c->weighted), kThreads, 0) !=
        hipSuccess) {
        (void)hipGetLastError();   // the query's own error only
        return;
    }
    c->fuse_cus = usable_cus(c->stream, c->device);
    if ((int64_t)nb * c->fuse_cus >= (int64_t)c->k * G) c->fuse_ok = 1;
}
// mode 0 (bpgl_panel_mm) is always the unmasked fold
int panel_reduce(bpgl_panel* c, double* out, int mode) {
    const dim3 grid((unsigned)(c->k * cdiv(c->m, kLspRows)));
    if (mode && c->weighted) hipLaunchKernelGGL(bpgl_wt::reduce(c->icpt), grid, dim3(kThreads), 0, c->stream, c->p, out, mode);
    else if (mode && c->icpt) hipLaunchKernelGGL((k_panel_reduce<true, true>), grid, dim3(kThreads), 0, c->stream, c->p, out, mode);
    else if (mode && c->masked) hipLaunchKernelGGL(k_panel_reduce<true>, grid, dim3(kThreads), 0, c->stream, c->p, out, mode);
    else hipLaunchKernelGGL(k_panel_reduce<false>, grid, dim3(kThreads), 0, c->stream, c->p, out, mode);
    LAUNCH_CHECK("k_panel_reduce");
    return 0;
}
// exact: with the carried gradient, this iteration computes G = A^T R exactly (and stores it);
// split_r: the update writes R's hi / lo images (with the carried gradient only the exact pass 1 reads
// them, so only an iteration followed by an exact one needs to)
int panel_iteration(bpgl_panel* c, int64_t it, bool exact = false, bool split_r = true) {
    int rc;
    c->gm_cur = panel_carry(c) ? (exact ? 1 : 2) : 0;
    // the update's carried-gradient operand: 0 none, 1 V = E + gamma S, 2 V = gamma S (G is exact now);
    // + 4: skip R's hi / lo images
    const int cflag = (c->gm_cur == 0 ? 0 : c->gm_cur == 1 ? 2 : 1) | (c->gm_cur && !split_r ? 4 : 0);
    rc = c->tm.timed(0, it, [&] { return panel_pass(c, 0); });
    c->gm_cur = 0;
    if (rc) return rc;
    if ((rc = c->tm.timed(1, it, [&] { return panel_pass(c, 1); }))) return rc;
    if (c->nblock == 1 && c->defer_x && c->fuse_update && c->fuse_ok)   // reduce + line search + R update
        return c->tm.timed(2, it, [&] { return panel_reduce_upd(c, cflag); });
    // its last block per RHS runs the line search
    if ((rc = c->tm.timed(2, it, [&] { return panel_reduce(c, c->p.S, 1); }))) return rc;
    return c->tm.timed(4, it, [&] {
        if (c->nblock == 1 && c->defer_x) {   // R only; x += gamma D' rides on the next pass-1 epilogue (or the flush)
            const dim3 ug((unsigned)std::min<int64_t>(cdiv((int64_t)c->k * c->m / 4, kThreads), 8192));
            if (c->icpt && c->weighted) hipLaunchKernelGGL(bpgl_wt::update1_icpt(), ug, dim3(kThreads), 0, c->stream, c->p, cflag);
            else if (c->icpt) hipLaunchKernelGGL(k_panel_update1<true>, ug, dim3(kThreads), 0, c->stream, c->p, cflag);
            else hipLaunchKernelGGL(k_panel_update1<false>, ug, dim3(kThreads), 0, c->stream, c->p, cflag);
        } else {
            const int64_t n = (int64_t)c->k * c->w / 8 + (int64_t)c->k * c->m / 4;   // work units
            const dim3 ug((unsigned)std::min<int64_t>(cdiv(n, kThreads), 8192));
            const bool nb1 = c->nblock == 1;
            const auto update = dispatch<1, 2>(c->dsplit, [&](auto ds) {
                return nb1 ? &k_panel_update<decltype(ds)::value, true> : &k_panel_update<decltype(ds)::value, false>;
            });
            hipLaunchKernelGGL(update, ug, dim3(kThreads), 0, c->stream, c->p, cflag);
        }
        LAUNCH_CHECK("k_panel_update");
        return 0;
    });
}
// src [k][len] fp64 -> hi/lo images [k][ld]
int panel_split(bpgl_panel* c, const double* src, int64_t len, int64_t ld, __bf16* hi, __bf16* lo, double sign,
                double* copy) {
    const int64_t n = (int64_t)c->k * len;
    hipLaunchKernelGGL(k_panel_split, dim3((unsigned)std::min<int64_t>(cdiv(n, kThreads), 2048)), dim3(kThreads), 0,
                       c->stream, src, n, len, ld, hi, lo, sign, copy);
    LAUNCH_CHECK("k_panel_split");
    return 0;
}
void drop_graphs(bpgl_panel* c) {
    if (c->gexec) { (void)hipGraphExecDestroy(c->gexec); c->gexec = nullptr; }
    if (c->gexec_ref) { (void)hipGraphExecDestroy(c->gexec_ref); c->gexec_ref = nullptr; }
}

// the certificate's view of the context: what both of its products and bpgl_panel_reset_x0's product 1 read
PanelGapArgs pgap_args(const bpgl_panel* c) {
    PanelGapArgs a{};
    a.A = c->p.A;
    a.lda = c->p.lda;
    a.m = c->m;
    a.n = c->n;
    a.w = c->w;
    a.nblock = c->nblock;
    a.k = c->k;
    a.X = c->p.X;
    a.B = c->p.B;
    a.R = c->p.R;
    a.diag = c->p.diag;
    a.mu = c->p.mu;
    a.part = c->at<double>(c->L.gpart);
    a.W = c->masked ? c->p.W : nullptr;
    a.Bh = c->at<double>(c->L.Bh);
    a.hpart = c->at<double>(c->L.ghold);
    a.ipart = c->at<double>(c->L.gipart);
    a.icp = c->at<double>(c->L.gicp);
    a.nw = c->p.nw;
    a.bmean = c->at<double>(c->L.bmean);
    a.Wt = c->weighted ? c->p.Wt : nullptr;
    a.Hd = c->at<double>(c->L.Hd);
    a.E = c->at<double>(c->L.gE);
    return a;
}
// bpgl_panel_reset_x0: R = A X - B (w o (A X - B) with a row mask, P_w(A X - B) with the intercept) from the
// stored X through the certificate's product 1, and with nblock > 1 also Ax[b] = A_b x_b
int panel_warm_residual(bpgl_panel* c) {
    PanelGapArgs a = pgap_args(c);
    if (c->nblock == 1) {   // the certificate's own chunking and fold, written to the solver's R
        a.Rf = c->p.R;
        a.spl = pgap_split(c->m / kPgTile, c->n / kPgK);
        a.chunk = c->n / kPgK / a.spl;
        return pgap_prod<1>(c, a, dim3((unsigned)(c->m / kPgTile * a.spl)));
    }
    // chunks aligned to the feature blocks: spb per block, chunk q inside block q / spb
    const int spb = pgap_split(c->m / kPgTile, c->w / kPgK);
    a.spl = c->nblock * spb;
    a.chunk = c->w / kPgK / spb;
    const dim3 blk(kThreads), grid((unsigned)(c->m / kPgTile * a.spl));
    const auto prod = dispatch_nt(c->k, [](auto nt) { return &k_pgap_prod<decltype(nt)::value, 1>; });
    hipLaunchKernelGGL(prod, grid, blk, 0, c->stream, a);
    LAUNCH_CHECK("k_pgap_prod");
    const dim3 fgrid((unsigned)cdiv((int64_t)c->k * c->m, kThreads));
    if (c->masked) hipLaunchKernelGGL(k_pgap_fold_ax<true>, fgrid, blk, 0, c->stream, a, spb, c->p.Ax, c->p.R);
    else hipLaunchKernelGGL(k_pgap_fold_ax<false>, fgrid, blk, 0, c->stream, a, spb, c->p.Ax, c->p.R);
    LAUNCH_CHECK("k_pgap_fold_ax");
    return 0;
}

// the mask in effect: the caller's, else (the intercept on) all ones, else none; with the intercept the
// in-row counts too.  Then the fused form's occupancy check for the variant that will run.
// With observation weights (never with a caller's mask) no byte mask is in effect: the WT variants read p.Wt, and the
// intercept's n_w is their sum.
int panel_install_mask(bpgl_panel* c) {
    unsigned char* W = c->at<unsigned char>(c->L.W);
    c->p.Wt = c->weighted ? c->at<double>(c->L.Wt) : nullptr;
    if (c->weighted) {
        c->masked = false;
        c->p.W = nullptr;
        if (c->icpt) {
            hipLaunchKernelGGL(bpgl_wt::sum_weights(), dim3((unsigned)c->k), dim3(kThreads), 0, c->stream, c->p.Wt,
                               (long long)c->m, c->at<double>(c->L.nw));
            LAUNCH_CHECK("k_panel_sum_weights");
        }
        c->solver = false;
        drop_graphs(c);
        panel_fuse_check(c);
        return 0;
    }
    if (c->icpt && !c->user_mask) HIP_TRY(hipMemsetAsync(W, 1, (int64_t)c->k * c->m, c->stream));
    c->masked = c->user_mask || c->icpt;
    c->p.W = c->masked ? W : nullptr;
    if (c->icpt) {
        hipLaunchKernelGGL(k_panel_count_rows, dim3((unsigned)c->k), dim3(kThreads), 0, c->stream, W, (long long)c->m,
                           c->at<double>(c->L.nw));
        LAUNCH_CHECK("k_panel_count_rows");
    }
    c->solver = false;   // B is stored masked and the graphs bake the kernel variant in: a reset must follow
    drop_graphs(c);
    panel_fuse_check(c);   // the occupancy of the variant that will run
    return 0;
}
int panel_run_diag(bpgl_panel* c) {
    const dim3 grid((unsigned)cdiv(c->n, 512));
    if (c->icpt) hipLaunchKernelGGL(k_panel_diag_centred, grid, dim3(kThreads), 0, c->stream, c->p,
                                    const_cast<double*>(c->p.diag), const_cast<double*>(c->p.rec));
    else hipLaunchKernelGGL(k_panel_diag, grid, dim3(kThreads), 0, c->stream, c->p,
                            const_cast<double*>(c->p.diag), const_cast<double*>(c->p.rec));
    LAUNCH_CHECK("k_panel_diag");
    c->have_diag = true;
    return 0;
}

int panel_ready(const bpgl_panel* c) {
    if (!c) return fail(BPGL_E_ARG, "null panel context");
    if (!c->bound) return fail(BPGL_E_STATE, "bpgl_panel_bind has not been called");
    return 0;
}
// the logistic model's view of the context (bpgl_panel_glm.h); the caller's pointers are filled in by the two calls
bpgl_glm::GlmArgs glm_args(const bpgl_panel* c) {
    bpgl_glm::GlmArgs g{};
    g.m = c->m;
    g.n = c->n;
    g.k = c->k;
    g.icpt = c->icpt ? 1 : 0;
    g.X = c->p.X;
    g.pen = c->penalty ? c->at<double>(c->L.pen) : nullptr;
    g.part = c->at<double>(c->L.gpart);
    g.AX = c->at<double>(c->L.glmAX);
    g.bpart = c->at<double>(c->L.glmpart);
    g.res = c->at<double>(c->L.glmres);
    g.scale = c->at<double>(c->L.glmsd);
    g.dual = c->at<double>(c->L.glmsd) + c->k;
    return g;
}
}  // namespace

extern "C" {

int bpgl_panel_create(bpgl_panel** out, int device, int64_t m, int64_t n, int32_t nblock, int32_t nrhs,
                      int32_t kchunks, void* hip_stream) {
    if (!out) return fail(BPGL_E_ARG, "out is null");
    *out = nullptr;
    if (nrhs != 16 && nrhs != 32 && nrhs != 64 && nrhs != 128)
        return fail(BPGL_E_ARG, "nrhs must be 16, 32, 64 or 128 (got %d)", nrhs);
    if (nblock <= 0 || n % nblock) return fail(BPGL_E_ARG, "n must be divisible by nblock");
    const int64_t w = n / nblock;
    if (m <= 0 || m % kPanelRows) return fail(BPGL_E_ARG, "m (%lld) must be a positive multiple of %d", (long long)m,
                                              kPanelRows);
    if (w <= 0 || w % kPanelRows) return fail(BPGL_E_ARG, "block width (%lld) must be a positive multiple of %d",
                                              (long long)w, kPanelRows);
    if (kchunks <= 0) {   // one pass-2 tile per CU (256), chunk width a multiple of two 64-deep stages
        kchunks = (int32_t)std::max<int64_t>(1, std::min<int64_t>(w / (2 * kPanelK), 256 / (m / kPanelRows)));
        while (kchunks > 1 && w % ((int64_t)kchunks * 2 * kPanelK)) --kchunks;
    }
    if (w % ((int64_t)kchunks * kPanelK)) return fail(BPGL_E_ARG, "w must be a multiple of 64 * kchunks");
    if ((int64_t)nrhs * w >= (1ll << 31) || (int64_t)nrhs * m >= (1ll << 31))
        return fail(BPGL_E_ARG, "nrhs * block width and nrhs * m must be below 2^31");
    HIP_TRY(hipSetDevice(device));
    bpgl_panel* c = new bpgl_panel();
    c->device = device;
    c->m = m;
    c->n = n;
    c->w = w;
    c->nblock = nblock;
    c->k = nrhs;
    c->kchunks = kchunks;
    if (hip_stream) {
        c->stream = (hipStream_t)hip_stream;
    } else {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
            delete c;
            return fail(BPGL_E_HIP, "hipStreamCreate failed");
        }
        c->own_stream = true;
    }
    c->tm.stream = c->stream;
    *out = c;
    return 0;
}

void bpgl_panel_destroy(bpgl_panel* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);   // destroy path: nothing to report to
    drop_graphs(c);
    for (auto e : c->tm.evs) (void)hipEventDestroy(e);
    for (auto e : c->gap_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int64_t bpgl_panel_scratch_bytes(const bpgl_panel* c) { return c ? panel_layout(c).total : -1; }

int bpgl_panel_bind(bpgl_panel* c, const void* A, int64_t lda, void* scratch, int64_t scratch_bytes) {
    if (!c) return fail(BPGL_E_ARG, "null panel context");
    if (!A || !scratch) return fail(BPGL_E_ARG, "A and scratch must be non-null");
    if (((uintptr_t)A) % 16) return fail(BPGL_E_ARG, "A must be 16-byte aligned");
    if (((uintptr_t)scratch) % 256) return fail(BPGL_E_ARG, "scratch must be 256-byte aligned");
    if (lda < c->n || lda % 8) return fail(BPGL_E_ARG, "lda must be >= n and a multiple of 8");
    const PanelLayout L = panel_layout(c);
    if (scratch_bytes < L.total) return fail(BPGL_E_SCRATCH, "scratch too small: %lld < %lld",
                                             (long long)scratch_bytes, (long long)L.total);
    c->scratch = (char*)scratch;
    c->L = L;
    PanelParams& p = c->p;
    p = PanelParams{};
    p.A = (const __bf16*)A;
    p.lda = lda;
    p.m = c->m;
    p.w = c->w;
    p.nblock = c->nblock;
    p.k = c->k;
    p.kchunks = c->kchunks;
    p.ldr = c->ldr();
    p.ldd = c->ldd();
    p.st = c->at<PanelState>(L.st);
    p.Rh = c->at<__bf16>(L.Rh);
    p.Rl = c->at<__bf16>(L.Rl);
    p.Dh = c->at<__bf16>(L.Dh);
    p.Dl = c->at<__bf16>(L.Dl);
    p.X = c->at<float>(L.X);
    p.Ax = c->at<double>(L.Ax);
    p.B = c->at<double>(L.B);
    p.R = c->at<double>(L.R);
    p.diag = c->at<double>(L.diag);
    p.rec = c->at<double>(L.rec);
    p.Sslab = c->at<float>(L.Sslab);
    p.S = c->at<double>(L.S);
    p.norms = c->at<double>(L.norms);
    p.lsp = c->at<double>(L.lsp);
    p.mu = c->at<double>(L.mu);
    p.gamma = c->at<double>(L.gamma);
    p.err_rhs = c->at<double>(L.err_rhs);
    p.cnt = c->at<unsigned long long>(L.cnt);
    p.Gc = c->at<float>(L.Gc);
    p.Ec = c->at<float>(L.Ec);
    p.ready = c->at<unsigned long long>(L.ready);
    p.lsdone = c->at<unsigned long long>(L.lsdone);
    p.At = c->at<__bf16>(L.At);
    p.A1t = c->at<__bf16>(L.A1t);
    p.lss = c->at<double>(L.lss);
    p.cshift = c->at<double>(L.cshift);
    p.nw = c->at<double>(L.nw);
    HIP_TRY(hipSetDevice(c->device));
    // Cleared here: every region up to the tiled copies -- the state, counters and partials, the operand
    // images, X, Ax, B, R, diag / rec and the carried gradient's G, operand and E -- so that nothing reads
    // a stale value before its first write (the solver's own reset clears again what it must).  Not
    // cleared, because each is written in full before it is read: At / A1t (the tile kernels below), the
    // certificate's buffers gpart, gparts, gcounts, gres and ghold (every bpgl_panel_gap writes them first),
    // W (bpgl_panel_set_row_mask, and p.W is null until then) and Bh (k_panel_mask_b at a masked reset; the
    // certificate reads it only under a mask); the intercept's pieces (nw: bpgl_panel_set_intercept; bmean: the
    // reset; lss and cshift: every iteration's line search before its update; gipart and gicp: every certificate).
    HIP_TRY(hipMemsetAsync(c->scratch, 0, L.At, c->stream));
    hipLaunchKernelGGL((k_panel_tile<256, 64, true>), dim3((unsigned)((c->m / 256) * (c->n / 64))), dim3(256), 0,
                       c->stream, p.A, p.lda, c->n, c->at<__bf16>(L.At));
    LAUNCH_CHECK("k_panel_tile");
    hipLaunchKernelGGL((k_panel_tile<64, 256, false>), dim3((unsigned)((c->m / 64) * (c->n / 256))), dim3(256), 0,
                       c->stream, p.A, p.lda, c->n, c->at<__bf16>(L.A1t));
    LAUNCH_CHECK("k_panel_tile");
    c->masked = c->user_mask = c->icpt = c->icpt_valid = c->positive = c->penalty = c->weighted = false;   // p.W, p.Wt are null again
    panel_fuse_check(c);
    c->bound = true;
    c->have_x = false;
    c->have_diag = false;
    c->solver = false;
    drop_graphs(c);
    return 0;
}

int bpgl_panel_diag(bpgl_panel* c, double* out) {
    int rc;
    if ((rc = panel_ready(c))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = panel_run_diag(c))) return rc;   // the diag in effect: the centred one with the intercept on
    if (out) HIP_TRY(hipMemcpyAsync(out, c->p.diag, 8 * c->n, hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

int bpgl_panel_mtm(bpgl_panel* c, int32_t block, const double* R, double* G) {
    int rc;
    if ((rc = panel_ready(c))) return rc;
    if (block < 0 || block >= c->nblock) return fail(BPGL_E_ARG, "block out of range");
    if (!R || !G) return fail(BPGL_E_ARG, "null operand");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = panel_split(c, R, c->m, c->ldr(), c->p.Rh, c->p.Rl, 1.0, nullptr))) return rc;
    c->solver = false;   // Rh/Rl now hold the caller's operand
    return panel_launch(c, 0, block, G, 0, 2);
}

int bpgl_panel_mm(bpgl_panel* c, int32_t block, const double* D, double* S) {
    int rc;
    if ((rc = panel_ready(c))) return rc;
    if (block < 0 || block >= c->nblock) return fail(BPGL_E_ARG, "block out of range");
    if (!D || !S) return fail(BPGL_E_ARG, "null operand");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = panel_split(c, D, c->w, c->ldd(), c->p.Dh, c->p.Dl, 1.0, nullptr))) return rc;
    c->solver = false;
    if ((rc = panel_launch(c, 1, block, nullptr, 0, 2))) return rc;
    return panel_reduce(c, S, 0);
}

int bpgl_panel_reset(bpgl_panel* c, const double* B, const double* mu, double* err_iter, int64_t record_len,
                     int use_graph) {
    return bpgl_panel_reset_x0(c, B, mu, nullptr, err_iter, record_len, use_graph);
}

int bpgl_panel_reset_x0(bpgl_panel* c, const double* B, const double* mu, const float* X0, double* err_iter,
                        int64_t record_len, int use_graph) {
    int rc;
    if ((rc = panel_ready(c))) return rc;
    if (!c->have_diag) return fail(BPGL_E_STATE, "bpgl_panel_diag must run before the solver");
    if (!B || !mu) return fail(BPGL_E_ARG, "B and mu must be non-null");
    if (((uintptr_t)X0) % 16) return fail(BPGL_E_ARG, "X0 must be 16-byte aligned");
    if (c->icpt && c->nblock > 1)
        return fail(BPGL_E_STATE, "the intercept needs one feature block (nblock is %d)", c->nblock);
    if (c->icpt && !c->defer_x)
        return fail(BPGL_E_STATE, "the intercept needs the deferred x update (the tuning key defer_x is 0)");
    if (c->weighted && c->nblock > 1)
        return fail(BPGL_E_STATE, "row weights need one feature block (nblock is %d)", c->nblock);
    if (c->weighted && !c->defer_x)
        return fail(BPGL_E_STATE, "row weights need the deferred x update (the tuning key defer_x is 0)");
    HIP_TRY(hipSetDevice(c->device));
    PanelParams& p = c->p;
    const int64_t km = (int64_t)c->k * c->m;
    c->icpt_valid = false;
    if (c->weighted && c->icpt) {   // the stored B is w o (b - bmean), bmean the weighted mean; the full B for the certificate
        hipLaunchKernelGGL(bpgl_wt::centre_b(), dim3((unsigned)c->k), dim3(kThreads), 0, c->stream, B, p.Wt, (long long)c->m,
                           p.nw, const_cast<double*>(p.B), c->at<double>(c->L.Bh), c->at<double>(c->L.bmean));
        LAUNCH_CHECK("k_panel_centre_b_wt");
    } else if (c->weighted) {       // the stored B is w o B (so R0 = -w o B); the full B for the certificate
        hipLaunchKernelGGL(bpgl_wt::weight_b(), dim3((unsigned)std::min<int64_t>(cdiv(km, kThreads), 2048)), dim3(kThreads),
                           0, c->stream, B, p.Wt, (long long)km, const_cast<double*>(p.B), c->at<double>(c->L.Bh));
        LAUNCH_CHECK("k_panel_weight_b");
    } else if (c->icpt) {   // the stored B is P_w B (so R0 = -P_w B), its in-row mean kept for the certificate; (1 - w) o B as below
        hipLaunchKernelGGL(k_panel_centre_b, dim3((unsigned)c->k), dim3(kThreads), 0, c->stream, B, p.W, (long long)c->m,
                           p.nw, const_cast<double*>(p.B), c->at<double>(c->L.Bh), c->at<double>(c->L.bmean));
        LAUNCH_CHECK("k_panel_centre_b");
    } else if (c->masked) {   // the stored B is w o B (so R0 = -w o B and A x - B stays masked); (1 - w) o B for the score
        hipLaunchKernelGGL(k_panel_mask_b, dim3((unsigned)std::min<int64_t>(cdiv(km, kThreads), 2048)), dim3(kThreads),
                           0, c->stream, B, p.W, (long long)km, const_cast<double*>(p.B), c->at<double>(c->L.Bh));
        LAUNCH_CHECK("k_panel_mask_b");
    } else {
        HIP_TRY(hipMemcpyAsync(const_cast<double*>(p.B), B, 8 * km, hipMemcpyDeviceToDevice, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(const_cast<double*>(p.mu), mu, 8 * c->k, hipMemcpyDeviceToDevice, c->stream));
    const int64_t xbytes = 4 * (int64_t)c->k * c->w * c->nblock;
    if (!X0) {
        HIP_TRY(hipMemsetAsync(p.X, 0, xbytes, c->stream));
        HIP_TRY(hipMemsetAsync(p.Ax, 0, 8 * km * c->nblock, c->stream));
        // x = 0 => Ax = 0, R = -B
        if ((rc = panel_split(c, p.B, c->m, c->ldr(), p.Rh, p.Rl, -1.0, p.R))) return rc;
    } else {
        // x = X0 (the stored iterate itself when X0 is bpgl_panel_x), R = A x - B and Ax from the fp64
        // product on that fp32 x, R's images from that R
        if (X0 != p.X) HIP_TRY(hipMemcpyAsync(p.X, X0, xbytes, hipMemcpyDeviceToDevice, c->stream));
        if (c->positive) {   // the start is max(X0, 0): feasible, and R below is formed from it
            const int64_t nx = xbytes / 4;
            hipLaunchKernelGGL(bpgl_pos::project_x(),
                               dim3((unsigned)std::min<int64_t>(cdiv(nx, kThreads), 2048)), dim3(kThreads), 0, c->stream,
                               p.X, (long long)nx);
            LAUNCH_CHECK("k_panel_project_x");
        }
        if ((rc = panel_warm_residual(c))) return rc;
        if ((rc = panel_split(c, p.R, c->m, c->ldr(), p.Rh, p.Rl, 1.0, nullptr))) return rc;
    }
    c->t_host = 0;
    c->n_exact = 0;
    p.err_iter = err_iter;
    p.rec_len = err_iter ? record_len : 0;
    HIP_TRY(hipMemsetAsync(p.cnt, 0, 8 * (int64_t)c->k, c->stream));   // arrival counters start at 0
    HIP_TRY(hipMemsetAsync(p.ready, 0, 8 * (int64_t)c->k, c->stream));
    HIP_TRY(hipMemsetAsync(p.lsdone, 0, 8, c->stream));
    hipLaunchKernelGGL(k_panel_reset_state, dim3(1), dim3(64), 0, c->stream, c->p);
    LAUNCH_CHECK("k_panel_reset_state");
    p.Sh = panel_carry(c) ? c->at<__bf16>(c->L.Sh) : nullptr;
    drop_graphs(c);
    if (use_graph) {
        // kGraphIters iterations; with the carried gradient a second graph whose first iteration is
        // the exact one (bpgl_panel_step replays it at every g_period-th iteration)
        const bool was = c->tm.on;
        c->tm.on = false;
        for (int g = 0; g < (panel_carry(c) ? 2 : 1) && !rc; ++g)
            rc = capture_graph(c->stream, g ? &c->gexec_ref : &c->gexec, [&] {
                int e = 0;
                // R's images from the graph's last iteration: the next replay may start with the exact one
                for (int k = 0; k < kGraphIters && !e; ++k)
                    e = panel_iteration(c, 0, g == 1 && k == 0, k == kGraphIters - 1);
                return e;
            });
        c->tm.on = was;
        if (rc) return rc;
    }
    c->solver = true;
    c->have_x = true;
    c->tm.iters = 0;
    return 0;
}

int bpgl_panel_step(bpgl_panel* c, int64_t n_iter) {
    int rc;
    if ((rc = panel_ready(c))) return rc;
    if (!c->solver) return fail(BPGL_E_STATE, "bpgl_panel_reset has not been called");
    HIP_TRY(hipSetDevice(c->device));
    int64_t i = 0;
    while (i < n_iter) {
        // carried gradient: every g_period-th iteration (the first included) computes G exactly
        const bool exact = panel_carry(c) && c->t_host % c->g_period == 0;
        if (!c->tm.on && c->gexec && i + kGraphIters <= n_iter && c->t_host % kGraphIters == 0) {
            HIP_TRY(hipGraphLaunch(exact ? c->gexec_ref : c->gexec, c->stream));
            c->n_exact += exact;
            i += kGraphIters;
            c->t_host += kGraphIters;
        } else {
            const bool next_exact = (c->t_host + 1) % c->g_period == 0;
            if ((rc = panel_iteration(c, c->tm.on ? c->tm.iters : 0, exact, next_exact || i + 1 == n_iter)))
                return rc;
            c->n_exact += exact;
            if (c->tm.on) c->tm.iters++;
            ++i;
            ++c->t_host;
        }
    }
    if (c->nblock == 1 && c->defer_x) {   // the last iteration's x update, so X is current between calls
        const dim3 fg((unsigned)std::min<int64_t>(cdiv((int64_t)c->k * c->w / 8, kThreads), 8192));
        const auto flush = dispatch<1, 2>(c->dsplit, [](auto ds) { return &k_panel_flush<decltype(ds)::value>; });
        hipLaunchKernelGGL(flush, fg, dim3(kThreads), 0, c->stream, c->p);
        LAUNCH_CHECK("k_panel_flush");
        hipLaunchKernelGGL(k_panel_clear_pending, dim3(1), dim3(64), 0, c->stream, c->p);
        LAUNCH_CHECK("k_panel_clear_pending");
    }
    return 0;
}

int bpgl_panel_status(bpgl_panel* c, int64_t* iters, double* last_err) {
    int rc;
    if ((rc = panel_ready(c))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    PanelState st;
    HIP_TRY(hipMemcpyAsync(&st, c->p.st, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (iters) *iters = st.iters;
    if (last_err) *last_err = st.last_err;
    if (st.fail)
        return fail(BPGL_E_EXCHANGE, "k_panel_reduce_upd: a block waited in vain for its right-hand side's step size "
                                     "(blocks not co-resident: another kernel held CUs); the iterates are not valid -- "
                                     "reset and run with the tuning key fuse_update = 0");
    return 0;
}

const float* bpgl_panel_x(bpgl_panel* c) { return c ? c->p.X : nullptr; }

int bpgl_panel_set_kernel_timing(bpgl_panel* c, int enable) {
    if (!c) return fail(BPGL_E_ARG, "null panel context");
    c->tm.on = enable != 0;
    c->tm.iters = 0;
    return 0;
}

int bpgl_panel_kernel_times(bpgl_panel* c, double* avg_ms /* 5 */, int64_t* samples) {
    if (!c || !avg_ms) return fail(BPGL_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return c->tm.collect(avg_ms, samples);
}

int bpgl_panel_set_tuning(bpgl_panel* c, const char* key, int64_t value) {
    if (!c || !key) return fail(BPGL_E_ARG, "null argument");
    const bool both = !strcmp(key, "interleave");
    if (both || !strcmp(key, "interleave1") || !strcmp(key, "interleave2")) {
        if (value < 0 || value > 2) return fail(BPGL_E_ARG, "interleave must be 0, 1 or 2");
        if (both || key[10] == '1') c->interleave[0] = (int)value;
        if (both || key[10] == '2') c->interleave[1] = (int)value;
    } else if (!strcmp(key, "fuse_grid")) {
        if (value != 256 && value != 512 && value != 1024) return fail(BPGL_E_ARG, "fuse_grid must be 256, 512 or 1024");
        c->fuse_grid = (int)value;
        panel_fuse_check(c);
        c->solver = false;
    } else if (!strcmp(key, "fuse_update")) {
        if (value != 0 && value != 1) return fail(BPGL_E_ARG, "fuse_update must be 0 or 1");
        c->fuse_update = (int)value;
        c->solver = false;   // the graphs bake the launch sequence in: a reset must follow
    } else if (!strcmp(key, "defer_x")) {
        if (value != 0 && value != 1) return fail(BPGL_E_ARG, "defer_x must be 0 or 1");
        c->defer_x = (int)value;
        c->solver = false;   // the graph bakes in where x is updated (and the flush): a reset must follow
    } else if (!strcmp(key, "d_split")) {
        if (value != 1 && value != 2) return fail(BPGL_E_ARG, "d_split must be 1 or 2");
        c->dsplit = (int)value;
    } else if (!strcmp(key, "carry_g")) {
        if (value != 0 && value != 1) return fail(BPGL_E_ARG, "carry_g must be 0 or 1");
        if (value && c->nblock != 1) return fail(BPGL_E_ARG, "carry_g needs one feature block");
        c->carry_g = (int)value;
        c->solver = false;   // the graphs and the operand image depend on it: a reset must follow
    } else if (!strcmp(key, "g_refresh")) {
        if (value < kGraphIters || value % kGraphIters)
            return fail(BPGL_E_ARG, "g_refresh must be a positive multiple of %d", kGraphIters);
        c->g_period = value;
        c->solver = false;
    } else {
        return fail(BPGL_E_ARG, "unknown panel tuning key '%s'", key);
    }
    drop_graphs(c);
    return 0;
}

int bpgl_panel_get_tuning(const bpgl_panel* c, const char* key, int64_t* value) {
    if (!c || !key || !value) return fail(BPGL_E_ARG, "null argument");
    if (!strcmp(key, "interleave1")) *value = panel_ilv(c, 0, c->dsplit);
    else if (!strcmp(key, "interleave2")) *value = panel_ilv(c, 1, c->dsplit);   // the solver's pass 2
    else if (!strcmp(key, "d_split")) *value = c->dsplit;
    else if (!strcmp(key, "defer_x")) *value = c->defer_x;
    else if (!strcmp(key, "fuse_grid")) *value = c->fuse_grid;
    else if (!strcmp(key, "fuse_update")) *value = c->nblock == 1 && c->defer_x && c->fuse_update && c->fuse_ok;   // in effect
    else if (!strcmp(key, "carry_g")) *value = panel_carry(c) ? 1 : 0;   // the form in effect
    else if (!strcmp(key, "g_refresh")) *value = c->g_period;
    else if (!strcmp(key, "positive")) *value = c->positive ? 1 : 0;   // bpgl_panel_set_positive
    else if (!strcmp(key, "penalty")) *value = c->penalty ? 1 : 0;     // bpgl_panel_set_penalty
    else if (!strcmp(key, "row_weights")) *value = c->weighted ? 1 : 0;   // bpgl_panel_set_row_weights
    else return fail(BPGL_E_ARG, "unknown panel tuning key '%s'", key);
    return 0;
}

int bpgl_panel_stat(const bpgl_panel* c, const char* key, int64_t* value) {
    if (!c || !key || !value) return fail(BPGL_E_ARG, "null argument");
    if (!strcmp(key, "iters_enqueued")) *value = c->t_host;
    else if (!strcmp(key, "exact_gradients")) *value = c->n_exact;
    else if (!strcmp(key, "fuse_cus")) *value = c->fuse_cus;   // CUs the fused-update check counted
    else if (!strcmp(key, "gap_prod1_ns")) *value = c->gap_ns[0];   // the last bpgl_panel_gap: R_fresh = A X - B
    else if (!strcmp(key, "gap_prod2_ns")) *value = c->gap_ns[1];   // ... and G = A^T R_fresh
    else if (!strcmp(key, "glm_ax_offset")) *value = c->L.glmAX;    // bpgl_panel_glm_model's A x [nrhs][m] fp64: its byte offset in the scratch
    else return fail(BPGL_E_ARG, "unknown panel stat '%s'", key);
    return 0;
}

const double* bpgl_panel_residual(bpgl_panel* c) { return c ? c->p.R : nullptr; }

int bpgl_panel_set_row_mask(bpgl_panel* c, const uint8_t* mask) {
    int rc;
    if ((rc = panel_ready(c))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    unsigned char* W = c->at<unsigned char>(c->L.W);
    if (mask) HIP_TRY(hipMemcpyAsync(W, mask, (int64_t)c->k * c->m, hipMemcpyDeviceToDevice, c->stream));
    c->user_mask = mask != nullptr;
    c->weighted = false;            // a mask and weights are alternatives: the last call wins
    return panel_install_mask(c);   // with the intercept on: all ones when cleared, and the in-row counts again
}

int bpgl_panel_set_row_weights(bpgl_panel* c, const double* wt, const double* hold) {
    int rc;
    if ((rc = panel_ready(c))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const int64_t km = (int64_t)c->k * c->m;
    if (wt) {
        // validated where the caller has them, so that refused weights leave what was installed in force
        double* dw = c->at<double>(c->L.Wt);
        double* dh = c->at<double>(c->L.Hd);
        int* flag = reinterpret_cast<int*>(dh + km);
        int bad = 0;
        const dim3 grid((unsigned)std::min<int64_t>(cdiv(km, kThreads), 2048));
        HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), c->stream));
        hipLaunchKernelGGL(bpgl_wt::check(), grid, dim3(kThreads), 0, c->stream, wt, hold, (long long)km, flag);
        LAUNCH_CHECK("k_panel_check_weights");
        HIP_TRY(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (bad) return fail(BPGL_E_ARG, "every row weight must be finite and in [0, 1], every scoring weight finite and >= 0");
        if (wt != dw) HIP_TRY(hipMemcpyAsync(dw, wt, 8 * km, hipMemcpyDeviceToDevice, c->stream));
        if (hold) {
            if (hold != dh) HIP_TRY(hipMemcpyAsync(dh, hold, 8 * km, hipMemcpyDeviceToDevice, c->stream));
        } else {
            hipLaunchKernelGGL(bpgl_wt::default_hold(), grid, dim3(kThreads), 0, c->stream, dw, (long long)km, dh);
            LAUNCH_CHECK("k_panel_default_hold");
        }
        HIP_TRY(hipStreamSynchronize(c->stream));   // a set-up call: done when it returns, so the caller's buffers are free
    }
    c->weighted = wt != nullptr;
    c->user_mask = false;           // a mask and weights are alternatives: the last call wins (also when it clears)
    return panel_install_mask(c);   // the weight sums with the intercept on; the fused form's occupancy check again
}

int bpgl_panel_set_intercept(bpgl_panel* c, int on) {
    int rc;
    if ((rc = panel_ready(c))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    c->icpt = on != 0;
    c->icpt_valid = false;
    if ((rc = panel_install_mask(c))) return rc;
    return panel_run_diag(c);   // centred norms and rec with the intercept, k_panel_diag's without
}

int bpgl_panel_set_positive(bpgl_panel* c, int on) {
    int rc;
    if ((rc = panel_ready(c))) return rc;
    c->positive = on != 0;
    c->solver = false;   // the graphs bake the pass-1 variant in: a reset must follow
    drop_graphs(c);
    return 0;
}

int bpgl_panel_set_penalty(bpgl_panel* c, const double* pen) {
    int rc;
    if ((rc = panel_ready(c))) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (pen) {
        // validated where the caller has it, so that a refused vector leaves the installed one in force
        double* dst = c->at<double>(c->L.pen);
        int* flag = reinterpret_cast<int*>(dst + c->n);
        int bad = 0;
        HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), c->stream));
        hipLaunchKernelGGL(bpgl_pen::check(), dim3((unsigned)std::min<int64_t>(cdiv(c->n, kThreads), 2048)), dim3(kThreads),
                           0, c->stream, pen, (long long)c->n, flag);
        LAUNCH_CHECK("k_panel_check_pen");
        HIP_TRY(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (bad) return fail(BPGL_E_ARG, "every penalty factor must be finite and > 0");
        if (pen != dst) {   // a set-up call: done when it returns, so the caller's buffer is free
            HIP_TRY(hipMemcpyAsync(dst, pen, 8 * c->n, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
    }
    c->penalty = pen != nullptr;
    c->solver = false;   // the graphs bake the pass-1 variant and its argument in: a reset must follow
    drop_graphs(c);
    return 0;
}

int bpgl_panel_intercept(bpgl_panel* c, double* out) {
    int rc;
    if ((rc = panel_ready(c))) return rc;
    if (!out) return fail(BPGL_E_ARG, "out is null");
    if (!c->icpt) {
        std::fill(out, out + c->k, 0.0);
        return 0;
    }
    if (!c->icpt_valid) return fail(BPGL_E_STATE, "no bpgl_panel_gap since the last reset");
    std::copy(c->icpt_host.begin(), c->icpt_host.end(), out);
    return 0;
}

int bpgl_panel_gap(bpgl_panel* c, double* G_all, double* R_fresh, uint8_t* keep, double* out) {
    int rc;
    if ((rc = panel_ready(c))) return rc;
    if (!c->have_diag) return fail(BPGL_E_STATE, "bpgl_panel_diag must run before bpgl_panel_gap");
    if (!c->solver) return fail(BPGL_E_STATE, "bpgl_panel_reset has not been called");
    if (!G_all || !R_fresh || !out) return fail(BPGL_E_ARG, "G_all, R_fresh and out must be non-null");
    if (((uintptr_t)G_all) % 16 || ((uintptr_t)R_fresh) % 16)
        return fail(BPGL_E_ARG, "G_all and R_fresh must be 16-byte aligned");
    if ((rc = bpgl_panel_status(c, nullptr, nullptr))) return rc;   // waits; reports a failed exchange
    const PanelLayout& L = c->L;
    double* parts = c->at<double>(L.gparts);
    double* res = c->at<double>(L.gres);
    int* counts = c->at<int>(L.gcounts);
    PanelGapArgs a = pgap_args(c);
    a.Rf = R_fresh;
    a.G = G_all;
    for (auto& e : c->gap_ev)
        if (!e) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(c->gap_ev[0], c->stream));
    // product 1: Rf = A X - B; product 2: G = A^T Rf.  Reads X, B, R, diag, mu and A only; writes the
    // caller's buffers and this call's own scratch.
    for (int prod = 1; prod <= 2; ++prod) {
        const int64_t len = prod == 1 ? c->m : c->n, stages = (prod == 1 ? c->n : c->m) / kPgK;
        a.spl = pgap_split(len / kPgTile, stages);
        a.chunk = stages / a.spl;
        const dim3 grid((unsigned)(len / kPgTile * a.spl));
        if ((rc = prod == 1 ? pgap_prod<1>(c, a, grid) : pgap_prod<2>(c, a, grid))) return rc;
        HIP_TRY(hipEventRecord(c->gap_ev[prod], c->stream));
    }
    const int nparts = pgap_nparts(c);
    const double* pen = c->at<double>(L.pen);
    if (c->weighted)   // sum w e^2 and sum w e b from the fold's e (pen is read with the factors only)
        hipLaunchKernelGGL(bpgl_wt::gap_partials(c->positive, c->penalty), dim3((unsigned)nparts, (unsigned)c->k),
                           dim3(kThreads), 0, c->stream, a, parts, pen);
    else if (c->penalty)
        hipLaunchKernelGGL(c->positive ? bpgl_pen::gap_partials_pos() : bpgl_pen::gap_partials(),
                           dim3((unsigned)nparts, (unsigned)c->k), dim3(kThreads), 0, c->stream, a, parts, pen);
    else
    hipLaunchKernelGGL(c->positive ? bpgl_pos::gap_partials() : &k_pgap_partials<false>,
                       dim3((unsigned)nparts, (unsigned)c->k), dim3(kThreads), 0, c->stream, a, parts);
    LAUNCH_CHECK("k_pgap_partials");
    hipLaunchKernelGGL(k_pgap_final, dim3((unsigned)c->k), dim3(kThreads), 0, c->stream, parts, nparts, a.mu, res);
    LAUNCH_CHECK("k_pgap_final");
    if (c->masked || c->weighted) {   // res[k][7], which k_pgap_final left at 0
        hipLaunchKernelGGL(k_pgap_holdout, dim3((unsigned)c->k), dim3(kThreads), 0, c->stream, a.hpart,
                           (long long)(c->m / kThreads), res);
        LAUNCH_CHECK("k_pgap_holdout");
    }
    if (keep) {
        const int64_t nb = cdiv(c->n, kThreads);
        if (c->penalty)
            hipLaunchKernelGGL(c->positive ? bpgl_pen::gap_screen_pos() : bpgl_pen::gap_screen(),
                               dim3((unsigned)nb, (unsigned)c->k), dim3(kThreads), 0, c->stream, a, res, keep, counts, pen);
        else
        hipLaunchKernelGGL(c->positive ? bpgl_pos::gap_screen() : &k_pgap_screen<false>,
                           dim3((unsigned)nb, (unsigned)c->k), dim3(kThreads), 0, c->stream, a, res, keep, counts);
        LAUNCH_CHECK("k_pgap_screen");
        hipLaunchKernelGGL(k_pgap_count, dim3((unsigned)c->k), dim3(kThreads), 0, c->stream, counts, (long long)nb, res);
        LAUNCH_CHECK("k_pgap_count");
    }
    HIP_TRY(hipMemcpyAsync(out, res, sizeof(double) * kPgRes * c->k, hipMemcpyDeviceToHost, c->stream));
    if (c->icpt) {   // beta0 per RHS, for bpgl_panel_intercept
        c->icpt_host.resize(c->k);
        HIP_TRY(hipMemcpyAsync(c->icpt_host.data(), a.icp + c->k, 8 * (int64_t)c->k, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->icpt_valid = c->icpt;
    for (int q = 0; q < 2; ++q) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->gap_ev[q], c->gap_ev[q + 1]));
        c->gap_ns[q] = (int64_t)((double)ms * 1e6);
    }
    if (!keep)
        for (int k = 0; k < c->k; ++k) out[(int64_t)k * kPgRes + 5] = (double)c->n;
    return 0;
}

int bpgl_panel_glm_model(bpgl_panel* c, int family, const double* Y, const double* Om, const double* Hd,
                         const int32_t* curv, double* beta0, double* W, double* Z, double* P, double* out) {
    int rc;
    if ((rc = panel_ready(c))) return rc;
    if (family != BPGL_GLM_BINOMIAL) return fail(BPGL_E_ARG, "family must be BPGL_GLM_BINOMIAL (got %d)", family);
    if (!Y || !Om || !beta0 || !W || !Z || !P || !out)
        return fail(BPGL_E_ARG, "Y, Om, beta0, W, Z, P and out must be non-null");
    if (((uintptr_t)Y | (uintptr_t)Om | (uintptr_t)Hd | (uintptr_t)beta0 | (uintptr_t)W | (uintptr_t)Z | (uintptr_t)P) % 8 ||
        ((uintptr_t)curv) % 4)
        return fail(BPGL_E_ARG, "Y, Om, Hd, beta0, W, Z and P must be 8-byte aligned, curv 4-byte aligned");
    if (c->nblock != 1) return fail(BPGL_E_STATE, "the logistic model needs one feature block (nblock is %d)", c->nblock);
    if (!c->have_x) return fail(BPGL_E_STATE, "bpgl_panel_reset has not been called since bpgl_panel_bind");
    if ((rc = bpgl_panel_status(c, nullptr, nullptr))) return rc;   // waits; reports a failed exchange
    // A x through the certificate's product 1, its chunking and its launch; the fold subtracts nothing
    PanelGapArgs a = pgap_args(c);
    a.spl = pgap_split(c->m / kPgTile, c->n / kPgK);
    a.chunk = c->n / kPgK / a.spl;
    const dim3 blk(kThreads);
    const auto prod = dispatch_nt(c->k, [](auto nt) { return &k_pgap_prod<decltype(nt)::value, 1>; });
    hipLaunchKernelGGL(prod, dim3((unsigned)(c->m / kPgTile * a.spl)), blk, 0, c->stream, a);
    LAUNCH_CHECK("k_pgap_prod");
    bpgl_glm::GlmArgs g = glm_args(c);
    g.spl = a.spl;
    g.Y = Y;
    g.Om = Om;
    g.Hd = Hd;
    g.curv = curv;
    g.beta0 = beta0;
    g.W = W;
    g.Z = Z;
    g.P = P;
    const dim3 rows((unsigned)((int64_t)c->k * c->m / kThreads)), rhs((unsigned)c->k);
    hipLaunchKernelGGL(bpgl_glm::fold(), rows, blk, 0, c->stream, g);
    LAUNCH_CHECK("k_glm_fold");
    hipLaunchKernelGGL(bpgl_glm::newton(), rhs, blk, 0, c->stream, g);
    LAUNCH_CHECK("k_glm_newton");
    hipLaunchKernelGGL(bpgl_glm::model(), rows, blk, 0, c->stream, g);
    LAUNCH_CHECK("k_glm_model");
    hipLaunchKernelGGL(bpgl_glm::l1_final(), rhs, blk, 0, c->stream, g);
    LAUNCH_CHECK("k_glm_l1_final");
    HIP_TRY(hipMemcpyAsync(out, g.res, sizeof(double) * bpgl_glm::kGlmRes * c->k, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int bpgl_panel_glm_dual(bpgl_panel* c, const double* P, const double* Y, const double* Om, const double* scale,
                        double* out) {
    int rc;
    if ((rc = panel_ready(c))) return rc;
    if (!P || !Y || !Om || !scale || !out) return fail(BPGL_E_ARG, "P, Y, Om, scale and out must be non-null");
    if (((uintptr_t)P | (uintptr_t)Y | (uintptr_t)Om) % 8) return fail(BPGL_E_ARG, "P, Y and Om must be 8-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    bpgl_glm::GlmArgs g = glm_args(c);
    g.P = const_cast<double*>(P);
    g.Y = Y;
    g.Om = Om;
    HIP_TRY(hipMemcpyAsync(const_cast<double*>(g.scale), scale, 8 * (int64_t)c->k, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(bpgl_glm::dual_sum(), dim3((unsigned)c->k), dim3(kThreads), 0, c->stream, g);
    LAUNCH_CHECK("k_glm_dual");
    HIP_TRY(hipMemcpyAsync(out, g.dual, 8 * (int64_t)c->k, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int bpgl_panel_gather_columns(bpgl_panel* c, const int32_t* cols, int64_t n_out, void* A_out, int64_t lda_out) {
    int rc;
    if ((rc = panel_ready(c))) return rc;
    const GatherArgs a{c->p.A, c->p.lda, 0, c->n, c->n, c->m, cols, n_out, A_out, lda_out};
    return gather_columns<2>(c->device, c->stream, 2, a, [&] {   // A_out [m][lda_out] against the bound A [m][lda]
        const uintptr_t a0 = (uintptr_t)c->p.A, a1 = a0 + 2 * (uintptr_t)((c->m - 1) * c->p.lda + c->n);
        const uintptr_t o0 = (uintptr_t)A_out, o1 = o0 + 2 * (uintptr_t)(c->m * lda_out);
        return o0 < a1 && a0 < o1 ? fail(BPGL_E_ARG, "A_out overlaps the bound A") : 0;
    });
}

int bpgl_panel_geometry(const bpgl_panel* c, int32_t* kchunks) {
    if (!c) return fail(BPGL_E_ARG, "null panel context");
    if (kchunks) *kchunks = c->kchunks;
    return 0;
}

}  // extern "C"


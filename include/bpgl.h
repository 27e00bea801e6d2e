/*
 * bpgl -- MI355X-native block proximal-gradient (best-response) lasso hot path.
 *
 * Flat C ABI of convex_optimization_amd/_lib/libbpgl.so.  Plain pointers and
 * sizes only; every device pointer is memory allocated by the caller (PyTorch
 * tensors on the Python side).  The library never calls hipMalloc: it borrows
 * the caller's buffers for the lifetime of a context.
 *
 * Problem (reference lasso.py:102-157, one "ISTA iteration" = one block update):
 *   minimise 1/2 ||A x - b||^2 + mu ||x||_1,  A: m x n, columns split into
 *   nblock feature blocks of width w = n / nblock.
 *
 * Device layout of A (one rank): element (i, j) of feature block b lives at
 *   A + b * block_stride + i * lda + j        (0 <= j < w_pad)
 * w_pad = w rounded up to 16 bytes worth of elements; padding columns must be 0.
 * The reference's own GPU layout (gpu_calculation.py:172-173, np.hsplit into a
 * (BLOCK, H, W) array) is block_stride = m * w_pad, lda = w_pad.
 *
 * Conventions: return 0 on success, a negative BPGL_E* code on failure; the
 * failing call's message is available from bpgl_last_error() (thread-local).
 * No C++ exception crosses this boundary.  A context is not thread-safe and is
 * bound to one device; all work is enqueued on the context's stream.
 */
#ifndef BPGL_H
#define BPGL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* dtype of A (the reference's class tunable TYPE, gpu_calculation.py:146) */
enum { BPGL_F32 = 0, BPGL_F64 = 1, BPGL_BF16 = 2 };

enum {
    BPGL_OK = 0,
    BPGL_E_ARG = -1,      /* bad argument / shape / alignment            */
    BPGL_E_STATE = -2,    /* call out of order (not bound / no solver)   */
    BPGL_E_HIP = -3,      /* HIP runtime error                           */
    BPGL_E_RCCL = -4,     /* RCCL error                                  */
    BPGL_E_SCRATCH = -5,  /* scratch buffer too small                    */
    BPGL_E_EXCHANGE = -6  /* one-pass row hand-off timed out (another
                             kernel held CUs) on an external-exchange
                             rank; the failed iterations committed
                             nothing: the solver state is intact at the
                             reported t (other ranks recover, see
                             bpgl_solver_status)                          */
};

typedef struct bpgl_ctx bpgl_ctx;

/* Message of the last failing call on this thread ("" if none). */
const char* bpgl_last_error(void);

/* Library / ABI version (major * 10000 + minor * 100 + patch).
 *   100 (0.1.0): the first ABI.
 *   200 (0.2.0): + bpgl_stream_create / bpgl_stream_destroy; bpgl_iterate always synchronises
 *                the solver stream before returning; the "onepass_cache_permille" default moved
 *                from 0 to -1 (automatic: 750 when the rank's A block fits the Infinity Cache);
 *                panel tuning keys "carry_g" (default 1: the carried gradient, one feature
 *                block) and "g_refresh".
 *   300 (0.3.0): the opt-in forms measured to lose were removed:
 *                tuning keys "fused", "onepass_fold", "onepass_variant"; panel keys "lo8",
 *                "r_refresh", "write_through", "op_pad", "waves*", interleave 3; panel stat
 *                "refreshes"; bpgl_panel_refresh.
 *   301 (0.3.1): tuning key "onepass_rows" and solver stat "onepass_rows".
 *   302 (0.3.2): RCCL row shards whose row needs more segment blocks than the stream's CUs run
 *                the two-pass row iteration instead of failing at bpgl_solver_reset; the panel's
 *                fused update is admitted against the stream's CUs; panel stat "fuse_cus"; tuning
 *                key and solver stat "onepass_sb1".
 *   303 (0.3.3): + bpgl_solver_gap (duality-gap certificate and gap-safe column screening) and
 *                bpgl_gather_columns; bpgl_scratch_bytes grows by the gap's partials and counts.
 *   304 (0.3.4): + bpgl_panel_gap (the panel's per-RHS duality-gap certificate, gap-safe screen and
 *                residual drift, from fp64 products on the stored x); bpgl_panel_scratch_bytes grows
 *                by its partials.
 *   305 (0.3.5): + bpgl_panel_set_row_mask (0/1 row weights per right-hand side: K-fold
 *                cross-validation as one panel); bpgl_panel_gap's out[8 k + 7] is the held-out sum of
 *                squares with a mask installed (0 without, as before); bpgl_panel_scratch_bytes grows
 *                by the mask, the held-out part of B and the certificate's held-out partials.
 *                Measured at 8192 x 65536, nrhs 128: 0.3774 ms per masked iteration against 0.3771
 *                unmasked (inside the run-to-run spread); the unmasked kernels are unchanged.
 *   306 (0.3.6): + bpgl_panel_reset_x0 (the panel solver started at a given x: R = A x - B from the
 *                certificate's fp64 product 1) and bpgl_panel_gather_columns (a column-compacted copy
 *                of the bound A); bpgl_panel_reset is bpgl_panel_reset_x0 with X0 = NULL, bit for bit
 *                as before.  bpgl_panel_scratch_bytes grows only for nblock > 1 where the product's
 *                block-aligned chunks need more than the certificate's partials (see below).
 *   307 (0.3.7): + bpgl_panel_set_intercept and bpgl_panel_intercept (an unpenalised intercept per
 *                right-hand side, profiled out over that right-hand side's in-rows, so K folds with K
 *                different centrings still share one bound A).  Opt-in: with it off
 *                every kernel that existed is unchanged.  bpgl_panel_scratch_bytes grows by the pieces
 *                laid out after everything that existed (one more line-search partial per 1024-row group,
 *                a few nrhs-long vectors, the certificate's in-row partials).
 *   308 (0.3.8): + bpgl_panel_set_positive (the sign constraint x >= 0 per right-hand side: the one-sided
 *                prox, a feasible bf16 direction image, the one-sided certificate and screen; DESIGN.md
 *                section 14) and the panel tuning key "positive" (bpgl_panel_get_tuning only).  Opt-in:
 *                with it off every kernel that existed is unchanged, bit for bit.
 *                bpgl_panel_scratch_bytes does not change.
 *   309 (0.3.9): + bpgl_panel_set_penalty (per-column l1 weights p_j > 0, glmnet's penalty.factor: column j pays
 *                mu_k p_j |x_j|; one vector shared by all right-hand sides, on the A that is bound -- no rescaled
 *                second copy) and the panel tuning key "penalty" (bpgl_panel_get_tuning
 *                only).  Opt-in: with it off every kernel that existed is unchanged, bit for bit, and a vector
 *                of ones gives the same bits as off.  bpgl_panel_scratch_bytes grows by the factors' piece, laid
 *                out after everything that existed (8 n + 256 bytes).
 *   310 (0.3.10): + bpgl_panel_set_row_weights (observation weights w_i in [0, 1] per right-hand side, glmnet's
 *                weights / scikit-learn's sample_weight, and scoring weights for out[8 k + 7]; on the A that is
 *                bound -- no row-rescaled copy; one feature block with the deferred x update)
 *                and the panel tuning key "row_weights" (bpgl_panel_get_tuning only).  Opt-in: with it off every
 *                kernel that existed is unchanged, bit for bit, and 0/1 weights compute what the row mask
 *                computes.  bpgl_panel_scratch_bytes grows by the weights' pieces, laid out after everything that
 *                existed (24 nrhs m + 256 bytes).
 *   311 (0.3.11): + bpgl_panel_glm_model and bpgl_panel_glm_dual (the logistic lasso by IRLS on the weighted panel:
 *                the piece between two inner solves -- A x in fp64, the intercept's Newton iteration, the working
 *                weights and response, the loss scalars -- and the dual sum of the logistic certificate; DESIGN.md
 *                section 18) and the panel stat "glm_ax_offset".  No iteration kernel has a new variant and no
 *                existing kernel's arguments move.  bpgl_panel_scratch_bytes grows by the model's pieces, laid out
 *                after everything that existed (about 8 nrhs m bytes). */
int bpgl_version(void);

/*
 * A HIP stream for a context, optionally restricted to a set of CUs
 * (hipExtStreamCreateWithCUMask; bit i of cu_mask[i / 32] enables CU i).  Several
 * processes (ranks) sharing one GPU each get disjoint CUs this way, so the
 * persistent one-pass grid of every rank stays resident beside the others.
 * bpgl_create sizes that grid to the CUs its stream may use (hipExtStreamGetCUMask;
 * the tuning key "cus" overrides it before bpgl_bind).  The mask should give
 * every XCD the same number of CUs: the python helper
 * distributed.xcd_symmetric_cu_mask builds one.  cu_mask NULL: an unrestricted
 * non-blocking stream.  No reference counterpart (pycuda used one context and
 * the default stream, gpu_calculation.py:4).
 */
int bpgl_stream_create(int device, const uint32_t* cu_mask, int32_t mask_words, void** stream_out);
int bpgl_stream_destroy(void* stream);

/*
 * Create a context for an m x n_local matrix split into nblock feature blocks.
 * Replaces GPU_Calculation.__init__ / init_cpu_array (gpu_calculation.py:148-220):
 * grid sizes and scratch needs are derived here instead of per-call numpy.
 * `hip_stream` may be NULL (the library then creates its own stream).
 */
int bpgl_create(bpgl_ctx** out, int device, int a_dtype, int64_t m, int64_t n_local,
                int32_t nblock, void* hip_stream);
void bpgl_destroy(bpgl_ctx* ctx);

/* The stream all work of this context is enqueued on. */
void* bpgl_stream(bpgl_ctx* ctx);

/* Bytes of device scratch the caller must provide to bpgl_bind. */
int64_t bpgl_scratch_bytes(const bpgl_ctx* ctx);

/* Padded block width (w rounded up to a 16-byte multiple of elements). */
int64_t bpgl_block_width_padded(const bpgl_ctx* ctx);

/*
 * Bind the device copy of A and a scratch buffer (both caller-owned).
 * Replaces init_gpu_array (gpu_calculation.py:222-236), whose H2D copy and
 * pycuda allocations become caller-side PyTorch allocations.
 */
int bpgl_bind(bpgl_ctx* ctx, const void* A, int64_t lda, int64_t block_stride,
              void* scratch, int64_t scratch_bytes);

/*
 * diag(A_b^T A_b) for every block b into out[b * w_pad + j] (device, fp64).
 * Replaces GPU_Calculation.diag_ATA + kernel get_diag_ATA
 * (gpu_calculation.py:246-261, :116-137).  Also caches 1/diag for the solver.
 */
int bpgl_diag_ata(bpgl_ctx* ctx, double* out);

/*
 * Install diag(A_b^T A_b) (device, nblock * w_pad fp64) computed elsewhere, and
 * 1/diag.  Used by external-exchange row shards, whose column norms are sums of
 * every rank's bpgl_diag_ata output (the RCCL path does that sum itself).
 */
int bpgl_set_diag(bpgl_ctx* ctx, const double* diag);

/*
 * g = A_b^T r  (device: r has m fp64 values, g receives w_pad fp64 values).
 * Replaces GPU_Calculation.mat_tMulVec_DiffSize + kernel mul_mat_t_vec_diffsize
 * (gpu_calculation.py:264-277, :20-55); the split-K reduction happens on the
 * device in a fixed order (no host partial sums, no atomics).
 */
int bpgl_mtv(bpgl_ctx* ctx, int32_t block, const double* r, double* g);

/*
 * s = A_b d  (device: d has w_pad fp64 values, s receives m fp64 values).
 * Replaces GPU_Calculation.matMulVec_DiffSize + kernel mul_mat_vec_diffsize
 * (gpu_calculation.py:280-292, :58-91).
 */
int bpgl_mv(bpgl_ctx* ctx, int32_t block, const double* d, double* s);

/*
 * Multi-GPU: column shards of every feature block across ranks (the
 * reference's P-way shards, cpu_calculation.py:23-27 / lasso.py:107-126,
 * lifted from Pool workers to GPUs).  bpgl_comm_unique_id fills 128 bytes on
 * one rank; the caller broadcasts them; every rank then calls bpgl_comm_init.
 * The solver then all-reduces (RCCL, SUM) m + 2 + nranks fp64 values per
 * iteration.
 */
int bpgl_comm_unique_id(void* out128);
int bpgl_comm_init(bpgl_ctx* ctx, const void* unique_id128, int rank, int nranks);

/*
 * Shard layout across ranks (call between bpgl_create and bpgl_bind):
 * BPGL_SHARD_COLUMNS (default) as above; BPGL_SHARD_ROWS: one feature block, rank
 * q holds rows [m_q, m_{q+1}) of A (the context's m is its row count, n_local the
 * full width), b and the residual are local, x is replicated.  Row shards run the
 * one-pass iteration (A read once per iteration): per iteration one all-reduce
 * (SUM) of [A^T A D | r.s23 | s23.s23 | failed] -- w_pad + 3 fp64, or (opt-in
 * tuning key "exchange_fp32") w_pad + 5 fp32 (U rounded, the scalars as hi + lo
 * pairs; fp32-accurate once summed over several ranks);
 * bpgl_diag_ata and every
 * exact gradient refresh all-reduce w_pad values.  There is no reference
 * counterpart: the reference shards columns only (cpu_calculation.py:23-27).
 */
enum { BPGL_SHARD_COLUMNS = 0, BPGL_SHARD_ROWS = 1 };
int bpgl_set_shard(bpgl_ctx* ctx, int mode);

/*
 * Caller-performed exchange (validation of the sharded kernels where RCCL
 * cannot run, e.g. several ranks on one GPU): bpgl_set_ranks declares this
 * context rank `rank` of `nranks` without a communicator.  Each iteration is
 * then bpgl_solver_phase(ctx, 0); the caller sums the
 * bpgl_solver_exchange_buffer (count = m + 2 + nranks fp64) over ranks and
 * writes the sum back on every rank; bpgl_solver_phase(ctx, 1).  Requires the
 * initial point x = 0.
 */
/* Row shards (count = w_pad + 3): the same two phases per iteration; in
 * addition the exact gradient g = A^T r is exchanged by phase 2 (this rank's
 * A_q^T r_q into the exchange buffer), the caller's sum, and phase 3 -- after
 * bpgl_solver_reset and again every "onepass_refresh" iterations.  With the
 * tuning key "exchange_fp32" = 1 phases 0/1 exchange w_pad + 5 fp32 at the same
 * address instead: [U (w_pad) | r.s23 hi, lo | s23.s23 hi, lo | failed]; phases
 * 2/3 stay fp64.  The `failed` slot is each rank's one-pass failure flag: a
 * nonzero sum makes every rank skip the iteration (bpgl_solver_status then
 * reports BPGL_E_EXCHANGE with the state intact, and the caller re-runs it). */
int bpgl_set_ranks(bpgl_ctx* ctx, int rank, int nranks);
int bpgl_solver_phase(bpgl_ctx* ctx, int phase);
double* bpgl_solver_exchange_buffer(bpgl_ctx* ctx, int64_t* count);

/*
 * Device-resident solver (the loop of ClassLasso.run, lasso.py:190-292, and
 * ClassLassoCB_v2.run, lasso.py:458-613, with every step on the device).
 *
 * bpgl_solver_reset: b (m, device fp64), x (nblock * w_pad, device fp64, in/out,
 *   initial point), order (device int32 block index per iteration, NULL =
 *   cyclic t % nblock as lasso.py:40-41), order_len, err_bound (< 0 disables
 *   the ERR_BOUND stopping rule of lasso.py:141-150), err_iter / time_iter
 *   (device fp64, NULL = not recorded; record_len entries of err_iter and
 *   record_len + 1 of time_iter, as lasso.py:54-62).
 * bpgl_solver_step: enqueue n_iter more iterations (asynchronous; with
 *   `use_graph`, replays of the captured hipGraphs of 1, 2, 4, ... iterations,
 *   the largest that fits each time -- tuning key "graph_max").
 * bpgl_solver_status: synchronise the stream and read (iterations done,
 *   stopped flag, last t, last step size, last error).  It also completes
 *   iterations a one-pass launch lost: a launch whose blocks were not all
 *   resident (another kernel or process held CUs) commits nothing, nor does
 *   any later iteration until this call re-runs them on the two-pass kernels,
 *   which stay in use for the rest of the solve (RCCL row shards: the two-pass
 *   row iteration, two passes over the local rows and two all-reduces per
 *   iteration; every rank switches at the same iteration, so RCCL row-shard
 *   ranks must all call it at the same point: the recovery is collective --
 *   it enqueues all-reduces, so every rank must enter bpgl_solver_status
 *   concurrently, one process or thread per rank).
 * bpgl_solver_stat: counters since the last reset -- "onepass" (1 while the
 *   one-pass iteration is in use), "refresh_period" (iterations between
 *   exact-gradient refreshes, 0 = none), "refreshes" (exact-gradient refreshes
 *   enqueued), "fallbacks" (recoveries above), "requested"
 *   (iterations asked of bpgl_solver_step), "enqueued", "cus" (CUs the
 *   persistent grid is sized for), "cu_masked" (1: narrower than the device,
 *   from the stream's CU mask), "onepass_grid" (its blocks), "onepass_rows" (1:
 *   the row groups own interleaved rows, see "onepass_rows" under bpgl_set_tuning).
 * bpgl_solver_residual: device pointer of the residual s11 = sum_k Ax_k - b (m).
 */
int bpgl_solver_reset(bpgl_ctx* ctx, const double* b, double mu, double* x,
                      const int32_t* order, int64_t order_len, double err_bound,
                      double* err_iter, double* time_iter, int64_t record_len,
                      int use_graph);
int bpgl_solver_step(bpgl_ctx* ctx, int64_t n_iter);
int bpgl_solver_status(bpgl_ctx* ctx, int64_t* iters_done, int* stopped, int64_t* t_last,
                       double* gamma, double* err);
int bpgl_solver_stat(bpgl_ctx* ctx, const char* key, int64_t* value);
const double* bpgl_solver_residual(bpgl_ctx* ctx);

/*
 * Optimality certificate and gap-safe screening at the solver's current point (single rank, since
 * ABI 303).  With r = A x - b, g = A^T r over ALL feature blocks and d_j = ||a_j||^2 (the diag):
 *   primal = 1/2 ||r||^2 + mu ||x||_1
 *   scale  = min(1, mu / ||g||_inf)  (1 when g = 0), so that theta = scale r is dual feasible
 *   dual   = -1/2 scale^2 ||r||^2 - scale r.b
 *   gap    = primal - dual >= P(x) - P*   (>= 0 up to rounding)
 *   score_j = scale |g_j| + sqrt(d_j) sqrt(2 max(gap, 0));  score_j < mu proves x*_j = 0.
 * g_all (device, nblock * w_pad fp64, required, caller-owned) receives g, block b at b * w_pad:
 *   an exact A_b^T r per block (never the one-pass iteration's carried gradient).
 * keep (device, nblock * w_pad bytes, may be NULL): keep[b * w_pad + j] = 1 unless score_j < mu
 *   (so a NaN keeps every column); padding entries (j >= w) are 0 and never counted.
 * out6 (host): [primal, dual, gap, scale, ||g||_inf, n_keep]; n_keep = nblock * w when keep is NULL.
 * The call first does what bpgl_solver_status does (synchronises, re-runs iterations a failed
 * one-pass launch lost), enqueues its work and synchronises again.  It is read-only for the
 * solve: x, r, the carried gradient, the refresh schedule and every stat counter are unchanged,
 * and its reductions have a fixed order (two calls on the same state return the same bits).
 * BPGL_E_STATE: before bpgl_solver_reset, before a diag is installed, or on any multi-rank
 * context (RCCL communicator, bpgl_set_ranks, row shards).
 */
int bpgl_solver_gap(bpgl_ctx* ctx, double* g_all, uint8_t* keep, double* out6);

/*
 * Column gather: A_out[i * lda_out + c] = A(i, cols[c]) for 0 <= c < n_out, in the context's
 * dtype.  cols (device, n_out int32) holds global column indices b * w + j, resolved through
 * the bound lda / block_stride, in any order; an index outside [0, nblock * w) (-1 by
 * convention) writes 0, as do the columns c in [n_out, lda_out).  A_out: device, 16-byte
 * aligned, row-major [m][lda_out], not overlapping A; lda_out >= n_out and a multiple of 16
 * bytes' worth of elements (so A_out can be bound in place by a new context).  Enqueued on the
 * context's stream; about one pass over A.  BPGL_E_ARG on bad arguments.
 */
int bpgl_gather_columns(bpgl_ctx* ctx, const int32_t* cols, int64_t n_out, void* A_out,
                        int64_t lda_out);

/*
 * One-call form: reset, run n_iter iterations, wait (bpgl_solver_status, so lost
 * one-pass iterations are re-run whether or not iters_done is given), report.
 * The survey's bpgl_iterate.  iters_done may be NULL.
 */
int bpgl_iterate(bpgl_ctx* ctx, int64_t n_iter, const int32_t* order, double mu,
                 const double* b, double* x, double* err_iter, double* time_iter,
                 double err_bound, int64_t* iters_done);

/* Timing of the most recent bpgl_solver_step window on the context stream:
 * average duration (ms) of each kernel kind over the window, measured with
 * HIP events when profiling was enabled by bpgl_set_kernel_timing(ctx, 1).
 * kinds: 0 colpass (A^T r), 1 shrink, 2 rowpass (A D), 3 rowreduce (+ line
 * search on one rank), 4 allreduce, 5 step (multi-rank line search), 6 update
 * (+ gradient update in one-pass mode), 7 onepass (A D and A^T (A D) in one
 * pass over A), 8 refresh (the one-pass exact-gradient refresh, amortised:
 * its total time over the window's iterations).  Row shards: 3 = fold of the
 * exchange contribution (the line search runs in 6). */
int bpgl_set_kernel_timing(bpgl_ctx* ctx, int enable);
int bpgl_kernel_times(bpgl_ctx* ctx, double* avg_ms /* 9 */, int64_t* samples);

/* Runtime tuning knobs (call before bpgl_solver_reset).  These do not change
 * results:
 *   "nt_loads" (default 1): stream A with non-temporal loads.
 *   "tail_permille" (default 120): with nt_loads, the share of every row chunk
 *   each pass reads last with cache-allocating loads (Infinity Cache reuse by
 *   the other pass).
 *   "reverse_rows" (default 0): the A D pass walks each row chunk bottom-up.
 *   "tail_row_blocks" (default 1): the one-pass tail runs the residual update on
 *   blocks of its own, beside its column blocks (0: every block first).
 *   "graph_max" (default 64; a power of two, at most 8 with an RCCL communicator):
 *   the largest hipGraph of iterations bpgl_solver_reset captures (use_graph).
 * These select the iteration's arithmetic path (results agree to rounding,
 * each path is bitwise deterministic):
 *   "onepass" (default -1 = when eligible, 0 = off, 1 = required): one pass
 *   over A per iteration, the gradient carried as g += gamma A^T (A D); needs
 *   one feature block, one rank (or row shards), at most
 *   128 x 4096 columns (fp32; 128 x 6144 for bf16, 128 x 2048 for fp64) and all
 *   of its blocks resident at once (nothing else running on the device): its segment
 *   blocks per row must fit the CUs the stream may use.  When they do not (e.g. a
 *   row of 524288 fp32 columns on a 64-CU partition), auto runs two passes; RCCL
 *   row shards then run the two-pass row iteration (exact g through an all-reduce
 *   of w, s23 on the local rows) -- since ABI 302; before, such a context was refused.
 *   "onepass_cache_permille" (default -1 = auto: 750 when this rank's A block is
 *   at most 320 MiB, i.e. about the 256 MiB Infinity Cache, else 0): share of every
 *   row group the one-pass kernel reads with cache-allocating loads (launches
 *   alternate the row direction, so the next launch starts on those rows).
 *   "onepass_rows" (default -1 = auto: interleaved when there are at least 8 row
 *   groups of at least 128 rows over at least 16 segment blocks, else 0): 1 = row
 *   group g of the one-pass kernel owns rows g, g + ngroups, ... (the groups read
 *   adjacent rows at once; with at most 64 segment blocks per row, else always 0),
 *   0 = R consecutive rows; bpgl_solver_stat("onepass_rows") reports the form in use.
 *   "onepass_sb1" (default -1 = on when a row is one segment block, 0 = off): with one
 *   segment block per row (e.g. 4096 fp32 columns) the row's s23 is folded from the 4 wave
 *   partials in LDS instead of a tagged granule through memory (configs[3] +2 %; results agree
 *   with the granule path to its parity bit; an explicit "onepass_rows" = 1 selects the
 *   granule path); bpgl_solver_stat("onepass_sb1") reports it.
 *   "onepass_refresh" (default 256; 0 = only at reset): recompute g = A^T r
 *   exactly every this many iterations (bounds the recurrence's drift).
 *   "exchange_fp32" (default 0 = never, -1 = with an RCCL communicator, 1 = also for
 *   a caller-side exchange): row shards' per-iteration exchange in fp32 -- half the
 *   bytes, x within 2e-7 (1 rank) to 1.5e-6 (8 ranks, 120 iterations) of the fp64 exchange;
 *   5.7e-6 from the one-GPU path after 300 iterations at 8 ranks (round 6: kept opt-in).
 *   "onepass_fail_at" (test hook, default -1): the one-pass launch of iteration t
 *   reports a row hand-off failure once (exercises the recovery above).
 *   "cus" (before bpgl_bind only; default: the stream's CU mask, else the device):
 *   the CU count the persistent one-pass grid (row groups x segment blocks) is
 *   sized for.
 * The environment variable BPGL_TARGET_BLOCKS (read by bpgl_create) sets the
 * number of (row chunk x column segment) tiles per two-pass launch (default
 * 1024 for fp32 A, 512 for fp64 / bf16). */
int bpgl_set_tuning(bpgl_ctx* ctx, const char* key, int64_t value);

/* Launch geometry chosen for this context (diagnostics). */
int bpgl_geometry(const bpgl_ctx* ctx, int32_t* nseg, int32_t* nchunk, int32_t* rows_per_chunk,
                  int32_t* seg_width);

/* ===========================================================================
 * Panel path (BASELINE configs[4]): nrhs in {16, 32, 64, 128} right-hand sides
 * solved together, A stored once in bf16 (row-major A [m][lda], caller-owned;
 * the A^T pass reads it through transposing LDS reads), both passes on CDNA4
 * MFMA (v_mfma_f32_16x16x32_bf16) with split-bf16 operands.  The reference
 * has no batched solver: each RHS follows the single-RHS iteration of
 * lasso.py:102-157 (cyclic blocks, fixed iteration count).  m and the block
 * width must be multiples of 256.  Layouts: B, R [nrhs][m]; G, D [nrhs][w];
 * x [nblock][nrhs][w] fp32.
 * =========================================================================== */
typedef struct bpgl_panel bpgl_panel;
int bpgl_panel_create(bpgl_panel** out, int device, int64_t m, int64_t n, int32_t nblock, int32_t nrhs,
                      int32_t kchunks /* <= 0: automatic */, void* hip_stream);
void bpgl_panel_destroy(bpgl_panel* ctx);
int64_t bpgl_panel_scratch_bytes(const bpgl_panel* ctx);
/* bind COPIES A's contents into two tiled m x n bf16 images inside the scratch (one per pass: each pass's
 * 64-deep stage is then one contiguous 32 KiB), so bpgl_panel_scratch_bytes includes 4 m n bytes for
 * them on top of the vectors.  The solver passes and bpgl_panel_mtm / _mm read those copies; only
 * bpgl_panel_diag reads A itself.  A must stay valid while the context is bound, and after A's
 * contents change the context must be bound again (the copies are not refreshed).  The fused
 * reduce + update form ("fuse_update" below) is admitted at bind only if its blocks fit on the CUs
 * the context's stream may use (a CU-masked stream counts its own CUs; stat "fuse_cus"). */
int bpgl_panel_bind(bpgl_panel* ctx, const void* A /* [m][lda] bf16 */, int64_t lda, void* scratch,
                    int64_t scratch_bytes);
int bpgl_panel_diag(bpgl_panel* ctx, double* out /* nullable, n fp64 */);
/* G = A_b^T R  and  S = A_b D  (fp64 in/out, device; split-bf16 MFMA inside) */
int bpgl_panel_mtm(bpgl_panel* ctx, int32_t block, const double* R, double* G);
int bpgl_panel_mm(bpgl_panel* ctx, int32_t block, const double* D, double* S);
int bpgl_panel_reset(bpgl_panel* ctx, const double* B, const double* mu /* nrhs */, double* err_iter,
                     int64_t record_len, int use_graph);
int bpgl_panel_step(bpgl_panel* ctx, int64_t n_iter);
int bpgl_panel_status(bpgl_panel* ctx, int64_t* iters, double* last_err);
const float* bpgl_panel_x(bpgl_panel* ctx);
int bpgl_panel_set_kernel_timing(bpgl_panel* ctx, int enable);
int bpgl_panel_kernel_times(bpgl_panel* ctx, double* avg_ms /* 5: pass1, pass2, reduce (+ line search), step (0: folded into reduce), update */,
                            int64_t* samples);
/* tuning knobs.  Results are bitwise independent of these: "interleave1",
 * "interleave2" (pass 1 / pass 2; "interleave" sets both) 0/1/2 -- LDS-DMA
 * pieces issued together after each stage barrier (0), spread over the stage's
 * MFMA groups (1), or spread and software-pipelined with fragment reads one MFMA
 * group ahead across the stage barrier (2).  Defaults: pass 1 -- 2; pass 2 -- 2 with the bf16 direction
 * (d_split 1) at k >= 64, else 1 (round 4); get_tuning reports the form in use.
 * This one selects the solver's arithmetic (every choice is an exact line
 * search along the direction it takes): "d_split" 1 (default since ABI 200) --
 * the direction enters the A D pass as its bf16 rounding alone (half the
 * pass-2 MFMA work); 2 -- as a hi + lo bf16 pair (~16-bit mantissa).  Both
 * converge to the same solution: after the reference's 1000 iterations at the
 * configs[4] shape both are within 1.7-2.2e-5 of the fp64 oracle on x and 1e-11
 * on the objective (the gradient pass, hi + lo always, sets the fixed point;
 * profiles/r04/accuracy); short runs follow slightly different trajectories.
 * bpgl_panel_mtm / _mm always use hi + lo operands.  bpgl_panel_get_tuning reads
 * "interleave1", "interleave2", "d_split", "defer_x", "carry_g", "g_refresh", "fuse_update",
 * "fuse_grid".
 * "fuse_update" (0 / 1; default 1; in effect with one feature block, defer_x and m a multiple of
 * 1024 -- get_tuning reports the form in effect; a reset must follow a change): the split-K reduce, each
 * RHS's line search and R += gamma S run as ONE launch whose blocks wait for their RHS's step size
 * (bitwise the two-kernel result); it needs its blocks co-resident, which bpgl_panel_bind checks with
 * the occupancy API against the stream's usable CUs (its CU mask, else the device) -- should a wait still run out (another kernel holding CUs), nothing is updated and
 * bpgl_panel_status returns BPGL_E_EXCHANGE.  "fuse_grid" (256 / 512 / 1024, default 1024): its grid.
 * "defer_x" (0 / 1; default 1, one feature block; a reset must follow a change): the
 * update x += gamma D' of an iteration is applied by the next pass-1 epilogue (and at
 * the end of every bpgl_panel_step), bitwise the same x.
 * "carry_g" (0 / 1; default 1, in effect with one feature block only -- set to 1
 * with more blocks is an error; a reset must follow a change): the gradient is
 * carried in fp32, G_t = G_{t-1} + gamma_{t-1} A^T S_{t-1} with S_{t-1} = A D'_{t-1}
 * the previous iteration's product (its bf16 image: one MFMA product in pass 1
 * instead of the residual's two), and recomputed exactly from R (hi + lo) every
 * "g_refresh" iterations (default 64, a multiple of 8) -- the single-RHS path's
 * carried gradient.  Measured at configs[4]: pass 1
 * 226 -> 196 us, and after 1000 iterations x within 4e-6 of the oracle instead of
 * 1.9e-5 (fp32 accumulation of small updates instead of re-reading R through its
 * 2^-17 pieces).  get_tuning("carry_g") reports the form in effect. */
int bpgl_panel_set_tuning(bpgl_panel* ctx, const char* key, int64_t value);
int bpgl_panel_get_tuning(const bpgl_panel* ctx, const char* key, int64_t* value);
int bpgl_panel_geometry(const bpgl_panel* ctx, int32_t* kchunks);
/* Counters since the last reset: "iters_enqueued", "exact_gradients" (carried
 * gradient: iterations whose pass 1 computed G = A^T R exactly -- every g_refresh-th).
 * Of the last bpgl_panel_gap (HIP events, nanoseconds): "gap_prod1_ns", "gap_prod2_ns". */
int bpgl_panel_stat(const bpgl_panel* ctx, const char* key, int64_t* value);
/* The solver's fp64 residual R = A X - B, [nrhs][m] in device memory (valid after
 * the stream has drained). */
const double* bpgl_panel_residual(bpgl_panel* ctx);
/*
 * Optimality certificate of the STORED iterate, per right-hand side (since ABI 304).  The fp32 x of
 * every feature block and the bf16 A (read from the caller's row-major image, widened to fp64, which
 * is exact) enter two fp64 panel products (v_mfma_f64_16x16x4_f64):
 *   R_fresh[k][i]  = sum_j A[i][j] x_k[j] - B[k][i]        (all feature blocks)
 *   G_all[b][k][j] = sum_i A[i][b w + j] R_fresh[k][i]     (from R_fresh: never the solver's R, its
 *                                                          bf16 images or the carried gradient)
 * and, with mu_k and d_j = ||a_j||^2 (the diag), the formulas of bpgl_solver_gap above give per k
 *   out[8 k + 0..7] = primal, dual, gap, scale, ||g||_inf, n_keep, drift, 0 (the held-out sum of
 *                     squares with a row mask, bpgl_panel_set_row_mask below)
 * with drift_k = max_i |R[k][i] - R_fresh[k][i]| against the solver's recurrence residual.
 * G_all (device, [nblock][nrhs][w] fp64) and R_fresh (device, [nrhs][m] fp64): required, 16-byte
 *   aligned, caller-owned.
 * keep (device, [nrhs][n] bytes, may be NULL): keep[k][j] = 1 unless score_j < mu_k (a NaN keeps every
 *   column); n_keep = n when keep is NULL.
 * out: host, nrhs x 8 doubles.
 * The call first does what bpgl_panel_status does (synchronises; BPGL_E_EXCHANGE as there), enqueues
 * on the context's stream and synchronises again.  It relies on bpgl_panel_step having applied the
 * deferred x update (it always has).  Read-only for the solve: X, R and its bf16 images, the
 * direction images, the carried gradient and its operands, the iteration and exact-gradient counters,
 * the device state, the captured graphs and the solver's validity are untouched, so a following
 * bpgl_panel_step continues bitwise as if the call had not happened.  Every reduction has a fixed
 * order and there are no floating-point atomics: two calls on the same state return the same bits.
 * Cost: 2 m n nrhs fp64 multiply-adds -- checkpoint work, not per-iteration work.
 * BPGL_E_STATE before bpgl_panel_reset or before bpgl_panel_diag; BPGL_E_ARG on a null or misaligned
 * required pointer.
 */
int bpgl_panel_gap(bpgl_panel* ctx, double* G_all, double* R_fresh, uint8_t* keep, double* out);
/*
 * Row mask (since ABI 305): 0/1 row weights w_k per right-hand side, so that one
 * panel holds problems that leave different rows of the shared A out of their objective,
 *   min_x 1/2 || w_k o (A x - b_k) ||^2 + mu_k ||x||_1        (K folds x J values of mu = one panel).
 * mask: device, [nrhs][m] bytes; a nonzero byte puts row i into right-hand side k's objective, a zero
 *   byte holds it out.  NULL clears the mask.  The library copies it into its scratch on the
 *   context's stream, so the caller's buffer is free once that copy has run.
 * The call invalidates the solver: bpgl_panel_step / bpgl_panel_gap return BPGL_E_STATE until the next
 * bpgl_panel_reset, which still takes the FULL B; the library stores w o B (so R0 = -w o B) and keeps
 * (1 - w) o B for scoring.  The graphs captured at that reset hold the masked kernel variants: the
 * split-K fold replaces S by w o S (by select, so an all-ones mask is bitwise the unmasked run) before
 * the line search, the carried operand and the residual update.  The column norms stay those of the
 * full A.  bpgl_panel_residual then returns w o (A x - b) (exactly 0 at held-out rows), and
 * bpgl_panel_gap certifies the masked problems: R_fresh[k][i] = w_ki (a_i . x_k - b_ki), G from it,
 * primal, dual, gap, scale, ||g||_inf and drift on the masked problem, the screen with the full diag
 * (safe, merely conservative), and out[8 k + 7] = sum_i (1 - w_ki)(a_i . x_k - b_ki)^2, the held-out
 * sum of squares (fixed-order, like every other output).  bpgl_panel_mm / _mtm are untouched.
 * Legal any time after bpgl_panel_bind (BPGL_E_STATE before it; BPGL_E_ARG on a null context); the
 * fused update's occupancy check is repeated for the variant that will run.
 */
int bpgl_panel_set_row_mask(bpgl_panel* ctx, const uint8_t* mask);
/*
 * Intercept (since ABI 307): with `on` nonzero every right-hand side solves
 *   min over x, beta0 of 1/2 || w_k o (A x + beta0 1 - b_k) ||^2 + mu_k ||x||_1
 * with beta0 unpenalised.  beta0 is profiled out: the objective is 1/2 ||P_w (A x - b)||^2 + mu ||x||_1 with
 * P_w v = w o (v - (w . v) / n_w) (centre over the in-rows, n_w = sum w), and the solver carries the
 * centred residual R = P_w (A x - b).  Pass 1 and pass 2 are the unchanged kernels; the split-K fold
 * publishes one more partial per 1024-row group (sum s), the line search uses c = sum s / n_w
 * (|P_w s|^2 = s.s - c sum s; gamma = 0 when that is <= 0) and publishes c beside gamma, and the update
 * adds gamma (s - c) at the in-rows and leaves the held-out rows exactly 0.
 * The call installs what the variant needs: without a caller's mask an all-ones mask of the library's own
 * (bpgl_panel_set_row_mask(NULL) then re-installs it; a caller's mask is kept and its rows recounted);
 * the in-row counts n_w; and the diag that fits -- on: d_j = sum_i (a_ij - mean_j)^2 over ALL rows (two
 * fixed-order fp64 walks: means, then squared deviations), which dominates every fold's curvature
 * ||P_w a_j||^2, with 1 / d_j = 0 stored where d_j = 0 (a constant column: its x stays 0, the intercept
 * absorbs it); off: bpgl_panel_diag's values, bitwise.  bpgl_panel_diag afterwards returns the diag in effect.
 * It invalidates the solver and drops the graphs exactly as bpgl_panel_set_row_mask does (bpgl_panel_step /
 * bpgl_panel_gap return BPGL_E_STATE until the next reset) and repeats the fused update's occupancy check.
 * The reset still takes the full B; the library stores P_w B (so R0 = -P_w B) and (1 - w) o B.
 * Limits: the intercept is built for one feature block with the deferred x update only.  With it on,
 * bpgl_panel_reset / bpgl_panel_reset_x0 return BPGL_E_STATE for nblock > 1 and for the tuning key
 * defer_x = 0.  An all-zero mask column (n_w = 0) takes no steps and reports zeros.
 * bpgl_panel_gap then certifies the profiled problems: R_fresh = P_w (A x - b) (exactly 0 at held-out rows;
 * it sums to zero over the in-rows, which is the intercept's dual constraint), G, primal, dual, gap, scale,
 * ||g||_inf and drift from it, the screen with the centred diag, and out[8 k + 7] = the held-out sum of
 * (a_i . x_k + beta0_k - b_ki)^2, each difference squared directly.  bpgl_panel_reset_x0 starts at
 * R = P_w (A X0 - B) through the same kernels, so a certificate right after it reports drift 0.
 * Legal any time after bpgl_panel_bind (BPGL_E_STATE before it; BPGL_E_ARG on a null context).
 */
int bpgl_panel_set_intercept(bpgl_panel* ctx, int on);
/*
 * beta0_k = -mean over the in-rows of (a_i . x_k - b_ki) at the x of the last bpgl_panel_gap (since ABI
 * 307).  out: host, nrhs doubles.  BPGL_E_STATE if no bpgl_panel_gap has run since the last reset; zeros
 * (and no such requirement) with the intercept off.
 */
int bpgl_panel_intercept(bpgl_panel* ctx, double* out);
/*
 * Non-negative lasso (since ABI 308): with `on` nonzero every right-hand side solves
 *   min 1/2 || w_k o (A x - b_k) ||^2 + mu_k sum_j x_j   subject to x >= 0
 * (with the row mask and / or the intercept's profiling when those are installed).  Only the pass-1 shrink
 * changes: the prox is the one-sided threshold x^_j = max(0, S(d_j x_j - g_j, mu) / d_j), and the direction's
 * bf16 image D' is made feasible -- where the nearest image has x + D' < 0 (a coordinate sent to 0:
 * bf16(-x) can exceed x in magnitude) it is replaced by its neighbour towards zero (d_split 1), or the lo
 * piece is moved one step up (d_split 2), so that x + D' >= 0 in the fp64 arithmetic that applies it.  The
 * step size lies in [0, 1], so EVERY stored iterate is >= 0 (no clamp after the update: R is a recurrence and
 * must stay A dx).  Pass 2, the fold, the line search (sum |x + D'| is sum (x + D')) and the updates are the
 * unchanged kernels.  The error record is the constrained prox residual max |x - max(0, x - g - mu)|.
 * bpgl_panel_gap then certifies the constrained problem: the dual constraint is one-sided, -a_j . theta <= mu,
 * so out[8 k + 4] is max_j (-g_j)+ instead of ||g||_inf, scale = min(1, mu / that) (1 when it is 0), primal,
 * dual and gap keep their formulas, and the screen is score_j = scale (-g_j) + sqrt(d_j) sqrt(2 max(gap, 0)),
 * keep_j = !(score_j < mu).  At x = 0 out[8 k + 4] is max_j (a_j . b)+: above it x = 0 is optimal.
 * drift, the held-out sum of squares and the intercept keep their meaning.
 * bpgl_panel_reset_x0 with the constraint on starts at X = max(X0, 0) elementwise -- X0 bitwise where
 * X0 >= 0 (-0 becomes +0), also for the in-place restart X0 == bpgl_panel_x(ctx) -- and forms R from that
 * projected X, so a certificate right after it reports drift 0 (one feature block).
 * It invalidates the solver and drops the graphs exactly as bpgl_panel_set_row_mask does (bpgl_panel_step /
 * bpgl_panel_gap return BPGL_E_STATE until the next reset); bpgl_panel_bind switches it off.
 * bpgl_panel_get_tuning("positive") reports it.  With it off every result is bitwise what ABI 307 computes.
 * Legal any time after bpgl_panel_bind (BPGL_E_STATE before it; BPGL_E_ARG on a null context).
 */
int bpgl_panel_set_positive(bpgl_panel* ctx, int on);
/*
 * Penalty factors (since ABI 309): with `pen` non-NULL every right-hand side solves
 *   min 1/2 || w_k o (A x - b_k) ||^2 + mu_k sum_j p_j |x_j|
 * (with the row mask, the intercept's profiling and / or x >= 0 when those are installed).  pen: device fp64 [n],
 * global column order (feature block b holds pen[b w .. (b + 1) w)), one vector for all right-hand sides; it is
 * copied into the context's scratch and the call returns when the copy is done, so the caller's buffer is free after it.  NULL switches it off.
 * The factors are used as given: there is no renormalisation to sum p = n (glmnet rescales; multiply by
 * n / sum p before the call for its convention).  Every entry must be finite and > 0: a validation kernel reads
 * the vector (one readback: a set-up call) and BPGL_E_ARG is returned, with nothing changed -- the factors
 * installed before stay in force -- when one is not.  (p_j = 0, an unpenalised column, makes the scaled residual
 * dual infeasible and needs profiling out as the intercept does; p_j = inf is a column to leave out.)
 * With tau_j = mu_k p_j and d_j the diag in effect, only the pass-1 shrink and two certificate kernels change:
 *   prox          x^_j = S(d_j x_j - g_j, tau_j) / d_j (max(0, .) with x >= 0; 0 where 1 / d_j is stored as 0)
 *   norms         sbx = sum_j p_j |x_j + D'_j|, sx = sum_j p_j |x_j|; the line search rs + mu (sbx - sx) is
 *                 unchanged and stays the exact line search of the weighted objective along D'
 *   error record  max_j |g_j - clip(g_j - x_j, -tau_j, tau_j)| (with x >= 0: |x_j - max(0, x_j - g_j - tau_j)|)
 *   certificate   primal = 1/2 |r|^2 + mu sum_j p_j |x_j|; out[8 k + 4] is max_j |g_j| / p_j (max_j (-g_j)+ / p_j
 *                 with x >= 0) instead of ||g||_inf; scale = min(1, mu / that), so theta = scale r has
 *                 |a_j . theta| <= mu p_j; dual and gap keep their formulas
 *   screen        score_j = scale |g_j| + sqrt(d_j) sqrt(2 max(gap, 0)) (-g_j for |g_j| with x >= 0),
 *                 keep_j = !(score_j < mu_k p_j)
 * At x = 0 out[8 k + 4] is max_j |a_j . b| / p_j: above it x = 0 is optimal (mu_max).  Pass 2, the fold, the
 * line search, the updates, the carried gradient and every other certificate kernel are the unchanged kernels.
 * A vector of ones computes the bits that NULL computes (mu * 1.0 and 1.0 * |x| are exact).
 * It invalidates the solver and drops the graphs exactly as bpgl_panel_set_positive does (bpgl_panel_step /
 * bpgl_panel_gap return BPGL_E_STATE until the next reset); bpgl_panel_bind switches it off.
 * bpgl_panel_get_tuning("penalty") reports it.  With it off every result is bitwise what ABI 308 computes.
 * Legal any time after bpgl_panel_bind (BPGL_E_STATE before it; BPGL_E_ARG on a null context).
 */
int bpgl_panel_set_penalty(bpgl_panel* ctx, const double* pen);
/*
 * Observation weights (since ABI 310): with `wt` non-NULL right-hand side k solves
 *   min 1/2 sum_i w_ki (a_i . x - b_ki)^2 + mu_k sum_j p_j |x_j|
 * (with the intercept's profiling -- then over the weighted mean --, x >= 0 and / or the penalty factors when those
 * are installed).  wt: device fp64 [nrhs][m], every entry finite and in [0, 1] (scale larger weights by their
 * maximum c and pass mu / c: the minimiser is the same).  hold: device fp64 [nrhs][m] or NULL, every entry finite
 * and >= 0: the scoring weights h of out[8 k + 7] = sum_i h_ki e_ki^2, e = a_i . x_k - b_ki (+ beta0 with the
 * intercept); NULL means h = 1 where wt is 0 and 0 elsewhere, the row mask's rule.  A validation kernel reads both
 * (one readback: a set-up call) and BPGL_E_ARG is returned, with nothing changed -- whatever was installed before
 * stays in force -- when an entry is out of range.  Both are copied into the context's scratch and the call
 * returns when the copies are done, so the caller's buffers are free after it.  wt == NULL clears the weights
 * (`hold` is then ignored).
 * Weights and a row mask are alternatives and the last call wins: bpgl_panel_set_row_mask clears the weights, and
 * this call (also with wt == NULL) clears a caller's mask.  The order of this call and bpgl_panel_set_intercept does
 * not matter; with the intercept n_w = sum_i w_ki (fp64, fixed order) stands where the in-row count stood and every
 * mean is the weighted one.  bpgl_panel_diag still returns the diag in effect, over all rows: d_j >= sum_i w_i a_ij^2
 * because w <= 1, so the step and the screen stay safe.
 * What the solver carries is R^ = w o (A x - b) (bpgl_panel_residual; exactly 0 at the zero-weight rows from the
 * reset on), the stored B is w o B, pass 1 and pass 2 are the unchanged kernels, and the fold differs:
 *   fold          s^ = w o s
 *   line search   rs = sum_i R^_i s_i (the UNWEIGHTED s), ss = sum_i s_i s^_i; gamma = clip(-(rs + mu (sbx - sx)) / ss, 0, 1),
 *                 0 when ss = 0; with the intercept sm = sum s^, c = sm / n_w, curvature ss - c sm
 *   update        R^ += gamma s^ (with the intercept gamma (s^ - c w)); the carried operand takes the same step
 *   certificate   R_fresh = w o e (w o (e - ebar_w) with the intercept) and G = A^T R_fresh; primal = 1/2 sum w e^2 +
 *                 mu sum p |x|, dual = -1/2 s^2 sum w e^2 - s sum w e b, both sums formed from e where a_i . x is at
 *                 hand, never by dividing R_fresh by w; scale, gap, out[8 k + 4] and the screen as without weights;
 *                 drift = max |R^ - R_fresh|; beta0 = -sum w e / n_w
 * With every w in {0, 1} each of these is, term for term, what the row mask computes.  A right-hand side whose
 * weights are all 0 takes no steps and reports zeros.
 * One feature block with the deferred x update: with weights installed bpgl_panel_reset and bpgl_panel_reset_x0
 * return BPGL_E_STATE for nblock > 1 and for the tuning key defer_x = 0.  bpgl_panel_reset_x0 starts at
 * R^ = w o (A X0 - B) (centred with the intercept) through the certificate's product 1.
 * It invalidates the solver and drops the graphs exactly as bpgl_panel_set_row_mask does, and repeats the fused
 * update's occupancy check for the variant that will run; bpgl_panel_bind switches the weights off.
 * bpgl_panel_get_tuning("row_weights") reports them.  bpgl_panel_gather_columns, bpgl_panel_mm and bpgl_panel_mtm
 * are unaffected.  With it off every result is bitwise what ABI 309 computes.
 * Legal any time after bpgl_panel_bind (BPGL_E_STATE before it; BPGL_E_ARG on a null context).
 */
int bpgl_panel_set_row_weights(bpgl_panel* ctx, const double* wt, const double* hold);
/*
 * Warm start (since ABI 306): bpgl_panel_reset at a given iterate.
 * X0: device fp32 [nblock][nrhs][w] (the layout of bpgl_panel_x), 16-byte aligned, caller-owned.
 *   NULL is bpgl_panel_reset exactly (that function is this one with X0 = NULL).  X0 == bpgl_panel_x(ctx)
 *   is legal and means "restart from the stored iterate": nothing is copied.
 * After the call the state is that of a fresh reset at X0: X = X0 bitwise; R = A X0 - B in fp64 from the
 * stored fp32 x and the bf16 A widened exactly -- bpgl_panel_gap's product 1 (the same kernel, reading
 * the caller's row-major A), never bpgl_panel_mm, whose hi + lo bf16 operand would round x to 16 bits;
 * Rh / Rl are that R's images.  With a row mask R = w o (A X0 - B), exactly 0 at held-out rows (by
 * select), and B is stored as bpgl_panel_reset stores it.  With nblock > 1 the product's reduction
 * chunks are aligned to the feature blocks and a fold writes Ax[b] = A_b x_b (its chunks in chunk
 * order) and R = sum_b Ax[b] - B with b in index order, as the update kernel sums them; with
 * nblock == 1 the chunking and the fold are the certificate's own, so a bpgl_panel_gap right after the
 * call reports drift 0.  The iteration and exact-gradient counters, the arrival counters, the pending
 * x update, the carried operand and error-feedback state, err_iter and the graphs are as
 * bpgl_panel_reset leaves them: the first iteration computes the gradient exactly from Rh / Rl.
 * Scratch: the chunk partials go into bpgl_panel_gap's buffer.  With nblock == 1 that buffer is
 * unchanged; with nblock > 1 it is the larger of the certificate's need and nrhs x nblock x
 * pgap_split(m / 64, w / 32) x m doubles, so bpgl_panel_scratch_bytes can be larger than under ABI 305
 * for such shapes (e.g. nblock not a power of two) and is the same for all others.
 * Cost over a plain reset: one product 1 (m n nrhs fp64 multiply-adds).  The new kernels contain no
 * inter-block waits.  Errors as bpgl_panel_reset, plus BPGL_E_ARG for a misaligned X0.
 */
int bpgl_panel_reset_x0(bpgl_panel* ctx, const double* B, const double* mu, const float* X0,
                        double* err_iter, int64_t record_len, int use_graph);
/*
 * Column gather of the bound A (since ABI 306): A_out[i * lda_out + c] = A[i][cols[c]] in bf16, read
 * from the row-major A given to bpgl_panel_bind.  cols: device int32, any order; an index outside
 * [0, n) writes 0, as do the columns c in [n_out, lda_out).  lda_out >= n_out and a multiple of 8;
 * A_out is 16-byte aligned and does not overlap A.  Enqueued on the context's stream (the kernel is
 * bpgl_gather_columns').  BPGL_E_STATE before bpgl_panel_bind, BPGL_E_ARG on bad arguments.
 */
int bpgl_panel_gather_columns(bpgl_panel* ctx, const int32_t* cols, int64_t n_out, void* A_out,
                              int64_t lda_out);

/*
 * The logistic lasso by IRLS on the weighted panel (since ABI 311).  Right-hand side k, with
 * labels y_ki in [0, 1] and prior weights om_ki in [0, 1], solves
 *   min over x, beta0 of sum_i om_i l(eta_i; y_i) + mu sum_j p_j |x_j|,  eta = A x + beta0,  l = log(1 + e^eta) - y eta
 * (x >= 0, the factors p and the intercept as the context has them installed; beta0 = 0 without the intercept).  The
 * inner solves are the weighted lasso as it stands; these two calls are what runs between them.
 *
 * bpgl_panel_glm_model, one outer step at the STORED x (fp32; everything below is fp64 on it and on the bf16 A
 * widened exactly):
 *   AX     = A x: bpgl_panel_gap's product 1 (the same kernel, chunking and launch), its chunk partials folded in
 *            chunk order, nothing subtracted
 *   beta0  with the intercept: the root of phi(beta) = sum_i om_i (sigma(AX_i + beta) - y_i) per right-hand side, by
 *            a Newton iteration started at beta0[k] and safeguarded by a bracket (a step that leaves it becomes the
 *            midpoint), at most 40 steps, stopped at |phi| <= 1e-14 sum om; written back to beta0[k].  A right-hand
 *            side with sum om y = 0 or = sum om has no finite root: its flag is set and beta0[k] is left as it was.
 *   P = sigma(eta);  v = max(P (1 - P), 1e-5) where curv[k] == 0, 1/4 where curv[k] != 0 (Boehning's bound: the
 *            quadratic model then majorises the loss);  W = 4 om v in [0, 1];  Z = eta + (y - P) / v
 *   out[8 k + 0..7] = sum om l, sum h l, sum h [(P > 1/2) != (y > 1/2)], sum om, sum_j p_j |x_j|, the final |phi|,
 *            the Newton steps taken, the flag (1: no finite root)
 * family: BPGL_GLM_BINOMIAL, the only one (BPGL_E_ARG otherwise).  Y, Om, W, Z, P: device fp64 [nrhs][m]; Hd: device
 * fp64 [nrhs][m], the scoring weights h >= 0, or NULL (both scoring sums are then 0); curv: device int32 [nrhs] or
 * NULL (all 0); beta0: device fp64 [nrhs], in / out; out: host, 8 nrhs doubles.  A null or misaligned pointer is
 * BPGL_E_ARG before any HIP call.  Needs a bpgl_panel_reset (or _reset_x0) since bpgl_panel_bind and one feature block
 * (BPGL_E_STATE otherwise).  Waits for the stream, as bpgl_panel_gap does.  Reads X and A only, so the solve may go on
 * after it without a reset, and two calls on the same state return the same bits (fixed-order sums, no atomics).
 *
 * The caller then installs W (and h) with bpgl_panel_set_row_weights and calls bpgl_panel_reset_x0 with B = Z,
 * 4 mu and X0 = bpgl_panel_x: the inner problem 1/2 sum W (a . x + beta0 - Z)^2 + 4 mu sum p |x| is 4 times the
 * quadratic model of the loss at x.  Right after that reset bpgl_panel_residual is 4 om o (P - y), so bpgl_panel_gap's
 * G is the logistic gradient (times 4) and its scale s = min(1, 4 mu / max_j |g_j| / p_j) the dual scaling.
 *
 * bpgl_panel_glm_dual: out[k] = D_k = -sum_i om_i Nh(s_k P_i + (1 - s_k) y_i), Nh(t) = t log t + (1 - t) log(1 - t)
 * with 0 log 0 = 0 -- the dual value at theta = s om o (P - y), so that sum om l + mu sum p |x| - D_k bounds the
 * suboptimality.  P, Y, Om: device fp64 [nrhs][m]; scale, out: host, nrhs doubles.  Fixed-order sums; waits.
 */
#define BPGL_GLM_BINOMIAL 1
int bpgl_panel_glm_model(bpgl_panel* ctx, int family, const double* Y, const double* Om, const double* Hd,
                         const int32_t* curv, double* beta0, double* W, double* Z, double* P, double* out);
int bpgl_panel_glm_dual(bpgl_panel* ctx, const double* P, const double* Y, const double* Om, const double* scale,
                        double* out);

#ifdef __cplusplus
}
#endif
#endif /* BPGL_H */

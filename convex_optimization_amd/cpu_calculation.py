"""Host-side helpers of the reference's ``cpu_calculation`` call surface.

The reference drivers import these eight functions (lasso.py:17-18,
cpu_vs_gpu.py:11) for the host part of each iteration.  They are kept here with
the same names, signatures, shapes and values so those drivers can import this
module in place of the reference's.  They act on host numpy arrays; the device
path (``gpu_calculation``) never calls them.

  soft_thresholding   cpu_calculation.py:5-6    S_tau(t) = sign(t) max(|t| - tau, 0)
  element_proj        cpu_calculation.py:10-11  clip(v, lo, hi)
  error_crit          cpu_calculation.py:15-20  || g - P_[-mu,mu](g - x) ||_inf
  A_bp_get            cpu_calculation.py:23-27  (N, K) -> (BLOCK, P, N, K/(BLOCK P)) view
  fun_s12             cpu_calculation.py:30-31  A_p^T s11
  fun_diag_ATA        cpu_calculation.py:35-42  per-block column sums of squares
  fun_s22             cpu_calculation.py:45-46  A_p s21
  fun_dd_p            cpu_calculation.py:49-50  (w, 1) -> (P, w/P, 1)

New beside them (no counterpart in the reference): ``duality_gap`` and ``gap_safe_keep``, the
numpy fp64 restatement of the device's optimality certificate and screening rule;
``panel_duality_gap``, the same per right-hand side of a panel, and ``mu_grid``, the geometric grid
of a regularization path; ``kfold_masks``, ``masked_panel_iterate`` and ``masked_duality_gap``, the
restatement of the panel's row-masked problems (K-fold cross-validation);
``compaction_columns``, the columns a screened panel keeps when it is compacted;
``centred_diag`` and the ``intercept_*``, ``positive_*``, ``penalty_*`` and ``weighted_*`` pairs
``*_panel_iterate`` / ``*_duality_gap``: the panel's intercept, non-negative lasso (x >= 0), penalty factors
(per-column l1 weights) and observation weights (DESIGN.md sections 13-16).  Those pairs and
``masked_duality_gap`` are thin wrappers of ONE statement of the iteration and ONE of the certificate,
``_panel_iterate`` and ``_panel_gap``; ``masked_panel_iterate`` alone stands beside them,
pinned bitwise to the C oracle.  ``logistic_model``, ``logistic_gap`` and ``logistic_panel_solve`` (with
``logistic_intercept``, ``logistic_dual`` and ``logistic_null_deviance``) restate the logistic lasso's outer step, its
certificate and its IRLS loop, ``_panel_iterate`` being the inner solve.
"""
import numpy as np


def soft_thresholding(tensor, threshold):
    shrunk = np.abs(tensor) - threshold
    np.maximum(shrunk, 0, out=shrunk)
    return np.sign(tensor) * shrunk


def element_proj(vec, lower_bound, upper_bound):
    return np.clip(vec, lower_bound, upper_bound) if np.ndim(vec) else \
        max(min(vec, upper_bound), lower_bound)


def error_crit(grad_fx, x, mu):
    resid = grad_fx - element_proj(grad_fx - x, -mu, mu)
    return np.max(np.abs(resid))


def A_bp_get(A, BLOCK, P):
    rows, cols = A.shape
    width = cols // (BLOCK * P)
    if width * BLOCK * P != cols:
        raise ValueError(f"K={cols} is not divisible by BLOCK*P={BLOCK * P}")
    # column c = (b P + p) width + j  ->  [b, p, :, j]
    return A.reshape(rows, BLOCK, P, width).transpose(1, 2, 0, 3)


def fun_s12(A_bp, s11):
    return A_bp.T @ s11


def fun_diag_ATA(A_bp):
    nblock, nshard, rows, width = A_bp.shape
    sq = np.einsum("bpij,bpij->bpj", A_bp, A_bp)
    return sq.reshape(nblock, nshard * width)[:, :, None]


def fun_s22(A_bp, s21):
    return A_bp @ s21


def fun_dd_p(P, descent_d):
    return np.reshape(descent_d, (P, -1, 1))


# ---------------------------------------------------------------------------
# New beside the reference's eight: the duality-gap certificate and the gap-safe
# screening rule, the host restatement of bpgl_solver_gap.
# ---------------------------------------------------------------------------
def _gap_terms(A, b, x, mu):
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    mu = float(mu)
    r = A @ x - b
    g = A.T @ r
    rr = float(r @ r)
    primal = 0.5 * rr + mu * float(np.abs(x).sum())
    gn = float(np.max(np.abs(g)))                  # NaN propagates
    scale = min(1.0, mu / gn) if gn > 0.0 else 1.0   # theta = scale r is dual feasible
    dual = -0.5 * scale * scale * rr - scale * float(r @ b)
    out = dict(primal=primal, dual=dual, gap=primal - dual, scale=scale, gnorm_inf=gn)
    return A, g, out


def duality_gap(A, b, x, mu):
    """dict(primal, dual, gap, scale, gnorm_inf) of 1/2 ||A x - b||^2 + mu ||x||_1 at x.

    With r = A x - b and g = A^T r: scale = min(1, mu / ||g||_inf) (1 when g = 0), the dual
    point scale r, dual = -1/2 scale^2 ||r||^2 - scale r.b and gap = primal - dual >= P(x) - P*."""
    return _gap_terms(A, b, x, mu)[2]


def gap_safe_keep(A, b, x, mu, return_score=False):
    """bool (K,): False where the gap-safe rule proves x*_j = 0.

    score_j = scale |g_j| + ||a_j|| sqrt(2 max(gap, 0)); column j is kept iff not (score_j < mu),
    so a NaN keeps everything.  ``return_score``: also return the scores."""
    A, g, t = _gap_terms(A, b, x, mu)
    radius = np.sqrt(2.0 * np.maximum(t["gap"], 0.0))
    score = t["scale"] * np.abs(g) + np.sqrt(np.square(A).sum(axis=0)) * radius
    keep = ~(score < float(mu))
    return (keep, score) if return_score else keep


def panel_duality_gap(A, B, X, mu):
    """``duality_gap`` and ``gap_safe_keep`` for every column k of B (m, k) and X (n, k) with mu[k]
    (a scalar serves all): dict of (k,) arrays primal, dual, gap, scale, gnorm_inf, n_keep and
    keep (k, n) bool -- the numpy restatement of bpgl_panel_gap."""
    A = np.asarray(A, dtype=np.float64)
    B = np.ascontiguousarray(np.asarray(B, dtype=np.float64).T)   # rows: contiguous columns, as a caller's own
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float64).T)   # per-column call would pass them
    k = B.shape[0]
    mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), (k,))
    cols = [duality_gap(A, B[j], X[j], mu[j]) for j in range(k)]
    out = {key: np.array([c[key] for c in cols]) for key in ("primal", "dual", "gap", "scale", "gnorm_inf")}
    out["keep"] = np.stack([gap_safe_keep(A, B[j], X[j], mu[j]) for j in range(k)])
    out["n_keep"] = out["keep"].sum(axis=1).astype(np.int64)
    return out


def mu_grid(mu_max, n_mus, hi=0.9, lo=0.1):
    """mu_max * geomspace(hi, lo, n_mus): a decreasing geometric grid below mu_max = ||A^T b||_inf
    (at and above which x = 0 solves the problem)."""
    return float(mu_max) * np.geomspace(hi, lo, int(n_mus))


# ---------------------------------------------------------------------------
# Row masks: min 1/2 || w o (A x - b) ||^2 + mu ||x||_1 with 0/1 row weights w,
# the host restatement of bpgl_panel_set_row_mask's solver and certificate.
# ---------------------------------------------------------------------------
def kfold_masks(m, n_folds, seed=0):
    """(n_folds, m) uint8: mask[f, i] = 0 where row i is held out of fold f, else 1.  The held-out sets
    are the strides perm[f::n_folds] of RandomState(seed).permutation(m), so every row is held out
    exactly once and the sets differ in size by at most one."""
    m, n_folds = int(m), int(n_folds)
    if not 2 <= n_folds <= m:
        raise ValueError("n_folds must be between 2 and m")
    perm = np.random.RandomState(int(seed)).permutation(m)
    masks = np.ones((n_folds, m), dtype=np.uint8)
    for f in range(n_folds):
        masks[f, perm[f::n_folds]] = 0
    return masks


def masked_panel_iterate(A, b, w, mu, Block, iters, diag=None, x0=None):
    """``iters`` block updates (cyclic over ``Block`` feature blocks) of the panel's iteration on the
    masked problem of one right-hand side, in fp64: with R = w o (A x - b), G = A_m^T R, the shrink
    x^ = S(x - G / d, mu / d), D = x^ - x, S = w o (A_m D), the exact line search along D and
    x += gamma D.  ``diag``: the d_j > 0 of the shrink, (n,); default the FULL column norms ||a_j||^2,
    as the device uses (not those of the masked rows).  Returns dict(x, r) with r the masked residual."""
    # Not a wrapper of _panel_iterate: it carries A x per block and forms r = sum Ax - w b, the reference's own order,
    # and tests/test_panel_cv_host.py::test_all_ones_mask_is_the_numpy_oracle_bitwise pins its bits to oracle.run_numpy.
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    Block = int(Block)
    wd = n // Block
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    w = (np.asarray(w).reshape(-1) != 0).astype(np.float64)
    mu = float(mu)
    dg = np.square(A).sum(axis=0) if diag is None else np.asarray(diag, dtype=np.float64).reshape(-1)
    dg = dg.reshape(Block, wd)
    x = (np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64).reshape(-1)).reshape(Block, wd).copy()
    Ax = np.stack([w * (A[:, q * wd:(q + 1) * wd] @ x[q]) for q in range(Block)])
    wb = w * b
    for t in range(int(iters)):
        mb = t % Block
        Am = A[:, mb * wd:(mb + 1) * wd]
        r = Ax.sum(axis=0) - wb
        g = Am.T @ r
        rx = dg[mb] * x[mb] - g
        Bx = (1.0 / dg[mb]) * (np.sign(rx) * np.maximum(np.abs(rx) - mu, 0))
        D = Bx - x[mb]
        s = w * (Am @ D)
        r1 = r @ s + mu * (np.abs(Bx).sum() - np.abs(x[mb]).sum())
        r2 = s @ s
        gamma = 0.0 if r2 == 0 else float(np.clip(-r1 / r2, 0, 1))
        x[mb] += gamma * D
        Ax[mb] += gamma * s
    return dict(x=x.reshape(-1), r=Ax.sum(axis=0) - wb)


def masked_duality_gap(A, b, w, x, mu, diag=None):
    """The certificate of ``duality_gap`` on the masked problem (0/1 row weights ``w``): ``_panel_gap`` with no
    factors, no intercept and no sign constraint.  ``diag``: default the FULL column norms (d_j >= ||w o a_j||^2, so
    the rule stays safe)."""
    return _panel_gap(A, b, _rows01(w, A), x, mu, None, diag, False, False, None)


# ---------------------------------------------------------------------------
# One fp64 restatement of every panel mode (the modes: sections 11, 13-16):
#   min over x (and beta0 with ``intercept``) of 1/2 sum_i w_i (a_i . x + beta0 - b_i)^2 + mu sum_j p_j |x_j|,
#   x >= 0 with ``positive``, with w_i in [0, 1] (0/1: a row mask) and p_j > 0.
# beta0 is profiled out: the residual is centred over its weighted mean and the iteration carries the centred one.
# ``_panel_iterate`` and ``_panel_gap`` state the device's solver and certificate once; the public names below fix a
# mode's flags and validate its arguments.
# ---------------------------------------------------------------------------
def centred_diag(A):
    """d_j = sum_i (a_ij - mean_j)^2 over all rows, (n,): the diag of the intercept's shrink and screen.
    d_j >= || P_w a_j ||^2 for every w in [0, 1], so one d serves every fold.  The deviations are taken from
    the column's first entry, so a constant column gives exactly 0."""
    A = np.asarray(A, dtype=np.float64)
    dev = A - A[:1]
    return np.square(dev - dev.sum(axis=0) / A.shape[0]).sum(axis=0)


def _diag_in_effect(A, diag, intercept):
    """``diag`` as given; otherwise ``centred_diag(A)`` with ``intercept``, else the FULL column norms ||a_j||^2 (not
    those of the weighted rows: d_j >= sum_i w_i a_ij^2 because w <= 1), as the device uses."""
    if diag is not None:
        return np.asarray(diag, dtype=np.float64).reshape(-1)
    return centred_diag(A) if intercept else np.square(A).sum(axis=0)


def _rows01(w, A):
    """A row mask as fp64 0/1; None: all rows."""
    return np.ones(np.shape(A)[0]) if w is None else (np.asarray(w).reshape(-1) != 0).astype(np.float64)


def _penalty(p, n):
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    if p.size != n or not np.all(np.isfinite(p) & (p > 0.0)):
        raise ValueError("penalty factors: n entries, each finite and > 0")
    return p


def _row_weights(w, m):
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if w.size != m or not np.all(np.isfinite(w) & (w >= 0.0) & (w <= 1.0)):
        raise ValueError("row weights: m entries, each finite and in [0, 1]")
    return w


def _wmean(w, v):
    """sum w v / sum w; 0 when sum w = 0."""
    nw = float(w.sum())
    return float(w @ v) / nw if nw > 0 else 0.0


def _panel_iterate(A, b, w, mu, p, Block, iters, diag, x0, intercept, positive):
    """``iters`` block updates (cyclic over ``Block`` feature blocks; ``intercept`` needs Block = 1, ValueError
    otherwise) of the panel's iteration on one right-hand side, in fp64.  ``w``: fp64 (m,) in [0, 1]; ``p``: None (all
    ones) or validated factors; ``diag``: see ``_diag_in_effect``.

    The carried residual is R = w o (A x - b), or w o (e - ebar_w) with ``intercept`` (ebar_w the weighted mean of
    e = A x - b).  Per update of block m: g = A_m^T R; the prox x^_j = S(d_j x_j - g_j, mu p_j) / d_j (max(0, .) with
    ``positive``; a column with d_j = 0 keeps x_j = 0); D = x^ - x_m; s = A_m D and s^ = w o s; c = sum s^ / sum w
    under ``intercept`` and 0 otherwise; the exact line search of the objective along D,
    gamma = clip(-(R . s + mu sum_j p_j (|x_j + D_j| - |x_j|)) / (s . s^ - c sum s^), 0, 1), 0 when the curvature is
    <= 0; x_m += gamma D and R += gamma (s^ - c w).  With ``positive`` ``x0`` is projected to max(x0, 0), and x >= 0 at
    every iteration (D >= -x and gamma <= 1, each rounding monotone).  Returns dict(x, r = R[, intercept =
    -sum w (A x - b) / sum w])."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[1]
    Block = int(Block)
    if intercept and Block != 1:
        raise ValueError("intercept needs Block = 1")
    wd = n // Block
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    nw = float(w.sum())
    mu = float(mu)
    pw = (np.ones(n) if p is None else p).reshape(Block, wd)
    dg = _diag_in_effect(A, diag, intercept)
    with np.errstate(divide="ignore"):
        rec = np.where(dg > 0, 1.0 / np.where(dg > 0, dg, 1.0), 0.0).reshape(Block, wd)
    dg = dg.reshape(Block, wd)
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64).reshape(-1)
    if positive:
        x = np.maximum(x, 0.0)
    x = x.reshape(Block, wd).copy()
    e = A @ x.reshape(-1) - b
    R = w * (e - _wmean(w, e) if intercept else e)
    for t in range(int(iters)):
        mb = t % Block
        Am = A[:, mb * wd:(mb + 1) * wd]
        g = Am.T @ R
        rx = dg[mb] * x[mb] - g
        Bx = rec[mb] * (np.sign(rx) * np.maximum(np.abs(rx) - mu * pw[mb], 0))
        if positive:
            Bx = np.maximum(Bx, 0.0)
        D = Bx - x[mb]
        s = Am @ D
        sh = w * s
        sm = float(sh.sum())
        c = (sm / nw if nw > 0 else 0.0) if intercept else 0.0
        # sum p (|x + D| - |x|) coordinate by coordinate, sign(x) D where the step keeps the sign: the two sums'
        # difference would lose the O(|D|^2) that is left of r1 near the optimum
        l1d = np.where(x[mb] * Bx > 0, np.sign(x[mb]) * D, np.abs(Bx) - np.abs(x[mb]))
        r1 = R @ s + mu * float(pw[mb] @ l1d)
        r2 = s @ sh - c * sm
        gamma = 0.0 if r2 <= 0 else float(np.clip(-r1 / r2, 0, 1))
        x[mb] = x[mb] + gamma * D
        R = R + gamma * (sh - c * w)
    out = dict(x=x.reshape(-1), r=R)
    if intercept:
        out["intercept"] = -_wmean(w, A @ out["x"] - b) if nw > 0 else 0.0
    return out


def _panel_gap(A, b, w, x, mu, p, diag, intercept, positive, hold):
    """The certificate at x (x >= 0 with ``positive``), arguments as ``_panel_iterate``: e = A x - b (minus its
    weighted mean c with ``intercept``, so that r sums to zero: the intercept's dual constraint), r = w o e,
    g = A^T r; primal = 1/2 sum w e^2 + mu sum p_j |x_j|.  The dual constraint is |a_j . theta| <= mu p_j
    (-a_j . theta <= mu p_j with ``positive``), so gnorm_inf = max_j |g_j| / p_j (max_j (-g_j)+ / p_j; NaN propagates;
    at x = 0 it is mu_max) and scale = min(1, mu / gnorm_inf) (1 when that is 0) makes scale r dual feasible:
    dual = -1/2 scale^2 sum w e^2 - scale sum w e b, gap = primal - dual >= P(x) - P*.  The dual point is theta_i =
    scale sqrt(w_i) e_i of the problem on (diag(sqrt w) A, sqrt(w) o b); it is never formed.  The gap-safe score is
    scale |g_j| + sqrt(d_j) sqrt(2 max(gap, 0)) (-g_j for |g_j| with ``positive``) and keep_j = not (score_j < mu p_j):
    a column that is not kept is 0 at every optimum, and a NaN keeps everything.  holdout_sse = sum_i h_i (a_i . x +
    intercept - b_i)^2 with ``hold`` = h >= 0 (default 1 where w = 0, else 0); intercept = -c with ``intercept``, else
    0.  Returns dict(primal, dual, gap, scale, gnorm_inf, holdout_sse, intercept, score, keep, g, r)."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    nw = float(w.sum())
    mu = float(mu)
    pw = np.ones(A.shape[1]) if p is None else p
    h = (w == 0.0).astype(np.float64) if hold is None else np.asarray(hold, dtype=np.float64).reshape(-1)
    e = A @ x - b
    c = _wmean(w, e) if intercept else 0.0
    ec = e - c
    r = w * ec
    g = A.T @ r
    wee = float(r @ ec)
    primal = 0.5 * wee + mu * float(pw @ np.abs(x))
    ga = np.where(g > 0, 0.0, -g) if positive else np.abs(g)
    gn = float(np.max(ga / pw))       # NaN propagates
    scale = min(1.0, mu / gn) if gn > 0.0 else 1.0
    dual = -0.5 * scale * scale * wee - scale * float(r @ b)
    gap = primal - dual
    dg = _diag_in_effect(A, diag, intercept)
    score = scale * (-g if positive else np.abs(g)) + np.sqrt(dg) * np.sqrt(2.0 * np.maximum(gap, 0.0))
    return dict(primal=primal, dual=dual, gap=gap, scale=scale, gnorm_inf=gn, holdout_sse=float(h @ (ec * ec)),
                intercept=-c if (intercept and nw > 0) else 0.0, score=score, keep=~(score < mu * pw), g=g, r=r)


# Intercept, 0/1 rows, one feature block.
def intercept_panel_iterate(A, b, w, mu, iters, diag=None, x0=None):
    """``_panel_iterate`` with the intercept on the masked problem; ``diag``: default ``centred_diag(A)``.  Returns
    dict(x, r, intercept)."""
    return _panel_iterate(A, b, _rows01(w, A), mu, None, 1, iters, diag, x0, True, False)


def intercept_duality_gap(A, b, w, x, mu, diag=None):
    """``_panel_gap`` with the intercept on the masked problem; ``diag``: default ``centred_diag(A)``."""
    return _panel_gap(A, b, _rows01(w, A), x, mu, None, diag, True, False, None)


# Non-negative lasso: x >= 0, 0/1 rows (``w`` None: all rows), with or without the intercept.
def positive_panel_iterate(A, b, w, mu, Block, iters, diag=None, x0=None, intercept=False):
    """``_panel_iterate`` with the sign constraint: the one-sided prox, ``x0`` projected to max(x0, 0), x >= 0 at
    every iteration."""
    return _panel_iterate(A, b, _rows01(w, A), mu, None, Block, iters, diag, x0, intercept, True)


def positive_duality_gap(A, b, w, x, mu, diag=None, intercept=False):
    """``_panel_gap`` with the sign constraint at a feasible x: the one-sided gnorm_inf and score."""
    return _panel_gap(A, b, _rows01(w, A), x, mu, None, diag, intercept, True, None)


# Penalty factors: per-column l1 weights ``p``, (n,), every entry finite and > 0 (ValueError
# otherwise), used as given (no renormalisation to sum p = n); 0/1 rows (``w`` None: all rows).
def penalty_panel_iterate(A, b, w, mu, p, Block, iters, diag=None, x0=None, intercept=False, positive=False):
    """``_panel_iterate`` with the factors ``p``."""
    return _panel_iterate(A, b, _rows01(w, A), mu, _penalty(p, np.shape(A)[1]), Block, iters, diag, x0, intercept,
                          positive)


def penalty_duality_gap(A, b, w, x, mu, p, diag=None, intercept=False, positive=False):
    """``_panel_gap`` with the factors ``p``."""
    return _panel_gap(A, b, _rows01(w, A), x, mu, _penalty(p, np.shape(A)[1]), diag, intercept, positive, None)


# Observation weights: ``w`` (m,), every entry finite and in [0, 1] (ValueError otherwise);
# ``p`` None: all ones.  One feature block, as the device has it.
def weighted_panel_iterate(A, b, w, mu, iters, diag=None, x0=None, intercept=False, positive=False, p=None):
    """``_panel_iterate`` with general row weights."""
    m, n = np.shape(A)
    return _panel_iterate(A, b, _row_weights(w, m), mu, None if p is None else _penalty(p, n), 1, iters, diag, x0,
                          intercept, positive)


def weighted_duality_gap(A, b, w, x, mu, diag=None, intercept=False, positive=False, p=None, hold=None):
    """``_panel_gap`` with general row weights; ``hold``: the held-out score's weights h >= 0 (default 1 where
    w = 0, else 0)."""
    m, n = np.shape(A)
    return _panel_gap(A, b, _row_weights(w, m), x, mu, None if p is None else _penalty(p, n), diag, intercept, positive,
                      hold)


# ---------------------------------------------------------------------------
# Compaction of a screened panel.
# ---------------------------------------------------------------------------
def compaction_columns(keep_union, q):
    """Sorted original indices (int64) of the columns a compacted panel keeps: the kept columns of
    ``keep_union`` (n,) bool -- the union over the panel's right-hand sides of the screen's keep -- padded
    up to the next multiple of ``q`` (at least ``q``) with the screened columns of smallest index.  A
    screened column is provably zero at every optimum of the panel, so keeping some is harmless; this
    rule needs no scores and is deterministic.  ValueError if q <= 0 or n is not a multiple of q."""
    keep = np.asarray(keep_union).reshape(-1) != 0
    n, q = keep.size, int(q)
    if q <= 0 or n % q:
        raise ValueError(f"q (got {q}) must be positive and divide n = {n}")
    kept = np.flatnonzero(keep)
    n_new = max(q, -(-kept.size // q) * q)
    pads = np.flatnonzero(~keep)[:n_new - kept.size]
    return np.sort(np.concatenate([kept, pads])).astype(np.int64)


# ---------------------------------------------------------------------------
# Logistic lasso by IRLS on the weighted panel: the host restatement of bpgl_panel_glm_model,
# bpgl_panel_glm_dual and the outer loop of ``panel.logistic_path``.
#   min over x, beta0 of sum_i om_i l(eta_i; y_i) + mu sum_j p_j |x_j|,  eta = A x + beta0,  l = log(1 + e^eta) - y eta
# with labels y in [0, 1], prior weights om in [0, 1]; x >= 0 with ``positive``; beta0 = 0 without the intercept.
# ---------------------------------------------------------------------------
GLM_FLOOR = 1e-5          # glmnet's floor of p (1 - p)
GLM_PHI_TOL = 1e-14       # the intercept's Newton iteration stops at |phi| <= this x sum om
GLM_NEWTON_MAX = 40


def _wave_fold(v):
    """(..., 64) -> (...): the device's wave_sum, lanes l and l ^ o added for o = 32, 16, ..., 1."""
    for o in (32, 16, 8, 4, 2, 1):
        v = v[..., :o] + v[..., o:2 * o]
    return v[..., 0]


def _block_sum(v):
    """The device's one-block sum of a vector: 256 threads, thread t adding entries t, t + 256, ... in index order,
    the lanes of each wave by ``_wave_fold``, the 4 waves in order."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    rows = -(-v.size // 256)
    v = np.concatenate([v, np.zeros(rows * 256 - v.size)]).reshape(rows, 256)
    t = np.zeros(256)
    for r in v:
        t = t + r
    w = _wave_fold(t.reshape(4, 64))
    return float(((w[0] + w[1]) + w[2]) + w[3])


def _blocks_sum(v):
    """The device's sum of one value per (rhs, row) thread: per 256-row block the lanes and the 4 waves in order, then
    the blocks in block order."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 4, 64)
    w = _wave_fold(v)
    tot = 0.0
    for b in ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]:
        tot += float(b)
    return tot


def _sigma(eta):
    t = np.exp(-np.abs(eta))
    return np.where(eta >= 0, 1.0 / (1.0 + t), t / (1.0 + t))


def _logloss(eta, y):
    return np.maximum(eta, 0.0) + np.log1p(np.exp(-np.abs(eta))) - y * eta


def _labels(y, m):
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    if y.size != m or not np.all(np.isfinite(y) & (y >= 0.0) & (y <= 1.0)):
        raise ValueError("labels: m entries, each in [0, 1]")
    return y


def _neg_entropy(t):
    """Nh(t) = t log t + (1 - t) log(1 - t) with 0 log 0 = 0 (a t rounded outside [0, 1] counts as the end point)."""
    u = 1.0 - t
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(t > 0, t * np.log(np.where(t > 0, t, 1.0)), 0.0) + \
            np.where(u > 0, u * np.log(np.where(u > 0, u, 1.0)), 0.0)


def logistic_null_deviance(y, omega, intercept=True):
    """sum om l at x = 0 and its own beta0: -sum om Nh(ybar) with the intercept (ybar the weighted mean label),
    sum om log 2 without.  The scale of the logistic stopping rule, as 1/2 ||b||^2 is of the lasso's."""
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    om = np.asarray(omega, dtype=np.float64).reshape(-1)
    sw = float(om.sum())
    if not intercept:
        return sw * float(np.log(2.0))
    return -sw * float(_neg_entropy(np.float64(float(om @ y) / sw)))


def logistic_intercept(ax, y, omega, beta0=0.0):
    """The root of phi(beta) = sum om (sigma(ax + beta) - y) by the device's safeguarded Newton iteration: the
    bracket [logit(ybar) - max ax, logit(ybar) - min ax] over the rows with a weight, the start ``beta0`` (the
    midpoint when outside), a step that leaves the bracket replaced by the midpoint, at most GLM_NEWTON_MAX steps, stop
    at |phi| <= GLM_PHI_TOL sum om; fixed-order sums.  Returns (beta, |phi|, steps, flag); flag 1 (and ``beta0`` back)
    when sum om y is 0 or sum om: no finite root."""
    sw, sy = _block_sum(omega), _block_sum(omega * y)

    def ev(beta):
        p = _sigma(ax + beta)
        return _block_sum(omega * (p - y)), _block_sum(omega * (p * (1.0 - p)))
    beta = float(beta0)
    if not (sy > 0.0 and sy < sw):
        return beta, abs(ev(beta)[0]), 0, 1
    lg = float(np.log(sy / (sw - sy)))
    live = omega > 0
    lo, hi = lg - float(ax[live].max()), lg + float((-ax[live]).max())
    if not (lo <= beta <= hi):
        beta = 0.5 * (lo + hi)
    steps = 0
    while True:
        f, d = ev(beta)
        if abs(f) <= GLM_PHI_TOL * sw or steps == GLM_NEWTON_MAX:
            break
        if f > 0.0:
            hi = beta
        else:
            lo = beta
        nb = beta - f / d if d > 0.0 else lo
        if not (lo < nb < hi):
            nb = 0.5 * (lo + hi)
        beta = nb
        steps += 1
    return beta, abs(f), steps, 0


def logistic_model(A, y, omega, x, beta0=0.0, intercept=True, curv=0, hold=None, p=None, solve=True):
    """One outer step at x, the restatement of bpgl_panel_glm_model for one right-hand side: ax = A x; beta0 the root of
    phi with ``intercept`` (``solve=False``: ``beta0`` as given; without ``intercept`` 0); eta = ax + beta0,
    p = sigma(eta), v = max(p (1 - p), GLM_FLOOR) (1/4 with ``curv``: Boehning's bound), w = 4 om v, z = eta + (y - p) / v;
    loss = sum om l, hold_loss = sum h l, hold_miss = sum h [(p > 1/2) != (y > 1/2)] (``hold`` = h, None: zeros),
    sum_omega, l1 = sum pen_j |x_j| (``p`` = pen, None: ones), phi = |phi(beta0)|, steps, flag.  The block sums follow the
    device's order."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    y = _labels(y, m)
    om = _row_weights(omega, m)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    pw = np.ones(n) if p is None else _penalty(p, n)
    h = np.zeros(m) if hold is None else np.asarray(hold, dtype=np.float64).reshape(-1)
    ax = A @ x
    if intercept and solve:
        b0, phi, steps, flag = logistic_intercept(ax, y, om, beta0)
    else:
        b0 = float(beta0) if intercept else 0.0
        phi, steps, flag = abs(_block_sum(om * (_sigma(ax + b0) - y))), 0, 0
    eta = ax + b0
    pr = _sigma(eta)
    v = np.full(m, 0.25) if curv else np.maximum(pr * (1.0 - pr), GLM_FLOOR)
    ls = _logloss(eta, y)
    miss = ((pr > 0.5) != (y > 0.5)).astype(np.float64)
    tot = _blocks_sum if m % 256 == 0 else _block_sum
    return dict(ax=ax, beta0=b0, eta=eta, p=pr, v=v, w=(4.0 * om) * v, z=eta + (y - pr) / v,
                loss=tot(om * ls), hold_loss=tot(h * ls), hold_miss=tot(h * miss), sum_omega=tot(om),
                l1=_block_sum(pw * np.abs(x)), phi=phi, steps=steps, flag=flag)


def logistic_dual(y, omega, p, scale):
    """D = -sum om Nh(s p + (1 - s) y): the dual value at theta = s om o (p - y) (bpgl_panel_glm_dual)."""
    s = float(scale)
    return -_block_sum(omega * _neg_entropy(s * p + (1.0 - s) * y))


def logistic_gap(A, y, omega, x, mu, beta0=0.0, intercept=True, positive=False, p=None, model=None):
    """The logistic certificate at x: with the model's p (``model``: a ``logistic_model`` of the same arguments, else
    computed here, beta0 re-solved), g = A^T (om o (p - y)) the loss's gradient, gnorm_inf = max_j |g_j| / pen_j
    (max_j (-g_j)+ / pen_j with ``positive``; at x = 0 it is mu_max), scale = min(1, mu / gnorm_inf) (1 when that is 0):
    theta = scale om o (p - y) satisfies |a_j . theta| <= mu pen_j and, beta0 being the root of phi, sum theta = 0.
    primal = sum om l + mu sum pen |x|, dual = ``logistic_dual``, gap = primal - dual >= P(x, beta0) - P*.
    Returns dict(primal, dual, gap, scale, gnorm_inf, g, beta0)."""
    A = np.asarray(A, dtype=np.float64)
    mod = logistic_model(A, y, omega, x, beta0, intercept, 0, None, p) if model is None else model
    om = _row_weights(omega, A.shape[0])
    yv = _labels(y, A.shape[0])
    pw = np.ones(A.shape[1]) if p is None else _penalty(p, A.shape[1])
    mu = float(mu)
    g = A.T @ (om * (mod["p"] - yv))
    ga = np.where(g > 0, 0.0, -g) if positive else np.abs(g)
    gn = float(np.max(ga / pw))
    scale = min(1.0, mu / gn) if gn > 0.0 else 1.0
    primal = mod["loss"] + mu * mod["l1"]
    dual = logistic_dual(yv, om, mod["p"], scale)
    return dict(primal=primal, dual=dual, gap=primal - dual, scale=scale, gnorm_inf=gn, g=g, beta0=mod["beta0"])


def logistic_panel_solve(A, y, omega, mu, outer_max=100, inner_iters=16, tol=1e-8, intercept=True, positive=False,
                         p=None, curv=0, x0=None, diag=None, round_x=False):
    """The IRLS outer loop on one right-hand side, ``_panel_iterate`` as the inner solve.  Per outer step, at the
    current x: ``logistic_model`` (beta0 re-solved from the last one); P = loss + mu l1; a P above the previous one
    switches to ``curv`` = 1 from then on (the model is formed again with it); the certificate ``logistic_gap``; stop
    when gap <= ``tol`` x the null deviance or after ``outer_max`` steps; else ``inner_iters`` iterations on
    1/2 sum w (a . x + beta0 - z)^2 + 4 mu sum pen |x| from x (x >= 0 with ``positive``), whose weighted-mean intercept is
    the next Newton start.  ``round_x``: x is rounded to fp32 after every inner solve, as the device stores it.
    Returns dict(x, intercept, primal, dual, gap, scale, null_deviance, reached, outer_iters, curvature, history (P at
    every outer step))."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    yv, om = _labels(y, m), _row_weights(omega, m)
    pen = None if p is None else _penalty(p, n)
    mu = float(mu)
    null = logistic_null_deviance(yv, om, intercept)
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64).reshape(-1)
    if positive:
        x = np.maximum(x, 0.0)
    if round_x:
        x = x.astype(np.float32).astype(np.float64)
    b0, curv, hist, outer = 0.0, int(bool(curv)), [], 0
    while True:
        mod = logistic_model(A, yv, om, x, b0, intercept, curv, None, pen)
        P = mod["loss"] + mu * mod["l1"]
        if hist and not curv and P > hist[-1]:
            curv = 1
            mod = logistic_model(A, yv, om, x, b0, intercept, curv, None, pen)
        b0 = mod["beta0"]
        cert = logistic_gap(A, yv, om, x, mu, b0, intercept, positive, pen, model=mod)
        hist.append(P)
        if cert["gap"] <= tol * null or outer >= int(outer_max):
            break
        inner = _panel_iterate(A, mod["z"], mod["w"], 4.0 * mu, pen, 1, inner_iters, diag, x, intercept, positive)
        x = inner["x"]
        if round_x:
            x = x.astype(np.float32).astype(np.float64)
        if intercept:
            b0 = inner["intercept"]
        outer += 1
    return dict(x=x, intercept=b0, primal=cert["primal"], dual=cert["dual"], gap=cert["gap"], scale=cert["scale"],
                null_deviance=null, reached=bool(cert["gap"] <= tol * null), outer_iters=outer, curvature=curv,
                history=np.array(hist))

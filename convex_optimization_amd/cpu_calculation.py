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
``centred_diag``, ``intercept_panel_iterate`` and ``intercept_duality_gap``, the restatement of the
panel's intercept; ``positive_panel_iterate`` and ``positive_duality_gap``, the
restatement of the panel's non-negative lasso (x >= 0); ``penalty_panel_iterate`` and
``penalty_duality_gap``, the restatement of the panel's penalty factors (per-column l1 weights, DESIGN.md
section 15).
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
    """The certificate of ``duality_gap`` on the masked problem: r = w o (A x - b), g = A^T r, and
    primal, dual, gap, scale, gnorm_inf from them (b enters through r . b, where the held-out rows
    of r are 0).  Also holdout_sse = sum (1 - w)(A x - b)^2, and the gap-safe score and keep with
    ``diag`` (default the FULL column norms: d_j >= ||w o a_j||^2, so the rule stays safe)."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    w = (np.asarray(w).reshape(-1) != 0).astype(np.float64)
    mu = float(mu)
    e = A @ x - b
    r = w * e
    g = A.T @ r
    rr = float(r @ r)
    primal = 0.5 * rr + mu * float(np.abs(x).sum())
    gn = float(np.max(np.abs(g)))
    scale = min(1.0, mu / gn) if gn > 0.0 else 1.0
    dual = -0.5 * scale * scale * rr - scale * float(r @ b)
    gap = primal - dual
    h = (1.0 - w) * e
    dg = np.square(A).sum(axis=0) if diag is None else np.asarray(diag, dtype=np.float64).reshape(-1)
    score = scale * np.abs(g) + np.sqrt(dg) * np.sqrt(2.0 * np.maximum(gap, 0.0))
    return dict(primal=primal, dual=dual, gap=gap, scale=scale, gnorm_inf=gn, holdout_sse=float(h @ h),
                score=score, keep=~(score < mu), g=g, r=r)


# ---------------------------------------------------------------------------
# Intercept: min over x, beta0 of 1/2 || w o (A x + beta0 - b) ||^2 + mu ||x||_1.
# beta0 is profiled out: the objective is 1/2 || P_w (A x - b) ||^2 + mu ||x||_1 with
# P_w v = w o (v - (w . v) / n_w), and the iteration carries the centred residual.  The host restatement
# of bpgl_panel_set_intercept's solver and certificate.
# ---------------------------------------------------------------------------
def _centre(w, v):
    """P_w v = w o (v - mean of v over the rows with w = 1); 0 when w has no such row."""
    nw = float(w.sum())
    return w * (v - (float(w @ v) / nw if nw > 0 else 0.0))


def centred_diag(A):
    """d_j = sum_i (a_ij - mean_j)^2 over all rows, (n,): the diag of the intercept's shrink and screen.
    d_j >= || P_w a_j ||^2 for every 0/1 w, so one d serves every fold.  The deviations are taken from
    the column's first entry, so a constant column gives exactly 0."""
    A = np.asarray(A, dtype=np.float64)
    dev = A - A[:1]
    return np.square(dev - dev.sum(axis=0) / A.shape[0]).sum(axis=0)


def intercept_panel_iterate(A, b, w, mu, iters, diag=None, x0=None):
    """``iters`` updates (one feature block) of the panel's iteration with the intercept on one
    right-hand side, in fp64: R = P_w (A x - b), G = A^T R, the shrink with ``diag`` (default
    ``centred_diag(A)``; a column with d_j = 0 keeps x_j = 0), S = w o (A D), c = sum S / n_w, the exact
    line search gamma = clip(-(R.S + mu (|x + D|_1 - |x|_1)) / (S.S - c sum S), 0, 1) (0 when the
    curvature is <= 0), x += gamma D and R += gamma w o (S - c).  Returns dict(x, r, intercept) with
    intercept = -mean over the in-rows of (A x - b)."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[1]
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    w = (np.asarray(w).reshape(-1) != 0).astype(np.float64)
    nw = float(w.sum())
    mu = float(mu)
    dg = centred_diag(A) if diag is None else np.asarray(diag, dtype=np.float64).reshape(-1)
    with np.errstate(divide="ignore"):
        rec = np.where(dg > 0, 1.0 / dg, 0.0)
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64).reshape(-1)
    R = _centre(w, A @ x - b)
    for _ in range(int(iters)):
        g = A.T @ R
        rx = dg * x - g
        Bx = rec * (np.sign(rx) * np.maximum(np.abs(rx) - mu, 0))
        D = Bx - x
        s = w * (A @ D)
        sm = float(s.sum())
        c = sm / nw if nw > 0 else 0.0
        r1 = R @ s + mu * (np.abs(Bx).sum() - np.abs(x).sum())
        r2 = s @ s - c * sm
        gamma = 0.0 if r2 <= 0 else float(np.clip(-r1 / r2, 0, 1))
        x += gamma * D
        R += gamma * w * (s - c)
    e = A @ x - b
    return dict(x=x, r=R, intercept=-(float(w @ e) / nw) if nw > 0 else 0.0)


def intercept_duality_gap(A, b, w, x, mu, diag=None):
    """``masked_duality_gap`` on the profiled problem: with e = A x - b and c = the in-row mean of e,
    r = w o (e - c) (it sums to zero over the in-rows: the intercept's dual constraint), g = A^T r,
    primal, dual, gap, scale, gnorm_inf from them; intercept = -c; holdout_sse = the held-out sum of
    (a_i . x + intercept - b_i)^2; score and keep with ``diag`` (default ``centred_diag(A)``)."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    w = (np.asarray(w).reshape(-1) != 0).astype(np.float64)
    nw = float(w.sum())
    mu = float(mu)
    e = A @ x - b
    c = float(w @ e) / nw if nw > 0 else 0.0
    r = w * (e - c)
    g = A.T @ r
    rr = float(r @ r)
    primal = 0.5 * rr + mu * float(np.abs(x).sum())
    gn = float(np.max(np.abs(g)))
    scale = min(1.0, mu / gn) if gn > 0.0 else 1.0
    dual = -0.5 * scale * scale * rr - scale * float(r @ b)
    gap = primal - dual
    h = (1.0 - w) * (e - c)
    dg = centred_diag(A) if diag is None else np.asarray(diag, dtype=np.float64).reshape(-1)
    score = scale * np.abs(g) + np.sqrt(dg) * np.sqrt(2.0 * np.maximum(gap, 0.0))
    return dict(primal=primal, dual=dual, gap=gap, scale=scale, gnorm_inf=gn, holdout_sse=float(h @ h),
                intercept=-c if nw > 0 else 0.0, score=score, keep=~(score < mu), g=g, r=r)


# ---------------------------------------------------------------------------
# Non-negative lasso: min 1/2 || w o (A x - b) ||^2 + mu sum_j x_j subject to x >= 0,
# with or without the intercept's profiling.  The host restatement of bpgl_panel_set_positive's solver and
# certificate.
# ---------------------------------------------------------------------------
def positive_panel_iterate(A, b, w, mu, Block, iters, diag=None, x0=None, intercept=False):
    """``iters`` block updates (cyclic over ``Block`` feature blocks; ``intercept`` needs Block = 1) of the
    panel's iteration on the non-negative problem of one right-hand side, in fp64: R = w o (A x - b)
    (P_w (A x - b) with ``intercept``), G = A_m^T R, the one-sided prox x^ = max(0, S(d x - G, mu) / d)
    (x^ = 0 where d = 0), D = x^ - x, S = w o (A_m D), the exact line search along D (curvature |P_w S|^2
    with ``intercept``) and x += gamma D.  ``w`` None: all rows.  ``diag``: default the full column norms
    (``centred_diag(A)`` with ``intercept``).  ``x0`` is projected to max(x0, 0).  Returns dict(x, r[,
    intercept]); x >= 0 at every iteration."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    Block = int(Block)
    if intercept and Block != 1:
        raise ValueError("intercept needs Block = 1")
    wd = n // Block
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    w = np.ones(m) if w is None else (np.asarray(w).reshape(-1) != 0).astype(np.float64)
    nw = float(w.sum())
    mu = float(mu)
    if diag is None:
        dg = centred_diag(A) if intercept else np.square(A).sum(axis=0)
    else:
        dg = np.asarray(diag, dtype=np.float64).reshape(-1)
    with np.errstate(divide="ignore"):
        rec = np.where(dg > 0, 1.0 / np.where(dg > 0, dg, 1.0), 0.0).reshape(Block, wd)
    dg = dg.reshape(Block, wd)
    x = np.maximum(np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64).reshape(-1), 0.0).reshape(Block, wd)
    proj = (lambda v: _centre(w, v)) if intercept else (lambda v: w * v)
    R = proj(A @ x.reshape(-1) - b)
    for t in range(int(iters)):
        mb = t % Block
        Am = A[:, mb * wd:(mb + 1) * wd]
        g = Am.T @ R
        rx = dg[mb] * x[mb] - g
        Bx = np.maximum(rec[mb] * (np.sign(rx) * np.maximum(np.abs(rx) - mu, 0)), 0.0)
        D = Bx - x[mb]
        s = w * (Am @ D)
        ps = proj(Am @ D)
        r1 = R @ s + mu * D.sum()          # |x + D|_1 - |x|_1 on the feasible set, without the cancellation
        r2 = ps @ ps
        gamma = 0.0 if r2 <= 0 else float(np.clip(-r1 / r2, 0, 1))
        x[mb] = x[mb] + gamma * D          # >= 0: D >= -x and gamma <= 1, each rounding monotone
        R = R + gamma * ps
    out = dict(x=x.reshape(-1), r=R)
    if intercept:
        e = A @ out["x"] - b
        out["intercept"] = -(float(w @ e) / nw) if nw > 0 else 0.0
    return out


def positive_duality_gap(A, b, w, x, mu, diag=None, intercept=False):
    """The certificate of the non-negative problem at a feasible x: r = w o (A x - b) (P_w (A x - b) with
    ``intercept``), g = A^T r.  The dual constraint is one-sided, -a_j . theta <= mu, so gnorm_inf is
    max_j (-g_j)+, scale = min(1, mu / that) (1 when it is 0) makes scale r dual feasible, and primal =
    1/2 |r|^2 + mu sum |x|, dual = -1/2 scale^2 |r|^2 - scale r.b, gap = primal - dual >= P(x) - P* as in
    ``masked_duality_gap``.  The gap-safe score is scale (-g_j) + sqrt(d_j) sqrt(2 max(gap, 0)), keep =
    not (score < mu): a column that is not kept is 0 at every optimum.  ``w`` None: all rows; ``diag``: default
    the full column norms (``centred_diag(A)`` with ``intercept``).  Also holdout_sse and intercept as in
    ``masked_duality_gap`` / ``intercept_duality_gap``."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    w = np.ones(A.shape[0]) if w is None else (np.asarray(w).reshape(-1) != 0).astype(np.float64)
    nw = float(w.sum())
    mu = float(mu)
    e = A @ x - b
    c = (float(w @ e) / nw if nw > 0 else 0.0) if intercept else 0.0
    r = w * (e - c)
    g = A.T @ r
    rr = float(r @ r)
    primal = 0.5 * rr + mu * float(np.abs(x).sum())
    gn = float(np.max(np.where(g > 0, 0.0, -g)))       # NaN propagates
    scale = min(1.0, mu / gn) if gn > 0.0 else 1.0
    dual = -0.5 * scale * scale * rr - scale * float(r @ b)
    gap = primal - dual
    h = (1.0 - w) * (e - c)
    if diag is None:
        dg = centred_diag(A) if intercept else np.square(A).sum(axis=0)
    else:
        dg = np.asarray(diag, dtype=np.float64).reshape(-1)
    score = scale * (-g) + np.sqrt(dg) * np.sqrt(2.0 * np.maximum(gap, 0.0))
    return dict(primal=primal, dual=dual, gap=gap, scale=scale, gnorm_inf=gn, holdout_sse=float(h @ h),
                intercept=-c if (intercept and nw > 0) else 0.0, score=score, keep=~(score < mu), g=g, r=r)


# ---------------------------------------------------------------------------
# Penalty factors: min 1/2 || w o (A x - b) ||^2 + mu sum_j p_j |x_j| with p_j > 0, with or
# without the intercept's profiling and the sign constraint.  The host restatement of bpgl_panel_set_penalty's
# solver and certificate.  The factors are used as given (no renormalisation to sum p = n).
# ---------------------------------------------------------------------------
def _penalty(p, n):
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    if p.size != n or not np.all(np.isfinite(p) & (p > 0.0)):
        raise ValueError("penalty factors: n entries, each finite and > 0")
    return p


def penalty_panel_iterate(A, b, w, mu, p, Block, iters, diag=None, x0=None, intercept=False, positive=False):
    """``iters`` block updates (cyclic over ``Block`` feature blocks; ``intercept`` needs Block = 1) of the
    panel's iteration on the weighted problem of one right-hand side, in fp64: R = w o (A x - b) (P_w (A x - b)
    with ``intercept``), G = A_m^T R, the prox x^_j = S(d_j x_j - G_j, mu p_j) / d_j (max(0, .) with ``positive``;
    0 where d_j = 0), D = x^ - x, S = w o (A_m D), the exact line search of the weighted objective along D,
    gamma = clip(-(R.S + mu (sum p |x + D| - sum p |x|)) / |P S|^2, 0, 1), and x += gamma D.  ``p``: (n,), every
    entry finite and > 0 (ValueError otherwise).  ``w`` None: all rows.  ``diag``: default the full column norms
    (``centred_diag(A)`` with ``intercept``).  With ``positive`` ``x0`` is projected to max(x0, 0).  Returns
    dict(x, r[, intercept])."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    Block = int(Block)
    if intercept and Block != 1:
        raise ValueError("intercept needs Block = 1")
    wd = n // Block
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    w = np.ones(m) if w is None else (np.asarray(w).reshape(-1) != 0).astype(np.float64)
    nw = float(w.sum())
    mu = float(mu)
    pw = _penalty(p, n).reshape(Block, wd)
    if diag is None:
        dg = centred_diag(A) if intercept else np.square(A).sum(axis=0)
    else:
        dg = np.asarray(diag, dtype=np.float64).reshape(-1)
    with np.errstate(divide="ignore"):
        rec = np.where(dg > 0, 1.0 / np.where(dg > 0, dg, 1.0), 0.0).reshape(Block, wd)
    dg = dg.reshape(Block, wd)
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64).reshape(-1)
    if positive:
        x = np.maximum(x, 0.0)
    x = x.reshape(Block, wd).copy()
    proj = (lambda v: _centre(w, v)) if intercept else (lambda v: w * v)
    R = proj(A @ x.reshape(-1) - b)
    for t in range(int(iters)):
        mb = t % Block
        Am = A[:, mb * wd:(mb + 1) * wd]
        g = Am.T @ R
        rx = dg[mb] * x[mb] - g
        Bx = rec[mb] * (np.sign(rx) * np.maximum(np.abs(rx) - mu * pw[mb], 0))
        if positive:
            Bx = np.maximum(Bx, 0.0)
        D = Bx - x[mb]
        s = w * (Am @ D)
        ps = proj(Am @ D)
        # sum p (|x + D| - |x|) coordinate by coordinate, sign(x) D where the step keeps the sign: the two sums'
        # difference would lose the O(|D|^2) that is left of r1 near the optimum
        l1d = np.where(x[mb] * Bx > 0, np.sign(x[mb]) * D, np.abs(Bx) - np.abs(x[mb]))
        r1 = R @ s + mu * float(pw[mb] @ l1d)
        r2 = ps @ ps
        gamma = 0.0 if r2 <= 0 else float(np.clip(-r1 / r2, 0, 1))
        x[mb] = x[mb] + gamma * D
        R = R + gamma * ps
    out = dict(x=x.reshape(-1), r=R)
    if intercept:
        e = A @ out["x"] - b
        out["intercept"] = -(float(w @ e) / nw) if nw > 0 else 0.0
    return out


def penalty_duality_gap(A, b, w, x, mu, p, diag=None, intercept=False, positive=False):
    """The certificate of the weighted problem at x (x >= 0 with ``positive``): r = w o (A x - b) (P_w (A x - b)
    with ``intercept``), g = A^T r.  The dual constraint is |a_j . theta| <= mu p_j (-a_j . theta <= mu p_j with
    ``positive``), so gnorm_inf is max_j |g_j| / p_j (max_j (-g_j)+ / p_j), scale = min(1, mu / that) (1 when it
    is 0) makes scale r dual feasible, and primal = 1/2 |r|^2 + mu sum p_j |x_j|, dual = -1/2 scale^2 |r|^2 -
    scale r.b, gap = primal - dual.  At x = 0 gnorm_inf is mu_max = max_j |a_j . b| / p_j.  The gap-safe score is
    scale |g_j| + sqrt(d_j) sqrt(2 max(gap, 0)) (-g_j for |g_j| with ``positive``), keep_j = not (score_j <
    mu p_j).  ``w`` None: all rows; ``diag``: default the full column norms (``centred_diag(A)`` with
    ``intercept``).  Also holdout_sse and intercept as in ``masked_duality_gap`` / ``intercept_duality_gap``."""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    w = np.ones(A.shape[0]) if w is None else (np.asarray(w).reshape(-1) != 0).astype(np.float64)
    nw = float(w.sum())
    mu = float(mu)
    p = _penalty(p, A.shape[1])
    e = A @ x - b
    c = (float(w @ e) / nw if nw > 0 else 0.0) if intercept else 0.0
    r = w * (e - c)
    g = A.T @ r
    rr = float(r @ r)
    primal = 0.5 * rr + mu * float(p @ np.abs(x))
    ga = np.where(g > 0, 0.0, -g) if positive else np.abs(g)
    gn = float(np.max(ga / p))       # NaN propagates
    scale = min(1.0, mu / gn) if gn > 0.0 else 1.0
    dual = -0.5 * scale * scale * rr - scale * float(r @ b)
    gap = primal - dual
    h = (1.0 - w) * (e - c)
    if diag is None:
        dg = centred_diag(A) if intercept else np.square(A).sum(axis=0)
    else:
        dg = np.asarray(diag, dtype=np.float64).reshape(-1)
    score = scale * (-g if positive else np.abs(g)) + np.sqrt(dg) * np.sqrt(2.0 * np.maximum(gap, 0.0))
    return dict(primal=primal, dual=dual, gap=gap, scale=scale, gnorm_inf=gn, holdout_sse=float(h @ h),
                intercept=-c if (intercept and nw > 0) else 0.0, score=score, keep=~(score < mu * p), g=g, r=r)


# ---------------------------------------------------------------------------
# Observation weights: min 1/2 sum_i w_i (a_i . x - b_i)^2 + mu sum_j p_j |x_j| with
# w_i in [0, 1], with or without the intercept's profiling (then over the weighted mean), the sign constraint and the
# penalty factors.  The host restatement of bpgl_panel_set_row_weights' solver and certificate; one feature block.
# ---------------------------------------------------------------------------
def _row_weights(w, m):
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if w.size != m or not np.all(np.isfinite(w) & (w >= 0.0) & (w <= 1.0)):
        raise ValueError("row weights: m entries, each finite and in [0, 1]")
    return w


def _wcentre(w, v):
    """v - (sum w v / sum w) at every row (unweighted); v itself when sum w = 0."""
    nw = float(w.sum())
    return v - (float(w @ v) / nw if nw > 0 else 0.0)


def weighted_panel_iterate(A, b, w, mu, iters, diag=None, x0=None, intercept=False, positive=False, p=None):
    """``iters`` updates (one feature block) of the panel's iteration on the weighted problem of one right-hand
    side, in fp64.  The carried residual is R^ = w o (A x - b) (w o (e - ebar_w) with ``intercept``, ebar_w the
    weighted mean); G = A^T R^; the prox of ``penalty_panel_iterate`` with ``diag`` (default the FULL column norms,
    ``centred_diag(A)`` with ``intercept``: d_j >= sum_i w_i a_ij^2 because w <= 1); s = A D and s^ = w o s; the exact
    line search of the weighted objective along D, gamma = clip(-(R^ . s + mu (sum p |x + D| - sum p |x|)) /
    (s . s^ - c sum s^), 0, 1) with c = sum s^ / sum w under ``intercept`` and 0 otherwise (gamma = 0 when the
    curvature is <= 0); x += gamma D and R^ += gamma (s^ - c w).  ``w``: (m,), every entry finite and in [0, 1]
    (ValueError otherwise).  ``p`` None: all ones.  With ``positive`` ``x0`` is projected to max(x0, 0).  Returns
    dict(x, r[, intercept]) with r = R^ and intercept = -sum w (A x - b) / sum w."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    w = _row_weights(w, m)
    nw = float(w.sum())
    mu = float(mu)
    pw = np.ones(n) if p is None else _penalty(p, n)
    if diag is None:
        dg = centred_diag(A) if intercept else np.square(A).sum(axis=0)
    else:
        dg = np.asarray(diag, dtype=np.float64).reshape(-1)
    with np.errstate(divide="ignore"):
        rec = np.where(dg > 0, 1.0 / np.where(dg > 0, dg, 1.0), 0.0)
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64).reshape(-1)
    if positive:
        x = np.maximum(x, 0.0)
    e = A @ x - b
    R = w * (_wcentre(w, e) if intercept else e)
    for _ in range(int(iters)):
        g = A.T @ R
        rx = dg * x - g
        Bx = rec * (np.sign(rx) * np.maximum(np.abs(rx) - mu * pw, 0))
        if positive:
            Bx = np.maximum(Bx, 0.0)
        D = Bx - x
        s = A @ D
        sh = w * s
        sm = float(sh.sum())
        c = (sm / nw if nw > 0 else 0.0) if intercept else 0.0
        l1d = np.where(x * Bx > 0, np.sign(x) * D, np.abs(Bx) - np.abs(x))   # as in penalty_panel_iterate
        r1 = R @ s + mu * float(pw @ l1d)
        r2 = s @ sh - c * sm
        gamma = 0.0 if r2 <= 0 else float(np.clip(-r1 / r2, 0, 1))
        x = x + gamma * D
        R = R + gamma * (sh - c * w)
    out = dict(x=x, r=R)
    if intercept:
        e = A @ x - b
        out["intercept"] = -(float(w @ e) / nw) if nw > 0 else 0.0
    return out


def weighted_duality_gap(A, b, w, x, mu, diag=None, intercept=False, positive=False, p=None, hold=None):
    """The certificate of the weighted problem at x (x >= 0 with ``positive``): e = A x - b (minus its weighted mean
    with ``intercept``), r = w o e, g = A^T r; primal = 1/2 sum w e^2 + mu sum p_j |x_j|, and with gnorm_inf =
    max_j |g_j| / p_j (max_j (-g_j)+ / p_j with ``positive``) and scale = min(1, mu / gnorm_inf) (1 when that is 0),
    dual = -1/2 scale^2 sum w e^2 - scale sum w e b, gap = primal - dual.  The dual point is theta_i = scale
    sqrt(w_i) e_i of the problem on (diag(sqrt w) A, sqrt(w) o b); it is never formed.  The gap-safe score is
    scale |g_j| + sqrt(d_j) sqrt(2 max(gap, 0)) (-g_j with ``positive``), keep_j = not (score_j < mu p_j), with ``diag``
    (default the FULL column norms, ``centred_diag(A)`` with ``intercept``, safe because w <= 1).  holdout_sse =
    sum_i h_i (a_i . x + intercept - b_i)^2 with ``hold`` = h >= 0 (default 1 where w = 0, else 0); intercept =
    -sum w (A x - b) / sum w with ``intercept``, else 0."""
    A = np.asarray(A, dtype=np.float64)
    m, n = A.shape
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    w = _row_weights(w, m)
    nw = float(w.sum())
    mu = float(mu)
    pw = np.ones(n) if p is None else _penalty(p, n)
    h = (w == 0.0).astype(np.float64) if hold is None else np.asarray(hold, dtype=np.float64).reshape(-1)
    e = A @ x - b
    c = (float(w @ e) / nw if nw > 0 else 0.0) if intercept else 0.0
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
    if diag is None:
        dg = centred_diag(A) if intercept else np.square(A).sum(axis=0)
    else:
        dg = np.asarray(diag, dtype=np.float64).reshape(-1)
    score = scale * (-g if positive else np.abs(g)) + np.sqrt(dg) * np.sqrt(2.0 * np.maximum(gap, 0.0))
    return dict(primal=primal, dual=dual, gap=gap, scale=scale, gnorm_inf=gn, holdout_sse=float(h @ (ec * ec)),
                intercept=-c if (intercept and nw > 0) else 0.0, score=score, keep=~(score < mu * pw), g=g, r=r)


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

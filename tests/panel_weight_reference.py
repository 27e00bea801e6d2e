"""Instances and the per-iteration check of the panel solver with observation weights (bpgl_panel_set_row_weights,
DESIGN.md section 16).  Helpers, constants and the unchanged checks are tests/panel_step_reference.py's.

With weights w in [0, 1] per right-hand side the solver carries R^ = w o (A x - b) (w o (e - ebar_w) with the
intercept, ebar_w = sum w e / n_w, n_w = sum w).  ``check_step_weighted`` looks at (x_t, R^_t) and (x_t+1, R^_t+1):

A.  dR^ = w o (A dx).  The device has dR^_i = gamma w_i s_i with s the fp32-accumulated A D', so the first two lines of
    panel_step_reference's bound A (what |gamma s_i - a_i . dx| can be) enter times w_i, and the fp64 line is its own:
        |dR^_i - w_i a_i . dx| <= w_i e_i + 3 * 2^-53 (|R^_t,i| + |R^_t+1,i| + 2 sum_j |a_ij| (|x_t,j| + |x_t+1,j|))
    (w s, gamma (.), R^ + (.): three roundings).  Where w_i = 0: dR^_i == 0 exactly.
    With the intercept dR^_i = gamma (w_i s_i - c w_i), c = sum w s / n_w:
        |dR^_i - w_i (a_i . dx - mean_w(a . dx))| <= w_i (e_i + mean_w(e))
                                                    + 5 * 2^-53 (|R^_t,i| + |R^_t+1,i| + 2 sum_j |a_ij| (|x_t,j| + |x_t+1,j|))
                                                    + 2^-52 m w_i sum_i w_i |a_i . dx| / n_w
    as tests/panel_intercept_reference.py derives it for 0/1 weights (one rounding more for w s; the last line is the
    fixed-order sum of m terms behind c).
B.  The exact line search of the weighted objective on observable state.  gamma = clip(-(rs + mu (...)) / curv, 0, 1)
    with rs = sum R^ s and curv = sum w s^2 (- c sum w s); times gamma, with dR^ = gamma w (s - c) over the rows with
    w_i > 0 (and sum R^ = 0 with the intercept):
        F(gamma) = sum dR^_i^2 / w_i + sum R^_t,i dR^_i / w_i + mu (|gamma x_t + dx|_1 - gamma |x_t|_1)
    is 0 or <= 0 exactly as in panel_step_reference's B, whose bound is used with the weighted sums in its fp64 term.
    A line search that squares w (s^ . s^ for the curvature, R^ . s^ for the numerator) solves another equation and
    leaves F at the size of its terms.
C, D.  panel_step_reference's, unchanged: g = A^T R^_t, the diag in effect, the carried operand V = dR^ + E.
0'. With the intercept sum_i R^_i stays at rounding level; bounded as tests/panel_intercept_reference.py bounds it, with
    its a-priori quantities taken over all rows (w <= 1 only makes them smaller).
"""
import functools

import numpy as np

import panel_intercept_reference as Q
import panel_step_reference as P

U53 = 2.0 ** -53
WEIGHT_SEED = 1610


def general_weights(m, k, seed=WEIGHT_SEED):
    """(m, k) fp64: uniform in (0.05, 1], about one row in eight exactly 0, different per right-hand side."""
    rs = np.random.RandomState(seed + m + k)
    w = 1.0 - 0.95 * rs.rand(m, k)                  # (0.05, 1]
    w[rs.rand(m, k) < 0.125] = 0.0
    return w


def pow4_weights(m, k, seed=WEIGHT_SEED + 1):
    """(m, k) fp64 with entries in {1, 1/4, 1/16, 0}: sqrt(w) is a power of two, so diag(sqrt w) A is exact in bf16."""
    rs = np.random.RandomState(seed + m + k)
    return np.array([1.0, 0.25, 0.0625, 0.0])[rs.randint(0, 4, size=(m, k))]


def holdout_weights(m, k, seed=WEIGHT_SEED + 2):
    """(m, k) fp64 scoring weights in [0, 2): an explicit ``holdout``, positive also at rows that carry a weight."""
    rs = np.random.RandomState(seed + m + k)
    return 2.0 * rs.rand(m, k) * (rs.rand(m, k) < 0.5)


@functools.lru_cache(maxsize=None)
def problem(m, n, k):
    """panel_step_reference.instance's (A, B, mu) with the general weights, read-only."""
    Ab, B, mu = P.instance(m, n, k, seed=m + n + k)
    Wt = general_weights(m, k)
    for a in (Ab, B, mu, Wt):
        a.setflags(write=False)
    return Ab, B, mu, Wt


@functools.lru_cache(maxsize=None)
def trajectory_instance(m, n, k):
    """(Ab, b, B (m, k), mus (k,), Wt (m, k)), read-only: panel_gap_instance's one b against a grid of mu, with general
    weights that differ per column."""
    from panel_gap_instance import instance
    Ab, b, Bm, mus, _ = instance(m, n, k)
    Wt = general_weights(m, k, seed=WEIGHT_SEED + 3)
    Wt.setflags(write=False)
    return Ab, b, Bm, mus, Wt


def weighted_half_norm(Wt, b, intercept):
    """(k,): 1/2 sum_i w_ik b_i^2, b centred over the column's weighted mean with ``intercept`` -- the objective at
    x = 0, which the drivers' GAP_BOUND multiplies."""
    Wk = np.asarray(Wt, dtype=np.float64).T
    Bt = np.repeat(np.asarray(b, dtype=np.float64)[None, :], Wk.shape[0], axis=0)
    bc = wcentre(Wk, Bt) if intercept else Bt
    return 0.5 * (Wk * bc * bc).sum(axis=1)


@functools.lru_cache(maxsize=None)
def weighted_t_ref(m, n, k, intercept, bound=1e-4):
    """The first multiple of 64 at which ``weighted_panel_iterate`` (the diag in effect), its x rounded to fp32, meets
    gap <= bound * weighted_half_norm in every column of ``trajectory_instance`` (tests/panel_cv_instance.cv_t_ref's rule)."""
    from convex_optimization_amd import cpu_calculation as C
    Ab, b, _, mus, Wt = trajectory_instance(m, n, k)
    dg = C.centred_diag(Ab) if intercept else np.square(Ab).sum(axis=0)
    target = bound * weighted_half_norm(Wt, b, intercept)
    X = np.zeros((n, k))
    done = np.zeros(k, dtype=bool)
    for t in range(64, 64 * 64 + 1, 64):
        for c in range(k):
            X[:, c] = C.weighted_panel_iterate(Ab, b, Wt[:, c], mus[c], 64, diag=dg, x0=X[:, c], intercept=intercept)["x"]
            x32 = X[:, c].astype(np.float32).astype(np.float64)
            done[c] = C.weighted_duality_gap(Ab, b, Wt[:, c], x32, mus[c], diag=dg, intercept=intercept)["gap"] <= target[c]
        if done.all():
            return t
    raise AssertionError("the restatement did not reach the bound")


def wcentre(Wk, V):
    """V - its weighted mean per right-hand side, (k, m); V where the weights sum to 0."""
    nw = Wk.sum(axis=1, keepdims=True)
    return V - np.where(nw > 0, (Wk * V).sum(axis=1, keepdims=True) / np.where(nw > 0, nw, 1.0), 0.0)


def check_step_weighted(Ab, diag, mu, Wt, B, t, snap_t, snap_t1, err_t, d_split, exact_iter, dR_prev, chain=None, q=0,
                        R_ref=None, stats=None, intercept=False):
    """Violations (a list of strings, empty = the step is the algorithm's) of A-D (and 0' with ``intercept``) in the
    module docstring for iteration ``t`` between ``snap_t`` and ``snap_t1``.  ``Wt`` (m, k) the weights; ``diag`` the
    diag in effect, (n,) or (1, n[, 1]); ``B`` (m, k) the full right-hand sides; the other arguments are
    ``panel_step_reference.check_step``'s, one feature block."""
    (x0, R0), (x1, R1) = snap_t, snap_t1
    n, k = x0.shape
    m = Ab.shape[0]
    mu = np.asarray(mu, dtype=np.float64)
    Wk = np.asarray(Wt, dtype=np.float64).T                              # (k, m)
    L = float(chain if chain is not None else d_split * n)
    st = {}
    # C, D and the exact parts of A and B (x outside the block, the zero-weight rows, "no direction") are
    # panel_step_reference's own checks on these snapshots; its product check A and its line search B belong to
    # the 0/1 problem and are restated below
    out = [v for v in P.check_step(Ab, np.asarray(diag, dtype=np.float64).reshape(1, n), mu, (Wk != 0).T, 0, snap_t,
                                   snap_t1, err_t, d_split, exact_iter, dR_prev, chain=chain, q=q, R_ref=R_ref, stats=st)
           if not v.startswith(("A: dR != w o (A dx)", "B: not an exact line search"))]
    dx, dR = x1 - x0, R1 - R0
    absA = np.abs(Ab)
    nw = Wk.sum(axis=1, keepdims=True)
    nws = np.where(nw > 0, nw, 1.0)

    def ratio(val, bound):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(bound > 0, val / bound, np.where(val > 0, np.inf, 0.0))

    def report(tag, bad, r):
        if np.any(bad):
            cols = np.flatnonzero(bad if bad.ndim == 1 else bad.any(axis=1))
            out.append(f"{tag}: rhs {cols[:8].tolist()}{'...' if cols.size > 8 else ''}, "
                       f"worst ratio {float(np.max(np.where(bad, r, 0.0))):.3g}")

    # ---- A ------------------------------------------------------------------------------------
    Adx = (Ab @ dx).T                                                    # (k, m)
    sx = (absA @ (np.abs(x0) + np.abs(x1))).T
    e = P.U24 * sx + L * P.U24 * (absA @ np.abs(dx)).T
    fp64 = U53 * (np.abs(R0) + np.abs(R1) + 2.0 * sx)
    if intercept:
        pred = Wk * wcentre(Wk, Adx)
        bound_a = Wk * (e + (Wk * e).sum(axis=1, keepdims=True) / nws) + 5.0 * fp64 \
            + 2.0 * U53 * m * Wk * (Wk * np.abs(Adx)).sum(axis=1, keepdims=True) / nws
    else:
        pred = Wk * Adx
        bound_a = Wk * e + 3.0 * fp64
    dev_a = np.abs(dR - pred)
    ra = ratio(dev_a, bound_a)
    report("A: dR != w o (A dx)" + (" centred" if intercept else ""), dev_a > bound_a, ra)
    st["A"] = float(ra.max())

    # ---- B ------------------------------------------------------------------------------------
    # what gamma^ is (panel_step_reference.gamma_interval, on the same direction bounds check C uses)
    d = np.asarray(diag, dtype=np.float64).reshape(-1)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        rec = np.where(d > 0, 1.0 / np.where(d > 0, d, 1.0), 0.0)
    g = Ab.T @ R0.T
    A2 = np.square(Ab)
    sigma = lambda R: 2.0 ** -17 * np.sqrt(A2.T @ np.square(R).T)      # noqa: E731
    if exact_iter:
        allow = P.C_G * sigma(R0)
    else:
        allow = P.C_G * (2.0 ** -9 * np.sqrt(A2.T @ np.square(dR_prev).T) + q * P.U24 * np.abs(g)
                         + (sigma(R_ref) if R_ref is not None else 0.0))
    D_lo = rec * P.soft_thr(d * x0 - (g + allow), mu) - x0
    D_hi = rec * P.soft_thr(d * x0 - (g - allow), mu) - x0
    g_lo, g_hi = P.gamma_interval(dx, x1, D_lo, D_hi, d_split)
    g_lo = np.minimum(g_lo, g_hi)
    gh, dgh = 0.5 * (g_lo + g_hi), 0.5 * (g_hi - g_lo)
    pos = Wk > 0
    iw = np.where(pos, 1.0 / np.where(pos, Wk, 1.0), 0.0)
    dRdR, RdR = np.einsum("km,km,km->k", dR, dR, iw), np.einsum("km,km,km->k", R0, dR, iw)
    l1_0, l1_1 = np.abs(x0).sum(axis=0), np.abs(x1).sum(axis=0)

    def F(gam):
        return dRdR + RdR + mu * (np.abs(gam * x0 + dx).sum(axis=0) - gam * l1_0)

    flip = (x0 != 0.0) & ((((gh - dgh) * x0 + dx) * x0 <= 0.0) | (((gh + dgh) * x0 + dx) * x0 <= 0.0))
    bound_b = 2.0 ** -22 * mu * (l1_0 + l1_1) + 1e-12 * (dRdR + np.abs(RdR)) \
        + 2.0 * mu * dgh * np.where(flip, np.abs(x0), 0.0).sum(axis=0)
    Fh = F(gh)
    dev_b = np.where(g_hi < 1.0 - 1e-6, np.abs(Fh), np.where(g_lo >= 1.0 - 1e-6, np.maximum(F(np.ones(k)), 0.0),
                                                            np.maximum(Fh, 0.0)))
    dev_b = np.where(~dx.any(axis=0), 0.0, dev_b)
    rb = ratio(dev_b, bound_b)
    report("B: not an exact line search of the weighted objective", dev_b > bound_b, rb)
    st["B"] = float(rb.max())

    # ---- 0' -----------------------------------------------------------------------------------
    if intercept:
        worst0 = 0.0
        ones = np.ones((k, m), dtype=bool)
        for tt, R in ((t, R0), (t + 1, R1)):
            s = np.abs(R.sum(axis=1))
            bnd = Q.sum_bound(Ab, B, mu, ones, tt)
            r0 = ratio(s, bnd)
            worst0 = max(worst0, float(r0.max()))
            if np.any(s > bnd):
                cols = np.flatnonzero(s > bnd)
                out.append(f"0': sum R_{tt} != 0: rhs {cols[:8].tolist()}, worst |sum| {float(s.max()):.3g} "
                           f"against {float(bnd[cols[0]]):.3g}")
        st["0"] = worst0
    if stats is not None:
        for key, v in st.items():
            if key == "gamma_min":
                stats[key] = min(stats.get(key, np.inf), v)
            else:
                stats[key] = max(stats.get(key, -np.inf if key == "gamma_max" else 0.0), v)
    return out

"""Per-iteration checks of the panel solver with the intercept (bpgl_panel_set_intercept, DESIGN.md
section 13): ``check_step_intercept`` restates checks A-D of tests/panel_step_reference.py for the
profiled problem and adds 0'.  Helpers, constants and the unchanged checks are panel_step_reference's.

With the intercept the solver carries R = P_w (A x - b), P_w v = w o (v - (w . v) / n_w), per right-hand
side; n_w = the in-rows, all rows without a user mask.  One feature block.

A.  dR = P_w (A dx); held-out rows exactly 0.  The device has dR_i = gamma (s_i - c) at the in-rows,
    c = sum_in s / n_w in fp64 from the fp32-accumulated S of panel_step_reference's A, whose first two
    lines e_i bound |gamma s_i - a_i . dx|.  The mean inherits the mean of those, so
        |dR_i - (a_i . dx - mean_in(a . dx))| <= e_i + mean_in(e)
                                                 + 4 * 2^-53 (|R_t,i| + |R_t+1,i| + 2 sum_j |a_ij| (|x_t,j| + |x_t+1,j|))
                                                 + 2^-52 sum_in |a . dx|
    the last two lines the fp64 part: s - c, gamma (.), R + (.) and c's division are four roundings of
    values no larger than the bracket, and c's fixed-order sum of n_w terms is off by at most
    n_w 2^-53 mean_in |gamma s| (doubled: it is a sum of sums).
B.  unchanged.  gamma = clip(-(R.s + mu (...)) / |P_w s|^2, 0, 1); times gamma, with P_w s = dR / gamma and
    R.s = R.(P_w s) because R is centred, F(gamma) of panel_step_reference is 0 or <= 0 as there.
C.  unchanged but for its inputs: g = A^T R_t with the centred R_t, and d the centred diag
    sum_i (a_ij - mean_j)^2 (the context's ``diag_ATA`` with the intercept on).
D.  unchanged.
0'. |sum_in R_t| stays at rounding level.  P_w is a projector, so the exact sum is 0; what the device
    accumulates, with u = 2^-53:
      reset: mean_in b is off by <= n_w u mean_in |b| and each b_i - mean is rounded once:
             |sum_in R_0| <= u (n_w sum_in |b_i| + sum_in |R_0,i|);
      each step: c is off by <= (n_w + 1) u sum_in |s| / n_w, and s - c, gamma (.), R + (.) round once each:
             the sum moves by <= u ((n_w + 4) sum_in gamma |s_i| + 3 sum_in |dR_i| + sum_in |R_t+1,i|).
    A priori, from the problem alone: every step is an exact line search, so the objective never exceeds
    F(0) = 1/2 |P_w b|^2 =: 1/2 beta^2; hence |R_s|_2 <= beta, sum_in |R_s,i| <= sqrt(n_w) beta,
    sum_in |dR_s,i| <= 2 sqrt(n_w) beta, mu |x_s|_1 <= 1/2 beta^2, and gamma |s_i| = |a_i . dx_s| (+ rounding)
    <= a_max (|x_s|_1 + |x_s+1|_1) <= a_max beta^2 / mu.  After t steps
        |sum_in R_t| <= 2^-53 [ n_w sum_in |b_i| + sqrt(n_w) beta
                                + t ((n_w + 4) n_w a_max beta^2 / mu + 7 sqrt(n_w) beta) ]
    (a warm reset at an iterate x of the same problem has sum_in |e_i| <= sum_in |b_i| + n_w a_max beta^2 / (2 mu)
    in the first term; the bracket's t-term covers it from t = 1 on, and the check counts a warm reset as
    one step more).  Loose by the factor n_w of every worst-case summation bound, and still eight or more
    orders below what a wrong centring leaves: c taken over all rows, or B stored uncentred, puts
    |sum_in R| at the size of |c| n_out or |mean b| n_w.
"""
import numpy as np

import panel_step_reference as P

U53 = 2.0 ** -53


def in_rows(W, k, m):
    """(k, m) bool: the rows in each right-hand side's objective (all of them without a mask)."""
    return np.ones((k, m), dtype=bool) if W is None else (np.asarray(W).T != 0)


def centre(Wk, V):
    """P_w of every row of V (k, m): 0 at the held-out entries, the in-row mean taken off the others."""
    nw = Wk.sum(axis=1, keepdims=True)
    mean = np.where(Wk, V, 0.0).sum(axis=1, keepdims=True) / np.maximum(nw, 1)
    return np.where(Wk, V - mean, 0.0)


def sum_bound(Ab, B, mu, Wk, t):
    """The a-priori bound of 0' on |sum_in R_t|, (k,), after ``t`` steps from a reset (module docstring)."""
    nw = Wk.sum(axis=1).astype(np.float64)
    Bt = np.asarray(B, dtype=np.float64).T
    beta = np.linalg.norm(centre(Wk, Bt), axis=1)
    a_max = float(np.abs(Ab).max())
    sb = np.where(Wk, np.abs(Bt), 0.0).sum(axis=1)
    with np.errstate(divide="ignore"):
        per_step = (nw + 4.0) * nw * a_max * beta ** 2 / np.asarray(mu, dtype=np.float64) + 7.0 * np.sqrt(nw) * beta
    return U53 * (nw * sb + np.sqrt(nw) * beta + t * per_step)


def check_step_intercept(Ab, diag, mu, W, B, t, snap_t, snap_t1, err_t, d_split, exact_iter, dR_prev, chain=None,
                         q=0, R_ref=None, stats=None, warm=0):
    """Violations (a list of strings, empty = the step is the algorithm's) of A-D and 0' in the module
    docstring for iteration ``t`` (counted from the reset; ``warm`` = 1 after a warm reset) between
    ``snap_t`` and ``snap_t1``.  ``diag`` is the centred diag (n,) or (1, n[, 1]); ``B`` (m, k) the full
    right-hand sides; the other arguments are ``panel_step_reference.check_step``'s, one feature block."""
    (x0, R0), (x1, R1) = snap_t, snap_t1
    n, k = x0.shape
    m = Ab.shape[0]
    mu = np.asarray(mu, dtype=np.float64)
    Wk = in_rows(W, k, m)
    L = float(chain if chain is not None else d_split * n)
    st = {}
    # B, C, D and the exact parts of A (x outside the block, held-out rows) are panel_step_reference's own
    # checks on these snapshots, with the centred diag; its product check A belongs to the masked problem
    # and is replaced by the centred one below
    out = [v for v in P.check_step(Ab, np.asarray(diag, dtype=np.float64).reshape(1, n), mu, W, 0, snap_t, snap_t1,
                                   err_t, d_split, exact_iter, dR_prev, chain=chain, q=q, R_ref=R_ref, stats=st)
           if not v.startswith("A: dR != w o (A dx)")]
    # ---- A ------------------------------------------------------------------------------------
    dx, dR = x1 - x0, R1 - R0
    absA = np.abs(Ab)
    Adx = (Ab @ dx).T                                                   # (k, m)
    pred = centre(Wk, Adx)
    nw = np.maximum(Wk.sum(axis=1, keepdims=True), 1)
    sx = (absA @ (np.abs(x0) + np.abs(x1))).T
    e = np.where(Wk, P.U24 * sx + L * P.U24 * (absA @ np.abs(dx)).T, 0.0)
    bound_a = e + e.sum(axis=1, keepdims=True) / nw + 4.0 * U53 * (np.abs(R0) + np.abs(R1) + 2.0 * sx) \
        + 2.0 * U53 * np.where(Wk, np.abs(Adx), 0.0).sum(axis=1, keepdims=True)
    dev_a = np.where(Wk, np.abs(dR - pred), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ra = np.where(bound_a > 0, dev_a / bound_a, np.where(dev_a > 0, np.inf, 0.0))
    bad = dev_a > bound_a
    if np.any(bad):
        cols = np.flatnonzero(bad.any(axis=1))
        out.append(f"A: dR != P_w (A dx): rhs {cols[:8].tolist()}{'...' if cols.size > 8 else ''}, "
                   f"worst ratio {float(ra.max()):.3g}")
    st["A"] = float(ra.max())
    # ---- 0' -----------------------------------------------------------------------------------
    worst0 = 0.0
    for tt, R in ((t + warm, R0), (t + 1 + warm, R1)):
        s = np.abs(np.where(Wk, R, 0.0).sum(axis=1))
        bnd = sum_bound(Ab, B, mu, Wk, tt)
        with np.errstate(divide="ignore", invalid="ignore"):
            r0 = np.where(bnd > 0, s / bnd, np.where(s > 0, np.inf, 0.0))
        worst0 = max(worst0, float(r0.max()))
        if np.any(s > bnd):
            cols = np.flatnonzero(s > bnd)
            out.append(f"0': sum_in R_{tt - warm} != 0: rhs {cols[:8].tolist()}, worst |sum| {float(s.max()):.3g} "
                       f"against {float(bnd[cols[0]]):.3g}")
    st["0"] = worst0
    if stats is not None:
        for key, v in st.items():
            if key in ("gamma_min",):
                stats[key] = min(stats.get(key, np.inf), v)
            else:
                stats[key] = max(stats.get(key, -np.inf if key == "gamma_max" else 0.0), v)
    return out


def check_certificate(cert, ref, rtol=1e-9):
    """Violations of a certificate's intercept and held-out score (dicts with ``intercept`` and
    ``holdout_sse``, scalars or (k,) arrays) against ``cpu_calculation.intercept_duality_gap``'s, to the
    certificate tests' relative 1e-9."""
    out = []
    for key in ("intercept", "holdout_sse"):
        a, b = np.asarray(cert[key], dtype=np.float64), np.asarray(ref[key], dtype=np.float64)
        if not np.all(np.abs(a - b) <= rtol * np.abs(b)):
            out.append(f"{key}: {a.reshape(-1)[:4]} against {b.reshape(-1)[:4]}")
    return out

"""Per-iteration checks of the panel solver with the sign constraint x >= 0 (bpgl_panel_set_positive,
DESIGN.md section 14): ``check_step_positive`` restates checks A-D of tests/panel_step_reference.py for

    min 1/2 || w o (A x - b) ||^2 + mu sum_j x_j   subject to x >= 0

(with the intercept's profiling: P_w in place of w o, and panel_intercept_reference's A and 0') and adds two
exact checks.  Helpers, constants and notation are panel_step_reference's.

A, B.  unchanged.  dR = w o (A_mb dx) is the reason the constraint is enforced on the direction's image and
    not by a clamp of x after the update: R is a recurrence, and a clamped x would leave dR != A dx (the
    clamp-after-update mutant of tests/test_panel_positive_host.py fails A).  The line search's
    |x_t + D'|_1 - |x_t|_1 is sum D' on the feasible set, so F(gamma) is the same function.

C.  dx = gamma D' with the one-sided prox D = max(0, S(d o x_t - g, mu) / d) - x_t.  max(0, .) is 1-Lipschitz,
    so the gradient allowance carries over.  The image: the device takes the nearest bf16 image of D (or the
    hi + lo pair), and where that has x_t + D' < 0 its neighbour towards zero (the lo piece one step up).
    That can happen only where x_t,j > 0 and the nearest image of some D in [D_lo,j, D_hi,j] lies below
    -x_t,j (``fire``); there the image error is one bf16 ulp instead of half, u_D = 2^-7 (2^-15 for hi + lo),
    everywhere else today's 2^-8 (2^-16).  ``gamma_interval`` uses the same images: bf16 with the
    towards-zero rule is monotone in D for a fixed x_t (if D_1 < D_2 and only D_1's image is moved, it moves to
    a bf16 value <= the image of D_2), and the pair's upper end gets 2^-15 on ``fire``.
    Coordinates with x_t,j = 0 and g_j >= -(mu - allow_j) have D = 0 on the device too and must be exactly 0
    in x_{t+1} (P2) -- one-sided: a large positive g_j keeps a zero at zero.

D.  err_t = max |x_t - max(0, x_t - g - mu)|_inf, the prox residual of the constrained problem; 1-Lipschitz
    in g as before.

P1. x_{t+1} >= 0 everywhere, exactly: x_t + D' >= 0 in fp64, gamma in [0, 1], and the fp32 store of a
    non-negative fp64 value is non-negative.
"""
import numpy as np

import panel_intercept_reference as Q
import panel_step_reference as P

U24, C_G = P.U24, P.C_G


def bf16_up(h):
    """The bf16 neighbour towards +inf of the bf16 values ``h`` (fp64 array holding bf16 values)."""
    b = np.asarray(h, dtype=np.float32).view(np.uint32) >> 16
    b = np.where(b & 0x8000, b - 1, b + 1).astype(np.uint32) << 16
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def feasible_image(D, x, d_split, nearest_only=False):
    """The direction image the device forms from D at x >= 0: the nearest bf16 (or hi + lo pair), moved one
    bf16 step up where x + image < 0.  Returns (image, fired)."""
    if d_split == 1:
        img = P.bf16(D)
        fired = x + img < 0.0
        if nearest_only:
            return img, fired
        return np.where(fired, bf16_up(img), img), fired
    hi, lo = P.split_bf16(D)
    fired = x + (hi + lo) < 0.0
    if nearest_only:
        return hi + lo, fired
    return hi + np.where(fired, bf16_up(lo), lo), fired


def prox_dir(d, x, g, mu):
    """D = max(0, S(d x - g, mu) / d) - x"""
    return np.maximum(P.soft_thr(d * x - g, mu) / d, 0.0) - x


def gamma_interval_positive(dxb, x0b, x1b, D_lo, D_hi, d_split, fire):
    """``panel_step_reference.gamma_interval`` with the feasible images (module docstring, C)."""
    if d_split == 1:
        lo_i, hi_i = feasible_image(D_lo, x0b, 1)[0], feasible_image(D_hi, x0b, 1)[0]
    else:
        lo_i = D_lo - 1.01 * 2.0 ** -16 * np.abs(D_lo)
        hi_i = D_hi + 1.01 * np.where(fire, 2.0 ** -15, 2.0 ** -16) * np.abs(D_hi)
    neg = hi_i < 0
    use = (lo_i > 2.0 ** -100) | (hi_i < -2.0 ** -100)
    near = np.where(neg, -hi_i, lo_i)
    far = np.where(neg, -lo_i, hi_i)
    num = np.where(neg, -dxb, dxb)
    e = U24 * np.abs(x1b) + 2.0 ** -149
    nl, nh = num - e, num + e
    with np.errstate(divide="ignore", invalid="ignore"):
        g_lo = np.where(use, np.where(nl >= 0, nl / far, nl / near), -np.inf)
        g_hi = np.where(use, np.where(nh >= 0, nh / near, nh / far), np.inf)
    return np.maximum(g_lo.max(axis=0), 0.0), np.minimum(g_hi.min(axis=0), 1.0)


def check_step_positive(Ab, diag, mu, W, block, snap_t, snap_t1, err_t, d_split, exact_iter, dR_prev, chain=None,
                        q=0, R_ref=None, stats=None, intercept=False, B=None, t=0, warm=0):
    """Violations (a list of strings, empty = the step is the constrained algorithm's) of A-D, P1 and P2 of the
    module docstring.  The arguments are ``panel_step_reference.check_step``'s; ``intercept``: the profiled
    problem (one feature block; ``diag`` the centred diag, ``B`` (m, k) the full right-hand sides, ``t`` the
    iteration counted from the reset and ``warm`` as in ``check_step_intercept``, for 0').  ``stats`` receives
    the worst ratio to bound of "A", "B", "C", "D" (and "0"), the smallest stored x ("x_min") and the number of
    coordinates on which the feasible-image rule can fire ("fire")."""
    (x0, R0), (x1, R1) = snap_t, snap_t1
    diag = np.asarray(diag, dtype=np.float64)
    n, k = x0.shape
    nblock = 1 if intercept else diag.shape[0]
    d = diag.reshape(nblock, -1)[block][:, None]                      # (w, 1)
    w = n // nblock
    sl = slice(block * w, (block + 1) * w)
    mu = np.asarray(mu, dtype=np.float64)
    L = float(chain if chain is not None else d_split * w)
    Wk = np.ones(R0.shape, dtype=bool) if W is None else (np.asarray(W).T != 0)   # (k, m)
    Am = Ab[:, sl]
    absA, A2 = np.abs(Am), np.square(Am)
    x0b, x1b = x0[sl], x1[sl]
    dxb = x1b - x0b
    dR = R1 - R0
    out = []
    worst = dict(A=0.0, B=0.0, C=0.0, D=0.0)

    def ratio(key, val, bound):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound > 0, val / bound, np.where(val > 0, np.inf, 0.0))
        worst[key] = max(worst.get(key, 0.0), float(np.max(r))) if r.size else worst.get(key, 0.0)
        return r

    def report(tag, bad, r, rhs_axis):
        if np.any(bad):
            cols = np.flatnonzero(bad if bad.ndim == 1 else bad.any(axis=1 - rhs_axis))
            out.append(f"{tag}: rhs {cols[:8].tolist()}{'...' if cols.size > 8 else ''}, "
                       f"worst ratio {float(np.max(np.where(bad, r, 0.0))):.3g}")

    # ---- P1 -----------------------------------------------------------------------------------
    if not np.all(x1 >= 0.0):
        out.append(f"P1: {int(np.count_nonzero(~(x1 >= 0.0)))} entries of x_t+1 are not >= 0, min {float(np.nanmin(x1)):.3g}")

    # ---- A ------------------------------------------------------------------------------------
    other = np.ones(n, dtype=bool)
    other[sl] = False
    if not np.array_equal(x0[other], x1[other]):
        out.append("A: x changed outside the iteration's block")
    if np.any(dR[~Wk] != 0.0):
        out.append(f"A: dR != 0 on {int(np.count_nonzero(dR[~Wk]))} held-out rows")
    sx_b = (absA @ (np.abs(x0b) + np.abs(x1b))).T
    if intercept:        # panel_intercept_reference's A
        Adx = (Am @ dxb).T
        pred = Q.centre(Wk, Adx)
        nw = np.maximum(Wk.sum(axis=1, keepdims=True), 1)
        e = np.where(Wk, U24 * sx_b + L * U24 * (absA @ np.abs(dxb)).T, 0.0)
        bound_a = e + e.sum(axis=1, keepdims=True) / nw + 4.0 * Q.U53 * (np.abs(R0) + np.abs(R1) + 2.0 * sx_b) \
            + 2.0 * Q.U53 * np.where(Wk, np.abs(Adx), 0.0).sum(axis=1, keepdims=True)
    else:
        pred = np.where(Wk, (Am @ dxb).T, 0.0)
        sx_all = (np.abs(Ab) @ (np.abs(x0) + np.abs(x1))).T if nblock > 1 else sx_b
        bound_a = U24 * sx_b + L * U24 * (absA @ np.abs(dxb)).T \
            + (nblock + 2) * 2.0 ** -53 * (np.abs(R0) + np.abs(R1) + 2.0 * sx_all)
    dev_a = np.where(Wk, np.abs(dR - pred), 0.0)
    r = ratio("A", dev_a, bound_a)
    report("A: dR != P_w (A dx)" if intercept else "A: dR != w o (A dx)", dev_a > bound_a, r, 0)
    still = ~dxb.any(axis=0)

    # ---- C: the direction ------------------------------------------------------------------------
    g = Am.T @ R0.T                                                    # (w, k)
    D = prox_dir(d, x0b, g, mu)
    sigma = lambda R: 2.0 ** -17 * np.sqrt(A2.T @ np.square(R).T)      # noqa: E731
    if exact_iter:
        allow = C_G * sigma(R0)
    else:
        allow = C_G * (2.0 ** -9 * np.sqrt(A2.T @ np.square(dR_prev).T) + q * U24 * np.abs(g)
                       + (sigma(R_ref) if R_ref is not None else 0.0))
    D_lo, D_hi = prox_dir(d, x0b, g + allow, mu), prox_dir(d, x0b, g - allow, mu)
    # where the towards-zero rule can fire: x_t > 0 and the nearest image of the most negative admissible D
    # overshoots -x_t
    near_lo = P.bf16(D_lo) if d_split == 1 else D_lo - 1.01 * 2.0 ** -16 * np.abs(D_lo)
    fire = (x0b > 0.0) & (x0b + near_lo < 0.0)
    u_half = 2.0 ** -8 if d_split == 1 else 2.0 ** -16
    u_D = np.where(fire, 2.0 * u_half, u_half)
    none = ~(D_lo.any(axis=0) | D_hi.any(axis=0))
    if np.any(dxb[:, none] != 0.0) or np.any(dR[none] != 0.0):
        moved = np.flatnonzero(none & (dR.any(axis=1) | ~still))
        out.append(f"B: no direction but the state moved, rhs {moved[:8].tolist()}")
    g_lo, g_hi = gamma_interval_positive(dxb, x0b, x1b, D_lo, D_hi, d_split, fire)
    bad = g_lo > g_hi * (1.0 + 1e-12)
    if np.any(bad):
        out.append(f"C: no step size explains dx: rhs {np.flatnonzero(bad)[:8].tolist()}, "
                   f"[{g_lo[bad][0]:.9g}, {g_hi[bad][0]:.9g}]")
    g_lo = np.minimum(g_lo, g_hi)
    gh, dgh = 0.5 * (g_lo + g_hi), 0.5 * (g_hi - g_lo)
    bound_c = gh * (allow / d + u_D * np.abs(D)) + 2.0 ** -23 * np.maximum(np.abs(x0b), np.abs(x1b)) + dgh * np.abs(D) \
        + 2.0 ** -148
    dev_c = np.abs(dxb - gh * D)
    r = ratio("C", dev_c, bound_c)
    report("C: dx != gamma^ D", dev_c > bound_c, r, 1)
    # ---- P2 -----------------------------------------------------------------------------------
    zero = (x0b == 0.0) & (g >= -(mu - allow))
    if np.any(x1b[zero] != 0.0):
        out.append(f"P2: {int(np.count_nonzero(x1b[zero]))} coordinates with x_t = 0 and g >= -(mu - allow) moved")

    # ---- B: the line search ---------------------------------------------------------------------
    l1_0, l1_1 = np.abs(x0b).sum(axis=0), np.abs(x1b).sum(axis=0)
    dRdR, RdR = np.einsum("km,km->k", dR, dR), np.einsum("km,km->k", R0, dR)

    def F(gam):
        return dRdR + RdR + mu * (np.abs(gam * x0b + dxb).sum(axis=0) - gam * l1_0)

    flip = (x0b != 0.0) & ((((gh - dgh) * x0b + dxb) * x0b <= 0.0) | (((gh + dgh) * x0b + dxb) * x0b <= 0.0))
    bound_b = 2.0 ** -22 * mu * (l1_0 + l1_1) + 1e-12 * (dRdR + np.abs(RdR)) \
        + 2.0 * mu * dgh * np.where(flip, np.abs(x0b), 0.0).sum(axis=0)
    Fh = F(gh)
    dev_b = np.where(g_hi < 1.0 - 1e-6, np.abs(Fh), np.where(g_lo >= 1.0 - 1e-6, np.maximum(F(np.ones(k)), 0.0),
                                                            np.maximum(Fh, 0.0)))
    dev_b = np.where(still, 0.0, dev_b)
    r = ratio("B", dev_b, bound_b)
    report("B: not an exact line search", dev_b > bound_b, r, 0)

    # ---- D: the error record --------------------------------------------------------------------
    if err_t is not None:
        err_ref = float(np.max(np.abs(x0b - np.maximum(x0b - g - mu, 0.0))))
        tol = float(np.max(allow))
        dev_d = abs(float(err_t) - err_ref)
        worst["D"] = max(worst["D"], dev_d / tol if tol > 0 else (np.inf if dev_d > 0 else 0.0))
        if not dev_d <= tol:
            out.append(f"D: err {float(err_t):.17g} against {err_ref:.17g}, allowance {tol:.3g}")

    # ---- 0' (intercept) -------------------------------------------------------------------------
    if intercept:
        worst["0"] = 0.0
        for tt, R in ((t + warm, R0), (t + 1 + warm, R1)):
            s = np.abs(np.where(Wk, R, 0.0).sum(axis=1))
            bnd = Q.sum_bound(Ab, B, mu, Wk, tt)
            ratio("0", s, bnd)
            if np.any(s > bnd):
                out.append(f"0': sum_in R_{tt - warm} != 0: rhs {np.flatnonzero(s > bnd)[:8].tolist()}")
    if stats is not None:
        for key, v in worst.items():
            stats[key] = max(stats.get(key, 0.0), v)
        stats["gamma_min"] = min(stats.get("gamma_min", np.inf), float(gh.min()))
        stats["gamma_max"] = max(stats.get("gamma_max", -np.inf), float(gh.max()))
        stats["dgamma"] = max(stats.get("dgamma", 0.0), float(dgh.max()))
        stats["x_min"] = min(stats.get("x_min", np.inf), float(x1.min()))
        stats["fire"] = stats.get("fire", 0) + int(np.count_nonzero(fire))
    return out


def drift_bound(Ab, xs, chain, R0_max):
    """Bound on max_i |R_T,i - (A x_T - b)_i| per right-hand side, (k,), for a solver whose every step meets check A
    from one feature block's stored iterates ``xs`` = [x_0, ..., x_T] ((n, k) each; R_0 exact): R is the recurrence
    R_t+1 = R_t + dR_t, so the drift is at most the sum over the steps of check A's bound,
        sum_t [ 2^-24 sum_j |a_ij| (|x_t,j| + |x_t+1,j|) + chain 2^-24 sum_j |a_ij| |x_t+1,j - x_t,j| ]
              + T 3 2^-53 (max |R_0| + 2 max_t sum_j |a_ij| |x_t,j|)
    (the fp32 store of x; the fp32 accumulation chain of pass 2; the fp64 roundings of R + gamma S, with |R_t| <=
    |R_0| for a descent method), maximised over the rows i.  Worst-case summation over T steps, so a correct run stays
    far inside it (the numpy model: 0.003 of it after 256 iterations at 256 x 512); a clamp of x after the update
    with the bf16 direction leaves 3.7 times the bound on its worst right-hand side there
    (tests/test_panel_positive_host.py::test_drift_bound_separates_the_clamp).  With the hi + lo direction the
    clamped overshoot is 2^-16 of x and no drift bound can tell it from rounding; checks A and P1 do."""
    absA = np.abs(Ab)
    T = len(xs) - 1
    tot = np.zeros((Ab.shape[0], xs[0].shape[1]))
    sx_max = np.zeros_like(tot)
    for t in range(T):
        sx = absA @ (np.abs(xs[t]) + np.abs(xs[t + 1]))
        tot += U24 * sx + chain * U24 * (absA @ np.abs(xs[t + 1] - xs[t]))
        sx_max = np.maximum(sx_max, sx)
    tot += T * 3.0 * 2.0 ** -53 * (R0_max + 2.0 * sx_max)
    return tot.max(axis=0)

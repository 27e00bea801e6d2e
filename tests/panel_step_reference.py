"""Per-iteration checks of the panel solver (csrc/bpgl_panel.h) from two snapshots of its own state.

``check_step`` looks at (x_t, R_t) and (x_{t+1}, R_{t+1}) of ONE iteration, all right-hand sides at once,
and decides in numpy fp64 on the stored bf16 A whether the step between them is the algorithm's step.
It emulates nothing: every bound below is an exact invariant of the device's state or follows from the
operand precisions that bpgl_panel.h documents (R as a hi + lo bf16 pair, the direction as bf16 or
hi + lo, fp32 MFMA accumulation inside a pass-2 column chunk, fp32 x, fp64 everything else).

Notation, per right-hand side: dx = x_{t+1} - x_t on the iteration's block mb = t % Block,
dR = R_{t+1} - R_t, w the mask column (ones without a mask), u = 2^-24 (fp32 unit roundoff), D' the
direction the MFMA saw (the bf16 image(s) of the shrink's D) and gamma the device's step size, neither
of which is observable: gamma D' = dx + rho with |rho_j| <= u |x_{t+1,j}| (x is stored once per step,
round to nearest).

A.  dR = w o (A_mb dx).  The device has dR = gamma S, S = w o (A_mb D') with fp32 accumulation over the
    L terms of one pass-2 chain, so
        |dR_i - w_i a_i.dx| <= u sum_j |a_ij| (|x_t,j| + |x_t+1,j|)       (a_i.rho, over the block)
                               + L u sum_j |a_ij| |dx_j|                  (recursive fp32 summation)
                               + (Block + 2) 2^-53 (|R_t,i| + |R_t+1,i| + 2 sum_j |a_ij| (|x_t,j| + |x_t+1,j|))
    The last line is the fp64 part: R + gamma S (one block) or sum_b Ax_b - B (several) is at most
    Block + 2 roundings of partial sums no larger than |B_i| + sum_b |Ax_b,i| <= |R_i| + 2 sum_j |a_ij||x_j|
    (j over all of x); it is ~2^-29 of the first line wherever x != 0.  Held-out rows: dR_i == 0 exactly
    (S is zeroed by select); other blocks' x bitwise unchanged.

C.  dx = gamma D' with D = S(d o x_t - g, mu) / d - x_t, g = A_mb^T R_t, d the context's diag.  The
    shrink is 1-Lipschitz in g, so |D_dev,j - D_j| <= |g_dev,j - g_j| / d_j, and D' = D_dev (1 + e),
    |e| <= 2^-8 (bf16 has an 8-bit significand) or 2^-16 (hi + lo).  The gradient allowance allow_j:
      exact iteration: C_g sigma_j, sigma_j = 2^-17 sqrt(sum_i a_ij^2 R_t,i^2) -- the scale of
        sum_i a_ij (R_i - hi_i - lo_i) for independent roundings of relative size <= 2^-16 (rms about
        2^-17); C_g = 8.  test_panel_step_host.py measures the model's noise at <= 1.8 sigma_j.
        The fp32 result adds <= 2^-24 |g_j| <= 2^-24 sqrt(m) sigma_j 2^17 < sigma_j for m < 2^14.
      carried iteration, q iterations after the refresh at t0 (panel_put_carry): V_i = dR_i + E_{i-1},
        E_i = V_i - bf16(V_i), E_{t0-1} := 0, and G_t = G_t0 + sum_{t0 <= i < t} A^T bf16(V_i) in fp32.
        The sum telescopes: sum bf16(V_i) = (R_t - R_t0) - E_{t-1}, so
            G_t - A^T R_t = (G_t0 - A^T R_t0) - A^T E_{t-1} + (q fp32 roundings of G, each <= u |g_j|)
        with |E_{t-1}| <= 2^-8 |V_{t-1}| (rms about 2^-9) and V_{t-1} = dR_{t-1} up to 2^-8.  Hence
            allow_j = C_g (2^-9 sqrt(sum_i a_ij^2 dR_{t-1,i}^2) + q u |g_j| + sigma_j(R_t0)).
        The last term is the refresh's own error, which the recurrence carries unchanged until the next
        refresh (``R_ref``; it is below the first term while |dR_{t-1}| > 2^-8 |R_t0|).
    gamma^ +- dgamma is the interval of step sizes that every coordinate admits (``gamma_interval``; empty:
    a violation).  Elementwise
        |dx_j - gamma^ D_j| <= gamma^ (allow_j / d_j + u_D |D_j|) + 2^-23 max(|x_t,j|, |x_t+1,j|) + dgamma |D_j|
    with u_D = 2^-8 (bf16) or 2^-16 (hi + lo): the image's rounding itself, no margin (the correct model
    reaches 0.99 of it).  Coordinates with x_t,j = 0 and |g_j| <= mu - allow_j shrink to D = 0 on the device
    too and must be exactly 0 in x_{t+1}.

B.  gamma = clip(-(R_t.S + mu (|x_t + D'|_1 - |x_t|_1)) / S.S, 0, 1) in fp64 on the device.  Times
    gamma, with S = dR / gamma and gamma D' = dx + rho:
        F(gamma) = |dR|^2 + R_t.dR + mu (|gamma x_t + dx|_1 - gamma |x_t|_1)
    is 0 (unclipped) or <= 0 (gamma = 1) up to mu |rho|_1 <= u mu |x_t+1|_1 and the fp64 roundings of
    the two dot products; the bound is 2^-22 mu (|x_t|_1 + |x_t+1|_1) + 1e-12 (|dR|^2 + |R_t.dR|) plus
    the uncertainty of gamma^, the midpoint of ``gamma_interval`` (dgamma its half width):
        dF/dgamma = mu sum_j (sign(gamma x_t,j + dx_j) - sign(x_t,j)) x_t,j
    is zero except on the coordinates the step carries through or onto zero, where it is -2 mu |x_t,j|, so
        |F(gamma^) - F(gamma)| <= 2 mu dgamma sum_{j in flip} |x_t,j|,
    flip = {j: x_t,j != 0 and (gamma' x_t,j + dx_j) x_t,j <= 0 at gamma' = gamma^ - dgamma or gamma^ + dgamma}
    (gamma' x + dx is linear in gamma': the two ends decide).  The interval also decides the case: hi < 1:
    |F(gamma^)| <= bound; lo = 1: F(1) <= bound; undecided: F(gamma^) <= bound, which holds either way.
    A right-hand side whose direction is surely zero (the shrink gives D = 0 at g -+ allow in every
    coordinate): dx == 0 and dR == 0 exactly.  (dx == 0 alone does not make dR zero: near convergence every
    gamma D'_j can fall below half an ulp of the fp32 x_j while the fp64 R still moves; A's first term
    covers exactly that.)

D.  err_t = max over the right-hand sides of |g - clip(g - x_t, -mu, mu)|_inf on the block at x_t, before
    the update.  1-Lipschitz in g: the device value is within max allow_j of the reference's.
"""
import numpy as np

U24 = 2.0 ** -24
C_G = 8.0


# --------------------------------------------------------------------------------------------------
# bf16 as csrc/bpgl_panel.h has it: to_bf16 is the compiler's float -> __bf16 conversion, round to
# nearest even (as torch's CPU bfloat16 is; test_panel_step_host.py compares the two), and split_bf16
# is f = (float)v, hi = bf16(f), lo = bf16((float)(v - hi))
# --------------------------------------------------------------------------------------------------
def bf16(v):
    """fp64 values of bf16((float)v), round to nearest even at both roundings."""
    b = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def split_bf16(v):
    v = np.asarray(v, dtype=np.float64)
    hi = bf16(v)
    return hi, bf16(v - hi)


def f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def soft_thr(t, tau):
    return np.sign(t) * np.maximum(np.abs(t) - tau, 0.0)


def instance(m, n, k, seed=0):
    """tests/test_panel.py::instance's A and B (same draws, same bf16 rounding), and per right-hand side
    mu_j = ||A^T b_j||_inf * geomspace(0.3, 0.05, k)_j: a distinct b and a distinct mu per column."""
    import torch
    rs = np.random.RandomState(seed)
    A = rs.randn(m, n)
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    Ab = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()
    X = rs.randn(n, k) * (rs.rand(n, k) < 0.4)
    B = Ab @ X + 0.01 * rs.randn(m, k)
    mu = np.abs(Ab.T @ B).max(axis=0) * np.geomspace(0.3, 0.05, k)
    return Ab, B, mu


def fold_mask(m, k, n_folds=4, seed=7):
    """(m, k) uint8: column c holds fold c % n_folds of ``kfold_masks(m, n_folds, seed)`` (0 = held out)."""
    from convex_optimization_amd.cpu_calculation import kfold_masks
    return np.ascontiguousarray(kfold_masks(m, n_folds, seed=seed)[np.arange(k) % n_folds].T)


def snapshot(pl):
    """(x (n, k) fp64 copy of the fp32 iterate, R (k, m) fp64 copy of the solver's residual)."""
    x = pl.solver_x()   # drains the stream
    return x, pl.residual_device().cpu().numpy().copy()


def gamma_interval(dxb, x1b, D_lo, D_hi, d_split):
    """Per right-hand side the interval [lo, hi] of step sizes gamma that every coordinate of dx admits.

    The least-squares fit of dx on D is off by up to 2^-8 gamma with the bf16 direction (D' = D (1 + e_j),
    |e_j| <= 2^-8), which is all the bf16 rounding the elementwise check allows and far more than the
    line-search identity B can take on coordinates that cross zero.  The interval uses what is known about
    D' instead.  The device's D_dev,j lies in [D_lo,j, D_hi,j], the shrink at g_j +- allow_j (the shrink is
    monotone in g; where it is flat -- a coordinate surely shrunk to zero, D_dev = -x_t exactly -- the two
    coincide), and the operand image is monotone, so D'_j lies in [img(D_lo,j), img(D_hi,j)]: img = bf16 (round to
    nearest even is monotone) or, for the hi + lo pair, v -+ 1.01 2^-16 |v| (|v - hi - lo| <= 2^-16 |v|).
    Where both ends have one sign, dx_j = gamma D'_j - rho_j, |rho_j| <= u |x_t+1,j|, confines gamma to
        [(dx_j - u |x_t+1,j|) / D'_far, (dx_j + u |x_t+1,j|) / D'_near]        (for D' > 0; mirrored below 0).
    A coordinate whose [D_lo, D_hi] holds no bf16 rounding boundary pins gamma to ~u |x_t+1,j| / |dx_j|.
    The intersection over j, and with [0, 1], is returned; lo > hi means that no step size explains dx
    (reported under C)."""
    if d_split == 1:
        lo_i, hi_i = bf16(D_lo), bf16(D_hi)
    else:
        lo_i, hi_i = D_lo - 1.01 * 2.0 ** -16 * np.abs(D_lo), D_hi + 1.01 * 2.0 ** -16 * np.abs(D_hi)
    neg = hi_i < 0
    # not below 2^-100: a coordinate that the hi + lo direction shrinks to zero keeps 2^-16 of itself each
    # time and ends among the fp32 / bf16 subnormals, where the relative roundings above do not hold
    use = (lo_i > 2.0 ** -100) | (hi_i < -2.0 ** -100)
    # mirror the negative coordinates, so that 0 < near <= D' <= far
    near = np.where(neg, -hi_i, lo_i)
    far = np.where(neg, -lo_i, hi_i)
    num = np.where(neg, -dxb, dxb)
    e = U24 * np.abs(x1b) + 2.0 ** -149
    nl, nh = num - e, num + e
    with np.errstate(divide="ignore", invalid="ignore"):
        g_lo = np.where(use, np.where(nl >= 0, nl / far, nl / near), -np.inf)
        g_hi = np.where(use, np.where(nh >= 0, nh / near, nh / far), np.inf)
    return np.maximum(g_lo.max(axis=0), 0.0), np.minimum(g_hi.min(axis=0), 1.0)


def check_step(Ab, diag, mu, W, block, snap_t, snap_t1, err_t, d_split, exact_iter, dR_prev, chain=None, q=0,
               R_ref=None, stats=None):
    """Violations (a list of strings, empty = the step is the algorithm's) of A-D in the module docstring
    for the iteration on feature block ``block`` between ``snap_t`` and ``snap_t1`` (``snapshot``), every
    right-hand side.  ``Ab`` (m, n) fp64 the stored bf16 A; ``diag`` (Block, w[, 1]) the context's
    diag_ATA; ``mu`` (k,); ``W`` (m, k) mask or None; ``err_t`` the iteration's error record (None: D is
    skipped); ``exact_iter``: g is the exact product this iteration, else carried, ``q`` iterations after
    the refresh whose residual is ``R_ref`` (k, m), and ``dR_prev`` = R_t - R_{t-1} (k, m); ``chain``: terms
    in one fp32 accumulation chain of pass 2 (default: the whole block, both direction pieces).  ``stats``:
    a dict that receives the worst ratio to bound of each check ("A", "B", "C", "D"; max-merged)."""
    (x0, R0), (x1, R1) = snap_t, snap_t1
    diag = np.asarray(diag, dtype=np.float64)
    nblock = diag.shape[0]
    d = diag.reshape(nblock, -1)[block][:, None]                      # (w, 1)
    n, k = x0.shape
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
        worst[key] = max(worst[key], float(np.max(r))) if r.size else worst[key]
        return r

    def report(tag, bad, r, rhs_axis):
        """one line per check: the right-hand sides that violate it and the worst ratio to bound"""
        if np.any(bad):
            cols = np.flatnonzero(bad if bad.ndim == 1 else bad.any(axis=1 - rhs_axis))
            out.append(f"{tag}: rhs {cols[:8].tolist()}{'...' if cols.size > 8 else ''}, "
                       f"worst ratio {float(np.max(np.where(bad, r, 0.0))):.3g}")

    # ---- A ------------------------------------------------------------------------------------
    other = np.ones(n, dtype=bool)
    other[sl] = False
    if not np.array_equal(x0[other], x1[other]):
        out.append("A: x changed outside the iteration's block")
    if np.any(dR[~Wk] != 0.0):
        out.append(f"A: dR != 0 on {int(np.count_nonzero(dR[~Wk]))} held-out rows")
    pred = np.where(Wk, (Am @ dxb).T, 0.0)
    sx_b = (absA @ (np.abs(x0b) + np.abs(x1b))).T
    sx_all = (np.abs(Ab) @ (np.abs(x0) + np.abs(x1))).T if nblock > 1 else sx_b
    bound_a = U24 * sx_b + L * U24 * (absA @ np.abs(dxb)).T \
        + (nblock + 2) * 2.0 ** -53 * (np.abs(R0) + np.abs(R1) + 2.0 * sx_all)
    dev_a = np.where(Wk, np.abs(dR - pred), 0.0)
    r = ratio("A", dev_a, bound_a)
    report("A: dR != w o (A dx)", dev_a > bound_a, r, 0)
    still = ~dxb.any(axis=0)

    # ---- C: the direction ------------------------------------------------------------------------
    g = Am.T @ R0.T                                                    # (w, k); R is 0 on held-out rows
    D = soft_thr(d * x0b - g, mu) / d - x0b
    sigma = lambda R: 2.0 ** -17 * np.sqrt(A2.T @ np.square(R).T)      # noqa: E731
    if exact_iter:
        allow = C_G * sigma(R0)
    else:
        allow = C_G * (2.0 ** -9 * np.sqrt(A2.T @ np.square(dR_prev).T) + q * U24 * np.abs(g)
                       + (sigma(R_ref) if R_ref is not None else 0.0))
    u_D = 2.0 ** -8 if d_split == 1 else 2.0 ** -16
    D_lo, D_hi = soft_thr(d * x0b - (g + allow), mu) / d - x0b, soft_thr(d * x0b - (g - allow), mu) / d - x0b
    # no direction at all (D' = 0 whatever the gradient noise: S = 0, R + gamma 0 = R): dR == 0 exactly.  A
    # dx == 0 alone does not give that: near convergence every gamma D'_j may fall below half an ulp of the
    # fp32 x_j while R, in fp64, still moves -- check A's first term is there for this
    none = ~(D_lo.any(axis=0) | D_hi.any(axis=0))
    if np.any(dxb[:, none] != 0.0) or np.any(dR[none] != 0.0):
        moved = np.flatnonzero(none & (dR.any(axis=1) | ~still))
        out.append(f"B: no direction but the state moved, rhs {moved[:8].tolist()}")
    g_lo, g_hi = gamma_interval(dxb, x1b, D_lo, D_hi, d_split)
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
    zero = (x0b == 0.0) & (np.abs(g) <= mu - allow)
    if np.any(x1b[zero] != 0.0):
        out.append(f"C: {int(np.count_nonzero(x1b[zero]))} coordinates with x_t = 0 and |g| <= mu - allow moved")

    # ---- B: the line search ---------------------------------------------------------------------
    l1_0, l1_1 = np.abs(x0b).sum(axis=0), np.abs(x1b).sum(axis=0)
    dRdR, RdR = np.einsum("km,km->k", dR, dR), np.einsum("km,km->k", R0, dR)

    def F(gam):
        return dRdR + RdR + mu * (np.abs(gam * x0b + dxb).sum(axis=0) - gam * l1_0)

    flip = (x0b != 0.0) & ((((gh - dgh) * x0b + dxb) * x0b <= 0.0) | (((gh + dgh) * x0b + dxb) * x0b <= 0.0))
    bound_b = 2.0 ** -22 * mu * (l1_0 + l1_1) + 1e-12 * (dRdR + np.abs(RdR)) \
        + 2.0 * mu * dgh * np.where(flip, np.abs(x0b), 0.0).sum(axis=0)
    # gamma surely below 1: F = 0; surely 1 (clipped): F(1) <= 0; undecided within the interval: F <= 0 either way
    Fh = F(gh)
    dev_b = np.where(g_hi < 1.0 - 1e-6, np.abs(Fh), np.where(g_lo >= 1.0 - 1e-6, np.maximum(F(np.ones(k)), 0.0),
                                                            np.maximum(Fh, 0.0)))
    dev_b = np.where(still, 0.0, dev_b)
    r = ratio("B", dev_b, bound_b)
    report("B: not an exact line search", dev_b > bound_b, r, 0)

    # ---- D: the error record --------------------------------------------------------------------
    if err_t is not None:
        err_ref = float(np.max(np.abs(g - np.clip(g - x0b, -mu, mu))))
        tol = float(np.max(allow))
        dev_d = abs(float(err_t) - err_ref)
        worst["D"] = max(worst["D"], dev_d / tol if tol > 0 else (np.inf if dev_d > 0 else 0.0))
        if not dev_d <= tol:
            out.append(f"D: err {float(err_t):.17g} against {err_ref:.17g}, allowance {tol:.3g}")
    if stats is not None:
        for key, v in worst.items():
            stats[key] = max(stats.get(key, 0.0), v)
        stats["gamma_min"] = min(stats.get("gamma_min", np.inf), float(gh.min()))
        stats["gamma_max"] = max(stats.get("gamma_max", -np.inf), float(gh.max()))
        stats["dgamma"] = max(stats.get("dgamma", 0.0), float(dgh.max()))
    return out

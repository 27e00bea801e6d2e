"""Per-iteration checks of the fp64 solver (csrc/bpgl_kernels.h, bpgl_onepass.h) from two snapshots of its state.

``check_step`` looks at (x_t, r_t) and (x_{t+1}, r_{t+1}) of ONE iteration (``solver_x`` and the residual
buffer of ``bpgl_solver_residual``), at the step size gamma that ``bpgl_solver_status`` reports and at the
iteration's error record, and decides in numpy fp64 on A as the device stores it whether the step between the
snapshots is the algorithm's step: ``oracle.run_numpy``'s loop, lasso.py:105-155.  It emulates nothing.  Every
device sum is fp64, so every bound below is an a-priori fp64 bound: u = 2^-53, gam(k) = k u / (1 - k u) (a
k-term sum or dot product in any order, fused or not), each rounding counted, none fitted.  The reference
products are numpy fp64 too, so each bound that holds a reference product counts that product's own
summation as well ("+ ref").

Notation: block mb of w columns, A = A_mb (m rows), d = the context's diag on the block, dx = x_{t+1} - x_t
on the block, dr = r_{t+1} - r_t, D the device's direction (never observable), s23 = A D as the device summed
it (never observable), |A| the matrix of absolute values.  The device's iteration is
    g (exact: A^T r_t; carried: G += gamma U, U = A^T s23);  D = S(d o x_t - g, mu) / d - x_t;  s23 = A D;
    gamma = clip(-(r_t.s23 + mu (|x_t + D|_1 - |x_t|_1)) / s23.s23, 0, 1);  err_t;  the stop rule;
    x += gamma D;  Ax_mb += gamma s23;  r = sum_q Ax_q - b.

0.  After the reset: x_0 is bitwise the start given; r_0 = A x_0 - b with
        |r_0,i - (A x_0 - b)_i| <= (gam(n + 1) + ref gam(n + 1)) (sum_j |a_ij| |x_0,j| + |b_i|)
    (Block products of w terms, Block - 1 additions, one subtraction).  Every step leaves the other blocks'
    x bitwise unchanged.

A.  dr = A dx.  gamma D_j = dx_j + rho_j with |rho_j| <= u |x_{t+1,j}| (x += gamma D is one fused operation
    on the device, stored once).  s23 is a w-term dot product in ``parts`` partials (segment blocks or
    segments) folded in a fixed order, any order: gam(w); the hand-off's parity bit moves each partial by <= 1
    ulp (the issue counts one per partial: + parts; the partials cover disjoint columns, so 2 would do);
    Ax += gamma s23, fused, is counted under rr; the host's dx = x_{t+1} - x_t and one spare: + 2.
        |dr_i - a_i.dx| <= (gam(w + parts + 2) + ref gam(w)) sum_j |a_ij| |dx_j|
                           + u sum_j |a_ij| |x_{t+1,j}|                               (a_i.rho)
                           + rr_i                                                     (the fp64 updates)
    rr_i, one block: Ax' = fl(Ax + gamma s23) and r = fl(Ax - b) at t and at t + 1 are three roundings,
    u (|r_t,i| + |r_{t+1},i| + |Ax'_i|) with |Ax'_i| <= |r_{t+1},i| + |b_i|; rr_i = gam(4) (|r_t,i| + |r_{t+1},i| + |b_i|).
    Several blocks: r = fl(sum_q Ax_q - b) is Block roundings of partial sums <= sum_q |Ax_q,i| + |b_i| at t and
    at t + 1, and the update of Ax_mb one more; |Ax_q,i| <= sum_{j in q} |a_ij| |x_j| to first order, so
    rr_i = gam(Block + 3) (|b_i| + sum_j |a_ij| (|x_t,j| + |x_{t+1},j|)), j over all of x.  (The issue states the
    one-block form only -- a block's Ax_q is not bounded by |r| + |b| -- the several-block form is this module's.)
    alpha_i names the device's part of the bound (everything but "ref").

C.  The direction: dx_j = gamma D_j - rho_j, D = S(d o x_t - g, mu) / d - x_t, g = A^T r_t.  The shrink is
    1-Lipschitz in g, so |D_dev,j - D_j| <= allow_j / d_j + the shrink's own fp64 arithmetic: rx = d x - g
    (u |d x| + u |rx|), the soft threshold (u), bx = (1 / d) st (2 u), D = bx - x (u):
        eps_j = gam(5) (|x_t,j| + |g_j| / d_j + |Bx_j|)                     (device; once more for the reference)
    The issue's statement has allow_j / d_j alone; the correct model of tests/test_solver_step_host.py exceeds
    it at 3 x 5 (ratio 1.05: with m = 3, gam(m) sum_i |a_ij| |r_i| is no larger than these roundings), so eps_j
    is counted.  The gradient allowance:
      exact iteration (two-pass, several blocks, the reset, a refresh): an m-term dot product in chunks, summed
        over ``nranks`` row shards (the per-rank fold): allow_j = gam(m + nranks - 1) sum_i |a_ij| |r_t,i|.
      carried iteration, after the refresh at t0: G_{s+1} = fl(G_s + gamma_s U_s), U_s = A^T s23_s in ``ngroups``
        row-group (and rank) partials.  Start from the refresh's own allowance; per carried iteration s add
            gamma_s (gam(m + ngroups) sum_i |a_ij| |s23_s,i| + sum_i |a_ij| ds_s,i)
              = gam(m + ngroups) sum_i |a_ij| |dr_s,i| + sum_i |a_ij| alpha_s,i        (s23 = dr / gamma, ds = alpha / gamma)
            + sum_i |a_ij| u (|r_s,i| + |r_{s+1},i|)      (the roundings of r, which the recurrence never sees)
        and one rounding u |g_j| of the stored G.  ``hist`` carries the sum from one call to the next.  (The
        recurrence multiplies the device's own s23, the one in dr, so of alpha only rr is strictly needed; the
        issue's wider term is kept as stated.)
    With the reference's g (+ ref gam(m) sum_i |a_ij| |r_t,i|) and eD_j = (allow_j + ref) / d_j + 2 eps_j:
        |dx_j - gamma D_j| <= gamma eD_j + u |x_{t+1,j}| + u gamma |D_j| + u |dx_j|
    (x's one rounding; the host's gamma D_j and dx_j).  Coordinates with x_t,j = 0 and |g_j| <= mu - allow_j - ref
    shrink to D = 0 on the device too (rx = -g exactly) and must be exactly 0 in x_{t+1}.

B.  The line search.  Times gamma, with gamma s23 = dr + a, |a_i| <= alpha_i (A's bound) and gamma D = dx + rho:
        F(gamma) = |dr|^2 + r_t.dr + mu (|gamma x_t + dx|_1 - gamma |x_t|_1)
    is 0 when 0 < gamma < 1 and <= 0 at gamma = 1, up to
        sum_i (2 |dr_i| + |r_t,i| + alpha_i) alpha_i + mu u sum_j (|x_{t+1,j}| + 4 |dx_j|)       (a, rho, fl(bx - x))
        + (gam(m + 8) + ref) (sum_i (|dr_i| + alpha_i)^2 + sum_i |r_t,i| (|dr_i| + alpha_i))     (the two dot products,
        + (gam(w + 8) + ref) mu (|gamma x_t + dx|_1 + gamma |x_t|_1)                              the two l1 sums,
    the division and mu (a - b) among the + 8).  gamma outside [0, 1] is a violation.  gamma = 0: dx == 0 and
    dr == 0 exactly, and the reference's own r1 = g.D + mu (|x_t + D|_1 - |x_t|_1) is >= 0 up to
    sum_j (|g_j| + mu) eD_j and its fp64 sums.  gamma > 0 with dr == 0 everywhere: s23.s23 == 0 gives gamma = 0.

D.  err_t = max_j |g_j - clip(g_j - x_t,j, -mu, mu)| over the w real columns of the block, 1-Lipschitz in g_j:
    within max_j (allow_j + ref) of the reference's.  status["err"] is bitwise the last record and
    status["gamma"] the gamma of A-C (the tests assert the first; the second is how gamma gets here).

E.  ``stop_bound`` picks an err_bound from the fp64 reference's err trace: the reference stops at an iteration in
    [10, 17] and no err up to there lies within a factor 1 +- 1e-3 of the bound (the device's record is within
    D of the reference's, orders below that margin, so it stops at the same iteration).
"""
import numpy as np

U = 2.0 ** -53
T_STEPS = 18
REFRESH = 8
TAGS = ("0", "A", "B", "C", "D")


def gam(k):
    return k * U / (1.0 - k * U)


def soft_thr(t, tau):
    return np.sign(t) * np.maximum(np.abs(t) - tau, 0.0)


def stored(A, type_name):
    """A as the device stores it, as fp64 (tests/test_gpu.py::stored, with numpy's bf16 rounding)."""
    if type_name == "double":
        return np.asarray(A, dtype=np.float64)
    f = np.asarray(A, dtype=np.float32)
    if type_name == "float":
        return f.astype(np.float64)
    b = f.view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


def instance(m, n, type_name, seed, mu_scale=0.1, common=0.0):
    """tests/test_onepass.py's recipe: randn / sqrt(n), 30 % support, mu = 0.1 |A^T b|_inf; A as stored.
    ``common``: every column also holds this multiple of one shared randn column (see COMMON)."""
    rs = np.random.RandomState(seed)
    A = rs.randn(m, n)
    if common:
        A = A + common * rs.randn(m, 1)
    As = stored(A / np.sqrt(n), type_name)
    b = As @ np.where(rs.rand(n) < 0.3, rs.randn(n), 0.0) + 0.01 * rs.randn(m)
    mu = mu_scale * float(np.abs(As.T @ b).max())
    return As, b, mu


def onepass_geometry(m, w, type_name, cus):
    """(SB, ngroups, R, GPL) as geometry() in csrc/bpgl.hip has them for one feature block."""
    V, bc = {"float": (4, 4096), "double": (2, 2048), "bf16": (8, 6144)}[type_name]
    wp = -(-w // V) * V
    SB = -(-wp // bc)
    ng = max(1, min(cus // SB, m, 256))
    R = -(-m // ng)
    return SB, -(-m // R), R, (2 if SB > 64 else 1)


def reference_run(As, b, mu, Block, iters, order=None, x0=None, diag=None):
    """``oracle.run_numpy``'s loop with every iterate kept: (snaps[0..iters], gammas, errs)."""
    m, n = As.shape
    w = n // Block
    dg = (np.square(As).sum(axis=0) if diag is None else np.asarray(diag, dtype=np.float64)).reshape(Block, w)
    x = np.zeros((Block, w)) if x0 is None else np.array(x0, dtype=np.float64).reshape(Block, w)
    Ax = np.stack([As[:, q * w:(q + 1) * w] @ x[q] for q in range(Block)])
    snaps, gammas, errs = [(x.reshape(-1).copy(), Ax.sum(axis=0) - b)], [], []
    for t in range(iters):
        mb = int(order[t]) if order is not None else t % Block
        Am = As[:, mb * w:(mb + 1) * w]
        r = Ax.sum(axis=0) - b
        g = Am.T @ r
        Bx = soft_thr(dg[mb] * x[mb] - g, mu) / dg[mb]
        D = Bx - x[mb]
        s23 = Am @ D
        r1 = r @ s23 + mu * (np.abs(Bx).sum() - np.abs(x[mb]).sum())
        r2 = s23 @ s23
        gamma = 0.0 if r2 == 0 else float(np.clip(-r1 / r2, 0, 1))
        errs.append(float(np.max(np.abs(g - np.clip(g - x[mb], -mu, mu)))))
        gammas.append(gamma)
        x[mb] += gamma * D
        Ax[mb] += gamma * s23
        snaps.append((x.reshape(-1).copy(), Ax.sum(axis=0) - b))
    return snaps, gammas, errs


def stop_rule(err, bound, Block, order=None):
    """The iteration at which lasso.py:141-150 stops on the trace ``err`` (None: it does not)."""
    cnt = 0
    for t, e in enumerate(err):
        mb = int(order[t]) if order is not None else t % Block
        cnt += e < bound
        if mb == Block - 1:
            if cnt == Block:
                return t
            cnt = 0
    return None


def stop_bound(ref_err, Block=1, order=None):
    """An err_bound at which the reference trace stops at an iteration in [10, 17] with no err up to there
    within a factor 1 +- 1e-3 of it (E): the midpoint, in the geometric sense, of two neighbouring values of
    the trace, the pair with the widest gap among those that qualify.  None when no bound qualifies."""
    ref_err = np.asarray(ref_err, dtype=np.float64)
    vals = np.unique(ref_err[ref_err > 0])
    best = None
    for lo, hi in zip(vals[:-1], vals[1:]):
        bound = float(np.sqrt(lo * hi))
        T = stop_rule(ref_err, bound, Block, order)
        if T is None or not 10 <= T <= 17:
            continue
        ratio = ref_err[:T + 1] / bound
        if np.any((ratio > 1.0 - 1e-3) & (ratio < 1.0 + 1e-3)):
            continue
        if best is None or hi / lo > best[1]:
            best = (bound, hi / lo, T)
    return None if best is None else (best[0], best[2])


def check_reset(As, b, x0, snap0, Block=1, stats=None):
    """Violations of check 0 for the snapshot after the reset; ``x0`` None: the start is 0."""
    x, r = snap0
    n = As.shape[1]
    x0 = np.zeros(n) if x0 is None else np.asarray(x0, dtype=np.float64).reshape(-1)
    out = []
    if x.tobytes() != x0.tobytes():
        out.append("0: x_0 is not bitwise the start given")
    dev = np.abs(r - (As @ x0 - b))
    bound = 2.0 * gam(n + 1) * (np.abs(As) @ np.abs(x0) + np.abs(b))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, dev / bound, np.where(dev > 0, np.inf, 0.0))
    if stats is not None:
        stats["0"] = max(stats.get("0", 0.0), float(ratio.max()))
    if np.any(dev > bound):
        out.append(f"0: r_0 != A x_0 - b on {int(np.count_nonzero(dev > bound))} rows, worst ratio {ratio.max():.3g}")
    return out


def check_step(As, diag, mu, Block, mb, snap_t, snap_t1, gamma, err, exact, hist, b=None, parts=1, ngroups=1,
               nranks=1, stopped=False, stats=None):
    """Violations (a list of strings, each starting with its check's letter; empty = the step is the
    algorithm's) of A-D in the module docstring for the iteration on block ``mb`` between ``snap_t`` and
    ``snap_t1`` (pairs (x (n,), r (m,)) of fp64 arrays).  ``As`` (m, n) fp64: A as stored; ``diag`` the
    context's diag_ATA (Block, w[, 1]); ``gamma``: the step size that the status call reports; ``err``: the
    iteration's error record (None: D is skipped); ``exact``: g is the exact product this iteration, else
    carried since the last exact one; ``hist``: a dict, one per run, in which the checker keeps the carried
    allowance and |A| (the iterations of a run must be checked in order); ``b`` the right-hand side;
    ``parts``: partials of one s23 dot product (segment blocks, or the two-pass segments); ``ngroups``: U
    partials of one carried update (row groups, over all ranks, plus the ranks); ``nranks``: row shards.
    ``stopped``: the stop rule fired in this iteration (E): the record is checked (D), the state must not have
    moved and the status reports gamma = 0.  ``stats`` receives the worst ratio to bound of each check
    (max-merged) and, under "steps", one
    (gamma, max_j allow_j / d_j, max_j |D_j|) per call."""
    (x0, r0), (x1, r1) = snap_t, snap_t1
    m, n = As.shape
    w = n // Block
    sl = slice(mb * w, (mb + 1) * w)
    d = np.asarray(diag, dtype=np.float64).reshape(Block, -1)[mb]
    Am = As[:, sl]
    cache = hist.setdefault("absA", {})
    if mb not in cache:
        cache[mb] = np.abs(Am)
    absA = cache[mb]
    if Block > 1 and "all" not in cache:
        cache["all"] = np.abs(As)
    babs = np.abs(np.asarray(b, dtype=np.float64).reshape(-1))
    gamma = float(gamma)
    x0b, x1b = x0[sl], x1[sl]
    dx, dr = x1b - x0b, r1 - r0
    out = []
    worst = dict(A=0.0, B=0.0, C=0.0, D=0.0)

    def ratio(key, val, bound):
        val, bound = np.atleast_1d(val), np.atleast_1d(bound)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound > 0, val / bound, np.where(val > 0, np.inf, 0.0))
        r = np.where(np.isnan(r), np.inf, r)
        worst[key] = max(worst[key], float(r.max()))
        return r

    # ---- other blocks --------------------------------------------------------------------------
    other = np.ones(n, dtype=bool)
    other[sl] = False
    if x0[other].tobytes() != x1[other].tobytes():
        out.append("0: x changed outside the iteration's block")
    if not 0.0 <= gamma <= 1.0:
        out.append(f"B: gamma = {gamma!r} outside [0, 1]")
    if stopped and (gamma != 0.0 or x0.tobytes() != x1.tobytes() or r0.tobytes() != r1.tobytes()):
        out.append("E: the stop iteration moved the state or reports gamma != 0")

    # ---- A -------------------------------------------------------------------------------------
    if Block == 1:
        rr = gam(4) * (np.abs(r0) + np.abs(r1) + babs)
    else:
        rr = gam(Block + 3) * (babs + cache["all"] @ (np.abs(x0) + np.abs(x1)))
    alpha_dev = gam(w + parts + 2) * (absA @ np.abs(dx)) + U * (absA @ np.abs(x1b)) + rr
    alpha = alpha_dev + gam(w) * (absA @ np.abs(dx))
    dev_a = np.abs(dr - Am @ dx)
    ra = ratio("A", dev_a, alpha)
    if np.any(dev_a > alpha):
        rows = np.flatnonzero(dev_a > alpha)
        out.append(f"A: dr != A dx on {rows.size} rows {rows[:6].tolist()}, worst ratio {ra.max():.3g}")

    # ---- C: the direction ----------------------------------------------------------------------
    g = Am.T @ r0
    ag = absA.T @ np.abs(r0)
    allow_ref = gam(m) * ag
    if exact or "carry" not in hist:
        allow = gam(m + nranks - 1) * ag
    else:
        allow = hist["carry"] + U * np.abs(g)
    Bx = soft_thr(d * x0b - g, mu) / d
    D = Bx - x0b
    eps = gam(5) * (np.abs(x0b) + np.abs(g) / d + np.abs(Bx))
    eD = (allow + allow_ref) / d + 2.0 * eps
    bound_c = gamma * eD + U * np.abs(x1b) + U * gamma * np.abs(D) + U * np.abs(dx)
    dev_c = np.abs(dx - gamma * D)
    rc = ratio("C", dev_c, bound_c)
    if np.any(dev_c > bound_c):
        cols = np.flatnonzero(dev_c > bound_c)
        out.append(f"C: dx != gamma D on {cols.size} columns {cols[:6].tolist()}, worst ratio {rc.max():.3g}")
    zero = (x0b == 0.0) & (np.abs(g) <= mu - allow - allow_ref)
    if np.any(x1b[zero] != 0.0):
        out.append(f"C: {int(np.count_nonzero(x1b[zero]))} coordinates with x_t = 0 and |g| <= mu - allow moved")
    # the allowance that the next iteration starts from, should it be carried
    hist["carry"] = allow + gam(m + ngroups) * (absA.T @ np.abs(dr)) \
        + absA.T @ (alpha_dev + U * (np.abs(r0) + np.abs(r1)))

    # ---- B: the line search --------------------------------------------------------------------
    l1_0 = np.abs(x0b).sum()
    if stopped:
        pass
    elif gamma == 0.0:
        if dx.any() or dr.any():
            out.append("B: gamma = 0 but the state moved")
        r1_ref = g @ D + mu * (np.abs(Bx).sum() - l1_0)
        tol = ((np.abs(g) + mu) * eD).sum() + gam(w + 4) * (np.abs(g) @ np.abs(D) + mu * (np.abs(Bx).sum() + l1_0))
        rb = ratio("B", max(-r1_ref, 0.0), tol)
        if -r1_ref > tol:
            out.append(f"B: gamma = 0 where the reference's r1 = {r1_ref:.6g} < 0, ratio {rb.max():.3g}")
    elif 0.0 < gamma <= 1.0:
        if not dr.any():
            out.append("B: gamma > 0 with dr == 0 everywhere (s23.s23 == 0 gives gamma = 0)")
        l1_g = np.abs(gamma * x0b + dx).sum()
        F = dr @ dr + r0 @ dr + mu * (l1_g - gamma * l1_0)
        da = np.abs(dr) + alpha
        bound_b = ((2.0 * np.abs(dr) + np.abs(r0) + alpha) * alpha).sum() \
            + mu * U * (np.abs(x1b).sum() + 4.0 * np.abs(dx).sum()) \
            + 2.0 * gam(m + 8) * (da @ da + np.abs(r0) @ da) + 2.0 * gam(w + 8) * mu * (l1_g + gamma * l1_0)
        dev_b = abs(F) if gamma < 1.0 else max(F, 0.0)
        rb = ratio("B", dev_b, bound_b)
        if dev_b > bound_b:
            out.append(f"B: not an exact line search, F({gamma:.9g}) = {F:.6g}, ratio {rb.max():.3g}")

    # ---- D: the error record -------------------------------------------------------------------
    if err is not None:
        err_ref = float(np.max(np.abs(g - np.clip(g - x0b, -mu, mu))))
        tol = float(np.max(allow + allow_ref))
        dev_d = abs(float(err) - err_ref)
        rd = ratio("D", dev_d if np.isfinite(dev_d) else np.inf, tol)
        if not dev_d <= tol:
            out.append(f"D: err {float(err):.17g} against {err_ref:.17g}, allowance {tol:.3g}, ratio {rd.max():.3g}")

    if stats is not None:
        for key, v in worst.items():
            stats[key] = max(stats.get(key, 0.0), v)
        stats.setdefault("steps", []).append((gamma, float(np.max(allow / d)), float(np.max(np.abs(D)))))
    return out


def check_run(As, b, diag, mu, Block, snaps, gammas, errs, carried, order=None, x0=None, refresh=REFRESH, parts=1,
              ngroups=1, nranks=1, exact_from=None, t_stop=None, stats=None):
    """Checks 0 and A-D over a whole run: ``snaps[0]`` after the reset, ``snaps[t + 1]``, ``gammas[t]`` and
    ``errs[t]`` after iteration t.  ``carried``: g is carried between refreshes every ``refresh`` iterations
    (one-pass), else exact throughout; ``exact_from``: the first iteration from which it is exact again (a
    fallback to the two-pass kernels); ``t_stop``: the iteration at which the stop rule fired (its record is
    checked; every later snapshot must equal ``snaps[t_stop]`` bitwise).  Returns [(t, violation)], t = -1 for the reset."""
    stats = {} if stats is None else stats
    bad = [(-1, v) for v in check_reset(As, b, x0, snaps[0], Block, stats)]
    hist = {}
    for t in range(len(snaps) - 1):
        mb = int(order[t]) if order is not None else t % Block
        if t_stop is not None and t > t_stop:
            if any(u.tobytes() != v.tobytes() for u, v in zip(snaps[t + 1], snaps[t_stop])):
                bad.append((t, "E: the state moved after the stop"))
            continue
        exact = (not carried) or t % refresh == 0 or (exact_from is not None and t >= exact_from)
        bad += [(t, v) for v in check_step(As, diag, mu, Block, mb, snaps[t], snaps[t + 1], gammas[t], errs[t], exact,
                                           hist, b=b, parts=parts, ngroups=ngroups, nranks=nranks,
                                           stopped=t == t_stop, stats=stats)]
    return bad


def informative(stats, need=12):
    """test_steps_are_informative's condition on the ``stats["steps"]`` of a reference run: at least ``need``
    steps with gamma > 0 whose gradient allowance, as a direction, is <= 1e-6 of the largest |D_j|."""
    return sum(1 for ga, a, dmax in stats["steps"] if ga > 0.0 and a <= 1e-6 * dmax) >= need


def line(stats):
    return " ".join(f"{c} {stats.get(c, 0.0):.3g}" for c in TAGS)


# --------------------------------------------------------------------------------------------------
# The cases of tests/test_solver_step.py (the MI355X run).  They live here so that
# tests/test_solver_step_host.py can hold every one of them to test_steps_are_informative and to E's
# conditions without a GPU.  ``seed`` is m + n unless SEEDS says otherwise.
# --------------------------------------------------------------------------------------------------
def case(m, n, ty, Block=1, knobs=(), order_seed=None, x0_seed=None, fail_at=None, world=1, stop=False, target=None):
    """``target``: BPGL_TARGET_BLOCKS while the context is created (None: the default tiling)"""
    return dict(m=m, n=n, ty=ty, Block=Block, knobs=tuple(knobs), order_seed=order_seed, x0_seed=x0_seed,
                fail_at=fail_at, world=world, stop=stop, target=target)


def case_id(c):
    s = f"{c['m']}x{c['n']}-{c['ty']}"
    s += f"-B{c['Block']}" if c["Block"] > 1 else ""
    s += "".join(f"-{k}={v}" for k, v in c["knobs"])
    s += "-order" if c["order_seed"] is not None else ""
    s += "-x0" if c["x0_seed"] is not None else ""
    s += f"-fail{c['fail_at']}" if c["fail_at"] is not None else ""
    s += f"-world{c['world']}" if c["world"] > 1 else ""
    s += f"-target{c['target']}" if c.get("target") is not None else ""
    return s + ("-stop" if c["stop"] else "")


SEEDS = {}
# Shapes whose columns share a common component.  With 131139 rows for 32 independent columns A^T A is the
# identity to 1 / sqrt(m / n): the block iteration converges by a factor ~60 per step, D reaches the rounding
# floor after 6 steps and the rest of the run is not informative.  One shared column of the same size couples
# the blocks (condition number ~ n) and all 18 steps stay informative.
COMMON = {(131139, 32, "float"): 1.0}
LDS =[(3, 5, "float"), (4099, 1536, "float"), (2000, 1000, "double"), (1500, 6000, "bf16")]
GRANULE = [(1000, 4100, "float"), (37, 9000, "float"), (777, 3000, "double"), (1500, 10000, "bf16")]
TAILW = [(300, 30000, "float")]
GPL2 = [(96, 266340, "float"), (64, 133126, "double"), (64, 399368, "bf16")]
TWO_PASS = [(77, 120, 3), (129, 1002, 2), (4099, 1536, 3)]

ONEPASS_CASES = (
    [case(*s, knobs=[("onepass_sb1", v)]) for s in LDS for v in (-1, 0)]
    + [case(*s, knobs=[("onepass_rows", v)]) for s in GRANULE + TAILW for v in (0, 1)]
    + [case(*s) for s in GPL2]
    + [case(1000, 4100, "float", knobs=[("tail_row_blocks", 0)]),
       case(777, 3000, "double", knobs=[("onepass_cache_permille", 0)]),
       case(777, 3000, "double", knobs=[("onepass_cache_permille", 1000)]),
       case(1500, 10000, "bf16", x0_seed=3)])
TWO_PASS_CASES = (
    [case(m, n, ty, Block=B) for (m, n, B) in TWO_PASS for ty in ("float", "double", "bf16")]
    + [case(77, 120, "float", Block=3, order_seed=1), case(1000, 4100, "float", knobs=[("onepass", 0)])])
FALLBACK_CASES = [case(1000, 4100, "float", fail_at=5)]
ROW_SHARD_CASES = [case(1000, 4100, "float", world=2), case(700, 9000, "bf16", world=3)]
STOP_CASES = [case(2000, 1000, "double", stop=True), case(1000, 4100, "float", stop=True),
              case(96, 266340, "float", stop=True), case(77, 120, "float", Block=3, stop=True),
              case(1000, 4100, "float", world=2, stop=True)]
ALL_CASES = ONEPASS_CASES + TWO_PASS_CASES + FALLBACK_CASES + ROW_SHARD_CASES + STOP_CASES


def case_problem(c):
    """(As, b, mu, order, x0) of a case: the instance, the block order (None: cyclic) and the start."""
    m, n, ty = c["m"], c["n"], c["ty"]
    As, b, mu = instance(m, n, ty, SEEDS.get((m, n, ty), m + n), common=COMMON.get((m, n, ty), 0.0))
    order = None if c["order_seed"] is None else np.random.RandomState(c["order_seed"]).randint(
        0, c["Block"], size=T_STEPS).astype(np.int32)
    x0 = None if c["x0_seed"] is None else np.random.RandomState(c["x0_seed"]).randn(n)
    return As, b, mu, order, x0


def case_carried(c):
    """Does the case run the one-pass iteration (g carried between refreshes)?"""
    return c["Block"] == 1 and ("onepass", 0) not in c["knobs"]

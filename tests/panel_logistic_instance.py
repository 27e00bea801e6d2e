"""Planted logistic instances for tests/test_panel_logistic_host.py, tests/test_panel_logistic.py and
tests/test_panel_logistic_edges.py, a reference solver written for the tests alone, and the edge
instances with the assertions the edge tests and their mutants share.  No GPU."""
import numpy as np
import torch

from convex_optimization_amd import cpu_calculation as C


def bf16(A):
    """A rounded to bf16, as fp64: the matrix the device's problems are defined by."""
    return torch.from_numpy(np.ascontiguousarray(A)).to(torch.bfloat16).to(torch.float64).numpy()


def instance(m, n, seed=0, nz=10, zeros=30, beta=0.3):
    """(A bf16-rounded fp64 (m, n) with unit rows, y (m,) 0/1 drawn from a planted sparse model with intercept ``beta``,
    omega (m,) in (0, 1) with ``zeros`` exact zeros)."""
    rs = np.random.RandomState(seed)
    A = rs.randn(m, n)
    A = bf16(A / np.linalg.norm(A, axis=1, keepdims=True))
    xt = np.zeros(n)
    xt[rs.choice(n, nz, replace=False)] = rs.randn(nz) * 6
    y = (rs.rand(m) < 1.0 / (1.0 + np.exp(-(A @ xt + beta)))).astype(np.float64)
    om = rs.rand(m)
    om[rs.choice(m, zeros, replace=False)] = 0.0
    return A, y, om


def panel_instance(m, n, k, seed=0, return_model=False):
    """One A and k columns of planted labels and weights: (A, Y (k, m), Om (k, m)), every column with its own planted
    model, its own weights and its own exact zeros among them.  ``return_model``: the planted models (n, k) as well."""
    A = instance(m, n, seed)[0]
    rs = np.random.RandomState(seed + 1)
    Y, Om, Xt = np.empty((k, m)), np.empty((k, m)), np.zeros((n, k))
    for c in range(k):
        xt = np.zeros(n)
        xt[rs.choice(n, 10, replace=False)] = rs.randn(10) * 6
        Y[c] = rs.rand(m) < 1.0 / (1.0 + np.exp(-(A @ xt + 0.1 * (c % 5 - 2))))
        Om[c] = rs.rand(m)
        Om[c, rs.choice(m, m // 8, replace=False)] = 0.0
        Xt[:, c] = xt
    return (A, Y, Om, Xt) if return_model else (A, Y, Om)


def sigma(eta):
    t = np.exp(-np.abs(eta))
    return np.where(eta >= 0, 1.0 / (1.0 + t), t / (1.0 + t))


def objective(A, y, om, x, b0, mu, pen=None):
    """sum om l(A x + b0; y) + mu sum pen |x|, plain numpy sums."""
    eta = A @ x + b0
    pw = np.ones(A.shape[1]) if pen is None else pen
    return float(om @ (np.maximum(eta, 0) + np.log1p(np.exp(-np.abs(eta))) - y * eta)) + mu * float(pw @ np.abs(x))


def lipschitz(A, om, intercept=True):
    """L = 1/4 lambda_max([A 1]^T diag(om) [A 1]): the gradient of the logistic loss in (x, beta0) is L-Lipschitz."""
    At = np.hstack([A, np.ones((A.shape[0], 1))]) if intercept else A
    return 0.25 * np.linalg.norm(At * np.sqrt(om)[:, None], 2) ** 2


def kkt_residual(A, y, om, x, b0, mu, intercept=True, positive=False, pen=None):
    """|| L (u - prox(u - grad f(u) / L)) ||_2 at u = (x, beta0): the gradient mapping with step 1 / L of the problem (the
    intercept an unpenalised coordinate).  0 exactly at an optimum, and <= sqrt(2 L (P(u) - P*)) everywhere."""
    n = A.shape[1]
    L = lipschitz(A, om, intercept)
    g = A.T @ (om * (sigma(A @ x + b0) - y))
    pw = np.ones(n) if pen is None else pen
    v = x - g / L
    xn = np.sign(v) * np.maximum(np.abs(v) - mu * pw / L, 0.0)
    if positive:
        xn = np.maximum(xn, 0.0)
    r = L * (x - xn)
    if intercept:
        r = np.r_[r, float(om @ (sigma(A @ x + b0) - y))]
    return float(np.linalg.norm(r)), L


def prox_gradient(A, y, om, mu, tol=1e-10, maxit=400000):
    """The reference solver: accelerated proximal gradient (restarted when the momentum points uphill) on (x, beta0),
    run until the unit-step prox-gradient residual in the infinity norm is <= ``tol``.  Returns (x, beta0, residual)."""
    m, n = A.shape
    At = np.hstack([A, np.ones((m, 1))])
    L = lipschitz(A, om)
    thr = np.r_[np.full(n, mu / L), 0.0]

    def step(u):
        v = u - At.T @ (om * (sigma(At @ u) - y)) / L
        return np.sign(v) * np.maximum(np.abs(v) - thr, 0.0)
    z = np.zeros(n + 1)
    w, t, res = z.copy(), 1.0, np.inf
    for it in range(maxit):
        zn = step(w)
        if (w - zn) @ (zn - z) > 0:
            t, wn = 1.0, zn
        else:
            tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
            wn, t = zn + (t - 1.0) / tn * (zn - z), tn
        z, w = zn, wn
        if it % 50 == 0:
            res = L * float(np.abs(z - step(z)).max())
            if res <= tol:
                break
    return z[:n], float(z[n]), res


# ---------------------------------------------------------------------------
# The path tests' instance and check (tests/test_panel_logistic.py, tests/test_panel_logistic_edges.py)
# ---------------------------------------------------------------------------
GAP_BOUND, OUTER_MAX = 1e-4, 32    # the fp32-rounded numpy model of the loop needs at most 3 outer steps of 64 iterations
                                   # on this grid (tests/test_panel_logistic_host.py runs it); 32 leaves the bf16
                                   # direction of the device's iteration a tenfold margin


def path_instance():
    return instance(256, 512, 1, 10, 30)


def check_path(A, y, om, out, **kw):
    null = out["null_deviance"]
    assert abs(null - C.logistic_null_deviance(y, om, kw.get("intercept", True))) <= 1e-12 * null
    assert out["reached"].all(), (out["gap"] / null, out["outer_iters"])
    assert (out["gap"] <= GAP_BOUND * null).all() and (out["outer_iters"] >= 0).all()
    assert np.all(np.diff(out["mus"]) < 0) and abs(out["mus"][0] / out["mu_max"] - 0.9) < 1e-12 \
        and abs(out["mus"][-1] / out["mu_max"] - 0.3) < 1e-12
    assert np.count_nonzero(out["x"][:, -1]) > 0
    for j, mu in enumerate(out["mus"]):
        ref = C.logistic_panel_solve(A, y, om, mu, outer_max=300, inner_iters=16, tol=1e-8, **kw)
        assert ref["reached"]
        P = objective(A, y, om, out["x"][:, j], out["intercept"][j], mu, kw.get("p"))
        assert abs(P - out["primal"][j]) <= 1e-9 * P
        # P* <= P <= P* + gap, and P* lies within the reference's own gap below P_ref
        assert ref["primal"] - 1e-8 * null <= P <= ref["primal"] + GAP_BOUND * null, (j, P, ref["primal"])


# ---------------------------------------------------------------------------
# The edges of the model (tests/test_panel_logistic_edges.py and its host checks): states placed with
# ``solver_reset(B, mu, x0=X)`` that reach the curvature floor, the safeguards of the intercept's Newton iteration, the
# one-class flag and fractional labels; a copy of the Newton loop with a trace and the mutants' switches; and the
# assertions themselves, so that the GPU tests and the CPU mutants run the same ones.
# ---------------------------------------------------------------------------
SEPS, YBARS = (12.0, 30.0, 45.0), (0.2, 0.5, 0.9)
FAR_START = 500.0        # a Newton start outside every bracket here
FAR_X = 200.0            # x_1 of the two-cluster columns: the zero-weight rows' A x lies this far outside the others'
ONE_CLASS_B0 = {"one_y0": 0.7, "one_y1": -1.3, "one_w0": 2.5}
SUMS = ("loss", "hold_loss", "hold_miss", "sum_omega", "l1")
EPS = 2.0 ** -52


def edge_kinds(k):
    """The cases of a k-wide panel, r = k / 16 of each block: 3 r saturated columns (the planted model x 8, 40, 1), 9 r
    two-cluster columns (sep x ybar; the Newton start FAR_START on every other one, and with r > 1 every (sep, ybar) has
    both starts), 3 r one-class columns, r columns of fractional labels.  A list of dicts, one per column."""
    r = k // 16
    assert k == 16 * r
    kinds = [dict(kind="sat", scale=(8.0, 40.0, 1.0)[t % 3]) for t in range(3 * r)]
    kinds += [dict(kind="two", sep=SEPS[(t % 9) // 3], ybar=YBARS[t % 3], far_start=(t % 9 + t // 9) % 2 == 1)
              for t in range(9 * r)]
    kinds += [dict(kind=("one_y0", "one_y1", "one_w0")[t % 3]) for t in range(3 * r)]
    kinds += [dict(kind="frac", scale=8.0) for t in range(r)]
    return kinds


def edge_instance(m, n, k, seed=0):
    """One A (m, n), exact in bf16, and k columns of (labels, weights, scoring weights, x, Newton start), one case each
    (``edge_kinds``).  A is ``panel_instance``'s with two columns replaced: A[:, 0] = +1 / -1 alternating by row,
    A[:, 1] = 1 on the 6 rows ``far`` and 0 elsewhere.  x is exact in fp32.

      sat     labels and weights of ``panel_instance``, x = scale x the planted model (entries 0 and 1 zeroed).  The
              scales go 8, 40, 1 over the columns: with the seeds used here every x 8 and every x 40 column has rows on
              the floor and rows above it, and no x 1 column has any (the host test asserts it per column).
      two     x_0 = sep, x_1 = FAR_X, the rest 0: A x = +-sep on the rows with a weight and FAR_X +- sep on ``far``,
              whose weight is 0; labels Bernoulli(ybar), independent of the cluster.
      one_y0  om y = 0 throughout; one_y1: y = 1 on every row with a weight; one_w0: om = 0.  Incoming beta0 != 0.
      frac    labels uniform in (0, 1), 12 each set to exactly 1/2, 0 and 1; scoring weights on every row.

    Returns dict(A, Y (k, m), Om, H, X (n, k), B0 (k,), kinds, far)."""
    A, Yp, Omp, Xp = panel_instance(m, n, k, seed, return_model=True)
    rs = np.random.RandomState(seed + 7)
    A = A.copy()
    far = np.sort(rs.choice(m, 6, replace=False))
    A[:, 0] = np.where(np.arange(m) % 2 == 0, 1.0, -1.0)
    A[:, 1] = 0.0
    A[far, 1] = 1.0
    assert (bf16(A) == A).all()
    Xp[:2] = 0.0
    kinds = edge_kinds(k)
    Y, Om, X, B0 = Yp.copy(), Omp.copy(), np.zeros((n, k)), np.zeros(k)
    H, hr = np.empty((k, m)), rs.rand(k, m)
    for c, kd in enumerate(kinds):
        u, w = rs.rand(m), rs.rand(m)
        if kd["kind"] in ("sat", "frac"):
            X[:, c] = kd["scale"] * Xp[:, c]
        if kd["kind"] == "two":
            X[0, c], X[1, c] = kd["sep"], FAR_X
            Y[c] = u < kd["ybar"]
            Om[c] = w
            Om[c, rs.choice(m, m // 8, replace=False)] = 0.0
            Om[c, far] = 0.0
            B0[c] = FAR_START if kd["far_start"] else 0.0
        elif kd["kind"].startswith("one"):
            X[:, c] = Xp[:, c]
            Y[c] = u < 0.5
            Om[c] = {"one_y0": w * (Y[c] == 0.0), "one_y1": w * (Y[c] == 1.0), "one_w0": np.zeros(m)}[kd["kind"]]
            B0[c] = ONE_CLASS_B0[kd["kind"]]
        elif kd["kind"] == "frac":
            Y[c] = u
            idx = rs.choice(m, 36, replace=False)
            Y[c, idx[:12]], Y[c, idx[12:24]], Y[c, idx[24:]] = 0.5, 0.0, 1.0
            H[c] = 0.25 + w
        if kd["kind"] != "frac":
            H[c] = (Om[c] == 0.0) * hr[c]      # scoring weights on the zero-weight rows
    X = X.astype(np.float32).astype(np.float64)
    return dict(A=A, Y=Y, Om=Om, H=H, X=X, B0=B0, kinds=kinds, far=far, m=m, n=n, k=k)


def without_one_class(inst):
    """(Y, Om, B0) with the one-class columns given column 0's labels, weights and start: every column has a root."""
    Y, Om, B0 = inst["Y"].copy(), inst["Om"].copy(), inst["B0"].copy()
    for c, kd in enumerate(inst["kinds"]):
        if kd["kind"].startswith("one"):
            Y[c], Om[c], B0[c] = Y[0], Om[0], B0[0]
    return Y, Om, B0


def columns_of(inst, *kinds):
    """the columns of these kinds ("sat", "two", "one" for the three one-class kinds, "frac"), in order"""
    return [c for c, kd in enumerate(inst["kinds"]) if kd["kind"].split("_")[0] in kinds]


def newton_trace(ax, y, omega, beta0=0.0, all_rows=False, fallback="mid", noise=None):
    """``cpu_calculation.logistic_intercept``, copied, with a trace and three switches.  ``all_rows``: the bracket over
    every row, not the rows with a weight (mutant).  ``fallback`` = "lo": a step that leaves the bracket goes to its lower
    end, not its midpoint (mutant).  ``noise``: a RandomState; every sigma is then moved by -1, 0 or +1 ulp, which is
    what separates two correct implementations of exp.  Returns dict(beta, phi, steps, flag, fallbacks (steps replaced
    by the midpoint), outside (the start lay outside the bracket), no_slope (d > 0 was false), lo, hi (the bracket))."""
    def sig(eta):
        p = C._sigma(eta)
        if noise is not None:
            e = noise.randint(-1, 2, size=p.shape)
            p = np.where(e < 0, np.nextafter(p, -1.0), np.where(e > 0, np.nextafter(p, 2.0), p))
        return p
    sw, sy = C._block_sum(omega), C._block_sum(omega * y)

    def ev(beta):
        p = sig(ax + beta)
        return C._block_sum(omega * (p - y)), C._block_sum(omega * (p * (1.0 - p)))
    beta = float(beta0)
    out = dict(fallbacks=0, outside=False, no_slope=0, lo=None, hi=None)
    if not (sy > 0.0 and sy < sw):
        return dict(out, beta=beta, phi=abs(ev(beta)[0]), steps=0, flag=1)
    lg = float(np.log(sy / (sw - sy)))
    live = np.ones(ax.size, dtype=bool) if all_rows else omega > 0
    lo, hi = lg - float(ax[live].max()), lg + float((-ax[live]).max())
    out.update(lo=lo, hi=hi)
    if not (lo <= beta <= hi):
        beta, out["outside"] = 0.5 * (lo + hi), True
    steps = 0
    while True:
        f, d = ev(beta)
        if abs(f) <= C.GLM_PHI_TOL * sw or steps == C.GLM_NEWTON_MAX:
            break
        if f > 0.0:
            hi = beta
        else:
            lo = beta
        out["no_slope"] += not d > 0.0
        nb = beta - f / d if d > 0.0 else lo
        if not (lo < nb < hi):
            nb = 0.5 * (lo + hi) if fallback == "mid" else lo
            out["fallbacks"] += 1
        beta = nb
        steps += 1
    return dict(out, beta=beta, phi=abs(f), steps=steps, flag=0)


def count_is_stable(ax, y, omega, beta0, draws=8, seed=0):
    """True when the step count of the Newton loop is the same under ``draws`` seeded draws of +-1 ulp noise on sigma:
    the columns in which a correct device must take exactly the restatement's number of steps."""
    want = newton_trace(ax, y, omega, beta0)["steps"]
    rs = np.random.RandomState(seed)
    return all(newton_trace(ax, y, omega, beta0, noise=rs)["steps"] == want for _ in range(draws))


def edge_model(A, y, omega, x, beta0=0.0, intercept=True, hold=None, floor=True, all_rows=False, fallback="mid",
               miss_ge=False):
    """``cpu_calculation.logistic_model`` (Newton curvature, unit factors), copied, with the mutants' switches: ``floor``
    False drops the floor of p (1 - p); ``all_rows`` / ``fallback`` as in ``newton_trace``; ``miss_ge`` counts a miss by
    (p >= 1/2) != (y >= 1/2).  With the defaults it returns what the original returns, bit for bit."""
    A = np.asarray(A, dtype=np.float64)
    m = A.shape[0]
    h = np.zeros(m) if hold is None else hold
    ax = A @ x
    if intercept:
        t = newton_trace(ax, y, omega, beta0, all_rows, fallback)
        b0, phi, steps, flag = t["beta"], t["phi"], t["steps"], t["flag"]
    else:
        b0, steps, flag = 0.0, 0, 0
        phi = abs(C._block_sum(omega * (C._sigma(ax) - y)))
    eta = ax + b0
    pr = C._sigma(eta)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.maximum(pr * (1.0 - pr), C.GLM_FLOOR) if floor else pr * (1.0 - pr)
        z = eta + (y - pr) / v
    ls = C._logloss(eta, y)
    miss = (((pr >= 0.5) != (y >= 0.5)) if miss_ge else ((pr > 0.5) != (y > 0.5))).astype(np.float64)
    tot = C._blocks_sum if m % 256 == 0 else C._block_sum
    return dict(ax=ax, beta0=b0, eta=eta, p=pr, v=v, w=(4.0 * omega) * v, z=z, loss=tot(omega * ls),
                hold_loss=tot(h * ls), hold_miss=tot(h * miss), sum_omega=tot(omega), l1=C._block_sum(np.abs(x)),
                phi=phi, steps=steps, flag=flag)


def dual_one_sided(y, omega, p, scale):
    """``cpu_calculation.logistic_dual`` with 0 log 0 = 0 on the t side only (mutant): (1 - t) log(1 - t) is NaN at
    t = 1."""
    t = float(scale) * p + (1.0 - float(scale)) * y
    u = 1.0 - t
    with np.errstate(divide="ignore", invalid="ignore"):
        nh = np.where(t > 0, t * np.log(np.where(t > 0, t, 1.0)), 0.0) + u * np.log(u)
    return -C._block_sum(omega * nh)


def root_longdouble(ax, y, omega):
    """The root of phi by bisection in np.longdouble, nothing shared with the Newton loop: (beta, phi'(beta))."""
    L = np.longdouble
    ax, y, om = ax.astype(L), y.astype(L), omega.astype(L)

    def phi(b):
        e = ax + b
        t = np.exp(-np.abs(e))
        return (om * (np.where(e >= 0, 1 / (1 + t), t / (1 + t)) - y)).sum()
    lo, hi = L(-2000.0), L(2000.0)
    assert phi(lo) < 0 < phi(hi)
    for _ in range(200):
        mid = (lo + hi) / 2
        if phi(mid) > 0:
            hi = mid
        else:
            lo = mid
    b = float((lo + hi) / 2)
    p = C._sigma(np.asarray(ax, dtype=np.float64) + b)
    return b, float(omega @ (p * (1.0 - p)))


def sum_rounding(m):
    """A bound, relative to sum om, on the rounding of the device's fixed-order sum of m terms om_i t_i with |t_i| <= 1:
    m / 256 serial additions per thread, 6 levels of the wave fold, 3 additions over the waves, and 2 roundings inside
    a term; each at most 2^-53 of the running sum."""
    return (m // 256 + 6 + 3 + 2) * 2.0 ** -53


def beta_tolerance(m, om, dphi, beta, dax):
    """How far two values of beta0 may lie apart when each has |phi| <= GLM_PHI_TOL sum om in its own arithmetic:
    the computed phi differs from the exact one by at most ``sum_rounding`` sum om, phi' = ``dphi`` = sum om p (1 - p) at
    the root turns a difference in phi into one in beta (phi' changes by a factor e^-|d beta| at most over the interval,
    1 here), an offset ``dax`` between the two sides' A x moves the root by at most ``dax``, and beta itself is rounded."""
    return 2.0 * (C.GLM_PHI_TOL + sum_rounding(m)) * float(om.sum()) / dphi + dax + 4.0 * EPS * max(1.0, abs(beta))


def check_model_column(got, ref, y, om, exact_steps, intercept=True, root=None, collect=None):
    """The assertions of the edge tests on one column: ``got`` (the device's, or a mutant's) against the restatement
    ``ref``.  Both are dicts with the keys of ``logistic_model``.  ``exact_steps``: the column is in the exact-count
    class (``count_is_stable``).  ``root``: ``root_longdouble`` of the column.  Every assertion carries its name as
    the first entry of its message; with ``collect`` (a list) a failed one is appended there, not raised, so that a
    mutant test sees every assertion that rejects.  Returns the measured errors."""
    def need(cond, msg):
        if collect is None:
            assert cond, msg
        elif not cond:
            collect.append(msg)
    m = y.size
    err = {}
    amax = max(np.abs(ref["ax"]).max(), 1e-300)
    dax = 1e-12 * amax                 # the AX bound; every tolerance below is computed from it and from ``ref`` alone
    err["ax"] = np.abs(got["ax"] - ref["ax"]).max() / amax
    need(err["ax"] <= 1e-12, ("AX", err["ax"], amax))
    deta = dax                         # the bound on the two sides' eta difference: A x, and beta0 where it is solved for
    need(got["flag"] == ref["flag"], ("flag", got["flag"], ref["flag"]))
    sw = float(om.sum())
    if not intercept:
        need(got["beta0"] == 0.0 and got["steps"] == 0, ("intercept off", got["beta0"], got["steps"]))
        need(abs(got["phi"] - ref["phi"]) <= 1e-9 * ref["phi"], ("phi(0)", got["phi"], ref["phi"]))
    elif ref["flag"]:
        need(got["steps"] == 0 and got["beta0"] == ref["beta0"], ("one class", got["steps"], got["beta0"]))
        need(abs(got["phi"] - ref["phi"]) <= 1e-9 * ref["phi"], ("one class phi", got["phi"], ref["phi"]))
    else:
        dphi = float(om @ (ref["p"] * (1.0 - ref["p"])))
        tol = beta_tolerance(m, om, dphi, ref["beta0"], dax)
        err["beta0"] = abs(got["beta0"] - ref["beta0"])
        need(err["beta0"] <= tol, ("beta0", got["beta0"], ref["beta0"], tol))
        deta = dax + tol
        if root is not None:
            err["beta0_ld"] = abs(got["beta0"] - root[0])
            # one side of this pair is exact: half the phi term
            tol_ld = (C.GLM_PHI_TOL + sum_rounding(m)) * sw / root[1] + dax + 4.0 * EPS * max(1.0, abs(root[0]))
            need(err["beta0_ld"] <= tol_ld, ("beta0 longdouble", got["beta0"], root[0], tol_ld))
        need(got["phi"] <= 1e-12 * sw and ref["phi"] <= 1e-12 * sw, ("phi", got["phi"], ref["phi"], sw))
        assert 0 <= ref["steps"] <= C.GLM_NEWTON_MAX
        slack = 0 if exact_steps else 1
        need(abs(got["steps"] - ref["steps"]) <= slack, ("steps", got["steps"], ref["steps"], slack))
    need(np.abs(got["p"] - ref["p"]).max() <= 1e-13, ("P", np.abs(got["p"] - ref["p"]).max()))
    need(np.abs(got["w"] - ref["w"]).max() <= 1e-13, ("W", np.abs(got["w"] - ref["w"]).max()))
    need((got["w"][om == 0.0] == 0.0).all() and np.max(got["w"]) <= 1.0, ("W where om = 0",))
    # rows the restatement puts on the floor with a margin: p (1 - p) not within 1e-3 relative of the floor
    pq = ref["p"] * (1.0 - ref["p"])
    fl = pq < C.GLM_FLOOR * (1.0 - 1e-3)
    need((got["w"][fl] == ((4.0 * om) * C.GLM_FLOOR)[fl]).all(), ("W on the floor",))
    # Z: v o (Z - eta) against y - p, where 1 / v does not enter
    eta = got["ax"] + got["beta0"]
    dz = np.abs(ref["v"] * (got["z"] - eta) - (y - ref["p"])).max()
    need(dz <= 1e-12, ("v (Z - eta)", dz))
    # and Z itself on the floor rows.  Z = eta + (y - p) / v with 1 / v = 1e5 exactly the same number on both sides, so
    # the two Z differ by the two eta's difference d (at most ``deta``, the AX bound plus beta0's), by 1e5 times the two p's
    # difference -- |dp / d eta| = p (1 - p) <= 1e-5 on these rows, so at most 1e-5 d, plus one ulp of p <= 1 (2^-53,
    # doubled: exp may differ by an ulp and turn a rounding) --, and by the roundings of y - p, the division and the
    # addition, 4 ulp in all of |eta| + |(y - p) / v| (which is |Z| unless the two cancel).
    if fl.any():
        d = deta
        size = np.abs(ref["eta"][fl]) + np.abs(ref["z"][fl] - ref["eta"][fl])
        tolz = (2.0 * d + 1e5 * 2.0 * 2.0 ** -53 + 4.0 * EPS * size) / np.abs(ref["z"][fl])
        rel = np.abs(got["z"][fl] - ref["z"][fl]) / np.abs(ref["z"][fl])
        err["z_floor"] = float(rel.max())
        need((rel <= tolz).all(), ("Z on the floor", float(rel.max()), float(tolz.min())))
    for key in SUMS:
        e = abs(got[key] - ref[key]) / (abs(ref[key]) if ref[key] != 0.0 else 1.0)
        err[key] = e
        need(e <= 1e-9, (key, got[key], ref[key]))
    return err


BOHNING_SHAPE, BOHNING_OUTER, BOHNING_ITERS, BOHNING_MU_FRAC = (256, 512, 16), 6, 16, 0.3
_bohning = {}


def bohning_reference():
    """The fp32-rounded numpy model of the IRLS loop with curvature 1 from the start, on every column of
    ``panel_instance(*BOHNING_SHAPE)`` at BOHNING_MU_FRAC x its own mu_max: dict(mu (k,), null (k,), history (k,
    BOHNING_OUTER + 1): P at every outer step).  Computed once."""
    if not _bohning:
        m, n, k = BOHNING_SHAPE
        A, Y, Om = panel_instance(m, n, k)
        mu, null, hist = np.empty(k), np.empty(k), np.empty((k, BOHNING_OUTER + 1))
        for c in range(k):
            mu[c] = BOHNING_MU_FRAC * C.logistic_gap(A, Y[c], Om[c], np.zeros(n), 1.0)["gnorm_inf"]
            run = C.logistic_panel_solve(A, Y[c], Om[c], mu[c], outer_max=BOHNING_OUTER, inner_iters=BOHNING_ITERS,
                                         tol=0.0, curv=1, round_x=True)
            assert run["outer_iters"] == BOHNING_OUTER
            null[c], hist[c] = run["null_deviance"], run["history"]
        _bohning.update(mu=mu, null=null, history=hist)
    return _bohning


def check_dual(D, y, om, p_ref, scale):
    """``glm_dual`` of one column against ``logistic_dual``: 1e-9 relative to sum om log 2 (D can be 0)."""
    ref = C.logistic_dual(y, om, p_ref, scale)
    tol = 1e-9 * float(om.sum()) * np.log(2.0)
    assert abs(D - ref) <= tol, ("dual", D, ref, scale)
    if scale == 0.0 and np.isin(y, (0.0, 1.0)).all():
        assert D == 0.0, ("dual at scale 0", D)
    return abs(D - ref) / max(tol / 1e-9, 1e-300)

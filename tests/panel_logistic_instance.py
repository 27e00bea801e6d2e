"""Planted logistic instances for tests/test_panel_logistic_host.py and tests/test_panel_logistic.py (DESIGN.md
section 18), and a reference solver written for the tests alone.  No GPU."""
import numpy as np
import torch


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


def panel_instance(m, n, k, seed=0):
    """One A and k columns of planted labels and weights: (A, Y (k, m), Om (k, m)), every column with its own planted
    model, its own weights and its own exact zeros among them."""
    A = instance(m, n, seed)[0]
    rs = np.random.RandomState(seed + 1)
    Y, Om = np.empty((k, m)), np.empty((k, m))
    for c in range(k):
        xt = np.zeros(n)
        xt[rs.choice(n, 10, replace=False)] = rs.randn(10) * 6
        Y[c] = rs.rand(m) < 1.0 / (1.0 + np.exp(-(A @ xt + 0.1 * (c % 5 - 2))))
        Om[c] = rs.rand(m)
        Om[c, rs.choice(m, m // 8, replace=False)] = 0.0
    return A, Y, Om


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

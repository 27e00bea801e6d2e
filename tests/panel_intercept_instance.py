"""The instances of the panel-intercept tests (test_panel_intercept_host.py, test_panel_intercept.py):
data whose response and features have a non-zero mean, so that the no-intercept model is the wrong one.

``offset_instance(m, n)``: a row-normalised A plus a per-column offset comparable to the column spread,
bf16-rounded; b = A x0 + 2.0 + noise; masks ``kfold_masks(m, n_folds, seed=7)`` and the grid
``mu_grid(||A^T (b - mean b)||_inf, n_mus)``, laid out as ``panel_cv_instance.cv_instance`` lays them out
(column c = f * n_mus + j).  ``big_offset_instance()``: column means about three times the spread, where
the centred diag matters (192 iterations to a relative gap of 1e-4 against 1472 with ||a_j||^2).
"""
import functools

import numpy as np

from convex_optimization_amd import cpu_calculation as C
from panel_gap_instance import bf16_round


def _data(m, n, rs, off):
    A = rs.randn(m, n)
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    Ab = bf16_round(A + off(rs))
    x0 = rs.randn(n) * (rs.rand(n) < 0.4)
    b = Ab @ x0 + 2.0 + 0.01 * rs.randn(m)
    return Ab, b


@functools.lru_cache(maxsize=None)
def offset_instance(m, n, n_folds=4, n_mus=4):
    """(Ab, b, B (m, k), W (m, k) uint8, mu_cols (k,), masks (n_folds, m), mus (n_mus,)), read-only;
    k = n_folds * n_mus."""
    Ab, b = _data(m, n, np.random.RandomState(m + n + 1), lambda rs: 0.5 * rs.rand(n) / np.sqrt(n))
    k = n_folds * n_mus
    masks = C.kfold_masks(m, n_folds, seed=7)
    mus = C.mu_grid(float(np.abs(Ab.T @ (b - b.mean())).max()), n_mus)
    cols = np.arange(k)
    W = np.ascontiguousarray(masks[cols // n_mus].T)
    mu_cols = mus[cols % n_mus].copy()
    B = np.repeat(b[:, None], k, axis=1)
    for a in (Ab, b, B, W, mu_cols, masks, mus):
        a.setflags(write=False)
    return Ab, b, B, W, mu_cols, masks, mus


@functools.lru_cache(maxsize=None)
def big_offset_instance():
    """(Ab, b, w (m,) uint8 fold 0 of kfold_masks(256, 4, seed=7), mu = 0.1 mu_max), 256 x 512, read-only."""
    m, n = 256, 512
    Ab, b = _data(m, n, np.random.RandomState(5), lambda rs: 3.0 / np.sqrt(n) * (0.5 + rs.rand(n)))
    w = C.kfold_masks(m, 4, seed=7)[0].copy()
    mu = 0.1 * float(np.abs(Ab.T @ (b - b.mean())).max())
    for a in (Ab, b, w):
        a.setflags(write=False)
    return Ab, b, w, mu


@functools.lru_cache(maxsize=None)
def sparse_offset_instance(m=256, n=2048, k=16, lo=0.05):
    """(Ab, b, mus), read-only: panel_screen_reference.screen_instance's draws (a 48-sparse solution on a wide
    A, where the gap-safe screen drops most columns) with ``offset_instance``'s column offsets and the
    response's + 2.0; mus = mu_grid(||Ab^T (b - mean b)||_inf, k, 0.9, lo)."""
    rs = np.random.RandomState(m + n)
    A = rs.randn(m, n)
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    Ab = bf16_round(A + 0.5 * rs.rand(n) / np.sqrt(n))
    x = np.zeros(n)
    idx = rs.permutation(n)[:48]
    x[idx] = rs.randn(48) + np.sign(rs.randn(48))
    b = Ab @ x + 2.0 + 0.01 * rs.randn(m)
    mus = C.mu_grid(float(np.abs(Ab.T @ (b - b.mean())).max()), k, 0.9, lo)
    for a in (Ab, b, mus):
        a.setflags(write=False)
    return Ab, b, mus


def screened_reference(Ab, b, mus, bound, iter_max, check_every, shrink):
    """``panel._screened_loop`` with the intercept in fp64 (no mask, one block), as
    panel_screen_reference.screened_reference states it without: dict(t, compactions, reached)."""
    n, k = Ab.shape[1], len(mus)
    w = np.ones(Ab.shape[0])
    bc = b - b.mean()
    target = bound * 0.5 * float(bc @ bc)
    A_cur, active, X = Ab, np.arange(n), np.zeros((n, k))
    t, compactions, reached = 0, [], np.zeros(k, dtype=bool)
    while t < iter_max:
        dg = C.centred_diag(A_cur)
        for j in range(k):
            X[:, j] = C.intercept_panel_iterate(A_cur, b, w, mus[j], check_every, diag=dg, x0=X[:, j])["x"]
        t += check_every
        certs = [C.intercept_duality_gap(A_cur, b, w, X[:, j].astype(np.float32).astype(np.float64), mus[j], diag=dg)
                 for j in range(k)]
        reached = np.array([c["gap"] for c in certs]) <= target
        if reached.all() or t >= iter_max:
            break
        sel = C.compaction_columns(np.any(np.stack([c["keep"] for c in certs]), axis=0), 256)
        if sel.size <= shrink * active.size:
            A_cur, active = np.ascontiguousarray(A_cur[:, sel]), active[sel]
            X = X[sel].astype(np.float32).astype(np.float64)
            compactions.append((t, int(active.size)))
    return dict(t=t, compactions=compactions, reached=reached)


def t_ref(Ab, b, w, mu, diag, bound=1e-4, every=64, t_max=8192):
    """The first multiple of ``every`` at which ``intercept_panel_iterate`` with ``diag``, its x rounded to
    fp32, has gap <= bound * 1/2 ||P_w b||^2 (the certificate always with the centred diag)."""
    wf = (np.asarray(w) != 0).astype(np.float64)
    pb = wf * (b - (wf @ b) / wf.sum())
    target = bound * 0.5 * float(pb @ pb)
    x, t = None, 0
    while t < t_max:
        x = C.intercept_panel_iterate(Ab, b, w, mu, every, diag=diag, x0=x)["x"]
        t += every
        x32 = x.astype(np.float32).astype(np.float64)
        if C.intercept_duality_gap(Ab, b, w, x32, mu)["gap"] <= target:
            return t
    raise AssertionError("the restatement did not reach the bound")


def cv_t_ref(m, n, bound=1e-4):
    """The largest ``t_ref`` (centred diag) over the 16 columns of ``offset_instance(m, n)``."""
    Ab, b, _, W, mu_cols, _, _ = offset_instance(m, n)
    dg = C.centred_diag(Ab)
    return max(t_ref(Ab, b, W[:, c], mu_cols[c], dg, bound) for c in range(W.shape[1]))


def row_deleted_reference(Ab, b, w, mu, iters=4096):
    """The fold's problem stated the long way: rows deleted, A and b explicitly centred over the remaining
    rows, no intercept in the solver (``masked_panel_iterate`` with the centred data's own column norms).
    Returns dict(x, intercept = mean b - mean a . x, holdout_sse, objective)."""
    idx = np.asarray(w) != 0
    Ai, bi = Ab[idx] - Ab[idx].mean(axis=0), b[idx] - b[idx].mean()
    dg = np.square(Ai).sum(axis=0)
    dg = np.where(dg > 0, dg, 1.0)
    x = C.masked_panel_iterate(Ai, bi, np.ones(int(idx.sum())), mu, 1, iters, diag=dg)["x"]
    b0 = float(b[idx].mean() - Ab[idx].mean(axis=0) @ x)
    h = Ab[~idx] @ x + b0 - b[~idx]
    r = Ai @ x - bi
    return dict(x=x, intercept=b0, holdout_sse=float(h @ h), objective=0.5 * float(r @ r) + mu * float(np.abs(x).sum()))

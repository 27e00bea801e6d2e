"""The screen instance of the panel warm-start / compaction tests and an fp64 reference of the drivers'
screened loop (``panel._screened_loop``), built on
``cpu_calculation.masked_panel_iterate(x0=...)``, ``panel_duality_gap`` / ``masked_duality_gap`` and
``compaction_columns``.

Instance: rs = RandomState(m + n), A = randn row-normalised and bf16-rounded, a solution with 48 nonzeros
randn + sign(randn) (two draws of 48) at rs.permutation(n)[:48], b = Ab x + 0.01 randn, and
mus = mu_grid(||Ab^T b||_inf, 16, 0.9, 0.05).  A sparse solution on a wide A: the gap-safe screen drops
most columns once the gap is small, which the dense instance of panel_gap_instance.py never does.

The reference iterates every right-hand side in fp64; at every check the certificate is taken of x rounded
to fp32 (what the device stores), as tests/test_panel_gap.py derives T_ref.
"""
import functools

import numpy as np

from convex_optimization_amd import cpu_calculation as C
from panel_gap_instance import bf16_round

N_SUPPORT = 48


@functools.lru_cache(maxsize=None)
def screen_instance(m=256, n=2048, k=16, lo=0.05):
    """(Ab, b, B, mus, mu_max), read-only."""
    rs = np.random.RandomState(m + n)
    A = rs.randn(m, n)
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    Ab = bf16_round(A)
    x = np.zeros(n)
    idx = rs.permutation(n)[:N_SUPPORT]
    x[idx] = rs.randn(N_SUPPORT) + np.sign(rs.randn(N_SUPPORT))   # two draws: magnitudes, then signs' offsets
    b = Ab @ x + 0.01 * rs.randn(m)
    B = np.repeat(b[:, None], k, axis=1)
    mu_max = float(np.abs(Ab.T @ b).max())
    mus = C.mu_grid(mu_max, k, 0.9, lo)
    for a in (Ab, b, B, mus):
        a.setflags(write=False)
    return Ab, b, B, mus, mu_max


def f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def screened_reference(Ab, b, mus, Block, bound, iter_max, check_every, shrink, W=None):
    """The screened loop in fp64: ``check_every`` block updates of every column, a certificate of the
    fp32-rounded x, stop when every column's gap <= its target (``bound`` * 1/2 ||w o b||^2), else compact
    when ``compaction_columns`` of the union of keep leaves at most ``shrink`` times the active columns.
    ``W``: (m, k) row mask or None.  Returns dict(t, x (n, k) scattered back, active, compactions,
    trace [(t, worst gap / (1/2 ||w o b||^2), union size, n_active)], reached)."""
    m, n = Ab.shape
    k = len(mus)
    Wk = np.ones((m, k)) if W is None else (np.asarray(W) != 0).astype(np.float64)
    hbb = np.array([0.5 * float((Wk[:, j] * b) @ (Wk[:, j] * b)) for j in range(k)])
    targets = bound * hbb
    q = Block * 256
    active = np.arange(n)
    A_cur = Ab
    X = np.zeros((n, k))
    t, trace, compactions = 0, [], []
    reached = np.zeros(k, dtype=bool)
    while t < iter_max:
        step = min(check_every, iter_max - t)
        for j in range(k):
            X[:, j] = C.masked_panel_iterate(A_cur, b, Wk[:, j], mus[j], Block, step, x0=X[:, j])["x"]
        t += step
        certs = [C.masked_duality_gap(A_cur, b, Wk[:, j], f32(X[:, j]), mus[j]) for j in range(k)]
        gaps = np.array([c["gap"] for c in certs])
        union = np.any(np.stack([c["keep"] for c in certs]), axis=0)
        trace.append((t, float(np.max(gaps / hbb)), int(union.sum()), int(active.size)))
        reached = gaps <= targets
        if reached.all() or t >= iter_max or shrink == 0.0:
            if reached.all():
                break
            continue
        sel = C.compaction_columns(union, q)
        if sel.size <= shrink * active.size:
            A_cur, X, active = np.ascontiguousarray(A_cur[:, sel]), f32(X[sel]), active[sel]
            compactions.append((t, int(active.size)))
    x = np.zeros((n, k))
    x[active] = X
    return dict(t=t, x=x, active=active, compactions=compactions, trace=trace, reached=reached)

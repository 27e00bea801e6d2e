"""The instance of the panel-certificate tests (test_panel_gap_host.py, test_panel_gap.py): one b in
every column of B and a geometric grid of mu below mu_max, on a row-normalised, bf16-rounded A."""
import functools

import numpy as np

from convex_optimization_amd.cpu_calculation import mu_grid


def bf16_round(A):
    """Round to nearest even to bf16, returned as fp64 (bitwise what torch's .to(bfloat16) gives on
    finite fp32 input, as tests/test_panel.py rounds)."""
    u = np.ascontiguousarray(A, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def instance(m, n, k):
    """(Ab, b, B, mus, mu_max), read-only."""
    rs = np.random.RandomState(m + n)
    A = rs.randn(m, n)
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    Ab = bf16_round(A)
    x0 = rs.randn(n) * (rs.rand(n) < 0.4)
    b = Ab @ x0 + 0.01 * rs.randn(m)
    B = np.repeat(b[:, None], k, axis=1)
    mu_max = float(np.abs(Ab.T @ b).max())
    mus = mu_grid(mu_max, k)
    for a in (Ab, b, B, mus):
        a.setflags(write=False)
    return Ab, b, B, mus, mu_max

"""The instance and the case table of tests/golden/panel/panel_restatement.npz (tests/golden/make_panel_restatement.py
writes it, tests/test_panel_restatement_host.py reads it): every public fp64 restatement of the panel's modes in
``cpu_calculation`` at every combination of its ``intercept`` / ``positive`` / ``p`` / ``Block`` arguments.

A case is (tag, family, rows, kwargs): ``rows`` names the row vector ("mask": 0/1, "weights": in [0, 1] with exact
zeros), kwargs holds the flags.  ``run(C, inst, case, mu)`` gives the case's record, of which the fixture keeps one
row per key: x, r (and intercept) after ``T`` iterations, then the certificate at that x.  ``mu`` is 0.3 of the case's
own mu_max (``mu_max``: its certificate's gnorm_inf at x = 0); the fixture keeps it, so the test does not take it from
the code under test.
"""
import numpy as np

M, N, T = 64, 32, 18          # 18: the step tests' horizon
SCALARS = ("primal", "dual", "gap", "scale", "gnorm_inf", "holdout_sse", "intercept")


def instance():
    """dict(A (64, 32), b, mask uint8 (about a quarter out), weights (exact zeros among them), p = exp(U[-1, 1])), a
    fixed seed."""
    rs = np.random.RandomState(20261)
    A = rs.randn(M, N) / np.sqrt(M)
    x = rs.randn(N) * (rs.rand(N) < 0.3)
    b = A @ x + 0.05 * rs.randn(M) + 1.5
    mask = (rs.rand(M) >= 0.25).astype(np.uint8)
    weights = 1.0 - 0.95 * rs.rand(M)
    weights[rs.rand(M) < 0.125] = 0.0
    p = np.exp(rs.uniform(-1.0, 1.0, N))
    return dict(A=A, b=b, mask=mask, weights=weights, p=p)


def _cases():
    out = [("masked/B1", "masked", "mask", dict(Block=1)), ("masked/B2", "masked", "mask", dict(Block=2)),
           ("intercept", "intercept", "mask", {})]
    for icpt, Block in ((False, 1), (False, 2), (True, 1)):
        out.append((f"positive/i{icpt:d}/B{Block}", "positive", "mask", dict(intercept=icpt, Block=Block)))
    for icpt in (False, True):
        for pos in (False, True):
            for Block in (1,) if icpt else (1, 2):
                out.append((f"penalty/i{icpt:d}/s{pos:d}/B{Block}", "penalty", "mask",
                            dict(intercept=icpt, positive=pos, Block=Block)))
            for rows in ("weights", "mask"):
                for use_p in (False, True):
                    out.append((f"weighted/{rows}/i{icpt:d}/s{pos:d}/p{use_p:d}", "weighted", rows,
                                dict(intercept=icpt, positive=pos, use_p=use_p)))
    return out


CASES = _cases()


def iterate(C, family, inst, w, mu, iters, p="own", **kw):
    """The family's iterate on the instance with row vector ``w``; ``p``: "own" takes the instance's factors where the
    case uses them."""
    A, b = inst["A"], inst["b"]
    pen = inst["p"] if isinstance(p, str) else p
    if family == "masked":
        return C.masked_panel_iterate(A, b, w, mu, kw["Block"], iters)
    if family == "intercept":
        return C.intercept_panel_iterate(A, b, w, mu, iters)
    if family == "positive":
        return C.positive_panel_iterate(A, b, w, mu, kw["Block"], iters, intercept=kw["intercept"])
    if family == "penalty":
        return C.penalty_panel_iterate(A, b, w, mu, pen, kw["Block"], iters, intercept=kw["intercept"],
                                       positive=kw["positive"])
    return C.weighted_panel_iterate(A, b, w, mu, iters, intercept=kw["intercept"], positive=kw["positive"],
                                    p=pen if kw["use_p"] else None)


def certificate(C, family, inst, w, mu, x, p="own", **kw):
    A, b = inst["A"], inst["b"]
    pen = inst["p"] if isinstance(p, str) else p
    if family == "masked":
        return C.masked_duality_gap(A, b, w, x, mu)
    if family == "intercept":
        return C.intercept_duality_gap(A, b, w, x, mu)
    if family == "positive":
        return C.positive_duality_gap(A, b, w, x, mu, intercept=kw["intercept"])
    if family == "penalty":
        return C.penalty_duality_gap(A, b, w, x, mu, pen, intercept=kw["intercept"], positive=kw["positive"])
    return C.weighted_duality_gap(A, b, w, x, mu, intercept=kw["intercept"], positive=kw["positive"],
                                  p=pen if kw["use_p"] else None)


def mu_max(C, inst, case):
    _, family, rows, kw = case
    return certificate(C, family, inst, inst[rows], 1.0, np.zeros(N), **kw)["gnorm_inf"]


def run(C, inst, case, mu, x=None):
    """The case's record; ``x``: take the certificate there instead of at the iterate's own x."""
    _, family, rows, kw = case
    it = iterate(C, family, inst, inst[rows], mu, T, **kw)
    cert = certificate(C, family, inst, inst[rows], mu, it["x"] if x is None else x, **kw)
    out = {"x": it["x"], "r": it["r"], "keep": cert["keep"], "g": cert["g"]}
    if "intercept" in it:
        out["x_intercept"] = np.float64(it["intercept"])
    for key in SCALARS:
        if key in cert:
            out[key] = np.float64(cert[key])
    return out

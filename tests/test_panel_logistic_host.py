"""The panel's logistic lasso (bpgl_panel_glm_model / bpgl_panel_glm_dual, ABI 311), without a GPU.

(1) the ABI is there: bpgl_version() >= 311 (311 is this feature's number; a later ABI keeps the symbols), both symbols
    exported, a null context is BPGL_E_ARG.
(2) the host restatement (``cpu_calculation.logistic_model`` / ``logistic_gap`` / ``logistic_panel_solve``): the
    certificate is tight at (0, mu_max) and weak duality holds at random points in every mode; the inner reset carries
    the logistic gradient; the loop converges to the optimum (KKT, and a reference solver written here); with
    Boehning's bound the objective is monotone.
(3) two mutants of the certificate, each caught by a negative gap.
(4) the drivers' ValueErrors, raised before any device work.

Bounds.  Weak duality is exact in exact arithmetic; -1e-12 P allows the fp64 rounding of sums of m <= 256 terms of
size <= P.  The KKT bound is not a free tolerance: the gradient mapping G_L of an L-smooth loss plus a prox-friendly
penalty satisfies ||G_L(u)||^2 <= 2 L (P(u) - P*), and the certificate's gap bounds P(u) - P*.
"""
import ctypes

import numpy as np
import pytest

import panel_logistic_instance as I
from convex_optimization_amd import _native as N
from convex_optimization_amd import cpu_calculation as C
from convex_optimization_amd import panel

SHAPES = {"64x32": (64, 32, 4, 6), "256x512": (256, 512, 10, 30)}


def make(shape, seed=1):
    m, n, nz, zeros = SHAPES[shape]
    return I.instance(m, n, seed, nz, zeros)


def mu_max_of(A, y, om, **kw):
    return C.logistic_gap(A, y, om, np.zeros(A.shape[1]), 1.0, **kw)["gnorm_inf"]


# ---------------------------------------------------------------------------
# (1) ABI
# ---------------------------------------------------------------------------
def test_abi_311_has_the_glm_calls():
    L = panel._lib()
    assert L.bpgl_version() >= 311
    raw = ctypes.CDLL(N.LIB_PATH)
    assert hasattr(raw, "bpgl_panel_glm_model") and hasattr(raw, "bpgl_panel_glm_dual")
    assert {"bpgl_panel_glm_model", "bpgl_panel_glm_dual"} <= set(N.header_functions())


def test_null_context_is_an_error():
    L = panel._lib()
    assert L.bpgl_panel_glm_model(None, 1, None, None, None, None, None, None, None, None, None) == -1
    assert L.bpgl_last_error().decode()
    assert L.bpgl_panel_glm_dual(None, None, None, None, None, None) == -1


# ---------------------------------------------------------------------------
# (2) the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gap_is_zero_at_mu_max(shape):
    A, y, om = make(shape)
    null = C.logistic_null_deviance(y, om)
    mm = mu_max_of(A, y, om)
    c = C.logistic_gap(A, y, om, np.zeros(A.shape[1]), mm)
    assert c["scale"] == 1.0 and abs(c["primal"] - null) <= 1e-12 * null
    assert abs(c["gap"]) <= 1e-12 * null, c["gap"] / null
    # just below mu_max the point x = 0 is no longer optimal and the certificate says so
    assert C.logistic_gap(A, y, om, np.zeros(A.shape[1]), 0.5 * mm)["gap"] > 1e-6 * null


def random_points(A, y, om, count, seed, positive=False):
    rs = np.random.RandomState(seed)
    n = A.shape[1]
    for _ in range(count):
        x = np.zeros(n)
        idx = rs.choice(n, rs.randint(1, 8), replace=False)
        x[idx] = rs.randn(idx.size) * rs.choice([0.1, 1.0, 5.0])
        yield (np.abs(x) if positive else x), rs.choice([0.05, 0.3, 0.9])


MODES = {"plain": dict(), "no_intercept": dict(intercept=False), "positive": dict(positive=True), "factors": dict()}


@pytest.mark.parametrize("mode", list(MODES))
def test_weak_duality_at_random_points(mode):
    A, y, om = make("256x512")
    kw = dict(MODES[mode])
    if mode == "factors":
        kw["p"] = np.exp(np.random.RandomState(5).uniform(-1, 1, A.shape[1]))
    mm = mu_max_of(A, y, om, **kw)
    worst = np.inf
    for x, frac in random_points(A, y, om, 40, 11, positive=kw.get("positive", False)):
        c = C.logistic_gap(A, y, om, x, frac * mm, **kw)
        worst = min(worst, c["gap"] / c["primal"])
        assert c["gap"] >= -1e-12 * c["primal"], (mode, c["gap"], c["primal"])
        assert 0.0 < c["scale"] <= 1.0
    assert worst > -1e-12


@pytest.mark.parametrize("intercept", [True, False])
@pytest.mark.parametrize("curv", [0, 1])
def test_inner_reset_carries_the_logistic_gradient(curv, intercept):
    """R^ = W o (e - ebar_W) = 4 om o (p - y) right after the inner reset (the floor of v cancels), through
    ``weighted_panel_iterate`` with no iterations; g and scale through ``weighted_duality_gap``."""
    A, y, om = make("256x512")
    n = A.shape[1]
    mu = 0.3 * mu_max_of(A, y, om, intercept=intercept)
    for x, _ in random_points(A, y, om, 6, 3):
        x = x * (14.0 / np.abs(A @ x).max())   # |eta| up to 14: p (1 - p) falls below the floor at some rows
        mod = C.logistic_model(A, y, om, x, 0.0, intercept, curv)
        assert curv or (mod["v"] == C.GLM_FLOOR).any()
        want = 4.0 * om * (mod["p"] - y)
        got = C.weighted_panel_iterate(A, mod["z"], mod["w"], 4.0 * mu, 0, x0=x, intercept=intercept)["r"]
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        inner = C.weighted_duality_gap(A, mod["z"], mod["w"], x, 4.0 * mu, intercept=intercept)
        cert = C.logistic_gap(A, y, om, x, mu, 0.0, intercept, model=mod)
        assert np.abs(inner["g"] - 4.0 * cert["g"]).max() <= 1e-12 * np.abs(4.0 * cert["g"]).max()
        assert abs(inner["scale"] - cert["scale"]) <= 1e-12
        if intercept:
            assert abs(inner["intercept"] - mod["beta0"]) <= 1e-12 * max(1.0, abs(mod["beta0"]))
            assert mod["phi"] <= 1e-12 * om.sum() and mod["flag"] == 0 and 0 < mod["steps"] <= C.GLM_NEWTON_MAX


@pytest.fixture(scope="module")
def solved():
    """every shape at 0.5 mu_max: the loop at 1e-8 x null, and the reference solver (computed once)"""
    out = {}
    for shape in SHAPES:
        A, y, om = make(shape)
        mu = 0.5 * mu_max_of(A, y, om)
        run = C.logistic_panel_solve(A, y, om, mu, outer_max=200, inner_iters=16, tol=1e-8)
        out[shape] = (A, y, om, mu, run, I.prox_gradient(A, y, om, mu, tol=1e-10))
    return out


@pytest.mark.parametrize("shape", list(SHAPES))
def test_loop_reaches_the_optimum(solved, shape):
    A, y, om, mu, run, (xr, br, res) = solved[shape]
    null = run["null_deviance"]
    assert run["reached"] and run["gap"] <= 1e-8 * null and run["outer_iters"] < 200
    assert np.count_nonzero(run["x"]) > 0
    # KKT, independently: the gradient mapping, bounded by the gap
    r, L = I.kkt_residual(A, y, om, run["x"], run["intercept"], mu)
    assert r <= np.sqrt(2.0 * L * 1e-8 * null), (r, np.sqrt(2.0 * L * 1e-8 * null))
    # the reference solver reached its own stopping rule, and the two agree
    assert res <= 1e-10
    assert np.abs(run["x"] - xr).max() <= 1e-6 and abs(run["intercept"] - br) <= 1e-6
    assert abs(run["primal"] - I.objective(A, y, om, xr, br, mu)) <= 1e-8 * null
    # the objective the loop reports is the objective
    assert abs(run["primal"] - I.objective(A, y, om, run["x"], run["intercept"], mu)) <= 1e-12 * run["primal"]


@pytest.mark.parametrize("frac", [0.5, 0.1])
def test_bohning_bound_is_monotone(frac):
    A, y, om = make("256x512")
    mu = frac * mu_max_of(A, y, om)
    run = C.logistic_panel_solve(A, y, om, mu, outer_max=400, inner_iters=16, tol=1e-6, curv=1)
    h = run["history"]
    assert run["reached"] and run["curvature"] == 1 and h.size > 3
    assert np.all(np.diff(h) <= 0.0), np.diff(h).max()
    # the Newton curvature gets there in fewer outer steps, and lands on the same objective
    fast = C.logistic_panel_solve(A, y, om, mu, outer_max=400, inner_iters=16, tol=1e-6)
    assert fast["reached"] and fast["outer_iters"] < run["outer_iters"]
    assert abs(fast["primal"] - run["primal"]) <= 2e-6 * run["null_deviance"]


def test_positive_and_factors_solve():
    A, y, om = make("256x512")
    pen = np.exp(np.random.RandomState(5).uniform(-1, 1, A.shape[1]))
    for kw in (dict(positive=True), dict(p=pen), dict(intercept=False)):
        mu = 0.5 * mu_max_of(A, y, om, **kw)
        run = C.logistic_panel_solve(A, y, om, mu, outer_max=300, inner_iters=16, tol=1e-8, **kw)
        assert run["reached"], kw
        assert not kw.get("positive") or (run["x"] >= 0).all()
        r, L = I.kkt_residual(A, y, om, run["x"], run["intercept"], mu, kw.get("intercept", True),
                              kw.get("positive", False), kw.get("p"))
        assert r <= np.sqrt(2.0 * L * 1e-8 * run["null_deviance"]), kw


def test_rounded_iterate_reaches_the_drivers_bound():
    """the numpy model of the device's loop (x stored in fp32) on the GPU tests' path grid"""
    A, y, om = make("256x512")
    mm = mu_max_of(A, y, om)
    for mu in mm * np.geomspace(0.9, 0.3, 8):
        run = C.logistic_panel_solve(A, y, om, mu, outer_max=64, inner_iters=64, tol=1e-4, round_x=True)
        assert run["reached"], (mu / mm, run["gap"] / run["null_deviance"])


# ---------------------------------------------------------------------------
# (3) mutants
# ---------------------------------------------------------------------------
def test_mutant_scale_fixed_at_one_is_caught():
    """theta = om o (p - y) unscaled is not dual feasible below mu_max: its 'dual value' exceeds the primal somewhere"""
    A, y, om = make("256x512")
    mm = mu_max_of(A, y, om)
    gaps = []
    for x, frac in random_points(A, y, om, 40, 11):
        mod = C.logistic_model(A, y, om, x)
        gaps.append(mod["loss"] + frac * mm * mod["l1"] - C.logistic_dual(y, om, mod["p"], 1.0))
    assert min(gaps) < -1e-6


def test_mutant_stale_intercept_is_caught():
    """Without re-solving beta0, sum theta != 0 and theta is not feasible for the intercept's dual constraint.  For a
    FIXED offset beta the dual value is the formula's + beta sum theta, so the formula overstates it where
    beta sum om (p - y) < 0: a beta between 0 and the root, an iteration stopped halfway.  The points are the random
    ones and x = 0 at mu_max, where the fixed-offset certificate is tight and the overstatement shows as a negative gap."""
    A, y, om = make("256x512")
    n = A.shape[1]
    root = C.logistic_model(A, y, om, np.zeros(n))["beta0"]
    assert abs(root) > 0.05
    stale = 0.5 * root
    mm = mu_max_of(A, y, om)
    points = list(random_points(A, y, om, 40, 11)) + [(np.zeros(n), 1.0), (np.zeros(n), 1.5)]
    gaps, honest = [], []
    for x, frac in points:
        mod = C.logistic_model(A, y, om, x, stale, solve=False)
        gaps.append(C.logistic_gap(A, y, om, x, frac * mm, model=mod)["gap"])
        honest.append(C.logistic_gap(A, y, om, x, frac * mm, stale)["gap"])     # re-solved from the same stale start
    assert min(gaps) < -1e-6, min(gaps)
    assert min(honest) >= -1e-12 * C.logistic_null_deviance(y, om)


# ---------------------------------------------------------------------------
# (4) the drivers refuse bad input before any device work
# ---------------------------------------------------------------------------
def test_driver_value_errors():
    A, y, om = make("64x32")
    A = np.zeros((256, 256))
    y = np.r_[np.ones(100), np.zeros(156)]
    for drv in (panel.logistic_path, panel.logistic_cv):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            drv(A, np.where(y > 0, 1.5, 0.0))
        with pytest.raises(ValueError, match="Block"):
            drv(A, y, Block=2)
        with pytest.raises(ValueError, match="one class"):
            drv(A, np.ones(256))
        with pytest.raises(ValueError, match="one class"):
            drv(A, y, sample_weight=(y == 0).astype(float))      # the weights leave one class only
    masks = np.ones((4, 256), dtype=np.uint8)
    for f in range(4):
        masks[f, f::4] = 0
    masks[2, :100] = 0                                            # fold 2 trains on zeros alone
    with pytest.raises(ValueError, match="fold 2"):
        panel.logistic_cv(A, y, masks=masks, n_mus=4)
    with pytest.raises(ValueError):
        C.logistic_model(np.zeros((4, 2)), [0, 1, 2, 0], np.ones(4), np.zeros(2))

"""The panel's logistic lasso (bpgl_panel_glm_model / bpgl_panel_glm_dual, ABI 311), without a GPU.

(1) the ABI is there: bpgl_version() >= 311 (311 is this feature's number; a later ABI keeps the symbols), both symbols
    exported, a null context is BPGL_E_ARG.
(2) the host restatement (``cpu_calculation.logistic_model`` / ``logistic_gap`` / ``logistic_panel_solve``): the
    certificate is tight at (0, mu_max) and weak duality holds at random points in every mode; the inner reset carries
    the logistic gradient; the loop converges to the optimum (KKT, and a reference solver written here); with
    Boehning's bound the objective is monotone.
(3) two mutants of the certificate, each caught by a negative gap.
(4) the drivers' ValueErrors, raised before any device work.
(5) the edge instances of tests/test_panel_logistic_edges.py reach the branches they are built for (the floor, p = 1
    exactly, the midpoint fallback, a start outside the bracket, the one-class flag), the copies of the Newton loop and
    of the model in the instance module return what the originals return, and the restatement passes the edge
    assertions against itself and against a bisection in long double.
(6) five mutants of the restatement, each rejected by the assertions the GPU tests run: the floor removed (W and Z on the
    floor rows), the bracket over all rows (the step count alone), the fallback to ``lo`` (the step count in every
    two-cluster column; the root itself where 40 steps no longer reach it), ``>=`` in the miss rule (hold_miss of the
    fractional labels), 0 log 0 guarded on one side only (the dual at s = 1 where p = 1, and at s = 0: NaN).

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


# ---------------------------------------------------------------------------
# (5) the edge instances of tests/test_panel_logistic_edges.py are what they claim to be
# ---------------------------------------------------------------------------
EDGE_SHAPES = {"256x512x16": (256, 512, 16), "768x256x32": (768, 256, 32), "256x512x64": (256, 512, 64),
               "4096x256x16": (4096, 256, 16)}
_edges = {}


def edge_state(shape):
    """the instance, per column the restatement, the Newton loop's trace, the exact-count class and the long double
    root; computed once per shape"""
    if shape not in _edges:
        inst = I.edge_instance(*EDGE_SHAPES[shape])
        A, Y, Om, H, X, B0 = (inst[q] for q in ("A", "Y", "Om", "H", "X", "B0"))
        k = inst["k"]
        ref = [C.logistic_model(A, Y[c], Om[c], X[:, c], B0[c], True, 0, H[c]) for c in range(k)]
        _edges[shape] = dict(
            inst=inst, ref=ref, trace=[I.newton_trace(ref[c]["ax"], Y[c], Om[c], B0[c]) for c in range(k)],
            stable=[bool(ref[c]["flag"]) or I.count_is_stable(ref[c]["ax"], Y[c], Om[c], B0[c]) for c in range(k)],
            root=[None if ref[c]["flag"] else I.root_longdouble(ref[c]["ax"], Y[c], Om[c]) for c in range(k)])
    return _edges[shape]


@pytest.mark.parametrize("shape", list(EDGE_SHAPES))
def test_edge_instances_reach_the_branches(shape):
    e = edge_state(shape)
    inst, ref, trace = e["inst"], e["ref"], e["trace"]
    A, Y, Om, X, B0, k = inst["A"], inst["Y"], inst["Om"], inst["X"], inst["B0"], inst["k"]
    assert (I.bf16(A) == A).all() and (X.astype(np.float32).astype(np.float64) == X).all()
    floor = np.array([np.mean(r["v"] == C.GLM_FLOOR) for r in ref])
    # the floor: a mixed share on every saturated column scaled by 8 or by 40, none at scale 1; and p rounded to
    # exactly 1 on rows with a weight
    sat = I.columns_of(inst, "sat")
    assert sorted({inst["kinds"][c]["scale"] for c in sat}) == [1.0, 8.0, 40.0] and len(sat) == 3 * (k // 16)
    assert all((floor[c] > 0) == (inst["kinds"][c]["scale"] != 1.0) for c in sat), floor[sat]
    assert all(floor[c] < 1 for c in sat)
    assert any(((ref[c]["p"] == 1.0) & (Om[c] > 0)).any() for c in I.columns_of(inst, "sat"))
    # the safeguards: every two-cluster column falls back to the midpoint, the far start lies outside the bracket,
    # and the zero-weight rows lie outside the weighted rows' range, so a bracket over all rows is another bracket
    two = I.columns_of(inst, "two")
    assert len(two) == 9 * (k // 16) and sum(inst["kinds"][c]["far_start"] for c in two) >= len(two) // 2
    for c in two:
        t, kd = trace[c], inst["kinds"][c]
        assert 6 <= t["steps"] <= 12 and 1 <= t["fallbacks"] <= 5, (c, kd, t)
        assert t["outside"] == kd["far_start"] and (B0[c] == I.FAR_START) == kd["far_start"]
        assert (Om[c, inst["far"]] == 0).all() and ref[c]["ax"][inst["far"]].min() > ref[c]["ax"][Om[c] > 0].max()
        assert I.newton_trace(ref[c]["ax"], Y[c], Om[c], B0[c], all_rows=True)["lo"] < t["lo"] - 100.0
        assert floor[c] > 0 and ref[c]["phi"] <= 1e-12 * Om[c].sum()
    assert all(trace[c]["fallbacks"] == 0 and not trace[c]["outside"] for c in I.columns_of(inst, "sat", "frac"))
    # the one-class flag, exactly there
    assert [c for c in range(k) if ref[c]["flag"] == 1] == I.columns_of(inst, "one")
    for c in I.columns_of(inst, "one"):
        assert ref[c]["steps"] == 0 and ref[c]["beta0"] == B0[c] != 0.0
    # fractional labels: the three exact values are there
    for c in I.columns_of(inst, "frac"):
        assert [(Y[c] == v).sum() for v in (0.5, 0.0, 1.0)] == [12, 12, 12] and floor[c] > 0
    # the step count is a property of the instance, not of the last bit of exp, in at least 90 % of the columns
    rooted = [c for c in range(k) if not ref[c]["flag"]]
    assert np.mean([e["stable"][c] for c in rooted]) >= 0.9


@pytest.mark.parametrize("shape", ["256x512x16", "768x256x32"])
def test_the_copies_return_what_the_originals_return(shape):
    e = edge_state(shape)
    inst = e["inst"]
    for c in range(inst["k"]):
        y, om, x, b0, h = inst["Y"][c], inst["Om"][c], inst["X"][:, c], inst["B0"][c], inst["H"][c]
        r, t = e["ref"][c], e["trace"][c]
        assert (t["beta"], t["phi"], t["steps"], t["flag"]) == C.logistic_intercept(r["ax"], y, om, b0)
        for icpt, want in ((True, r), (False, C.logistic_model(inst["A"], y, om, x, b0, False, 0, h))):
            mine = I.edge_model(inst["A"], y, om, x, b0, icpt, h)
            assert mine.keys() == want.keys()
            for key in want:
                assert np.asarray(mine[key]).tobytes() == np.asarray(want[key]).tobytes(), (c, icpt, key)
        assert I.dual_one_sided(y, om, np.clip(r["p"], 1e-3, 0.999), 0.7) == \
            C.logistic_dual(y, om, np.clip(r["p"], 1e-3, 0.999), 0.7)


@pytest.mark.parametrize("shape", list(EDGE_SHAPES))
def test_the_restatement_passes_its_own_edge_assertions(shape):
    """with itself as the other side, the long double root included: the derived beta0 bound holds for the Newton root"""
    e = edge_state(shape)
    inst = e["inst"]
    for c in range(inst["k"]):
        y, om, h, r = inst["Y"][c], inst["Om"][c], inst["H"][c], e["ref"][c]
        I.check_model_column(r, r, y, om, e["stable"][c], root=e["root"][c])
        for sc in (1.0, 0.0, 0.5, 1e-8):
            I.check_dual(C.logistic_dual(y, om, r["p"], sc), y, om, r["p"], sc)


def test_bohning_reference_has_steps_that_descend():
    """at 0.3 mu_max every column lowers P by more than 1e-6 x the null deviance in at least 4 of the 6 outer steps"""
    want = I.bohning_reference()
    drop = -np.diff(want["history"], axis=1)
    assert drop.shape == (I.BOHNING_SHAPE[2], I.BOHNING_OUTER)
    assert ((drop > 1e-6 * want["null"][:, None]).sum(axis=1) >= 4).all(), (drop / want["null"][:, None]).round(7)
    assert (drop >= 0.0).all()


# ---------------------------------------------------------------------------
# (6) mutants of the restatement, each rejected by the assertions the GPU tests run (``check_model_column``, ``check_dual``)
# ---------------------------------------------------------------------------
def rejections(shape="256x512x16", **mutant):
    """{assertion name: [columns]} over the columns of the shape, the mutant ``edge_model`` against the restatement"""
    e = edge_state(shape)
    inst, out = e["inst"], {}
    for c in range(inst["k"]):
        y, om, x, b0, h = inst["Y"][c], inst["Om"][c], inst["X"][:, c], inst["B0"][c], inst["H"][c]
        failed = []
        I.check_model_column(I.edge_model(inst["A"], y, om, x, b0, True, h, **mutant), e["ref"][c], y, om,
                             e["stable"][c], root=e["root"][c], collect=failed)
        for msg in failed:
            out.setdefault(msg[0], []).append(c)
    return inst, out


def test_no_mutation_no_rejection():
    assert rejections()[1] == {}


def test_mutant_floor_removed_is_caught():
    inst, out = rejections(floor=False)
    floored = [c for c in range(inst["k"]) if inst["kinds"][c]["kind"] in ("sat", "two", "frac")
               and inst["kinds"][c].get("scale") != 1.0]
    assert set(out["W on the floor"]) >= set(I.columns_of(inst, "two")) and len(out["W on the floor"]) >= 11
    assert set(out["Z on the floor"]) == set(out["W on the floor"]) <= set(floored)
    assert "beta0" not in out and "steps" not in out           # nothing else moved


def test_mutant_bracket_over_all_rows_is_caught():
    """the root is the same root: only the step count tells"""
    inst, out = rejections(all_rows=True)
    assert set(out) == {"steps"} and set(out["steps"]) <= set(I.columns_of(inst, "two")) and len(out["steps"]) >= 3


def test_mutant_fallback_to_lo_is_caught():
    inst, out = rejections(fallback="lo")
    assert set(out["steps"]) == set(I.columns_of(inst, "two"))


def test_mutant_miss_rule_with_ge_is_caught():
    inst, out = rejections(miss_ge=True)
    assert out == {"hold_miss": I.columns_of(inst, "frac")}


def test_mutant_one_sided_zero_log_zero_is_caught():
    e = edge_state("256x512x16")
    inst, caught = e["inst"], {1.0: [], 0.0: []}
    for c in range(inst["k"]):
        y, om, p = inst["Y"][c], inst["Om"][c], e["ref"][c]["p"]
        for sc in caught:
            try:
                I.check_dual(I.dual_one_sided(y, om, p, sc), y, om, p, sc)
            except AssertionError as err:
                assert err.args[0][0] == "dual" and np.isnan(err.args[0][1])
                caught[sc].append(c)
    # s = 1: where p rounds to 1 on a row with a weight; s = 0: t = y, every column with a label 1
    assert set(caught[1.0]) >= {c for c in I.columns_of(inst, "sat") if inst["kinds"][c]["scale"] == 40.0}
    assert len(caught[0.0]) >= inst["k"] - 2

"""GPU tests of the panel's logistic lasso (``PanelLasso.glm_model`` / ``glm_dual``, ``logistic_path``, ``logistic_cv``;
bpgl_panel_glm_model / bpgl_panel_glm_dual, ABI 311).

Shapes: 256 x 512, k = 16 (one fold block per right-hand side, product 1 split in 8 chunks); 1024 x 512, k = 16 (four
fold blocks per right-hand side); 256 x 256, k = 128.  Labels planted per column, exact zeros among the prior weights.

 1. ``glm_model`` after 32 lasso iterations against ``cpu_calculation.logistic_model`` on the same fp32 x.
 2. after install + ``solver_reset(Z, 4 mu, x0=stored)``: the residual is 4 om o (p - y), drift 0, g the restatement's.
 3. P - ``glm_dual`` against ``logistic_gap``.
 4. ``logistic_path``: every mu reached, the objective between the two bounds the two gaps give; ``positive``; factors.
 5. ``logistic_cv``: the scores against numpy from x_folds / intercept_folds; a one-class fold is refused.
 6. a plain lasso run on the same context before and after the GLM calls: bitwise the same x.

Bounds.  AX: both sides sum n <= 512 exact products in fp64 in different orders, 1e-12 relative to max |AX|.  p, W: smooth
functions of eta with slope <= 1/4 (W <= 1), 1e-13 absolute.  Z is compared as v o (Z - eta) against y - p, so that 1 / v
(up to 1e5) does not enter.  The five sums are certificate scalars: the project's 1e-9 relative.  |phi| is rounding noise
and has its own bound, 1e-12 sum om, on both sides; the Newton step count is compared as a count.  Measured worst
relative error of the sums on one MI355X: 2.2e-16 (256 x 512), 2.0e-16 (1024 x 512), 2.2e-16 (256 x 256, k = 128).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import panel_logistic_instance as I  # noqa: E402
from convex_optimization_amd import cpu_calculation as C  # noqa: E402
from convex_optimization_amd import panel  # noqa: E402
from convex_optimization_amd.panel import PanelLasso  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = {"256x512x16": (256, 512, 16), "1024x512x16": (1024, 512, 16), "256x256x128": (256, 256, 128)}
SUMS = ("loss", "hold_loss", "hold_miss", "sum_omega", "l1")
MU_FRAC = 0.3


def dev(v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda()


def snapshot(mod):
    """everything a ``glm_model`` call returns, as bytes"""
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).tobytes() for k, v in mod.items()}


@pytest.fixture(scope="module", params=list(SHAPES))
def state(request):
    """One context per shape, driven once through: a plain lasso run; 32 lasso iterations; the model (twice, and with
    curvature 1); install + inner reset + certificate + dual; the plain lasso run again.  The tests assert on what it
    recorded; the host references are computed here once."""
    m, n, k = SHAPES[request.param]
    A, Y, Om = I.panel_instance(m, n, k)
    H = (Om == 0.0) * np.random.RandomState(9).rand(k, m)          # scoring weights on the zero-weight rows
    B = (2.0 * Y - 1.0).T.copy()
    mu_ls = 0.3 * np.abs(A.T @ B).max(axis=0)
    pl = PanelLasso(A.copy(), 1, nrhs=k, device=0)
    s = dict(A=A, Y=Y, Om=Om, H=H, k=k)
    s["plain_before"] = pl.run(B, mu_ls, 32)["x"]

    pl.set_intercept(True)
    pl.solver_reset(B, mu_ls)
    pl.solver_step(32)
    s["x"] = x = pl.solver_x()
    Yd, Omd, Hd = dev(Y), dev(Om), dev(H)
    zeros = lambda: torch.zeros(k, dtype=torch.float64, device="cuda")   # noqa: E731
    mod = pl.glm_model(Yd, Omd, Hd, None, zeros())
    s["mod"] = {key: (v.cpu().numpy().copy() if isinstance(v, torch.Tensor) else v.copy()) for key, v in mod.items()}
    s["bytes1"] = snapshot(mod)
    s["bytes2"] = snapshot(pl.glm_model(Yd, Omd, Hd, None, zeros()))
    s["x_after_model"] = pl.solver_x()
    ones = torch.ones(k, dtype=torch.int32, device="cuda")
    s["W_curv1"] = pl.glm_model(Yd, Omd, Hd, ones, zeros())["W"].cpu().numpy().copy()
    mod = pl.glm_model(Yd, Omd, Hd, None, zeros())

    # the inner reset, the certificate at it, and the dual
    g0 = np.array([np.abs(A.T @ (Om[c] * (s["mod"]["P"][c] - Y[c]))).max() for c in range(k)])
    s["mu"] = mu = MU_FRAC * g0
    pl.set_row_weights_device(mod["W"], Hd)
    pl.solver_reset(mod["Z"].t(), 4.0 * mu, x0=pl.solver_x_device())
    pl.stream.synchronize()
    s["R"] = pl.residual_device().cpu().numpy().copy()
    cert = pl.duality_gap(screen=False)
    s["cert"] = {key: (v.cpu().numpy().copy() if isinstance(v, torch.Tensor) else np.copy(v))
                 for key, v in cert.items() if v is not None}
    s["D"] = pl.glm_dual(cert["scale"])
    s["x_after_reset"] = pl.solver_x()

    pl.set_row_weights(None)
    pl.set_intercept(False)
    s["plain_after"] = pl.run(B, mu_ls, 32)["x"]

    s["ref"] = [C.logistic_model(A, Y[c], Om[c], x[:, c], 0.0, True, 0, H[c]) for c in range(k)]
    return s


# ---------------------------------------------------------------------------
# 1. the model
# ---------------------------------------------------------------------------
def test_model_matches_the_restatement(state):
    s, mod, ref, k = state, state["mod"], state["ref"], state["k"]
    assert np.count_nonzero(s["x"]) > 0
    worst = 0.0
    for c in range(k):
        r, om, y = ref[c], s["Om"][c], s["Y"][c]
        assert np.abs(mod["AX"][c] - r["ax"]).max() <= 1e-12 * np.abs(r["ax"]).max()
        assert abs(mod["beta0"][c] - r["beta0"]) <= 1e-12 * max(1.0, abs(r["beta0"]))
        assert np.abs(mod["P"][c] - r["p"]).max() <= 1e-13
        assert np.abs(mod["W"][c] - r["w"]).max() <= 1e-13
        assert (mod["W"][c][om == 0.0] == 0.0).all() and mod["W"][c].max() <= 1.0
        eta = mod["AX"][c] + mod["beta0"][c]
        assert np.abs(r["v"] * (mod["Z"][c] - eta) - (y - r["p"])).max() <= 1e-12
        for key in SUMS:
            err = abs(mod[key][c] - r[key]) / (abs(r[key]) if r[key] != 0.0 else 1.0)
            worst = max(worst, err)
            assert err <= 1e-9, (c, key, mod[key][c], r[key])
        assert mod["phi"][c] <= 1e-12 * om.sum() and r["phi"] <= 1e-12 * om.sum()
        assert mod["steps"][c] == r["steps"] and 0 < r["steps"] <= C.GLM_NEWTON_MAX
        assert mod["flag"][c] == 0
    print(f"glm_model scalars, worst relative error over {k} columns: {worst:.2e}")
    assert (np.array([r["hold_loss"] for r in ref]) > 0).all() and (np.array([r["hold_miss"] for r in ref]) > 0).any()


def test_model_is_repeatable_and_read_only(state):
    assert state["bytes1"].keys() == state["bytes2"].keys()
    for key in state["bytes1"]:
        assert state["bytes1"][key] == state["bytes2"][key], key
    assert state["x_after_model"].tobytes() == state["x"].tobytes()
    assert state["x_after_reset"].tobytes() == state["x"].tobytes()


def test_bohning_curvature_gives_the_prior_weights(state):
    assert state["W_curv1"].tobytes() == state["Om"].tobytes()


# ---------------------------------------------------------------------------
# 2. the inner reset carries the logistic gradient
# ---------------------------------------------------------------------------
def test_inner_reset_residual_and_gradient(state):
    s, k = state, state["k"]
    for c in range(k):
        r = s["ref"][c]
        want = 4.0 * s["Om"][c] * (r["p"] - s["Y"][c])
        assert np.abs(s["R"][c] - want).max() <= 1e-12 * np.abs(want).max()
        g = 4.0 * (s["A"].T @ (s["Om"][c] * (r["p"] - s["Y"][c])))
        assert np.abs(s["cert"]["g"][c] - g).max() <= 1e-12 * np.abs(g).max()
        assert abs(s["cert"]["intercept"][c] - r["beta0"]) <= 1e-9 * max(1.0, abs(r["beta0"]))
    assert (s["cert"]["drift"] == 0.0).all()
    assert (s["cert"]["scale"] < 1.0).all()      # MU_FRAC < 1: the scaling is at work


# ---------------------------------------------------------------------------
# 3. the logistic certificate
# ---------------------------------------------------------------------------
def test_gap_matches_the_restatement(state):
    s, k = state, state["k"]
    for c in range(k):
        ref = C.logistic_gap(s["A"], s["Y"][c], s["Om"][c], s["x"][:, c], s["mu"][c], model=s["ref"][c])
        P = s["mod"]["loss"][c] + s["mu"][c] * s["mod"]["l1"][c]
        assert abs(P - ref["primal"]) <= 1e-9 * ref["primal"]
        assert abs(s["cert"]["scale"][c] - ref["scale"]) <= 1e-9
        assert abs((P - s["D"][c]) - ref["gap"]) <= 1e-9 * ref["primal"], (c, P - s["D"][c], ref["gap"])
        assert P - s["D"][c] > 0.0


# ---------------------------------------------------------------------------
# 6. the plain lasso is untouched
# ---------------------------------------------------------------------------
def test_plain_lasso_is_bitwise_the_same_after_the_glm_calls(state):
    assert np.count_nonzero(state["plain_before"]) > 0
    assert state["plain_before"].tobytes() == state["plain_after"].tobytes()


# ---------------------------------------------------------------------------
# 4. paths
# ---------------------------------------------------------------------------
GAP_BOUND, OUTER_MAX, check_path = I.GAP_BOUND, I.OUTER_MAX, I.check_path    # shared with the edge tests


@pytest.fixture(scope="module")
def path_instance():
    return I.path_instance()


def test_logistic_path(path_instance):
    A, y, om = path_instance
    out = panel.logistic_path(A, y, n_mus=8, hi=0.9, lo=0.3, GAP_BOUND=GAP_BOUND, OUTER_MAX=OUTER_MAX,
                              sample_weight=om, device=0)
    mm = C.logistic_gap(A, y, om, np.zeros(A.shape[1]), 1.0)["gnorm_inf"]
    assert abs(out["mu_max"] - mm) <= 1e-9 * mm
    check_path(A, y, om, out)


def test_logistic_path_positive(path_instance):
    A, y, om = path_instance
    out = panel.logistic_path(A, y, n_mus=8, hi=0.9, lo=0.3, GAP_BOUND=GAP_BOUND, OUTER_MAX=OUTER_MAX,
                              sample_weight=om, positive=True, device=0)
    assert (out["x"] >= 0.0).all()
    check_path(A, y, om, out, positive=True)


def test_logistic_path_penalty_factors(path_instance):
    A, y, om = path_instance
    pen = np.exp(np.random.RandomState(5).uniform(-1, 1, A.shape[1]))
    out = panel.logistic_path(A, y, n_mus=8, hi=0.9, lo=0.3, GAP_BOUND=GAP_BOUND, OUTER_MAX=OUTER_MAX,
                              sample_weight=om, penalty_factors=pen, device=0)
    check_path(A, y, om, out, p=pen)


# ---------------------------------------------------------------------------
# 5. cross-validation
# ---------------------------------------------------------------------------
def test_logistic_cv_scores(path_instance):
    A, y, om = path_instance
    mm = C.logistic_gap(A, y, om, np.zeros(A.shape[1]), 1.0)["gnorm_inf"]
    mus = mm * np.geomspace(0.8, 0.3, 4)
    out = panel.logistic_cv(A, y, n_folds=4, mus=mus, GAP_BOUND=GAP_BOUND, OUTER_MAX=OUTER_MAX, sample_weight=om,
                            return_x=True, device=0)
    assert out["reached"].all() and out["refit_reached"].all()
    assert out["deviance"].shape == out["error"].shape == (4, 4)
    for f in range(4):
        h = (1.0 - out["masks"][f]) * om
        for j in range(4):
            eta = A @ out["x_folds"][:, f, j] + out["intercept_folds"][f, j]
            loss = np.maximum(eta, 0) + np.log1p(np.exp(-np.abs(eta))) - y * eta
            dev_ref = 2.0 * float(h @ loss) / h.sum()
            err_ref = float(h @ ((eta > 0) != (y > 0.5))) / h.sum()
            assert abs(out["deviance"][f, j] - dev_ref) <= 1e-9 * dev_ref
            assert abs(out["error"][f, j] - err_ref) <= 1e-9
    assert np.allclose(out["mean_deviance"], out["deviance"].mean(axis=0), rtol=1e-14, atol=0)
    assert out["best"] == int(np.argmin(out["mean_deviance"])) and out["mus"][out["best_1se"]] >= out["mus"][out["best"]]
    assert 0.0 <= out["error"].min() and out["error"].max() <= 1.0
    assert out["x"].shape == (A.shape[1], 4) and np.count_nonzero(out["x"][:, -1]) > 0


def test_logistic_cv_refuses_a_one_class_fold(path_instance):
    A, y, om = path_instance
    masks = np.ones((4, y.size), dtype=np.uint8)
    for f in range(4):
        masks[f, f::4] = 0
    masks[1, y > 0.5] = 0          # fold 1 trains on zeros alone
    with pytest.raises(ValueError, match="fold 1"):
        panel.logistic_cv(A, y, masks=masks, n_mus=4, sample_weight=om, device=0)

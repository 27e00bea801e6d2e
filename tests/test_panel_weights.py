"""GPU tests of the panel's observation weights (``PanelLasso.set_row_weights``, bpgl_panel_set_row_weights, ABI 310;
DESIGN.md section 16).

Forms (the smallest shape at which each exists): the two-kernel fold 256 x 512, k = 16; the fused reduce + update with
U = 1 group per block 1024 x 512, k = 16; U = 2 and 4 at k = 128, fuse_grid 256, n = 256, m = 4096 and 8192.  Every run that
means the fused form asserts ``get_tuning("fuse_update") == 1`` first.

 1. 0/1 weights are the row mask (``==``), every form, graph and eager launches, intercept off and on, one case with
    ``positive`` and penalty factors.
 2. all-ones weights are the plain run (``==``); ``set_row_weights(None)`` gives the plain run bitwise.
 3. an independent oracle on the device: weights in {1, 1/4, 1/16, 0}, the same for every column, against a second,
    unweighted context bound to diag(sqrt w) A (exact in bf16) with sqrt(w) o b.
 4. general weights: the certificate against ``weighted_duality_gap``; repeatable; read-only.
 5. general weights: the 18-step protocol of tests/test_panel_step.py with ``check_step_weighted``.
 6. general weights: monotone primal, iterations to a relative gap of 1e-4 against the fp64 reference, x and objective.
 7. zero-weight rows.
 8. warm start and compaction.
 9. errors.
10. drivers: ``lasso_path`` / ``lasso_cv`` with ``sample_weight``.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import panel_step_reference as P  # noqa: E402
import panel_weight_reference as WR  # noqa: E402
from convex_optimization_amd import _native as N  # noqa: E402
from convex_optimization_amd import cpu_calculation as C  # noqa: E402
from convex_optimization_amd import panel  # noqa: E402
from convex_optimization_amd.panel import PanelLasso  # noqa: E402
from panel_gap_instance import instance as gap_instance  # noqa: E402
from panel_screen_reference import screen_instance  # noqa: E402

pytestmark = pytest.mark.gpu

T_STEPS, G_REFRESH = 18, 8
SCALARS = ("primal", "dual", "gap", "scale", "gnorm_inf", "n_keep", "drift", "holdout_sse", "intercept")
# name -> (m, n, k, fuse_grid, fused)
FORMS = {"two_kernel": (256, 512, 16, None, 0), "fused_u1": (1024, 512, 16, None, 1),
         "fused_u2": (4096, 256, 128, 256, 1), "fused_u4": (8192, 256, 128, 256, 1)}


def make(form, intercept=False, g_refresh=G_REFRESH):
    m, n, k, fuse_grid, fused = FORMS[form]
    Ab = WR.problem(m, n, k)[0]
    pl = PanelLasso(Ab.copy(), 1, nrhs=k, device=0)
    pl.set_tuning("g_refresh", g_refresh)
    if fuse_grid is not None:
        pl.set_tuning("fuse_grid", fuse_grid)
    if intercept:
        pl.set_intercept(True)
    return pl


def assert_form(pl, form):
    """the form in effect is the one the case means (after the weights / mask are installed: the check is per variant)"""
    assert pl.get_tuning("fuse_update") == FORMS[form][4]


def record(pl, B, mu, iters, use_graph=True, x0=None, screen=True):
    """reset, ``iters`` iterations, then everything observable: x, the solver's residual, the error record and every
    output of ``duality_gap`` (copies)."""
    pl.solver_reset(B.copy(), mu, record_len=max(iters, 1), use_graph=use_graph, x0=x0)
    if iters:
        pl.solver_step(iters)
    out = dict(x=pl.solver_x(), R=pl.residual_device().cpu().numpy().copy(), err=pl._err_iter.cpu().numpy().copy(),
               status=pl.solver_status())
    cert = pl.duality_gap(screen=screen)
    for key in SCALARS:
        out[key] = cert[key].copy()
    out["g"], out["r"] = cert["g"].cpu().numpy().copy(), cert["r"].cpu().numpy().copy()
    out["keep"] = cert["keep"].cpu().numpy().copy() if screen else None
    return out


def assert_same(a, b, what, bitwise=False):
    for key in a:
        if key == "status":
            assert a[key] == b[key], (what, key)
        elif a[key] is None:
            assert b[key] is None
        elif bitwise:
            assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), (what, key)
        else:
            assert np.array_equal(a[key], b[key]), (what, key)      # ``==``: -0 is 0


# ---------------------------------------------------------------------------
# 1. 0/1 weights are the row mask
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("intercept", [False, True])
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("form", list(FORMS))
def test_zero_one_weights_are_the_mask(form, use_graph, intercept):
    m, n, k, _, _ = FORMS[form]
    _, B, mu, _ = WR.problem(m, n, k)
    W = P.fold_mask(m, k)
    pl = make(form, intercept)
    pl.set_row_mask(W.copy())
    assert_form(pl, form)
    ref = record(pl, B, mu, 24, use_graph)
    pl.set_row_weights(W.astype(np.float64))
    assert_form(pl, form)
    assert pl.get_tuning("row_weights") == 1
    got = record(pl, B, mu, 24, use_graph)
    assert ref["x"].any() and ref["holdout_sse"].all() and (ref["R"] == 0).any()
    assert_same(ref, got, (form, use_graph, intercept))
    # the order of set_intercept and set_row_weights does not matter
    if intercept and use_graph:
        pl2 = make(form, False)
        pl2.set_row_weights(W.astype(np.float64))
        pl2.set_intercept(True)
        assert_same(got, record(pl2, B, mu, 24, use_graph), "order", bitwise=True)


def test_zero_one_weights_are_the_mask_with_positive_and_penalty():
    form = "fused_u1"
    m, n, k, _, _ = FORMS[form]
    _, B, mu, _ = WR.problem(m, n, k)
    W = P.fold_mask(m, k)
    pen = np.exp(np.random.RandomState(3).uniform(-1.0, 1.0, n))
    pl = make(form, True)
    pl.set_positive(True)
    pl.set_penalty_factors(pen)
    pl.set_row_mask(W.copy())
    ref = record(pl, B, mu, 24)
    pl.set_row_weights(W.astype(np.float64))
    assert_form(pl, form)
    assert_same(ref, record(pl, B, mu, 24), "positive + penalty")
    assert ref["x"].any() and np.all(ref["x"] >= 0)


# ---------------------------------------------------------------------------
# 2. all-ones weights, and weights cleared
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["two_kernel", "fused_u1", "fused_u4"])
def test_ones_are_the_plain_run_and_none_restores_it(form):
    m, n, k, _, _ = FORMS[form]
    _, B, mu, Wt = WR.problem(m, n, k)
    pl = make(form)
    plain = record(pl, B, mu, 24)
    pl.set_row_weights(np.ones((m, k)))
    assert_form(pl, form)
    assert_same(plain, record(pl, B, mu, 24), "ones")
    pl.set_row_weights(Wt.copy())
    assert not np.array_equal(record(pl, B, mu, 24)["x"], plain["x"])
    pl.set_row_weights(None)
    assert pl.get_tuning("row_weights") == 0
    assert_same(plain, record(pl, B, mu, 24), "cleared", bitwise=True)


# ---------------------------------------------------------------------------
# 3. the independent oracle: a second, unweighted context on diag(sqrt w) A
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["two_kernel", "fused_u1"])
def test_scaled_context_oracle(form):
    m, n, k, _, _ = FORMS[form]
    Ab, B, mu, _ = WR.problem(m, n, k)
    w = WR.pow4_weights(m, 1)[:, 0]
    sq = np.sqrt(w)
    At = sq[:, None] * Ab
    assert np.array_equal(P.bf16(At), At)                       # exact in bf16
    Bt = sq[:, None] * B
    pa = make(form)
    pa.set_row_weights(w)
    assert_form(pa, form)
    pb = PanelLasso(At.copy(), 1, nrhs=k, device=0)
    # (i) the same x: a warm start, 0 iterations
    pa.solver_reset(B.copy(), mu)
    pa.solver_step(32)
    x0 = pa.solver_x()
    a, b = record(pa, B, mu, 0, x0=x0), record(pb, Bt, mu, 0, x0=x0)
    assert x0.any() and np.array_equal(a["x"], b["x"])
    for c in range(k):
        np.testing.assert_allclose(a["g"][c], b["g"][c], rtol=1e-11, atol=1e-12 * np.abs(b["g"][c]).max())
        np.testing.assert_allclose(a["r"][c], sq * b["r"][c], rtol=1e-11, atol=1e-12 * np.abs(b["r"][c]).max())
    for key in ("primal", "dual", "scale", "gnorm_inf"):
        assert np.all(np.abs(a[key] - b[key]) <= 1e-9 * np.abs(b[key])), key
    assert np.all(np.abs(a["gap"] - b["gap"]) <= 1e-9 * b["primal"])
    assert np.all(a["keep"] | ~b["keep"])                       # weighted keep contains the scaled keep (the larger diag)
    assert np.all(a["drift"] == 0.0)
    # (ii) both solved to a relative gap of 1e-6: the two certificates bound the difference of the optimal values.  mu
    # from 0.8 to 0.45 of each column's mu_max: 1e-6 is where the fp32 x ends.  Below that the
    # iterate of the 256 x 512 instance stalls at 1.1e-6 to 3e-6, 3.5e-5 in one column, and stays there from 1024 to 2048
    # iterations -- measured alike on the weighted context, on the scaled unweighted one and on a plain one (section 16)
    mu2 = np.abs(Ab.T @ (w[:, None] * B)).max(axis=0) * np.geomspace(0.8, 0.45, k)
    target = 1e-6 * 0.5 * np.einsum("m,mk,mk->k", w, B, B)
    done = []
    for pl, Bx in ((pa, B), (pb, Bt)):
        pl.solver_reset(Bx.copy(), mu2)
        for _ in range(32):
            pl.solver_step(64)
            cert = pl.duality_gap(screen=False)
            if np.all(cert["gap"] <= target):
                break
        done.append({key: cert[key].copy() for key in ("primal", "gap")})
    da, db = done
    print(f"scaled oracle {form}: worst gap / target weighted {np.max(da['gap'] / target):.3g}, scaled {np.max(db['gap'] / target):.3g}")
    assert np.all(da["gap"] <= target) and np.all(db["gap"] <= target) and np.all(da["primal"] > 0)
    assert np.all(np.abs(da["primal"] - db["primal"]) <= np.maximum(da["gap"], db["gap"]) + 1e-9 * db["primal"])


# ---------------------------------------------------------------------------
# 4. general weights: the certificate
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("intercept", [False, True])
@pytest.mark.parametrize("form", ["two_kernel", "fused_u1"])
def test_weighted_gap_matches_numpy(form, intercept):
    m, n, k, _, _ = FORMS[form]
    Ab, B, mu, Wt = WR.problem(m, n, k)
    H = WR.holdout_weights(m, k)
    pl = make(form, intercept, g_refresh=64)
    pl.set_row_weights(Wt.copy(), H.copy())
    assert_form(pl, form)
    dg = pl.diag_ATA.reshape(-1)
    for T in (0, 64):
        rec = record(pl, B, mu, T)
        ref = [C.weighted_duality_gap(Ab, B[:, c], Wt[:, c], rec["x"][:, c].copy(), mu[c], diag=dg, intercept=intercept,
                                      hold=H[:, c]) for c in range(k)]
        get = lambda key: np.array([r[key] for r in ref])   # noqa: E731
        keys = ("primal", "dual", "scale", "gnorm_inf", "holdout_sse") + (("intercept",) if intercept else ())
        rel = {key: float(np.max(np.abs(rec[key] - get(key)) / np.abs(get(key)))) for key in keys}
        print(f"weighted gap {form} intercept={intercept} t={T}: worst rel {rel}, drift {rec['drift'].max():.2e}")
        for key in keys:
            assert np.all(np.abs(rec[key] - get(key)) <= 1e-9 * np.abs(get(key))), key
        if not intercept:
            assert not rec["intercept"].any()
        assert np.all(np.abs(rec["gap"] - get("gap")) <= 1e-9 * get("primal"))
        g_ref, r_ref, score, keep = get("g"), get("r"), get("score"), get("keep")
        for c in range(k):
            np.testing.assert_allclose(rec["g"][c], g_ref[c], rtol=1e-11, atol=1e-12 * np.abs(g_ref[c]).max())
            np.testing.assert_allclose(rec["r"][c], r_ref[c], rtol=1e-11, atol=1e-12 * np.abs(r_ref[c]).max())
        clear = np.abs(score - mu[:, None]) > 1e-9 * mu[:, None]
        assert (~clear).sum() <= 0.01 * k * n
        assert np.array_equal(rec["keep"][clear], keep[clear])
        assert np.array_equal(rec["n_keep"], rec["keep"].sum(axis=1))
        assert np.array_equal(rec["drift"], np.abs(rec["R"] - rec["r"]).max(axis=1))
        if T == 0 and not intercept:   # (with the intercept the fresh residual subtracts a mean of rounding size once more)
            assert np.all(rec["drift"] == 0.0)
    # the default scoring weights: the zero-weight rows, weight 1
    pl.set_row_weights(Wt.copy())
    rec = record(pl, B, mu, 64)
    for c in range(0, k, 5):
        ref = C.weighted_duality_gap(Ab, B[:, c], Wt[:, c], rec["x"][:, c].copy(), mu[c], diag=dg, intercept=intercept)
        assert abs(rec["holdout_sse"][c] - ref["holdout_sse"]) <= 1e-9 * ref["holdout_sse"]


@pytest.mark.parametrize("form", ["two_kernel", "fused_u1", "fused_u2"])
def test_weighted_gap_is_read_only_and_deterministic(form):
    m, n, k, _, _ = FORMS[form]
    _, B, mu, Wt = WR.problem(m, n, k)

    def snap(pl):
        cert = pl.duality_gap()
        return {key: (v.cpu().numpy().copy() if isinstance(v, torch.Tensor) else np.array(v)) for key, v in cert.items()}

    pl = make(form, True, g_refresh=64)
    pl.set_row_weights(Wt.copy())
    assert_form(pl, form)
    pl.solver_reset(B.copy(), mu)
    pl.solver_step(64)
    d1, d2 = snap(pl), snap(pl)
    assert_same(d1, d2, "two calls", bitwise=True)
    pl.solver_step(64)
    x_a, R_a = P.snapshot(pl)
    pl.solver_reset(B.copy(), mu)
    pl.solver_step(128)
    x_b, R_b = P.snapshot(pl)
    assert x_a.tobytes() == x_b.tobytes() and R_a.tobytes() == R_b.tobytes()


# ---------------------------------------------------------------------------
# 5. general weights: every step
# ---------------------------------------------------------------------------
WORST = {}


@pytest.mark.parametrize("intercept", [False, True])
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("form", list(FORMS))
def test_weighted_steps(form, use_graph, intercept):
    m, n, k, _, _ = FORMS[form]
    Ab, B, mu, Wt = WR.problem(m, n, k)
    pl = make(form, intercept)
    pl.set_row_weights(Wt.copy())
    assert_form(pl, form)
    assert pl.get_tuning("carry_g") == 1
    diag = pl.diag_ATA.reshape(-1)
    np.testing.assert_allclose(diag, C.centred_diag(Ab) if intercept else np.square(Ab).sum(axis=0), rtol=1e-12)
    chain = n // pl.kchunks
    pl.solver_reset(B.copy(), mu, record_len=T_STEPS, use_graph=use_graph)
    snaps, errs, stats, bad = [P.snapshot(pl)], [], {}, []
    R0 = -Wt.T * (WR.wcentre(Wt.T, B.T) if intercept else B.T)
    assert not snaps[0][0].any()
    np.testing.assert_allclose(snaps[0][1], R0, rtol=0, atol=1e-14 * np.abs(B).max())
    if not intercept:
        assert np.array_equal(snaps[0][1], R0)
    for t in range(T_STEPS):
        pl.solver_step(1)
        snaps.append(P.snapshot(pl))
        errs.append(float(pl._err_iter.cpu().numpy()[t]))
        assert pl.solver_status()["iters"] == t + 1
        q = t % G_REFRESH
        exact = q == 0
        viol = WR.check_step_weighted(Ab, diag, mu, Wt, B, t, snaps[t], snaps[t + 1], errs[t], 1, exact,
                                      None if exact else snaps[t][1] - snaps[t - 1][1], chain=chain, q=q,
                                      R_ref=None if exact else snaps[t - q][1], stats=stats, intercept=intercept)
        bad += [(t, v) for v in viol]
    assert pl.stat("exact_gradients") == 3
    line = " ".join(f"{c} {stats[c]:.3g}" for c in "ABCD") + (f" 0' {stats['0']:.3g}" if intercept else "")
    print(f"weighted step {form} graph={use_graph} intercept={intercept}: worst ratio to bound {line}")
    for c in stats:
        if c in "ABCD0":
            WORST[c] = max(WORST.get(c, 0.0), stats[c])
    print("  so far over all cases: " + " ".join(f"{c} {v:.3g}" for c, v in sorted(WORST.items())))
    assert not bad, bad
    # the same eighteen iterations in one call
    pl.solver_reset(B.copy(), mu, record_len=T_STEPS, use_graph=use_graph)
    pl.solver_step(T_STEPS)
    x, R = P.snapshot(pl)
    assert np.array_equal(x, snaps[-1][0]) and np.array_equal(R, snaps[-1][1])
    assert pl._err_iter.cpu().numpy().tobytes() == np.array(errs).tobytes()


# ---------------------------------------------------------------------------
# 6. general weights: the trajectory
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("intercept", [False, True])
def test_weighted_trajectory(intercept):
    m, n, k, ITER_MAX = 256, 512, 16, 4096
    Ab, b, Bm, mus, Wt = WR.trajectory_instance(m, n, k)
    T = WR.weighted_t_ref(m, n, k, intercept)
    assert T <= ITER_MAX // 4
    pl = PanelLasso(Ab.copy(), 1, nrhs=k, device=0)
    if intercept:
        pl.set_intercept(True)
    pl.set_row_weights(Wt.copy())
    dg = pl.diag_ATA.reshape(-1)
    target = 1e-4 * WR.weighted_half_norm(Wt, b, intercept)
    pl.solver_reset(Bm.copy(), mus, use_graph=False)
    objs, reached = [pl.duality_gap(screen=False)["primal"]], None
    for t in range(16, 4 * T + 1, 16):
        pl.solver_step(16)
        cert = pl.duality_gap(screen=False)
        objs.append(cert["primal"])
        if reached is None and np.all(cert["gap"] <= target):
            reached = t
    objs = np.array(objs)
    print(f"weighted trajectory intercept={intercept}: T_ref {T}, device reached at {reached}, largest objective ratio "
          f"between checks 1 + {np.max(objs[1:] / objs[:-1]) - 1:.2e}")
    assert np.all(objs[1:] <= objs[:-1] * (1 + 1e-12))
    assert reached is not None and reached <= 4 * T
    # x and the objective against the fp64 restatement after the same number of iterations
    Tc = 100
    X = record(pl, Bm, mus, Tc)["x"]
    worst_x = worst_f = 0.0
    for c in range(k):
        ref = C.weighted_panel_iterate(Ab, b, Wt[:, c], mus[c], Tc, diag=dg, intercept=intercept)["x"]
        assert np.linalg.norm(X[:, c] - ref) <= 1e-2 * np.linalg.norm(ref), c
        if ref.any():
            worst_x = max(worst_x, np.linalg.norm(X[:, c] - ref) / np.linalg.norm(ref))
        f_dev = C.weighted_duality_gap(Ab, b, Wt[:, c], X[:, c].copy(), mus[c], diag=dg, intercept=intercept)["primal"]
        f_ref = C.weighted_duality_gap(Ab, b, Wt[:, c], ref, mus[c], diag=dg, intercept=intercept)["primal"]
        worst_f = max(worst_f, abs(f_dev - f_ref) / f_ref)
    print(f"  worst rel x {worst_x:.2e}, worst rel objective {worst_f:.2e}")
    assert worst_f <= 1e-4


# ---------------------------------------------------------------------------
# 7. zero-weight rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["two_kernel", "fused_u1"])
def test_zero_weight_rows(form):
    m, n, k, _, _ = FORMS[form]
    _, B, mu, Wt = WR.problem(m, n, k)
    W2 = Wt.copy()
    W2[:, 3] = 0.0               # a column with nothing in its objective
    zero = (W2 == 0.0).T
    pl = make(form, g_refresh=64)
    pl.set_row_weights(W2.copy())
    assert_form(pl, form)
    pl.solver_reset(B.copy(), mu)
    t = 0
    for T in (16, 64, 256):
        pl.solver_step(T - t)
        t = T
        x, R = P.snapshot(pl)
        assert np.all(R[zero] == 0.0) and np.all(R[~zero] != 0.0), T
    ref = record(pl, B, mu, 64)
    for key in SCALARS + ("x", "g", "r", "R"):
        assert np.all(np.isfinite(ref[key])), key
    assert not ref["x"][:, 3].any() and not ref["R"][3].any() and not ref["g"][3].any()
    for key in ("primal", "dual", "gap", "drift"):
        assert ref[key][3] == 0.0, key
    assert abs(ref["holdout_sse"][3] - B[:, 3] @ B[:, 3]) <= 1e-9 * (B[:, 3] @ B[:, 3])
    # b at the zero-weight rows reaches nothing but the held-out score
    B2 = B.copy()
    B2[zero.T] += 1.0
    got = record(pl, B2, mu, 64)
    for key in ref:
        if key == "holdout_sse":
            assert np.all(got[key] != ref[key])
        elif key != "status":
            assert np.asarray(got[key]).tobytes() == np.asarray(ref[key]).tobytes(), key


def test_all_zero_column_with_the_intercept():
    form = "fused_u1"
    m, n, k, _, _ = FORMS[form]
    _, B, mu, Wt = WR.problem(m, n, k)
    W2 = Wt.copy()
    W2[:, 3] = 0.0
    pl = make(form, True)
    pl.set_row_weights(W2.copy())
    rec = record(pl, B, mu, 64)
    for key in SCALARS + ("x", "g", "r", "R"):
        assert np.all(np.isfinite(rec[key])), key
    assert not rec["x"][:, 3].any() and not rec["R"][3].any()
    for key in ("primal", "dual", "gap", "drift", "intercept"):
        assert rec[key][3] == 0.0, key
    assert rec["x"][:, 2].any() and rec["intercept"][2] != 0.0


# ---------------------------------------------------------------------------
# 8. warm start and compaction
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("intercept", [False, True])
@pytest.mark.parametrize("form", ["two_kernel", "fused_u1"])
def test_warm_start_has_no_drift(form, intercept):
    m, n, k, _, _ = FORMS[form]
    Ab, B, mu, Wt = WR.problem(m, n, k)
    pl = make(form, intercept)
    pl.set_row_weights(Wt.copy())
    pl.solver_reset(B.copy(), mu)
    pl.solver_step(40)
    x0 = pl.solver_x()
    rec = record(pl, B, mu, 0, x0=x0)
    assert x0.any() and np.array_equal(rec["x"], x0)
    assert np.all(rec["drift"] == 0.0) and np.array_equal(rec["R"], rec["r"])
    e = (Ab @ x0 - B).T
    want = Wt.T * (WR.wcentre(Wt.T, e) if intercept else e)
    np.testing.assert_allclose(rec["R"], want, rtol=0, atol=1e-12 * np.abs(e).max())
    if intercept:
        assert np.all(np.abs(rec["R"].sum(axis=1)) <= 1e-12 * np.abs(rec["R"]).sum(axis=1))
    # and the solve goes on from there as a cold run's does: 24 more iterations keep the objective falling
    pl.solver_step(24)
    assert np.all(pl.duality_gap(screen=False)["primal"] <= rec["primal"] * (1 + 1e-12))


def test_lasso_path_sample_weight_shrink():
    Ab, b, _, _, _ = screen_instance()
    m, n = Ab.shape
    om = 3.0 * WR.general_weights(m, 1, seed=5)[:, 0]
    bound = 3e-6
    mu_max = float(np.abs(Ab.T @ (om * b)).max())
    mus = C.mu_grid(mu_max, 16, 0.9, 0.1)
    kw = dict(mus=mus, GAP_BOUND=bound, ITER_MAX=4096, check_every=64, device=0, sample_weight=om)
    plain = panel.lasso_path(Ab, b, **kw)
    res = panel.lasso_path(Ab, b, shrink=0.75, **kw)
    rel = np.linalg.norm(res["x"] - plain["x"]) / np.linalg.norm(plain["x"])
    print(f"lasso_path sample_weight shrink: compactions {res['compactions']}, iters {res['iters']} "
          f"(plain {plain['iters']}), x against shrink=0 {rel:.2e}")
    assert plain["compactions"] == [] and np.all(plain["reached"])
    widths = [wd for _, wd in res["compactions"]]
    assert widths and widths[-1] < n and all(wd % 256 == 0 for wd in widths)
    assert res["active"].size == widths[-1] and np.all(res["reached"])
    assert np.all(res["n_keep"] == n)                                        # the final certificate is on the full A
    cw = om.max()
    for j in range(mus.size):
        cert = C.weighted_duality_gap(Ab, b, om / cw, res["x"][:, j].copy(), mus[j] / cw)
        assert abs(res["gap"][j] - cw * cert["gap"]) <= 1e-9 * cw * cert["primal"]
        assert abs(res["primal"][j] - cw * cert["primal"]) <= 1e-9 * cw * cert["primal"]
        assert cw * cert["gap"] <= bound * 0.5 * float(om @ (b * b)) * (1 + 1e-9)


# ---------------------------------------------------------------------------
# 9. errors
# ---------------------------------------------------------------------------
def test_row_weight_errors():
    form = "two_kernel"
    m, n, k, _, _ = FORMS[form]
    Ab, B, mu, Wt = WR.problem(m, n, k)
    L = panel._lib()
    assert L.bpgl_panel_set_row_weights(None, None, None) == -1
    raw = ctypes.c_void_p()
    assert L.bpgl_panel_create(ctypes.byref(raw), 0, m, n, 1, 16, 0, None) == 0
    assert L.bpgl_panel_set_row_weights(raw, None, None) == -2            # before bpgl_panel_bind
    assert "bpgl_panel_bind" in L.bpgl_last_error().decode()
    L.bpgl_panel_destroy(raw)
    pl = make(form)
    pl.set_row_weights(Wt.copy())
    ref = record(pl, B, mu, 24)
    # a refused call changes nothing: the next reset + run is the run with the weights installed before
    good = torch.from_numpy(np.ascontiguousarray(Wt.T)).to(pl.device)
    for what, bad in (("wt", 1.5), ("wt", -0.25), ("wt", np.nan), ("hold", -1.0), ("hold", np.nan)):
        t = good.clone()
        t[2, 7] = bad
        wt, hold = (t, None) if what == "wt" else (good, t)
        rc = L.bpgl_panel_set_row_weights(pl._ctx, N.ptr(wt), N.ptr(hold))
        torch.cuda.synchronize()
        assert rc == -1 and "weight" in L.bpgl_last_error().decode(), (what, bad)
        assert pl.get_tuning("row_weights") == 1
        assert_same(ref, record(pl, B, mu, 24), (what, bad), bitwise=True)
    # installing invalidates the solver, as the row mask does
    pl.set_row_weights(Wt.copy())
    with pytest.raises(N.BpglError, match=r"\(-2\): .*bpgl_panel_reset"):
        pl.solver_step(1)
    with pytest.raises(N.BpglError, match=r"\(-2\): .*bpgl_panel_reset"):
        pl.duality_gap()
    # the form limits: one feature block, the deferred x update
    pl.set_tuning("defer_x", 0)
    with pytest.raises(N.BpglError, match=r"\(-2\): .*defer_x"):
        pl.solver_reset(B.copy(), mu)
    pl.set_tuning("defer_x", 1)
    p2 = PanelLasso(Ab.copy(), 2, nrhs=k, device=0)
    p2.set_row_weights(Wt.copy())
    with pytest.raises(N.BpglError, match=r"\(-2\): .*one feature block"):
        p2.solver_reset(B.copy(), mu)
    p2.set_row_weights(None)
    p2.solver_reset(B.copy(), mu)
    # a mask and weights are alternatives: the last call wins
    W = P.fold_mask(m, k)
    pm = make(form)
    pm.set_row_mask(W.copy())
    only_mask = record(pm, B, mu, 24)
    pl.set_row_mask(W.copy())
    assert pl.get_tuning("row_weights") == 0
    assert_same(only_mask, record(pl, B, mu, 24), "weights then mask", bitwise=True)
    pl.set_row_weights(Wt.copy())
    assert_same(ref, record(pl, B, mu, 24), "mask then weights", bitwise=True)
    # the Python checks
    for bad in (1.5, -0.25, np.nan):
        v = Wt.copy()
        v[7, 2] = bad
        with pytest.raises(ValueError):
            pl.set_row_weights(v)
    with pytest.raises(ValueError):
        pl.set_row_weights(Wt.T.copy())
    with pytest.raises(ValueError):
        pl.set_row_weights(Wt.copy(), -np.ones((m, k)))
    assert_same(ref, record(pl, B, mu, 24), "after the ValueErrors", bitwise=True)
    om = np.ones(m)
    b = B[:, 0].copy()
    for kw in (dict(sample_weight=np.zeros(m)), dict(sample_weight=-om), dict(sample_weight=om * np.nan),
               dict(sample_weight=om, Block=2), dict(sample_weight=om[:-1])):
        with pytest.raises(ValueError):
            panel.lasso_path(Ab, b, n_mus=4, device=0, **kw)
        with pytest.raises(ValueError):
            panel.lasso_cv(Ab, b, n_folds=4, n_mus=4, device=0, **kw)


# ---------------------------------------------------------------------------
# 10. the drivers
# ---------------------------------------------------------------------------
def test_lasso_path_sample_weight_scale_and_ones():
    m, n = 256, 512
    Ab, b, _, _, _ = gap_instance(m, n, 16)
    om = 2.0 * WR.general_weights(m, 1, seed=9)[:, 0]
    kw = dict(GAP_BOUND=1e-4, ITER_MAX=1024, check_every=64, device=0)
    auto = panel.lasso_path(Ab, b, n_mus=16, sample_weight=om, **kw)
    mu_max = float(np.abs(Ab.T @ (om * b)).max())
    assert abs(auto["mu_max"] - mu_max) <= 1e-12 * mu_max
    M = auto["mus"]
    one = panel.lasso_path(Ab, b, mus=M, sample_weight=om, **kw)
    four = panel.lasso_path(Ab, b, mus=4.0 * M, sample_weight=4.0 * om, **kw)
    assert np.all(one["reached"]) and one["x"].any()
    assert one["x"].tobytes() == four["x"].tobytes() and one["iters"] == four["iters"]
    assert np.array_equal(four["primal"], 4.0 * one["primal"]) and np.array_equal(four["gap"], 4.0 * one["gap"])
    cw = om.max()
    for j in (0, 7, 15):
        cert = C.weighted_duality_gap(Ab, b, om / cw, one["x"][:, j].copy(), M[j] / cw)
        for key in ("primal", "dual", "gnorm_inf"):
            assert abs(one[key][j] - cw * cert[key]) <= 1e-9 * abs(cw * cert[key]), key
        assert abs(one["gap"][j] - cw * cert["gap"]) <= 1e-9 * cw * cert["primal"]
        assert one["gap"][j] <= 1e-4 * 0.5 * float(om @ (b * b))
    # all-ones weights are sample_weight=None
    none = panel.lasso_path(Ab, b, mus=M, **kw)
    ones = panel.lasso_path(Ab, b, mus=M, sample_weight=np.ones(m), **kw)
    for key in ("x", "primal", "dual", "gap", "scale", "gnorm_inf", "n_keep", "drift", "iters", "reached"):
        assert np.array_equal(none[key], ones[key]), key


def test_lasso_path_replication():
    """omega in {1, 2}: the weighted path is the unweighted path on the data with the weight-2 rows written twice."""
    m, n = 512, 512
    Ab, b, _, _, _ = gap_instance(m, n, 16)
    om = np.where(np.random.RandomState(12).permutation(m) < m // 2, 2.0, 1.0)
    assert (om == 2.0).sum() == 256
    rows = np.concatenate([np.arange(m), np.flatnonzero(om == 2.0)])
    A2, b2 = Ab[rows], b[rows]
    assert A2.shape == (768, n)
    # mu from 0.9 to 0.3 of mu_max: 1e-6 is where the fp32 x ends; below 0.12 mu_max this instance's
    # iterate stalls above it
    mus = C.mu_grid(float(np.abs(Ab.T @ (om * b)).max()), 16, 0.9, 0.3)
    kw = dict(mus=mus, GAP_BOUND=1e-6, ITER_MAX=2048, check_every=64, device=0)
    a = panel.lasso_path(Ab, b, sample_weight=om, **kw)
    r = panel.lasso_path(A2, b2, **kw)
    half = 0.5 * float(om @ (b * b))
    print(f"replication: worst rel gap weighted {np.max(a['gap']) / half:.3g}, replicated {np.max(r['gap']) / half:.3g}")
    assert np.all(a["reached"]) and np.all(r["reached"])
    dev = np.abs(a["primal"] - r["primal"])
    bnd = np.maximum(a["gap"], r["gap"]) + 1e-9 * r["primal"]
    print(f"replication: iters {a['iters']} / {r['iters']}, worst |P_w - P_rep| / bound {np.max(dev / bnd):.3g}")
    assert np.all(dev <= bnd)


@pytest.mark.parametrize("fit_intercept", [False, True])
def test_lasso_cv_sample_weight(fit_intercept):
    m, n, nf, nm, bound = 256, 512, 4, 4, 1e-4
    Ab, b, _, _, _ = gap_instance(m, n, 16)
    b = b + (1.5 if fit_intercept else 0.0)
    om = 2.0 * WR.general_weights(m, 1, seed=21)[:, 0]
    cw = om.max()
    masks = C.kfold_masks(m, nf, seed=7)
    bw = b - (om @ b) / om.sum() if fit_intercept else b
    mus = C.mu_grid(float(np.abs(Ab.T @ (om * bw)).max()), nm)
    res = panel.lasso_cv(Ab, b, mus=mus, masks=masks, return_x=True, sample_weight=om, fit_intercept=fit_intercept,
                         GAP_BOUND=bound, ITER_MAX=4096, check_every=64, device=0)
    assert np.all(res["reached"]) and res["x_folds"].shape == (n, nf, nm) and res["x"].shape == (n, nm)
    dg = C.centred_diag(Ab) if fit_intercept else None
    for f in range(nf):
        wf, hf = masks[f] * om, (1 - masks[f]) * om
        for j in range(nm):
            x = res["x_folds"][:, f, j].copy()
            cert = C.weighted_duality_gap(Ab, b, wf / cw, x, mus[j] / cw, diag=dg, intercept=fit_intercept, hold=hf)
            e = Ab @ x - b + cert["intercept"]
            mse = float(hf @ (e * e)) / float(hf.sum())
            assert abs(res["mse"][f, j] - mse) <= 1e-9 * mse
            assert abs(res["gap"][f, j] - cw * cert["gap"]) <= 1e-9 * cw * cert["primal"]
            bc = b - (wf @ b) / wf.sum() if fit_intercept else b
            assert res["gap"][f, j] <= bound * 0.5 * float(wf @ (bc * bc)) * (1 + 1e-9)
            if fit_intercept:
                b0 = -float(wf @ (Ab @ x - b)) / float(wf.sum())           # the weighted mean
                assert abs(res["intercept_folds"][f, j] - b0) <= 1e-9 * abs(b0)
    # the refit is the weighted path, with the weights and no mask
    path = panel.lasso_path(Ab, b, mus=mus, sample_weight=om, fit_intercept=fit_intercept, GAP_BOUND=bound,
                            ITER_MAX=4096, check_every=64, device=0)
    assert np.array_equal(res["x"], path["x"]) and np.array_equal(res["refit_gap"], path["gap"])
    assert np.array_equal(res["mean_mse"], res["mse"].mean(axis=0)) and res["best"] == int(np.argmin(res["mean_mse"]))

"""GPU tests of the panel's row masks (``PanelLasso.set_row_mask``, bpgl_panel_set_row_mask) and of
``panel.lasso_cv``, K-fold cross-validation over a grid of mu as one panel.

Instance (panel_cv_instance.py): panel_gap_instance's A and b, masks ``kfold_masks(m, 4, seed=7)`` laid
out as 4 folds x 4 mu (``mu_grid(mu_max, 4)``) = 16 columns, column c = 4 f + j.  Shapes (m, n, Block, k),
the smallest at which each form of the masked fold runs: (1024, 512, 1, 16) the fused reduce + update,
(256, 512, 1, 16) the two-kernel path, (256, 1024, 2, 16) the multi-block update, and
(256, 256, 1, 128) with 8 folds x 16 mu the full panel width.

The references are numpy fp64 (``masked_duality_gap``, ``masked_panel_iterate``) on the stored bf16 A and,
for soundness, the fp64 per-RHS oracle on the row-DELETED problem.  The bounds are those of
tests/test_panel_gap.py (1e-9 relative on the scalars, 1e-9 of the primal on the gap, rtol 1e-11 + atol
1e-12 max|.| on g and r, its allowance of borderline mask entries per case, 1 % of k n) and
tests/test_panel.py's for the default path (x within 1e-2 relative l2, the objective within 1e-4) as they
stand there.  A borderline entry is one whose numpy score lies within 1e-9 mu of mu, where the comparison
with mu cannot be decided in fp64: a support coordinate of a column that has converged (|g_j| = mu, gap
-> 0).  test_panel_gap.py met one, in the single column at the largest mu; here every fold has a column
at that mu, and the MI355X run met 0, 1, 0 and 2 (1024 x 512, 256 x 512, 256 x 1024, 256 x 256 k = 128).
Measured on the MI355X over all shapes and checkpoints: the scalars (holdout_sse included) within 1.1e-15
relative, the gap within 8.8e-16 of the primal, g within 7.6e-16 and r within 5.9e-17 of their largest
entries, drift 1e-7 to 6e-7; after 100 Block iterations x within 5.0e-5 and the objective within 2.2e-8 of
``masked_panel_iterate``; lasso_cv stops at 192 (T_ref 192) and 448 (T_ref 512) iterations.

0.9 mu_max of the full data lies above a fold's own mu_max = ||A^T (w o b)||_inf on these instances, so the
columns at the largest mu keep x = 0 with gap exactly 0: the tests ask for gap >= 0 there, not > 0.
"""
import concurrent.futures
import ctypes
import functools
import os

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from convex_optimization_amd import _native as N  # noqa: E402
from convex_optimization_amd import cpu_calculation as C  # noqa: E402
from convex_optimization_amd import panel  # noqa: E402
from convex_optimization_amd.panel import PanelLasso  # noqa: E402
from panel_cv_instance import cv_instance, cv_t_ref  # noqa: E402

NT = min(16, os.cpu_count() or 1)
# (m, n, Block, n_folds, n_mus)
FUSED, TWO_KERNEL, MULTI_BLOCK, FULL_WIDTH = (1024, 512, 1, 4, 4), (256, 512, 1, 4, 4), (256, 1024, 2, 4, 4), \
    (256, 256, 1, 8, 16)
SHAPES3 = [FUSED, TWO_KERNEL, MULTI_BLOCK]
SHAPES = SHAPES3 + [FULL_WIDTH]
SCALARS = ("primal", "dual", "gap", "scale", "gnorm_inf", "n_keep", "drift", "holdout_sse")


def make(m, n, B, nf, nm):
    pl = PanelLasso(cv_instance(m, n, nf, nm)[0], B, nrhs=nf * nm, device=0)
    if m == 1024:
        assert pl.get_tuning("fuse_update") == 1   # the fused reduce + update is in effect
    else:
        assert pl.get_tuning("fuse_update") == 0
    return pl


def snapshot(pl, t=0):
    """One certificate with host copies of everything the tests look at (the device buffers are reused)."""
    d = pl.duality_gap()
    rec = {key: d[key].copy() for key in SCALARS}
    rec.update(t=t, x=pl.solver_x(), g=d["g"].cpu().numpy(), r=d["r"].cpu().numpy(), keep=d["keep"].cpu().numpy(),
               R=pl.residual_device().cpu().numpy())
    return rec


def same_bits(a, b, skip=()):
    for key in a:
        if key in skip:
            continue
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def run_to(pl, Bm, mus, W, stops, use_graph=True, record=0):
    """Mask (None: leave the context as it is), reset, and a snapshot after each of ``stops`` iterations."""
    if W is not None:
        pl.set_row_mask(W)
    pl.solver_reset(Bm, mus, record_len=record, use_graph=use_graph)
    out, t = [], 0
    for stop in stops:
        pl.solver_step(stop - t)
        t = stop
        out.append(snapshot(pl, t))
    assert pl.solver_status()["iters"] == t
    if record:
        pl.stream.synchronize()
        out[-1]["err_iter"] = pl._err_iter.cpu().numpy().copy()
    return out


@functools.lru_cache(maxsize=None)
def checkpoints(m, n, B, nf, nm):
    """One masked device run per shape: certificates after 16 B, 64 B and 256 B iterations."""
    _, _, Bm, W, mu_cols, _, _ = cv_instance(m, n, nf, nm)
    return run_to(make(m, n, B, nf, nm), Bm, mu_cols, W, (16 * B, 64 * B, 256 * B))


@functools.lru_cache(maxsize=None)
def oracle_row_deleted(m, n, B, nf, nm):
    """X (n, k) of the fp64 oracle on each column's row-deleted problem after 4096 B iterations, and its
    objectives (k,)."""
    Ab, b, _, W, mu_cols, _, _ = cv_instance(m, n, nf, nm)

    def solve(c):
        rows = np.flatnonzero(W[:, c])
        Ar, br = np.ascontiguousarray(Ab[rows]), np.ascontiguousarray(b[rows])
        x = oracle.run(Ar, br, mu_cols[c], B, 4096 * B, nthreads=1)["x"]
        return x, C.duality_gap(Ar, br, x, mu_cols[c])["primal"]

    with concurrent.futures.ThreadPoolExecutor(NT) as ex:
        cols = list(ex.map(solve, range(W.shape[1])))
    X = np.stack([c[0] for c in cols], axis=1)
    X.setflags(write=False)
    return X, np.array([c[1] for c in cols])


# ---------------------------------------------------------------------------
# 1. an all-ones mask is the unmasked run, bitwise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("m,n,B,nf,nm", SHAPES3)
def test_all_ones_mask_is_no_mask(m, n, B, nf, nm, use_graph):
    _, _, Bm, W, mu_cols, _, _ = cv_instance(m, n, nf, nm)
    T = 128 * B
    base = run_to(make(m, n, B, nf, nm), Bm, mu_cols, None, (T,), use_graph, record=T)[0]
    pl = make(m, n, B, nf, nm)
    ones = run_to(pl, Bm, mu_cols, np.ones_like(W), (T,), use_graph, record=T)[0]
    same_bits(base, ones)
    assert np.all(ones["holdout_sse"] == 0.0) and np.all(base["holdout_sse"] == 0.0)
    assert base["x"].any() and np.all(base["gap"] > 0)   # unmasked: every mu is below mu_max
    # a real mask in between, then cleared: the unmasked run again
    masked = run_to(pl, Bm, mu_cols, W, (T,), use_graph, record=T)[0]
    assert not np.array_equal(masked["x"], base["x"]) and np.all(masked["holdout_sse"] > 0)
    pl.set_row_mask(None)
    same_bits(base, run_to(pl, Bm, mu_cols, None, (T,), use_graph, record=T)[0])


# ---------------------------------------------------------------------------
# 2. held-out rows stay out
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,B,nf,nm", SHAPES)
def test_held_out_rows_stay_out(m, n, B, nf, nm):
    _, _, Bm, W, mu_cols, _, _ = cv_instance(m, n, nf, nm)
    recs = checkpoints(m, n, B, nf, nm)
    held = (W == 0).T                                          # (k, m)
    for rec in recs:
        assert np.all(rec["R"][held] == 0.0) and np.all(rec["r"][held] == 0.0), rec["t"]
        assert np.all(rec["R"][~held] != 0.0)
        assert np.all(rec["holdout_sse"] > 0)
    # b changed at the held-out rows of each column only: nothing but the held-out score moves
    B2 = Bm.copy()
    B2[W == 0] += np.random.RandomState(5).randn(int((W == 0).sum()))
    again = run_to(make(m, n, B, nf, nm), B2, mu_cols, W, (16 * B, 64 * B, 256 * B))
    for rec, rec2 in zip(recs, again):
        same_bits(rec, rec2, skip=("holdout_sse",))
        assert np.all(rec["holdout_sse"] != rec2["holdout_sse"])


# ---------------------------------------------------------------------------
# 3. the columns of a panel are independent problems
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,B,nf,nm", SHAPES)
def test_columns_are_independent(m, n, B, nf, nm):
    _, _, Bm, W, mu_cols, _, _ = cv_instance(m, n, nf, nm)
    base = checkpoints(m, n, B, nf, nm)[1]
    perm = np.random.RandomState(11).permutation(W.shape[1])
    assert not np.array_equal(perm, np.arange(perm.size))
    rec = run_to(make(m, n, B, nf, nm), Bm[:, perm], mu_cols[perm], W[:, perm], (64 * B,))[0]
    assert np.array_equal(rec["x"], base["x"][:, perm])
    assert np.array_equal(rec["R"], base["R"][perm])
    for key in SCALARS:
        assert np.array_equal(rec[key], base[key][perm]), key


# ---------------------------------------------------------------------------
# 4. the certificate against the numpy restatement on the device's own x
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,B,nf,nm", SHAPES)
def test_masked_gap_matches_numpy(m, n, B, nf, nm):
    Ab, b, _, W, mu_cols, _, _ = cv_instance(m, n, nf, nm)
    k = W.shape[1]
    for rec in checkpoints(m, n, B, nf, nm):
        ref = [C.masked_duality_gap(Ab, b, W[:, c], rec["x"][:, c].copy(), mu_cols[c]) for c in range(k)]
        get = lambda key: np.array([r[key] for r in ref])   # noqa: E731
        rel = {key: np.max(np.abs(rec[key] - get(key)) / np.abs(get(key)))
               for key in ("primal", "dual", "scale", "gnorm_inf", "holdout_sse")}
        gap_err = np.max(np.abs(rec["gap"] - get("gap")) / get("primal"))
        score, keep = get("score"), get("keep")
        clear = np.abs(score - mu_cols[:, None]) > 1e-9 * mu_cols[:, None]
        g_ref, r_ref = get("g"), get("r")
        print(f"{m}x{n} B{B} k{k} t={rec['t']}: worst rel {rel}, gap err / primal {gap_err:.2e}, "
              f"g err {np.abs(rec['g'] - g_ref).max() / np.abs(g_ref).max():.2e} of max, "
              f"r err {np.abs(rec['r'] - r_ref).max() / np.abs(r_ref).max():.2e} of max, "
              f"borderline {int((~clear).sum())}, n_keep {rec['n_keep'].min()}..{rec['n_keep'].max()}, "
              f"drift {rec['drift'].max():.2e}")
        for key in rel:
            assert np.all(np.abs(rec[key] - get(key)) <= 1e-9 * np.abs(get(key))), key
        assert np.all(np.abs(rec["gap"] - get("gap")) <= 1e-9 * get("primal"))
        for c in range(k):
            np.testing.assert_allclose(rec["g"][c], g_ref[c], rtol=1e-11, atol=1e-12 * np.abs(g_ref[c]).max())
            np.testing.assert_allclose(rec["r"][c], r_ref[c], rtol=1e-11, atol=1e-12 * np.abs(r_ref[c]).max())
        # the mask of columns (full diag): exact wherever the numpy score is farther than 1e-9 mu from mu
        # (borderline entries: test_panel_gap.py's allowance as it stands there)
        assert (~clear).sum() <= 0.01 * k * n
        assert np.array_equal(rec["keep"][clear], keep[clear])
        assert np.array_equal(rec["n_keep"], rec["keep"].sum(axis=1))
        assert np.array_equal(rec["drift"], np.abs(rec["R"] - rec["r"]).max(axis=1))


@pytest.mark.parametrize("m,n,B,nf,nm", [FUSED, MULTI_BLOCK])
def test_masked_gap_is_read_only_and_deterministic(m, n, B, nf, nm):
    _, _, Bm, W, mu_cols, _, _ = cv_instance(m, n, nf, nm)

    def fresh():
        pl = make(m, n, B, nf, nm)
        pl.set_row_mask(W)
        pl.solver_reset(Bm, mu_cols)
        return pl

    pa = fresh()
    pa.solver_step(64)
    d1 = snapshot(pa)
    d2 = snapshot(pa)
    pa.solver_step(64)
    pb = fresh()
    pb.solver_step(64)
    pb.solver_step(64)
    assert torch.equal(pa.solver_x_device(), pb.solver_x_device())
    assert torch.equal(pa.residual_device(), pb.residual_device())
    assert pa.solver_status() == pb.solver_status() and pa.stat("exact_gradients") == pb.stat("exact_gradients")
    same_bits(d1, d2)
    # (0.9 mu_max of the full data is above a fold's own mu_max: those columns stay at x = 0, gap 0)
    assert np.all(d1["gap"] >= 0) and np.any(d1["gap"] > 0) and np.all(d1["holdout_sse"] > 0)


# ---------------------------------------------------------------------------
# 5. sound against the row-deleted problem, and the screen (full diag) is safe
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,B,nf,nm", SHAPES)
def test_masked_gap_is_sound_for_the_row_deleted_problem(m, n, B, nf, nm):
    Ab, b, _, W, mu_cols, _, _ = cv_instance(m, n, nf, nm)
    k = W.shape[1]
    X_ref, P_ref = oracle_row_deleted(m, n, B, nf, nm)
    supp = (np.abs(X_ref) > 2.0 ** -52 * np.abs(X_ref).max(axis=0, keepdims=True)).T     # (k, n)
    # (a fold's own mu_max can lie below 0.9 mu_max of the full data: such a column's optimum is x = 0)
    assert np.any(supp.sum(axis=1) > 0) and np.all(supp.sum(axis=1) < n)
    for rec in checkpoints(m, n, B, nf, nm):
        P_dev = np.array([C.masked_duality_gap(Ab, b, W[:, c], rec["x"][:, c].copy(), mu_cols[c])["primal"]
                          for c in range(k)])
        pos = rec["gap"] > 0   # (a column whose optimum is x = 0 has gap 0 and P(x) = P_ref)
        print(f"{m}x{n} B{B} k{k} t={rec['t']}: worst (P(x) - P_ref) / gap {np.max((P_dev - P_ref)[pos] / rec['gap'][pos]):.3f}, "
              f"worst dual / P_ref {np.max(rec['dual'] / P_ref):.9f}, screened {int((~rec['keep']).sum())} of {k * n}")
        assert np.all(rec["dual"] <= P_ref * (1 + 1e-9))
        assert np.all(P_dev - P_ref <= rec["gap"] + 1e-9 * rec["primal"])
        assert int((supp & ~rec["keep"]).sum()) == 0, rec["t"]


# ---------------------------------------------------------------------------
# 6. the trajectory is the restatement's, and the objective never increases
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,B,nf,nm", SHAPES)
def test_masked_trajectory(m, n, B, nf, nm):
    Ab, b, Bm, W, mu_cols, _, _ = cv_instance(m, n, nf, nm)
    k, T = W.shape[1], 100 * B
    pl = make(m, n, B, nf, nm)
    X = run_to(pl, Bm, mu_cols, W, (T,))[0]["x"]
    worst_x = worst_f = 0.0
    for c in range(0, k, max(1, k // 16)):
        ref = C.masked_panel_iterate(Ab, b, W[:, c], mu_cols[c], B, T)["x"]
        assert np.linalg.norm(X[:, c] - ref) <= 1e-2 * np.linalg.norm(ref), c
        if ref.any():
            worst_x = max(worst_x, np.linalg.norm(X[:, c] - ref) / np.linalg.norm(ref))
        f_dev = C.masked_duality_gap(Ab, b, W[:, c], X[:, c].copy(), mu_cols[c])["primal"]
        f_ref = C.masked_duality_gap(Ab, b, W[:, c], ref, mu_cols[c])["primal"]
        worst_f = max(worst_f, abs(f_dev - f_ref) / f_ref)
    print(f"masked panel {m}x{n} B{B} k{k}: worst rel x {worst_x:.2e}, worst rel objective {worst_f:.2e}")
    assert worst_f <= 1e-4
    # exact line search along the direction taken: the masked objective of every column never increases
    pl.solver_reset(Bm, mu_cols, use_graph=False)
    objs = [pl.duality_gap(screen=False)["primal"]]
    for _ in range(6):
        pl.solver_step(16)
        objs.append(pl.duality_gap(screen=False)["primal"])
    objs = np.array(objs)
    print(f"  largest objective ratio between checks 1 + {np.max(objs[1:] / objs[:-1]) - 1:.2e}")
    assert np.all(objs[1:] <= objs[:-1] * (1 + 1e-12))
    assert np.any(objs[-1] < objs[0])


# ---------------------------------------------------------------------------
# 7. degenerate masks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,B,nf,nm", SHAPES3)
def test_degenerate_masks(m, n, B, nf, nm):
    Ab, b, Bm, W, mu_cols, _, _ = cv_instance(m, n, nf, nm)
    W2 = W.copy()
    W2[:, 3] = 0                 # nothing in the objective
    W2[:, 9] = 1
    W2[m // 2 + 1, 9] = 0        # a single row held out
    for rec in run_to(make(m, n, B, nf, nm), Bm, mu_cols, W2, (16 * B, 64 * B)):
        for key in SCALARS + ("x", "g", "r", "R"):
            assert np.all(np.isfinite(rec[key])), key
        assert not rec["x"][:, 3].any() and not rec["R"][3].any() and not rec["g"][3].any()
        for key in ("primal", "dual", "gap", "drift"):
            assert rec[key][3] == 0.0, key
        assert abs(rec["holdout_sse"][3] - b @ b) <= 1e-9 * (b @ b)
        ref = C.masked_duality_gap(Ab, b, W2[:, 9], rec["x"][:, 9].copy(), mu_cols[9])
        for key in ("primal", "dual", "scale", "gnorm_inf", "holdout_sse"):
            assert abs(rec[key][9] - ref[key]) <= 1e-9 * abs(ref[key]), key
        assert abs(rec["gap"][9] - ref["gap"]) <= 1e-9 * ref["primal"]
        assert rec["R"][9, m // 2 + 1] == 0.0 and np.count_nonzero(rec["R"][9]) == m - 1
        assert rec["x"][:, 9].any() and rec["holdout_sse"][9] > 0


# ---------------------------------------------------------------------------
# 8. the cross-validation driver
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,B,T_expect", [(256, 512, 1, 192), (256, 1024, 2, 512)])
def test_lasso_cv(m, n, B, T_expect):
    nf, nm, bound = 4, 4, 1e-4
    Ab, b, _, W, mu_cols, masks, mus = cv_instance(m, n, nf, nm)
    T = cv_t_ref(m, n, B, bound)
    assert T == T_expect
    kw = dict(Block=B, GAP_BOUND=bound, ITER_MAX=4 * T, check_every=64, device=0)
    res = panel.lasso_cv(Ab, b, mus=mus, masks=masks, return_x=True, **kw)
    print(f"lasso_cv {m}x{n} B{B}: T_ref {T}, device iters {res['iters']}, mean mse {res['mean_mse']}, "
          f"best {res['best']}, best_1se {res['best_1se']}, refit iters {res['refit_iters']}")
    assert np.all(res["reached"]) and res["iters"] <= 4 * T and res["iters"] % 64 == 0
    assert res["x_folds"].shape == (n, nf, nm) and res["mse"].shape == (nf, nm) and res["x"].shape == (n, nm)
    assert np.array_equal(res["mus"], mus) and np.array_equal(res["masks"], masks)
    count = (masks == 0).sum(axis=1)
    for f in range(nf):
        wb = masks[f] * b
        target = bound * 0.5 * float(wb @ wb)
        for j in range(nm):
            cert = C.masked_duality_gap(Ab, b, masks[f], res["x_folds"][:, f, j].copy(), mus[j])
            assert abs(res["mse"][f, j] * count[f] - cert["holdout_sse"]) <= 1e-9 * cert["holdout_sse"]
            assert abs(res["gap"][f, j] - cert["gap"]) <= 1e-9 * cert["primal"]
            assert cert["gap"] <= target and res["gap"][f, j] <= target
    mean = res["mse"].mean(axis=0)
    se = res["mse"].std(axis=0, ddof=1) / np.sqrt(nf)
    assert np.array_equal(res["mean_mse"], mean) and np.array_equal(res["se_mse"], se)
    assert res["best"] == int(np.argmin(mean))
    ok = np.flatnonzero(mean <= mean[res["best"]] + se[res["best"]])
    assert res["best_1se"] == int(ok[np.argmax(mus[ok])]) and mus[res["best_1se"]] >= mus[res["best"]]
    # the default masks are kfold_masks(m, n_folds, seed), and mus=None takes the grid off the device's mu_max
    auto = panel.lasso_cv(Ab, b, n_folds=nf, n_mus=nm, seed=7, refit=False, **kw)
    assert np.array_equal(auto["masks"], masks) and "x" not in auto and "x_folds" not in auto
    np.testing.assert_allclose(auto["mus"], mus, rtol=1e-9)
    assert np.all(auto["reached"])
    # the refit is lasso_path on the same grid, on the context that ran the folds
    path = panel.lasso_path(Ab, b, mus=mus, **kw)
    assert np.array_equal(res["x"], path["x"]) and np.array_equal(res["refit_gap"], path["gap"])
    assert res["refit_iters"] == path["iters"]
    # 3 folds x 5 mu = 15 columns pad to 16 with a copy of column 0: the explicit 16-column run, bitwise
    m3, mu5 = C.kfold_masks(m, 3, seed=7), C.mu_grid(mus[0] / 0.9, 5)
    part = panel.lasso_cv(Ab, b, mus=mu5, masks=m3, return_x=True, refit=False, **kw)
    cols = np.concatenate([np.arange(15), [0]])
    pl = PanelLasso(Ab, B, nrhs=16, device=0)
    full = run_to(pl, np.repeat(b[:, None], 16, axis=1), mu5[cols % 5], m3[cols // 5].T, (part["iters"],))[0]
    assert part["x_folds"].shape == (n, 3, 5) and part["mse"].shape == (3, 5)
    assert np.array_equal(part["x_folds"].reshape(n, 15), full["x"][:, :15])
    assert np.array_equal(part["gap"].reshape(-1), full["gap"][:15])
    assert np.array_equal(part["n_keep"].reshape(-1), full["n_keep"][:15])
    assert np.array_equal(part["mse"].reshape(-1), full["holdout_sse"][:15] / np.repeat((m3 == 0).sum(axis=1), 5))
    assert np.array_equal(full["x"][:, 15], full["x"][:, 0])


def test_lasso_cv_rejects_bad_shapes():
    Ab, b = cv_instance(256, 512)[:2]
    with pytest.raises(ValueError):
        panel.lasso_cv(Ab, b, n_folds=9, n_mus=16, device=0)
    with pytest.raises(ValueError):
        panel.lasso_cv(Ab, b, n_folds=1, n_mus=4, device=0)
    with pytest.raises(ValueError):
        panel.lasso_cv(Ab, b, masks=np.ones((1, 256), dtype=np.uint8), n_mus=4, device=0)


# ---------------------------------------------------------------------------
# 9. errors
# ---------------------------------------------------------------------------
def test_row_mask_errors():
    m, n, B, nf, nm = TWO_KERNEL
    _, _, Bm, W, mu_cols, _, _ = cv_instance(m, n, nf, nm)
    L = panel._lib()
    assert L.bpgl_panel_set_row_mask(None, None) == -1
    assert "null" in L.bpgl_last_error().decode()
    raw = ctypes.c_void_p()
    assert L.bpgl_panel_create(ctypes.byref(raw), 0, m, n, B, 16, 0, None) == 0
    assert L.bpgl_panel_set_row_mask(raw, None) == -2            # before bpgl_panel_bind
    assert "bpgl_panel_bind" in L.bpgl_last_error().decode()
    L.bpgl_panel_destroy(raw)
    pl = make(m, n, B, nf, nm)
    pl.solver_reset(Bm, mu_cols)
    pl.solver_step(8)
    pl.set_row_mask(W)
    with pytest.raises(N.BpglError, match=r"\(-2\): .*bpgl_panel_reset"):
        pl.solver_step(1)
    with pytest.raises(N.BpglError, match=r"\(-2\): .*bpgl_panel_reset"):
        pl.duality_gap()
    pl.set_row_mask(None)                                        # clearing invalidates the solver too
    with pytest.raises(N.BpglError, match=r"\(-2\): .*bpgl_panel_reset"):
        pl.solver_step(1)
    with pytest.raises(ValueError):
        pl.set_row_mask(W.T)
    pl.solver_reset(Bm, mu_cols)
    pl.solver_step(8)
    assert np.all(pl.duality_gap()["holdout_sse"] == 0.0)

"""GPU tests of the panel's intercept (``PanelLasso.set_intercept``, bpgl_panel_set_intercept /
bpgl_panel_intercept, ``lasso_path`` / ``lasso_cv`` with ``fit_intercept``).

Instance (panel_intercept_instance.py): ``offset_instance(m, n)`` -- column offsets comparable to the column
spread, b = A x0 + 2.0 + noise, masks ``kfold_masks(m, 4, seed=7)``, 4 folds x ``mu_grid(.., k / 4)`` columns.
Shapes (m, n, k, fuse_grid), the smallest at which each form of the intercept's fold runs:

    256 x 512, k 16          two-kernel (k_panel_reduce<true, true> + k_panel_update1<true>)
    1024 x 512, k 16         fused, G 1, U 1
    2048 x 512, k 16         fused, G 2: the waiting blocks read c
    4096 x 256, k 128, 256   fused, G 2, U 2
    8192 x 256, k 128, 256   fused, G 2, U 4

G = min(fuse_grid / k, m / 1024) blocks per right-hand side of U = m / 1024 / G groups each (panel_fused_geo);
the tests assert through ``get_tuning`` that the fused form is in effect and what fuse_grid is.

The references are numpy fp64 on the stored bf16 A: ``check_step_intercept`` (A-D and 0', proved against a
model and its mutants in tests/test_panel_intercept_host.py), ``intercept_duality_gap`` at
tests/test_panel_cv.py's certificate bounds (1e-9 relative on the scalars, holdout_sse and intercept included,
1e-9 of the primal on the gap, rtol 1e-11 + atol 1e-12 max|.| on g and r), and for the trajectory the
iteration on each column's row-DELETED, explicitly centred data at test_masked_trajectory's bounds (x within
1e-2 relative l2, the objective within 1e-4).  Every case runs with graphs and with eager launches and the
two agree bitwise.

Measured on the MI355X over all shapes: worst ratio to bound of the step checks A 0.37, B 0.18, C 0.99 (no
margin by construction: the bf16 image's own rounding), D 0.44, 0' 0.011; the certificate's scalars
(holdout_sse and intercept included) within 1.3e-14 relative, the gap within 1.3e-14 of the primal, g within
3.7e-15 and r within 3.5e-16 of their largest entries, drift 1.9e-7 to 5.9e-7; after 256 iterations x within
4.1e-6 and the objective within 1.7e-12 of the row-deleted centred iteration; lasso_cv stops at 128 (T_ref 128).
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import panel_intercept_reference as Q  # noqa: E402
import panel_step_reference as P  # noqa: E402
from convex_optimization_amd import _native as N  # noqa: E402
from convex_optimization_amd import cpu_calculation as C  # noqa: E402
from convex_optimization_amd import panel  # noqa: E402
from convex_optimization_amd.panel import PanelLasso  # noqa: E402
from panel_intercept_instance import cv_t_ref, offset_instance, sparse_offset_instance  # noqa: E402

T_STEPS = 18
G_REFRESH = 8
# (m, n, k, fuse_grid or None)
TWO_KERNEL = (256, 512, 16, None)
FUSED_G1, FUSED_G2, FUSED_U2, FUSED_U4 = (1024, 512, 16, None), (2048, 512, 16, None), (4096, 256, 128, 256), \
    (8192, 256, 128, 256)
FUSED = [FUSED_G1, FUSED_G2, FUSED_U2, FUSED_U4]
SHAPES = [TWO_KERNEL] + FUSED
SCALARS = ("primal", "dual", "gap", "scale", "gnorm_inf", "n_keep", "drift", "holdout_sse", "intercept")


def problem(m, n, k):
    """(Ab, b, B, W, mu_cols) of ``offset_instance`` with 4 folds x k / 4 mu"""
    return offset_instance(m, n, 4, k // 4)[:5]


def make(m, n, k, fuse_grid, intercept=True, fuse_update=1, Ab=None):
    pl = PanelLasso((problem(m, n, k)[0] if Ab is None else Ab).copy(), 1, nrhs=k, device=0)
    if fuse_grid:
        pl.set_tuning("fuse_grid", fuse_grid)
    pl.set_tuning("fuse_update", fuse_update)
    if intercept:
        pl.set_intercept(True)
    # the form in effect, for the variant that will run (set_intercept repeated the occupancy check)
    assert pl.get_tuning("fuse_update") == int(m % 1024 == 0 and fuse_update == 1)
    assert pl.get_tuning("fuse_grid") == (fuse_grid or 1024)
    assert pl.get_tuning("defer_x") == 1 and pl.get_tuning("carry_g") == 1
    return pl


def snapshot(pl, t=0):
    d = pl.duality_gap()
    rec = {key: d[key].copy() for key in SCALARS}
    rec.update(t=t, x=pl.solver_x(), g=d["g"].cpu().numpy(), r=d["r"].cpu().numpy(), keep=d["keep"].cpu().numpy(),
               R=pl.residual_device().cpu().numpy())
    return rec


def same_bits(a, b):
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def reference_certs(Ab, b, W, mu_cols, X):
    ref = [C.intercept_duality_gap(Ab, b, W[:, c], X[:, c].copy(), mu_cols[c]) for c in range(W.shape[1])]
    return lambda key: np.array([r[key] for r in ref])


# ---------------------------------------------------------------------------
# 1. every iteration is the algorithm's step
# ---------------------------------------------------------------------------
def stepped(pl, Ab, B, mu, W, d_split, t0_warm=0, steps=T_STEPS, x0=None, stats=None):
    """Reset (at x0 when given), then ``steps`` single iterations with ``check_step_intercept`` on each pair of
    snapshots.  Returns (violations, snapshots, error records)."""
    pl.solver_reset(B.copy(), mu, record_len=steps, use_graph=True, x0=x0)
    diag = pl.diag_ATA.reshape(-1)
    chain = d_split * (Ab.shape[1] // pl.kchunks)
    snaps, errs, bad = [P.snapshot(pl)], [], []
    for t in range(steps):
        pl.solver_step(1)
        snaps.append(P.snapshot(pl))
        err_iter = pl._err_iter.cpu().numpy()
        errs.append(float(err_iter[t]))
        assert pl.solver_status()["iters"] == t + 1
        q = t % G_REFRESH
        exact = q == 0
        viol = Q.check_step_intercept(Ab, diag, mu, W, B, t, snaps[t], snaps[t + 1], errs[t], d_split, exact,
                                      None if exact else snaps[t][1] - snaps[t - 1][1], chain=chain, q=q,
                                      R_ref=None if exact else snaps[t - q][1], stats=stats, warm=t0_warm)
        bad += [(t, v) for v in viol]
    return bad, snaps, errs


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("d_split", [1, 2])
@pytest.mark.parametrize("m,n,k,fuse_grid", SHAPES)
def test_steps(m, n, k, fuse_grid, d_split, masked):
    """The 18-step protocol of tests/test_panel_step.py (two refreshes at g_refresh 8), with the fold mask and
    with no user mask (the library's all-ones one)."""
    Ab, b, B, W, mu = problem(m, n, k)
    W = W if masked else None
    pl = make(m, n, k, fuse_grid)
    pl.set_tuning("d_split", d_split)
    pl.set_tuning("g_refresh", G_REFRESH)
    if masked:
        pl.set_row_mask(W.copy())
    np.testing.assert_allclose(pl.diag_ATA.reshape(-1), C.centred_diag(Ab), rtol=1e-12)
    stats = {}
    bad, snaps, errs = stepped(pl, Ab, B, mu, W, d_split, stats=stats)
    Wk = Q.in_rows(W, k, m)
    np.testing.assert_allclose(snaps[0][1], -Q.centre(Wk, B.T), rtol=0, atol=1e-14 * np.abs(B).max())
    assert not snaps[0][0].any() and not snaps[0][1][~Wk].any()
    print(f"intercept step {(m, n, k, fuse_grid)} d_split={d_split} masked={masked}: worst ratio to bound "
          + " ".join(f"{c} {stats[c]:.3g}" for c in ("A", "B", "C", "D", "0"))
          + f", gamma in [{stats['gamma_min']:.3g}, {stats['gamma_max']:.3g}]")
    assert not bad, bad
    assert pl.stat("exact_gradients") == 3
    # the same eighteen iterations in one call, graphs replayed and eager: bitwise the stepped run
    for use_graph in (True, False):
        pl.solver_reset(B.copy(), mu, record_len=T_STEPS, use_graph=use_graph)
        pl.solver_step(T_STEPS)
        x, R = P.snapshot(pl)
        assert np.array_equal(x, snaps[-1][0]) and np.array_equal(R, snaps[-1][1]), use_graph
        assert pl._err_iter.cpu().numpy().tobytes() == np.array(errs).tobytes()


# ---------------------------------------------------------------------------
# 2. the certificate against the numpy restatement on the device's own x; read-only, repeatable
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("m,n,k,fuse_grid", SHAPES)
def test_certificate_matches_numpy(m, n, k, fuse_grid, masked):
    Ab, b, B, W, mu = problem(m, n, k)
    Wn = W if masked else np.ones_like(W)

    def fresh(use_graph):
        pl = make(m, n, k, fuse_grid)
        if masked:
            pl.set_row_mask(W.copy())
        pl.solver_reset(B.copy(), mu, use_graph=use_graph)
        return pl

    pa = fresh(True)
    pa.solver_step(64)
    d1 = snapshot(pa, 64)
    d2 = snapshot(pa, 64)
    pa.solver_step(64)
    d3 = snapshot(pa, 128)
    pb = fresh(False)                                   # eager launches, no certificate in between
    pb.solver_step(128)
    assert torch.equal(pa.solver_x_device(), pb.solver_x_device())
    assert torch.equal(pa.residual_device(), pb.residual_device())
    assert pa.solver_status() == pb.solver_status() and pa.stat("exact_gradients") == pb.stat("exact_gradients")
    same_bits(d1, d2)
    same_bits(d3, snapshot(pb, 128))
    for rec in (d1, d3):
        get = reference_certs(Ab, b, Wn, mu, rec["x"])
        keys = ("primal", "dual", "scale", "gnorm_inf", "holdout_sse", "intercept")
        rel = {key: float(np.max(np.abs(rec[key] - get(key)) / np.maximum(np.abs(get(key)), 1e-300))) for key in keys}
        g_ref, r_ref = get("g"), get("r")
        print(f"{m}x{n} k{k} masked={masked} t={rec['t']}: worst rel {rel}, gap err / primal "
              f"{np.max(np.abs(rec['gap'] - get('gap')) / get('primal')):.2e}, "
              f"g err {np.abs(rec['g'] - g_ref).max() / np.abs(g_ref).max():.2e} of max, "
              f"r err {np.abs(rec['r'] - r_ref).max() / np.abs(r_ref).max():.2e} of max, drift {rec['drift'].max():.2e}")
        for key in keys:
            assert np.all(np.abs(rec[key] - get(key)) <= 1e-9 * np.abs(get(key))), key
        assert np.all(np.abs(rec["gap"] - get("gap")) <= 1e-9 * get("primal"))
        for c in range(k):
            np.testing.assert_allclose(rec["g"][c], g_ref[c], rtol=1e-11, atol=1e-12 * np.abs(g_ref[c]).max())
            np.testing.assert_allclose(rec["r"][c], r_ref[c], rtol=1e-11, atol=1e-12 * np.abs(r_ref[c]).max())
        score, keep = get("score"), get("keep")
        clear = np.abs(score - mu[:, None]) > 1e-9 * mu[:, None]
        assert (~clear).sum() <= 0.01 * k * n
        assert np.array_equal(rec["keep"][clear], keep[clear])
        assert np.array_equal(rec["n_keep"], rec["keep"].sum(axis=1))
        assert np.array_equal(rec["drift"], np.abs(rec["R"] - rec["r"]).max(axis=1))
        assert np.all(rec["r"][Wn.T == 0] == 0.0) and np.all(rec["R"][Wn.T == 0] == 0.0)
        assert np.all(rec["holdout_sse"] > 0) if masked else np.all(rec["holdout_sse"] == 0.0)
        assert rec["x"].any() and np.all(rec["intercept"] != 0.0)


# ---------------------------------------------------------------------------
# 3. the fused reduce + update equals the two-kernel form, bitwise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k,fuse_grid", FUSED)
def test_fused_equals_two_kernel(m, n, k, fuse_grid):
    Ab, b, B, W, mu = problem(m, n, k)
    recs = []
    for fuse in (1, 0):
        for use_graph in (True, False):
            pl = make(m, n, k, fuse_grid, fuse_update=fuse)
            pl.set_row_mask(W.copy())
            pl.solver_reset(B.copy(), mu, record_len=40, use_graph=use_graph)
            pl.solver_step(40)
            rec = snapshot(pl, 40)
            rec["err_iter"] = pl._err_iter.cpu().numpy().copy()
            recs.append(rec)
    assert recs[0]["x"].any()
    for rec in recs[1:]:
        same_bits(recs[0], rec)


# ---------------------------------------------------------------------------
# 4. a warm reset starts at the centred residual of x0
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k,fuse_grid", [TWO_KERNEL, FUSED_G2, FUSED_U2])
def test_warm_reset(m, n, k, fuse_grid):
    Ab, b, B, W, mu = problem(m, n, k)
    pl = make(m, n, k, fuse_grid)
    pl.set_tuning("g_refresh", G_REFRESH)
    pl.set_row_mask(W.copy())
    pl.solver_reset(B.copy(), mu)
    pl.solver_step(64)
    x64 = pl.solver_x()
    for use_graph in (True, False):
        pl.solver_reset(B.copy(), mu, use_graph=use_graph, x0=pl.solver_x_device())
        rec = snapshot(pl)
        assert np.array_equal(rec["x"], x64) and np.all(rec["drift"] == 0.0) and np.array_equal(rec["R"], rec["r"])
    get = reference_certs(Ab, b, W, mu, x64)
    for c in range(k):
        np.testing.assert_allclose(rec["R"][c], get("r")[c], rtol=1e-11, atol=1e-12 * np.abs(get("r")[c]).max())
    stats = {}
    bad, snaps, _ = stepped(pl, Ab, B, mu, W, 1, t0_warm=1, steps=3, x0=x64, stats=stats)
    print(f"warm intercept steps {(m, n, k)}: worst ratio to bound "
          + " ".join(f"{c} {stats[c]:.3g}" for c in ("A", "B", "C", "D", "0")))
    assert np.array_equal(snaps[0][0], x64) and not bad, bad


# ---------------------------------------------------------------------------
# 5. the trajectory is the one of the row-deleted, explicitly centred problem
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k,fuse_grid", SHAPES)
def test_trajectory(m, n, k, fuse_grid):
    Ab, b, B, W, mu = problem(m, n, k)
    T = 256
    pl = make(m, n, k, fuse_grid)
    pl.set_row_mask(W.copy())
    pl.solver_reset(B.copy(), mu)
    pl.solver_step(T)
    X = pl.solver_x()
    dg = C.centred_diag(Ab)                              # the device's diag: one d for every fold
    dg1 = np.where(dg > 0, dg, 1.0)
    worst_x = worst_f = 0.0
    nm = k // 4
    # every column at k = 16; at k = 128 one column per fold, at the smallest mu and two inside the grid
    cols = range(k) if k == 16 else [f * nm + j for f, j in enumerate((nm - 1, 2 * nm // 3, nm // 3, nm - 1))]
    for c in cols:
        rows = W[:, c] != 0
        Ai, bi = Ab[rows] - Ab[rows].mean(axis=0), b[rows] - b[rows].mean()
        ref = C.masked_panel_iterate(Ai, bi, np.ones(int(rows.sum())), mu[c], 1, T, diag=dg1)["x"]
        obj = lambda x: 0.5 * float((Ai @ x - bi) @ (Ai @ x - bi)) + mu[c] * float(np.abs(x).sum())  # noqa: E731
        assert np.linalg.norm(X[:, c] - ref) <= 1e-2 * np.linalg.norm(ref), c
        if ref.any():
            worst_x = max(worst_x, np.linalg.norm(X[:, c] - ref) / np.linalg.norm(ref))
        worst_f = max(worst_f, abs(obj(X[:, c].copy()) - obj(ref)) / obj(ref))
    print(f"intercept panel {m}x{n} k{k}: worst rel x {worst_x:.2e}, worst rel objective {worst_f:.2e}")
    assert worst_f <= 1e-4
    # exact line search along the direction taken: the profiled objective never increases
    pl.solver_reset(B.copy(), mu, use_graph=False)
    objs = [pl.duality_gap(screen=False)["primal"]]
    for _ in range(4):
        pl.solver_step(16)
        objs.append(pl.duality_gap(screen=False)["primal"])
    objs = np.array(objs)
    assert np.all(objs[1:] <= objs[:-1] * (1 + 1e-12)) and np.any(objs[-1] < objs[0])


# ---------------------------------------------------------------------------
# 6. degenerate data: a constant column of A, an all-zero mask column
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k,fuse_grid", [TWO_KERNEL, FUSED_G1])
def test_constant_column_and_empty_mask(m, n, k, fuse_grid):
    Ab, b, B, W, mu = problem(m, n, k)
    A2 = Ab.copy()
    A2[:, 7] = A2[0, 7]
    A2[:, 300] = 0.0
    W2 = W.copy()
    W2[:, 3] = 0
    pl = make(m, n, k, fuse_grid, Ab=A2)
    pl.set_row_mask(W2.copy())
    d = pl.diag_ATA.reshape(-1)
    assert d[7] == 0.0 and d[300] == 0.0 and np.all(np.delete(d, [7, 300]) > 0)
    for use_graph in (True, False):
        pl.solver_reset(B.copy(), mu, use_graph=use_graph)
        for t in (16, 64):
            pl.solver_step(t if t == 16 else 48)
            rec = snapshot(pl, t)
            for key in SCALARS + ("x", "g", "r", "R"):
                assert np.all(np.isfinite(rec[key])), key
            assert not rec["x"][[7, 300]].any() and rec["x"].any()
            assert not rec["x"][:, 3].any() and not rec["R"][3].any() and not rec["g"][3].any()
            for key in ("primal", "dual", "gap", "drift", "intercept"):
                assert rec[key][3] == 0.0, key
            assert abs(rec["holdout_sse"][3] - b @ b) <= 1e-9 * (b @ b)
            ref = C.intercept_duality_gap(A2, b, W2[:, 9], rec["x"][:, 9].copy(), mu[9])
            for key in ("primal", "dual", "scale", "gnorm_inf", "holdout_sse", "intercept"):
                assert abs(rec[key][9] - ref[key]) <= 1e-9 * abs(ref[key]), key


# ---------------------------------------------------------------------------
# 7. cross-validation with the intercept
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_best(m, n):
    """argmin over mu of the mean over folds of the held-out mse of the fp64 restatement run to 1024 iterations"""
    Ab, b, _, _, _, masks, mus = offset_instance(m, n)
    mse = np.zeros((masks.shape[0], mus.size))
    for f in range(masks.shape[0]):
        for j in range(mus.size):
            x = C.intercept_panel_iterate(Ab, b, masks[f], mus[j], 1024)["x"]
            mse[f, j] = C.intercept_duality_gap(Ab, b, masks[f], x, mus[j])["holdout_sse"] / (masks[f] == 0).sum()
    return int(np.argmin(mse.mean(axis=0))), mse.mean(axis=0)


def test_lasso_cv_fit_intercept():
    m, n, nf, nm, bound = 256, 512, 4, 4, 1e-4
    Ab, b, _, W, mu_cols, masks, mus = offset_instance(m, n)
    T = cv_t_ref(m, n, bound)
    assert T == 128
    kw = dict(GAP_BOUND=bound, ITER_MAX=4 * T, check_every=64, device=0)
    res = panel.lasso_cv(Ab, b, mus=mus, masks=masks, return_x=True, fit_intercept=True, **kw)
    plain = panel.lasso_cv(Ab, b, mus=mus, masks=masks, refit=False, **kw)
    best_ref, mean_ref = reference_best(m, n)
    print(f"lasso_cv fit_intercept {m}x{n}: T_ref {T}, device iters {res['iters']}, mean mse {res['mean_mse']} "
          f"(fp64 reference {mean_ref}), without the intercept {plain['mean_mse']}, best {res['best']}, "
          f"refit iters {res['refit_iters']}, intercept {res['intercept']}")
    assert np.all(res["reached"]) and res["iters"] <= 4 * T and res["iters"] % 64 == 0
    assert res["intercept_folds"].shape == (nf, nm) and res["intercept"].shape == (nm,) and res["x"].shape == (n, nm)
    count = (masks == 0).sum(axis=1)
    for f in range(nf):
        wf = masks[f].astype(np.float64)
        pb = wf * (b - (wf @ b) / wf.sum())
        target = bound * 0.5 * float(pb @ pb)
        for j in range(nm):
            cert = C.intercept_duality_gap(Ab, b, masks[f], res["x_folds"][:, f, j].copy(), mus[j])
            assert abs(res["mse"][f, j] * count[f] - cert["holdout_sse"]) <= 1e-9 * cert["holdout_sse"]
            assert abs(res["intercept_folds"][f, j] - cert["intercept"]) <= 1e-9 * abs(cert["intercept"])
            assert abs(res["gap"][f, j] - cert["gap"]) <= 1e-9 * cert["primal"]
            assert cert["gap"] <= target and res["gap"][f, j] <= target
    assert res["best"] == best_ref
    # (on the fp64 restatement 0.21 against 0.62 at the smallest mu: n > m and a dense x0, so no model
    # predicts the held-out rows well, but the one without an intercept is three times worse)
    assert res["mean_mse"].min() < plain["mean_mse"].min()
    # the refit is lasso_path(fit_intercept=True) on the same grid, on the context that ran the folds
    path = panel.lasso_path(Ab, b, mus=mus, fit_intercept=True, **kw)
    assert np.array_equal(res["x"], path["x"]) and np.array_equal(res["refit_gap"], path["gap"])
    assert np.array_equal(res["intercept"], path["intercept"]) and res["refit_iters"] == path["iters"]
    ones = np.ones(m)
    for j in range(nm):
        cert = C.intercept_duality_gap(Ab, b, ones, path["x"][:, j].copy(), mus[j])
        assert abs(path["intercept"][j] - cert["intercept"]) <= 1e-9 * abs(cert["intercept"])
    # mus=None takes the grid off the certificate at x = 0 with the intercept on: || A^T (b - mean b) ||_inf
    # ... and the warm refit starts from the folds' mean
    auto = panel.lasso_cv(Ab, b, n_folds=nf, n_mus=nm, seed=7, fit_intercept=True, warm_refit=True, **kw)
    np.testing.assert_allclose(auto["mus"], mus, rtol=1e-9)
    bc = b - b.mean()
    assert np.all(auto["reached"]) and np.all(auto["refit_gap"] <= bound * 0.5 * float(bc @ bc))
    assert auto["refit_iters"] <= res["refit_iters"]
    np.testing.assert_allclose(auto["intercept"], res["intercept"], rtol=1e-3)
    with pytest.raises(ValueError):
        panel.lasso_cv(Ab, b, mus=mus, masks=masks, Block=2, fit_intercept=True, device=0)
    with pytest.raises(ValueError):
        panel.lasso_path(Ab, b, mus=mus, Block=2, fit_intercept=True, device=0)


# ---------------------------------------------------------------------------
# 8. the path with the intercept and gap-safe compaction
# ---------------------------------------------------------------------------
def test_lasso_path_fit_intercept_shrink():
    Ab, b, mus = sparse_offset_instance()
    n = Ab.shape[1]
    bound = 3e-6
    kw = dict(mus=mus, GAP_BOUND=bound, ITER_MAX=512, check_every=64, device=0, fit_intercept=True)
    plain = panel.lasso_path(Ab, b, **kw)
    res = panel.lasso_path(Ab, b, shrink=0.75, **kw)
    rel = np.linalg.norm(res["x"] - plain["x"]) / np.linalg.norm(plain["x"])
    bc = b - b.mean()
    print(f"lasso_path fit_intercept shrink: compactions {res['compactions']}, iters {res['iters']} "
          f"(plain {plain['iters']}), full-A rel gap {(res['gap'] / (0.5 * bc @ bc)).max():.2e}, x against shrink=0 {rel:.2e}")
    assert plain["compactions"] == [] and np.all(plain["reached"])
    assert res["compactions"] and res["active"].size < n and np.all(res["reached"])
    assert np.all(res["n_keep"] == n)                   # the certificate of the final x on the full A
    ones = np.ones(Ab.shape[0])
    for j in range(mus.size):
        cert = C.intercept_duality_gap(Ab, b, ones, res["x"][:, j].copy(), mus[j])
        assert abs(res["gap"][j] - cert["gap"]) <= 1e-9 * cert["primal"]
        assert abs(res["intercept"][j] - cert["intercept"]) <= 1e-9 * abs(cert["intercept"])
        assert cert["gap"] <= bound * 0.5 * float(bc @ bc) * (1 + 1e-9)


# ---------------------------------------------------------------------------
# 9. errors
# ---------------------------------------------------------------------------
def test_intercept_errors():
    m, n, k, _ = TWO_KERNEL
    Ab, b, B, W, mu = problem(m, n, k)
    L = panel._lib()
    assert L.bpgl_panel_set_intercept(None, 1) == -1
    raw = ctypes.c_void_p()
    assert L.bpgl_panel_create(ctypes.byref(raw), 0, m, n, 1, 16, 0, None) == 0
    assert L.bpgl_panel_set_intercept(raw, 1) == -2            # before bpgl_panel_bind
    assert "bpgl_panel_bind" in L.bpgl_last_error().decode()
    out = (ctypes.c_double * 16)()
    assert L.bpgl_panel_intercept(raw, out) == -2
    L.bpgl_panel_destroy(raw)
    # two feature blocks, and the undeferred x update: not built
    p2 = PanelLasso(Ab.copy(), 2, nrhs=k, device=0)
    p2.set_intercept(True)
    with pytest.raises(N.BpglError, match=r"\(-2\): .*one feature block"):
        p2.solver_reset(B.copy(), mu)
    pl = make(m, n, k, None, intercept=False)
    pl.set_tuning("defer_x", 0)
    pl.set_intercept(True)
    with pytest.raises(N.BpglError, match=r"\(-2\): .*defer_x"):
        pl.solver_reset(B.copy(), mu)
    pl.set_tuning("defer_x", 1)
    pl.solver_reset(B.copy(), mu)
    with pytest.raises(N.BpglError, match=r"\(-2\): .*bpgl_panel_gap"):     # no certificate since the reset
        N.check(L.bpgl_panel_intercept(pl._ctx, out), "bpgl_panel_intercept")
    pl.solver_step(8)
    assert np.all(pl.duality_gap()["intercept"] != 0.0)
    for on in (False, True):                                   # either way invalidates the solver
        pl.set_intercept(on)
        with pytest.raises(N.BpglError, match=r"\(-2\): .*bpgl_panel_reset"):
            pl.solver_step(1)
        with pytest.raises(N.BpglError, match=r"\(-2\): .*bpgl_panel_reset"):
            pl.duality_gap()
    pl.set_intercept(False)
    pl.solver_reset(B.copy(), mu)
    pl.solver_step(8)
    assert np.all(pl.duality_gap()["intercept"] == 0.0)


# ---------------------------------------------------------------------------
# 10. switching the intercept off restores the unmasked run, bitwise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("m,n,k,fuse_grid", [TWO_KERNEL, FUSED_G2])
def test_intercept_off_is_the_plain_run(m, n, k, fuse_grid, use_graph):
    Ab, b, B, W, mu = problem(m, n, k)
    T = 64

    def run(pl):
        pl.solver_reset(B.copy(), mu, record_len=T, use_graph=use_graph)
        pl.solver_step(T)
        rec = snapshot(pl, T)
        rec["err_iter"] = pl._err_iter.cpu().numpy().copy()
        rec["diag"] = pl.diag_ATA.copy()
        return rec

    base = run(make(m, n, k, fuse_grid, intercept=False))
    pl = make(m, n, k, fuse_grid)
    on = run(pl)
    assert not np.array_equal(on["x"], base["x"]) and not np.array_equal(on["diag"], base["diag"])
    pl.set_intercept(False)
    same_bits(base, run(pl))
    assert np.all(base["intercept"] == 0.0) and np.all(base["holdout_sse"] == 0.0)

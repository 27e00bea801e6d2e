"""GPU tests of the panel's non-negative lasso (``PanelLasso.set_positive``, bpgl_panel_set_positive, ABI 308;
``lasso_path`` / ``lasso_cv`` with ``positive``).

Instance: ``panel_step_reference.instance(m, n, k)`` (seed 0) -- x_true has both signs, so the unconstrained
solution has >= 21 negative coordinates per column and the constrained one >= 25 positive ones (asserted from the
fp64 reference in ``reference``), and the towards-zero rule of the direction image fires thousands of times in
the 18 checked iterations (asserted from the checker's count of the coordinates where it can).  The intercept
cases run on ``panel_intercept_instance.offset_instance``.  Shapes (m, n, k, Block), the smallest at which each
form runs:

    256 x 512, k 16, Block 1     two-kernel update
    256 x 512, k 16, Block 2     k_panel_update
    256 x 256, k 128             the widest RHS tiling of the epilogue (the LDS-staged form)
    1024 x 512, k 16             fused update
    2048 x 512, k 16             fused update, G 2

References, numpy fp64 on the stored bf16 A: ``check_step_positive`` (A-D, P1, P2; proved against a model and
its mutants in tests/test_panel_positive_host.py), ``positive_duality_gap`` at tests/test_panel_cv.py's certificate
bounds, ``positive_panel_iterate`` at test_masked_trajectory's bounds.  Graphs and eager launches agree bitwise.

Measured on the MI355X over all cases: worst ratio to bound of the step checks A 0.37, B 0.29, C 0.98 (no margin
by construction: the image's own rounding), D 0.23, 0' 0.011; the towards-zero rule can fire on 8168 to 9490
coordinates over the 18 iterations at 256 x 512; min x exactly 0 at every one of 32 snapshots of 256 iterations, drift
6.2e-7 (d_split 1) and 6.8e-7 (d_split 2), 0.0058 and 0.0037 of ``drift_bound`` (5.6e-5 to 2.9e-4 at t = 256); the certificate's gap within 9.3e-15 of the primal, max_j g_j up to 5.2 mu
(what a two-sided certificate would have scaled by); after 256 iterations x within 4.8e-6 and the objective within
8.4e-11 of ``positive_panel_iterate`` and 0.54 to 0.66 from the unconstrained reference; ``lasso_path`` stops at 64
with 1 nonzero at the largest mu and 189 at the smallest; with ``shrink=0.75`` it compacts 2048 -> 1536 -> 512 -> 256
(t = 64, 128, 192), stops at 256 as without, and returns x within 1.4e-6 of ``shrink=0``.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import panel_positive_reference as R  # noqa: E402
import panel_step_reference as P  # noqa: E402
from convex_optimization_amd import _native as N  # noqa: E402
from convex_optimization_amd import cpu_calculation as C  # noqa: E402
from convex_optimization_amd import panel  # noqa: E402
from convex_optimization_amd.panel import PanelLasso  # noqa: E402
from panel_intercept_instance import offset_instance  # noqa: E402
from panel_screen_reference import screen_instance  # noqa: E402

T_STEPS = 18
G_REFRESH = 8
# (m, n, k, Block)
TWO_KERNEL, MULTI, WIDE, FUSED_G1, FUSED_G2 = (256, 512, 16, 1), (256, 512, 16, 2), (256, 256, 128, 1), \
    (1024, 512, 16, 1), (2048, 512, 16, 1)
SHAPES = [TWO_KERNEL, MULTI, WIDE, FUSED_G1, FUSED_G2]
SCALARS = ("primal", "dual", "gap", "scale", "gnorm_inf", "n_keep", "drift", "holdout_sse", "intercept")
WORST = {}


@functools.lru_cache(maxsize=None)
def problem(m, n, k):
    Ab, B, mu = P.instance(m, n, k)
    W = P.fold_mask(m, k)
    for a in (Ab, B, mu, W):
        a.setflags(write=False)
    return Ab, B, mu, W


@functools.lru_cache(maxsize=None)
def reference(m, n, k, Block, T=256):
    """Per column the fp64 constrained iterate after T iterations and the unconstrained one; the instance is
    informative: >= 21 negative coordinates without the constraint, >= 25 positive ones with it."""
    Ab, B, mu, _ = problem(m, n, k)
    cols = range(k) if k == 16 else (0, k // 3, 2 * k // 3, k - 1)
    pos = {c: C.positive_panel_iterate(Ab, B[:, c], None, mu[c], Block, T)["x"] for c in cols}
    unc = {c: C.masked_panel_iterate(Ab, B[:, c], np.ones(m), mu[c], Block, T)["x"] for c in cols}
    for c in cols:
        assert (unc[c] < 0).sum() >= 21, (c, int((unc[c] < 0).sum()))
        assert (pos[c] > 0).sum() >= 25 and np.all(pos[c] >= 0), (c, int((pos[c] > 0).sum()))
    return pos, unc


def make(m, n, k, Block, positive=True, Ab=None, **tuning):
    pl = PanelLasso((problem(m, n, k)[0] if Ab is None else Ab).copy(), Block, nrhs=k, device=0)
    for key, v in tuning.items():
        pl.set_tuning(key, v)
    if positive:
        pl.set_positive(True)
    assert pl.get_tuning("positive") == int(positive)
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


# ---------------------------------------------------------------------------
# 1. every iteration is the constrained algorithm's step
# ---------------------------------------------------------------------------
def run_steps(m, n, k, Block, d_split, carry, defer_x, variant, use_graph=True):
    if variant == "intercept":
        Ab, _, B, W, mu = offset_instance(m, n, 4, k // 4)[:5]
    else:
        Ab, B, mu, W = problem(m, n, k)
    W = None if variant == "plain" else W
    icpt = variant == "intercept"
    pl = make(m, n, k, Block, Ab=Ab, d_split=d_split)
    if Block == 1:
        pl.set_tuning("carry_g", carry)
        pl.set_tuning("g_refresh", G_REFRESH)
        pl.set_tuning("defer_x", defer_x)
    if icpt:
        pl.set_intercept(True)
    if W is not None:
        pl.set_row_mask(W.copy())
    carried = pl.get_tuning("carry_g") == 1
    assert carried == (Block == 1 and carry == 1) and pl.get_tuning("positive") == 1
    assert pl.get_tuning("fuse_update") == int(m % 1024 == 0 and Block == 1 and defer_x == 1)
    diag = pl.diag_ATA
    chain = d_split * (n // Block // pl.kchunks)
    pl.solver_reset(B.copy(), mu, record_len=T_STEPS, use_graph=use_graph)
    snaps, errs, stats, bad = [P.snapshot(pl)], [], {}, []
    for t in range(T_STEPS):
        pl.solver_step(1)
        snaps.append(P.snapshot(pl))
        errs.append(float(pl._err_iter.cpu().numpy()[t]))
        assert pl.solver_status()["iters"] == t + 1
        q = t % G_REFRESH if carried else 0
        exact = not carried or q == 0
        viol = R.check_step_positive(Ab, diag.reshape(-1) if icpt else diag, mu, W, t % Block, snaps[t], snaps[t + 1],
                                     errs[t], d_split, exact, None if exact else snaps[t][1] - snaps[t - 1][1],
                                     chain=chain, q=q, R_ref=None if exact else snaps[t - q][1], stats=stats,
                                     intercept=icpt, B=B, t=t)
        bad += [(t, v) for v in viol]
    line = " ".join(f"{c} {stats[c]:.3g}" for c in ("A", "B", "C", "D") + (("0",) if icpt else ()))
    for c in stats:
        if c in ("A", "B", "C", "D", "0"):
            WORST[c] = max(WORST.get(c, 0.0), stats[c])
    print(f"positive step {(m, n, k, Block)} d_split={d_split} carry={carry} defer_x={defer_x} {variant}: worst ratio to "
          f"bound {line}, rule can fire on {stats['fire']} coordinates, min x {stats['x_min']}, gamma in "
          f"[{stats['gamma_min']:.3g}, {stats['gamma_max']:.3g}]; so far " + " ".join(f"{c} {v:.3g}" for c, v in WORST.items()))
    assert not bad, bad
    assert stats["x_min"] >= 0.0
    if variant == "plain":
        assert stats["fire"] >= 2000, stats["fire"]        # the instance exercises the towards-zero rule
    assert pl.stat("exact_gradients") == (3 if carried else 0)
    # the same eighteen iterations in one call, graphs replayed (x deferred into the epilogues) and eager: bitwise
    for ug in (True, False):
        pl.solver_reset(B.copy(), mu, record_len=T_STEPS, use_graph=ug)
        pl.solver_step(T_STEPS)
        x, Rr = P.snapshot(pl)
        assert np.array_equal(x, snaps[-1][0]) and np.array_equal(Rr, snaps[-1][1]), ug
        assert pl._err_iter.cpu().numpy().tobytes() == np.array(errs).tobytes()


@pytest.mark.parametrize("variant", ["plain", "masked"])
@pytest.mark.parametrize("carry,defer_x", [(1, 1), (0, 1), (1, 0), (0, 0)])
@pytest.mark.parametrize("d_split", [1, 2])
@pytest.mark.parametrize("m,n,k,Block", [TWO_KERNEL, WIDE, FUSED_G1, FUSED_G2])
def test_one_block_steps(m, n, k, Block, d_split, carry, defer_x, variant):
    run_steps(m, n, k, Block, d_split, carry, defer_x, variant)


@pytest.mark.parametrize("variant", ["plain", "masked"])
@pytest.mark.parametrize("d_split", [1, 2])
def test_multi_block_steps(d_split, variant):
    m, n, k, Block = MULTI
    run_steps(m, n, k, Block, d_split, 0, 0, variant)


@pytest.mark.parametrize("carry", [1, 0])
@pytest.mark.parametrize("d_split", [1, 2])
@pytest.mark.parametrize("m,n,k,Block", [TWO_KERNEL, FUSED_G1, FUSED_G2])
def test_intercept_steps(m, n, k, Block, d_split, carry):
    run_steps(m, n, k, Block, d_split, carry, 1, "intercept")


# ---------------------------------------------------------------------------
# 2. the invariant over a longer run
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("d_split", [1, 2])
def test_invariant_over_256_iterations(d_split):
    """256 iterations in graph replays of 8, a certificate and a snapshot after each: min x >= 0 exactly, and the
    certificate's drift within ``drift_bound`` -- the sum of check A's per-step bound over the run, from every
    iterate, which a first run of the same 256 iterations, launched one by one, records (the two runs agree bitwise
    at the snapshots)."""
    m, n, k, Block = TWO_KERNEL
    Ab, B, mu, _ = problem(m, n, k)
    pl = make(m, n, k, Block, d_split=d_split)
    pl.solver_reset(B.copy(), mu, use_graph=False)
    xs = [pl.solver_x()]
    for _ in range(256):
        pl.solver_step(1)
        xs.append(pl.solver_x())
    chain = d_split * (n // pl.kchunks)
    pl.solver_reset(B.copy(), mu)
    drift, xmin, worst = 0.0, np.inf, 0.0
    for t in range(8, 257, 8):
        pl.solver_step(8)
        cert = pl.duality_gap(screen=False)
        x = pl.solver_x()
        assert np.array_equal(x, xs[t]), t
        xmin = min(xmin, float(x.min()))
        assert np.all(x >= 0.0), (t, float(x.min()))
        bound = R.drift_bound(Ab, xs[:t + 1], chain, np.abs(B).max())
        drift = max(drift, float(cert["drift"].max()))
        worst = max(worst, float((cert["drift"] / bound).max()))
        assert np.all(cert["drift"] <= bound), (t, cert["drift"], bound)
    print(f"positive invariant d_split={d_split}: min x over 32 snapshots {xmin}, worst drift {drift:.3g}, worst ratio to "
          f"drift_bound {worst:.3g} (bound at t = 256: {bound.min():.3g} to {bound.max():.3g})")
    assert xmin == 0.0


# ---------------------------------------------------------------------------
# 3. the certificate against the numpy restatement on the device's own x; repeatable
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k,Block,variant", [s + (v,) for s in SHAPES for v in ("plain", "masked", "intercept")
                                                 if v != "intercept" or s[3] == 1])
def test_certificate_matches_numpy(m, n, k, Block, variant):
    if variant == "intercept":
        Ab, _, B, W, mu = offset_instance(m, n, 4, k // 4)[:5]
    else:
        Ab, B, mu, W = problem(m, n, k)
    icpt = variant == "intercept"
    pl = make(m, n, k, Block, Ab=Ab)
    if icpt:
        pl.set_intercept(True)
    if variant != "plain":
        pl.set_row_mask(W.copy())
    Wn = np.ones((m, k), dtype=np.uint8) if variant == "plain" else W
    pl.solver_reset(B.copy(), mu)
    diag = pl.diag_ATA.reshape(-1)
    recs = [snapshot(pl, 0)]
    pl.solver_step(64)
    recs.append(snapshot(pl, 64))
    same_bits(recs[-1], snapshot(pl, 64))
    for rec in recs:
        ref = [C.positive_duality_gap(Ab, B[:, c], Wn[:, c], rec["x"][:, c].copy(), mu[c], diag=diag, intercept=icpt)
               for c in range(k)]
        get = lambda key: np.array([r[key] for r in ref])  # noqa: E731
        keys = ("primal", "dual", "scale", "gnorm_inf") + (("holdout_sse",) if variant != "plain" else ()) \
            + (("intercept",) if icpt else ())
        for key in keys:
            assert np.all(np.abs(rec[key] - get(key)) <= 1e-9 * np.abs(get(key))), key
        assert np.all(np.abs(rec["gap"] - get("gap")) <= 1e-9 * get("primal"))
        g_ref, r_ref = get("g"), get("r")
        for c in range(k):
            np.testing.assert_allclose(rec["g"][c], g_ref[c], rtol=1e-11, atol=1e-12 * np.abs(g_ref[c]).max())
            np.testing.assert_allclose(rec["r"][c], r_ref[c], rtol=1e-11, atol=1e-12 * np.abs(r_ref[c]).max())
        score, keep = get("score"), get("keep")
        clear = np.abs(score - mu[:, None]) > 1e-9 * mu[:, None]
        assert (~clear).sum() <= 0.001 * k * n
        assert np.array_equal(rec["keep"][clear], keep[clear])
        assert np.array_equal(rec["n_keep"], rec["keep"].sum(axis=1))
        assert np.array_equal(rec["gnorm_inf"], np.maximum(-rec["g"], 0.0).max(axis=1))
        # one-sided: it differs from the two-sided certificate (some g_j > mu is allowed)
        print(f"positive certificate {(m, n, k, Block)} {variant} t={rec['t']}: gap err / primal "
              f"{np.max(np.abs(rec['gap'] - get('gap')) / get('primal')):.2e}, drift {rec['drift'].max():.2e}, "
              f"n_keep {rec['n_keep'].min()}..{rec['n_keep'].max()}, max g / mu {(rec['g'].max(axis=1) / mu).max():.2f}")
    assert np.all(recs[1]["x"] >= 0) and recs[1]["x"].any()
    assert (recs[1]["g"].max(axis=1) > mu).any()           # a two-sided certificate would scale by this


# ---------------------------------------------------------------------------
# 4. the trajectory is the constrained one, and not the unconstrained one
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k,Block", SHAPES)
def test_trajectory(m, n, k, Block):
    Ab, B, mu, _ = problem(m, n, k)
    T = 256
    pos, unc = reference(m, n, k, Block, T)
    pl = make(m, n, k, Block)
    pl.solver_reset(B.copy(), mu)
    pl.solver_step(T)
    X = pl.solver_x()
    assert np.all(X >= 0.0)
    wx = wf = 0.0
    far = np.inf
    for c, ref in pos.items():
        obj = lambda x: 0.5 * float((Ab @ x - B[:, c]) @ (Ab @ x - B[:, c])) + mu[c] * float(np.abs(x).sum())  # noqa: E731
        wx = max(wx, np.linalg.norm(X[:, c] - ref) / np.linalg.norm(ref))
        wf = max(wf, abs(obj(X[:, c].copy()) - obj(ref)) / obj(ref))
        far = min(far, np.linalg.norm(X[:, c] - unc[c]) / np.linalg.norm(unc[c]))
    print(f"positive trajectory {(m, n, k, Block)}: worst rel x {wx:.2e}, worst rel objective {wf:.2e}, "
          f"nearest to the unconstrained reference {far:.2f}")
    assert wx <= 1e-2 and wf <= 1e-4
    assert far > 1e-1


# ---------------------------------------------------------------------------
# 5. warm start: max(X0, 0), drift 0, bitwise X0 when X0 >= 0
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k,Block", [TWO_KERNEL, MULTI, FUSED_G2])
def test_warm_start_projects(m, n, k, Block):
    Ab, B, mu, _ = problem(m, n, k)
    pl = make(m, n, k, Block)
    X0 = np.random.RandomState(1).randn(n, k).astype(np.float32) * (np.random.RandomState(2).rand(n, k) < 0.3)
    assert (X0 < 0).sum() > 100
    Xp = np.maximum(X0, 0.0).astype(np.float64)
    for use_graph in (True, False):
        pl.solver_reset(B.copy(), mu, use_graph=use_graph, x0=X0)
        rec = snapshot(pl)
        assert np.array_equal(rec["x"], Xp)
        if Block == 1:
            assert np.all(rec["drift"] == 0.0) and np.array_equal(rec["R"], rec["r"])
        else:
            assert np.all(rec["drift"] <= 1e-12 * np.abs(rec["r"]).max())
        np.testing.assert_allclose(rec["R"], (Ab @ Xp - B).T, rtol=1e-11, atol=1e-12 * np.abs(B).max())
    pl.solver_reset(B.copy(), mu, x0=Xp)                    # X0 >= 0: bitwise X0
    assert np.array_equal(pl.solver_x(), Xp)
    pl.solver_step(16)
    x16 = pl.solver_x()
    assert np.all(x16 >= 0) and not np.array_equal(x16, Xp)
    if Block == 1:                                          # the in-place restart from the stored iterate
        pl.solver_reset(B.copy(), mu, x0=pl.solver_x_device())
        rec = snapshot(pl)
        assert np.array_equal(rec["x"], x16) and np.all(rec["drift"] == 0.0)
    # without the constraint a warm start keeps its negative entries
    pl.set_positive(False)
    pl.solver_reset(B.copy(), mu, x0=X0)
    assert np.array_equal(pl.solver_x(), X0.astype(np.float64))


# ---------------------------------------------------------------------------
# 6. off is off
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("m,n,k,Block", [TWO_KERNEL, MULTI, WIDE, FUSED_G2])
def test_positive_off_is_the_plain_run(m, n, k, Block, use_graph):
    Ab, B, mu, _ = problem(m, n, k)
    T = 32

    def run(pl):
        pl.solver_reset(B.copy(), mu, record_len=T, use_graph=use_graph)
        pl.solver_step(T)
        rec = snapshot(pl, T)
        rec["err_iter"] = pl._err_iter.cpu().numpy().copy()
        return rec

    base = run(make(m, n, k, Block, positive=False))
    pl = make(m, n, k, Block)
    on = run(pl)
    assert np.all(on["x"] >= 0) and (base["x"] < 0).any() and not np.array_equal(on["x"], base["x"])
    pl.set_positive(False)
    with pytest.raises(N.BpglError, match=r"\(-2\): .*bpgl_panel_reset"):      # a reset must follow
        pl.solver_step(1)
    same_bits(base, run(pl))


def test_positive_errors():
    m, n, k, _ = TWO_KERNEL
    L = panel._lib()
    assert L.bpgl_version() >= 308
    assert L.bpgl_panel_set_positive(None, 1) == -1
    raw = ctypes.c_void_p()
    assert L.bpgl_panel_create(ctypes.byref(raw), 0, m, n, 1, 16, 0, None) == 0
    assert L.bpgl_panel_set_positive(raw, 1) == -2             # before bpgl_panel_bind
    assert "bpgl_panel_bind" in L.bpgl_last_error().decode()
    L.bpgl_panel_destroy(raw)
    Ab, B, mu, _ = problem(m, n, k)
    pl = make(m, n, k, 1, positive=False)
    pl.solver_reset(B.copy(), mu)
    pl.solver_step(8)
    for on in (True, False):
        pl.set_positive(on)
        with pytest.raises(N.BpglError, match=r"\(-2\): .*bpgl_panel_reset"):
            pl.duality_gap()
        pl.solver_reset(B.copy(), mu)
        assert pl.get_tuning("positive") == int(on)


# ---------------------------------------------------------------------------
# 7. the drivers
# ---------------------------------------------------------------------------
def test_lasso_path_positive():
    m, n = 256, 512
    Ab, B, _, _ = problem(m, n, 16)
    b = B[:, 0].copy()
    bound = 1e-4
    res = panel.lasso_path(Ab, b, n_mus=16, positive=True, GAP_BOUND=bound, ITER_MAX=2048, check_every=64, device=0)
    nnz = (res["x"] > 0).sum(axis=0)
    print(f"lasso_path positive: iters {res['iters']}, mu_max {res['mu_max']:.6g}, nonzeros {nnz.tolist()}, "
          f"rel gap {(res['gap'] / (0.5 * b @ b)).max():.2e}")
    assert np.all(res["reached"]) and np.all(res["gap"] <= bound * 0.5 * float(b @ b))
    assert np.all(res["x"] >= 0.0)
    mu_max = float(np.max(Ab.T @ b))
    assert mu_max > 0 and abs(res["mu_max"] - mu_max) <= 1e-12 * mu_max
    np.testing.assert_allclose(res["mus"], C.mu_grid(mu_max, 16), rtol=1e-12)
    assert nnz[0] < nnz[-1]                                 # the largest mu is the sparsest
    for j in (0, 7, 15):
        cert = C.positive_duality_gap(Ab, b, None, res["x"][:, j].copy(), res["mus"][j])
        assert abs(cert["gap"] - res["gap"][j]) <= 1e-9 * cert["primal"]
    # no column correlates positively with b: ValueError, not a grid of zeros
    with pytest.raises(ValueError, match="positive"):
        panel.lasso_path(np.abs(Ab), -np.abs(b) - 1.0, n_mus=4, positive=True, device=0)
    # lasso_path's own check without the flag still passes on that data (mu_max = ||A^T b||_inf > 0)
    assert panel.lasso_path(np.abs(Ab), -np.abs(b) - 1.0, n_mus=4, ITER_MAX=64, check_every=64, device=0)["mu_max"] > 0


def test_lasso_path_positive_shrink():
    Ab, b, _, _, _ = screen_instance()
    n = Ab.shape[1]
    bound = 3e-6
    mus = C.mu_grid(float(np.max(Ab.T @ b)), 16, 0.9, 0.1)
    kw = dict(mus=mus, GAP_BOUND=bound, ITER_MAX=4096, check_every=64, device=0, positive=True)
    plain = panel.lasso_path(Ab, b, **kw)
    res = panel.lasso_path(Ab, b, shrink=0.75, **kw)
    rel = np.linalg.norm(res["x"] - plain["x"]) / np.linalg.norm(plain["x"])
    print(f"lasso_path positive shrink: compactions {res['compactions']}, iters {res['iters']} (plain {plain['iters']}), "
          f"x against shrink=0 {rel:.2e}")
    assert plain["compactions"] == [] and np.all(plain["reached"])
    assert res["compactions"] and res["active"].size < n and np.all(res["reached"])
    assert np.all(res["x"] >= 0.0) and np.all(plain["x"] >= 0.0)
    assert rel <= 1e-4
    for j in range(mus.size):
        cert = C.positive_duality_gap(Ab, b, None, res["x"][:, j].copy(), mus[j])
        assert abs(res["gap"][j] - cert["gap"]) <= 1e-9 * cert["primal"]
        assert cert["gap"] <= bound * 0.5 * float(b @ b) * (1 + 1e-9)


@pytest.mark.parametrize("fit_intercept", [False, True])
def test_lasso_cv_positive(fit_intercept):
    m, n, nf, nm = 256, 512, 4, 4
    if fit_intercept:
        Ab, b = offset_instance(m, n)[:2]
    else:
        Ab, B, _, _ = problem(m, n, 16)
        b = B[:, 0].copy()
    res = panel.lasso_cv(Ab, b, n_folds=nf, n_mus=nm, seed=7, positive=True, fit_intercept=fit_intercept,
                         return_x=True, warm_refit=True, GAP_BOUND=1e-4, ITER_MAX=2048, check_every=64, device=0)
    masks, mus = res["masks"], res["mus"]
    print(f"lasso_cv positive fit_intercept={fit_intercept}: iters {res['iters']}, mean mse {res['mean_mse']}, "
          f"best {res['best']}, refit iters {res['refit_iters']}")
    assert np.all(res["reached"]) and np.all(res["x_folds"] >= 0) and np.all(res["x"] >= 0) and res["x"].any()
    bc = b - b.mean() if fit_intercept else b
    np.testing.assert_allclose(mus, C.mu_grid(float(np.max(Ab.T @ bc)), nm), rtol=1e-9)
    count = (masks == 0).sum(axis=1)
    for f in range(nf):
        out = masks[f] == 0
        for j in range(nm):
            x = res["x_folds"][:, f, j]
            b0 = res["intercept_folds"][f, j] if fit_intercept else 0.0
            sse = float(np.square(Ab[out] @ x + b0 - b[out]).sum())
            assert abs(res["mse"][f, j] * count[f] - sse) <= 1e-9 * sse
            cert = C.positive_duality_gap(Ab, b, masks[f], x.copy(), mus[j], intercept=fit_intercept)
            assert abs(res["gap"][f, j] - cert["gap"]) <= 1e-9 * cert["primal"]
            if fit_intercept:
                assert abs(b0 - cert["intercept"]) <= 1e-9 * abs(cert["intercept"])
    # the refit is lasso_path(positive=True) on the same grid; started from the folds' mean it needs no more iterations
    path = panel.lasso_path(Ab, b, mus=mus, positive=True, fit_intercept=fit_intercept, GAP_BOUND=1e-4, ITER_MAX=2048,
                            check_every=64, device=0)
    assert res["refit_iters"] <= path["iters"]
    assert np.linalg.norm(res["x"] - path["x"]) <= 1e-2 * np.linalg.norm(path["x"])

"""GPU tests of the panel's penalty factors (``PanelLasso.set_penalty_factors``, bpgl_panel_set_penalty, ABI 309;
``lasso_path`` / ``lasso_cv`` with ``penalty_factors``).

Instance: ``panel_penalty_reference.instance(m, n, k)`` -- ``panel_step_reference.instance`` with the factors
p_j = exp(u_j), u uniform in [-1, 1], and a second vector of powers of two; tests/test_panel_penalty_host.py shows
that the weighted and the unweighted solutions differ in support on every right-hand side.  The intercept cases
run on ``panel_intercept_instance.offset_instance``.  Shapes (m, n, k, Block), the smallest at which each form runs:

    256 x 512, k 16, Block 1     two-kernel update
    256 x 512, k 16, Block 2     k_panel_update; the per-block offset into p
    256 x 256, k 128             the LDS-staged epilogue (p staged by LDS-DMA)
    1024 x 512, k 16             fused update
    2048 x 512, k 16             fused update, G 2

References, numpy fp64 on the stored bf16 A: ``check_step_penalty`` (proved against a model and its mutants in
tests/test_panel_penalty_host.py), ``penalty_duality_gap`` at 1e-9 relative, ``penalty_panel_iterate`` at the
non-negative lasso's trajectory bounds.  Graphs and eager launches agree bitwise.  The step size has no accessor;
where the issue compares gamma, x and R are compared after every single iteration instead (dx = gamma D',
dR = gamma S).

Measured on the MI355X over all cases (135, 10 s together): worst ratio to bound of the step checks A 0.28, B 0.13,
C 0.98 (no margin by construction: the image's own rounding), D 0.20, 0' 0.011; the certificate's gap within 5e-15 of
the primal, 0 borderline screen entries; after 256 iterations x within 9.3e-6 and the objective within 5.2e-9 of
``penalty_panel_iterate`` and 0.11 to 0.61 from the unweighted reference; ``lasso_path`` stops at 64 with 1 nonzero at
the largest mu and 204 at the smallest; with ``shrink=0.75`` it compacts 2048 -> 512 -> 256 (t = 64, 128), stops at 192
against 256 and returns x within 1.0e-6 of ``shrink=0``.  Power-of-two factors: see the test.
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import panel_penalty_reference as PR  # noqa: E402
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
    Ab, B, mu, pen, pen2 = PR.instance(m, n, k)
    W = P.fold_mask(m, k)
    W.setflags(write=False)
    return Ab, B, mu, pen, pen2, W


@functools.lru_cache(maxsize=None)
def reference(m, n, k, Block, T=256):
    """Per column (four of them at k = 128 and at m >= 1024) the fp64 weighted iterate after T iterations and the unweighted one."""
    Ab, B, mu, pen, _, _ = problem(m, n, k)
    cols = range(k) if k == 16 and m == 256 else (0, k // 3, 2 * k // 3, k - 1)
    wei = {c: C.penalty_panel_iterate(Ab, B[:, c], None, mu[c], pen, Block, T)["x"] for c in cols}
    unw = {c: C.masked_panel_iterate(Ab, B[:, c], np.ones(m), mu[c], Block, T)["x"] for c in cols}
    return wei, unw


def make(m, n, k, Block, pen=None, positive=False, Ab=None, **tuning):
    pl = PanelLasso((problem(m, n, k)[0] if Ab is None else Ab).copy(), Block, nrhs=k, device=0)
    for key, v in tuning.items():
        pl.set_tuning(key, v)
    if positive:
        pl.set_positive(True)
    if pen is not None:
        pl.set_penalty_factors(pen)
    assert pl.get_tuning("penalty") == int(pen is not None) and pl.get_tuning("positive") == int(positive)
    return pl


def snapshot(pl, t=0):
    d = pl.duality_gap()
    rec = {key: d[key].copy() for key in SCALARS}
    rec.update(t=t, x=pl.solver_x(), g=d["g"].cpu().numpy(), r=d["r"].cpu().numpy(), keep=d["keep"].cpu().numpy(),
               R=pl.residual_device().cpu().numpy())
    return rec


def same_bits(a, b, skip=()):
    for key in a:
        if key not in skip:
            assert np.array_equal(a[key], b[key], equal_nan=True), key


# ---------------------------------------------------------------------------
# 1. every iteration is the weighted algorithm's step
# ---------------------------------------------------------------------------
def run_steps(m, n, k, Block, d_split, carry, defer_x, variant, positive):
    if variant == "intercept":
        Ab, _, B, W, mu = offset_instance(m, n, 4, k // 4)[:5]
        pen = PR.factors(n)
    else:
        Ab, B, mu, pen, _, W = problem(m, n, k)
    W = None if variant == "plain" else W
    icpt = variant == "intercept"
    pl = make(m, n, k, Block, pen=pen, positive=positive, Ab=Ab, d_split=d_split)
    if Block == 1:
        pl.set_tuning("carry_g", carry)
        pl.set_tuning("g_refresh", G_REFRESH)
        pl.set_tuning("defer_x", defer_x)
    if icpt:
        pl.set_intercept(True)
    if W is not None:
        pl.set_row_mask(W.copy())
    carried = pl.get_tuning("carry_g") == 1
    assert carried == (Block == 1 and carry == 1) and pl.get_tuning("penalty") == 1
    assert pl.get_tuning("fuse_update") == int(m % 1024 == 0 and Block == 1 and defer_x == 1)
    diag = pl.diag_ATA
    chain = d_split * (n // Block // pl.kchunks)
    pl.solver_reset(B.copy(), mu, record_len=T_STEPS, use_graph=True)
    snaps, errs, stats, bad = [P.snapshot(pl)], [], {}, []
    for t in range(T_STEPS):
        pl.solver_step(1)
        snaps.append(P.snapshot(pl))
        errs.append(float(pl._err_iter.cpu().numpy()[t]))
        assert pl.solver_status()["iters"] == t + 1
        q = t % G_REFRESH if carried else 0
        exact = not carried or q == 0
        viol = PR.check_step_penalty(Ab, diag.reshape(-1) if icpt else diag, mu, pen, W, t % Block, snaps[t], snaps[t + 1],
                                     errs[t], d_split, exact, None if exact else snaps[t][1] - snaps[t - 1][1],
                                     chain=chain, q=q, R_ref=None if exact else snaps[t - q][1], stats=stats,
                                     positive=positive, intercept=icpt, B=B, t=t)
        bad += [(t, v) for v in viol]
    line = " ".join(f"{c} {stats[c]:.3g}" for c in ("A", "B", "C", "D") + (("0",) if icpt else ()))
    for c in stats:
        if c in ("A", "B", "C", "D", "0"):
            WORST[c] = max(WORST.get(c, 0.0), stats[c])
    print(f"penalty step {(m, n, k, Block)} d_split={d_split} carry={carry} defer_x={defer_x} {variant} positive={positive}: "
          f"worst ratio to bound {line}, gamma in [{stats['gamma_min']:.3g}, {stats['gamma_max']:.3g}]; so far "
          + " ".join(f"{c} {v:.3g}" for c, v in WORST.items()))
    assert not bad, bad
    if positive:
        assert stats["x_min"] >= 0.0
    assert snaps[-1][0].any()
    assert pl.stat("exact_gradients") == (3 if carried else 0)
    # the same eighteen iterations in one call, graphs replayed (x deferred into the epilogues) and eager: bitwise
    for ug in (True, False):
        pl.solver_reset(B.copy(), mu, record_len=T_STEPS, use_graph=ug)
        pl.solver_step(T_STEPS)
        x, Rr = P.snapshot(pl)
        assert np.array_equal(x, snaps[-1][0]) and np.array_equal(Rr, snaps[-1][1]), ug
        assert pl._err_iter.cpu().numpy().tobytes() == np.array(errs).tobytes()


# plain, without and with x >= 0 (the PF and the PF + POS instantiations): every (d_split, carry_g, defer_x); masked: the
# two corners of that cube (the default form and its opposite) -- the mask does not reach the pass-1 kernels
ONE_BLOCK = [(ds, cg, dx, "plain", pos) for pos in (False, True) for ds in (1, 2) for cg in (1, 0) for dx in (1, 0)] \
    + [(ds, cg, dx, "masked", False) for ds, cg, dx in ((1, 1, 1), (2, 0, 0))]


@pytest.mark.parametrize("d_split,carry,defer_x,variant,positive", ONE_BLOCK)
@pytest.mark.parametrize("m,n,k,Block", [TWO_KERNEL, WIDE, FUSED_G1, FUSED_G2])
def test_one_block_steps(m, n, k, Block, d_split, carry, defer_x, variant, positive):
    run_steps(m, n, k, Block, d_split, carry, defer_x, variant, positive)


@pytest.mark.parametrize("variant,positive", [("plain", False), ("masked", False), ("plain", True)])
@pytest.mark.parametrize("d_split", [1, 2])
def test_multi_block_steps(d_split, variant, positive):
    m, n, k, Block = MULTI
    run_steps(m, n, k, Block, d_split, 0, 0, variant, positive)


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("d_split,carry", [(1, 1), (2, 0)])
def test_intercept_steps(d_split, carry, positive):
    m, n, k, Block = TWO_KERNEL
    run_steps(m, n, k, Block, d_split, carry, 1, "intercept", positive)


# ---------------------------------------------------------------------------
# 2. all-ones factors, and off after on, are the feature-off run bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("m,n,k,Block", SHAPES)
def test_all_ones_is_the_feature_off_run(m, n, k, Block, positive):
    Ab, B, mu, pen, _, _ = problem(m, n, k)
    T = 32

    def run(pl, use_graph=True):
        pl.solver_reset(B.copy(), mu, record_len=T, use_graph=use_graph)
        pl.solver_step(T)
        rec = snapshot(pl, T)
        rec["err_iter"] = pl._err_iter.cpu().numpy().copy()
        return rec

    base = run(make(m, n, k, Block, positive=positive))
    same_bits(base, run(make(m, n, k, Block, pen=np.ones(n), positive=positive)))
    same_bits(base, run(make(m, n, k, Block, pen=np.ones(n), positive=positive, d_split=1), use_graph=False))
    pl = make(m, n, k, Block, pen=pen, positive=positive)
    on = run(pl)
    assert not np.array_equal(on["x"], base["x"]) and not np.array_equal(on["gnorm_inf"], base["gnorm_inf"])
    pl.set_penalty_factors(None)
    assert pl.get_tuning("penalty") == 0
    with pytest.raises(N.BpglError, match=r"\(-2\): .*bpgl_panel_reset"):      # a reset must follow
        pl.solver_step(1)
    same_bits(base, run(pl))
    if (m, n, k, Block) == TWO_KERNEL and not positive:       # hi + lo direction too
        b2 = run(make(m, n, k, Block, d_split=2))
        same_bits(b2, run(make(m, n, k, Block, pen=np.ones(n), d_split=2)))


# ---------------------------------------------------------------------------
# 3. power-of-two factors against the feature-off run on the column-rescaled A
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k,Block", SHAPES)
def test_power_of_two_factors_are_the_rescaled_run(m, n, k, Block):
    """With p_j = 2^e_j the run on A is the feature-off run on A diag(1 / p) (exact in bf16) with z = p o x: after each
    of 18 single iterations z == p o x and the residuals agree, bitwise.  (The error record is not scale-invariant
    and is left out.)

    Not so after 256 iterations, on the device as in the numpy model of tests/test_panel_penalty_host.py: a coordinate
    that the prox sends to zero keeps 2^-8 of itself per visit with the bf16 direction and reaches the fp32 subnormals
    after about 20 iterations (the model's first mismatch is at t = 21, smallest |x| 7e-41), where a scaling by p is
    no longer exact.  Measured on the MI355X at 256 x 512 k 16 Block 1: 1635 of 8192 entries of z differ from p o x at
    t = 256, 109 of them above 2^-100, max |R - R'| 7.1e-7, smallest nonzero |x| 1.4e-45.  The two runs are then two
    trajectories of one problem, and what is asserted at t = 256 is the bound of the trajectory tests (this file's
    and tests/test_panel_positive.py's, against the host iterate): 1e-2 in x and 1e-4 in the objective, relative."""
    Ab, B, mu, _, p2, _ = problem(m, n, k)
    As = Ab / p2
    assert np.array_equal(P.bf16(As), As)
    on = make(m, n, k, Block, pen=p2)
    off = make(m, n, k, Block, Ab=As)
    np.testing.assert_array_equal(off.diag_ATA.reshape(-1), on.diag_ATA.reshape(-1) / p2 ** 2)
    on.solver_reset(B.copy(), mu)
    off.solver_reset(B.copy(), mu)
    for t in range(T_STEPS):
        on.solver_step(1)
        off.solver_step(1)
        (x, R1), (z, R2) = P.snapshot(on), P.snapshot(off)
        assert np.array_equal(z, p2[:, None] * x), t
        assert np.array_equal(R1, R2), t
    on.solver_step(256 - T_STEPS)
    off.solver_step(256 - T_STEPS)
    a, b = snapshot(on, 256), snapshot(off, 256)
    z, px = b["x"], p2[:, None] * a["x"]
    big = np.maximum(np.abs(z), np.abs(px)) >= 2.0 ** -100
    print(f"power-of-two factors {(m, n, k, Block)} at t = 256: {int((z != px).sum())} entries of z differ from p o x, "
          f"{int((z[big] != px[big]).sum())} of them above 2^-100; max |R - R'| {np.abs(a['R'] - b['R']).max():.3g}; "
          f"smallest nonzero |x| {np.abs(a['x'][a['x'] != 0]).min():.3g}")
    wx = wf = 0.0
    for c in range(0, k, max(1, k // 16)):
        obj = lambda v: 0.5 * float((As @ v - B[:, c]) @ (As @ v - B[:, c])) + mu[c] * float(np.abs(v).sum())  # noqa: E731
        wx = max(wx, np.linalg.norm(z[:, c] - px[:, c]) / np.linalg.norm(px[:, c]))
        wf = max(wf, abs(obj(z[:, c].copy()) - obj(px[:, c].copy())) / obj(px[:, c].copy()))
    print(f"  worst rel z - p o x {wx:.2e}, worst rel objective {wf:.2e}")
    assert wx <= 1e-2 and wf <= 1e-4
    assert np.all(np.abs(a["primal"] - b["primal"]) <= 1e-4 * b["primal"])
    assert a["x"].any()


# ---------------------------------------------------------------------------
# 4. the certificate against the numpy restatement on the device's own x; repeatable
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("m,n,k,Block,variant", [s + (v,) for s in SHAPES for v in ("plain", "masked", "intercept")
                                                 if v != "intercept" or s == TWO_KERNEL])
def test_certificate_matches_numpy(m, n, k, Block, variant, positive):
    if variant == "intercept":
        Ab, _, B, W, mu = offset_instance(m, n, 4, k // 4)[:5]
        pen = PR.factors(n)
    else:
        Ab, B, mu, pen, _, W = problem(m, n, k)
    icpt = variant == "intercept"
    pl = make(m, n, k, Block, pen=pen, positive=positive, Ab=Ab)
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
    cols = range(k) if k == 16 else range(0, k, 8)
    for rec in recs:
        ref = {c: C.penalty_duality_gap(Ab, B[:, c], Wn[:, c], rec["x"][:, c].copy(), mu[c], pen, diag=diag,
                                        intercept=icpt, positive=positive) for c in cols}
        idx = np.array(list(cols))
        get = lambda key: np.array([ref[c][key] for c in cols])  # noqa: E731
        keys = ("primal", "dual", "scale", "gnorm_inf") + (("holdout_sse",) if variant != "plain" else ()) \
            + (("intercept",) if icpt else ())
        viol = PR.check_certificate({key: rec[key][idx] for key in keys + ("gap",)},
                                    {key: get(key) for key in keys + ("gap",)}, keys=keys)
        assert not viol, viol
        g_ref, r_ref = get("g"), get("r")
        for i, c in enumerate(cols):
            np.testing.assert_allclose(rec["g"][c], g_ref[i], rtol=1e-11, atol=1e-12 * np.abs(g_ref[i]).max())
            np.testing.assert_allclose(rec["r"][c], r_ref[i], rtol=1e-11, atol=1e-12 * np.abs(r_ref[i]).max())
        score, keep = get("score"), get("keep")
        thr = mu[idx][:, None] * pen[None, :]
        clear = np.abs(score - thr) > 1e-9 * thr
        assert (~clear).sum() <= 0.01 * n * len(idx), int((~clear).sum())
        assert np.array_equal(rec["keep"][idx][clear], keep[clear])
        assert np.array_equal(rec["n_keep"], rec["keep"].sum(axis=1))
        ga = np.maximum(-rec["g"], 0.0) if positive else np.abs(rec["g"])
        assert np.array_equal(rec["gnorm_inf"], (ga / pen).max(axis=1))
        print(f"penalty certificate {(m, n, k, Block)} {variant} positive={positive} t={rec['t']}: gap err / primal "
              f"{np.max(np.abs(rec['gap'][idx] - get('gap')) / get('primal')):.2e}, drift {rec['drift'].max():.2e}, "
              f"n_keep {rec['n_keep'].min()}..{rec['n_keep'].max()}, borderline {int((~clear).sum())}")
    # at x = 0 the slot is mu_max = max |A^T b| / p (the in-rows' centred b with the intercept; one-sided with x >= 0)
    if variant == "plain":
        g0 = Ab.T @ B
        ga = np.maximum(g0, 0.0) if positive else np.abs(g0)         # g = -A^T b at x = 0
        want = (ga / pen[:, None]).max(axis=0)
        assert np.all(np.abs(recs[0]["gnorm_inf"] - want) <= 1e-12 * want)
    assert recs[1]["x"].any()


# ---------------------------------------------------------------------------
# 5. the trajectory is the weighted one, and not the unweighted one
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,k,Block", SHAPES)
def test_trajectory(m, n, k, Block):
    Ab, B, mu, pen, _, _ = problem(m, n, k)
    T = 256
    wei, unw = reference(m, n, k, Block, T)
    # on the CPU first: the two references are far apart
    far_ref = min(np.linalg.norm(wei[c] - unw[c]) / np.linalg.norm(unw[c]) for c in wei)
    assert far_ref > 1e-1, far_ref
    pl = make(m, n, k, Block, pen=pen)
    pl.solver_reset(B.copy(), mu)
    pl.solver_step(T)
    X = pl.solver_x()
    wx = wf = 0.0
    far = np.inf
    for c, ref in wei.items():
        obj = lambda x: 0.5 * float((Ab @ x - B[:, c]) @ (Ab @ x - B[:, c])) + mu[c] * float(pen @ np.abs(x))  # noqa: E731
        wx = max(wx, np.linalg.norm(X[:, c] - ref) / np.linalg.norm(ref))
        wf = max(wf, abs(obj(X[:, c].copy()) - obj(ref)) / obj(ref))
        far = min(far, np.linalg.norm(X[:, c] - unw[c]) / np.linalg.norm(unw[c]))
    print(f"penalty trajectory {(m, n, k, Block)}: worst rel x {wx:.2e}, worst rel objective {wf:.2e}, "
          f"nearest to the unweighted reference {far:.2f} (the references: {far_ref:.2f})")
    assert wx <= 1e-2 and wf <= 1e-4
    assert far > 1e-1


# ---------------------------------------------------------------------------
# 6. warm start: drift 0
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("m,n,k,Block", [TWO_KERNEL, FUSED_G2])
def test_warm_start_reports_no_drift(m, n, k, Block, positive):
    Ab, B, mu, pen, _, _ = problem(m, n, k)
    pl = make(m, n, k, Block, pen=pen, positive=positive)
    X0 = np.random.RandomState(1).randn(n, k).astype(np.float32) * (np.random.RandomState(2).rand(n, k) < 0.3)
    Xs = (np.maximum(X0, 0.0) if positive else X0).astype(np.float64)
    for use_graph in (True, False):
        pl.solver_reset(B.copy(), mu, use_graph=use_graph, x0=X0)
        rec = snapshot(pl)
        assert np.array_equal(rec["x"], Xs)
        assert np.all(rec["drift"] == 0.0) and np.array_equal(rec["R"], rec["r"])
        ref = C.penalty_duality_gap(Ab, B[:, 3], None, Xs[:, 3].copy(), mu[3], pen, positive=positive)
        assert abs(rec["primal"][3] - ref["primal"]) <= 1e-9 * ref["primal"]
    pl.solver_step(16)
    x16 = pl.solver_x()
    pl.solver_reset(B.copy(), mu, x0=pl.solver_x_device())      # the in-place restart from the stored iterate
    rec = snapshot(pl)
    assert np.array_equal(rec["x"], x16) and np.all(rec["drift"] == 0.0)


# ---------------------------------------------------------------------------
# 7. errors
# ---------------------------------------------------------------------------
def test_penalty_errors():
    m, n, k, _ = TWO_KERNEL
    L = panel._lib()
    assert L.bpgl_version() >= 309
    assert L.bpgl_panel_set_penalty(None, None) == -1
    raw = ctypes.c_void_p()
    assert L.bpgl_panel_create(ctypes.byref(raw), 0, m, n, 1, 16, 0, None) == 0
    assert L.bpgl_panel_set_penalty(raw, None) == -2             # before bpgl_panel_bind
    assert "bpgl_panel_bind" in L.bpgl_last_error().decode()
    L.bpgl_panel_destroy(raw)
    Ab, B, mu, pen, _, _ = problem(m, n, k)
    pl = make(m, n, k, 1, pen=pen)
    pl.solver_reset(B.copy(), mu)
    pl.solver_step(8)
    want = snapshot(pl, 8)
    # a refused vector leaves the factors in force, and the solver as it was
    for j, v in ((5, 0.0), (n - 1, np.nan), (0, -1.0), (17, np.inf)):
        bad = torch.from_numpy(np.where(np.arange(n) == j, v, pen)).to("cuda:0")
        with pl._on_stream():
            rc = L.bpgl_panel_set_penalty(pl._ctx, N.ptr(bad))
        assert rc == -1, (j, v, rc)                               # BPGL_E_ARG
        assert "penalty factor" in L.bpgl_last_error().decode()
        assert pl.get_tuning("penalty") == 1
    same_bits(want, snapshot(pl, 8))
    pl.solver_reset(B.copy(), mu)
    pl.solver_step(8)
    same_bits(want, snapshot(pl, 8))
    # the Python layer refuses them before the native call
    for badp in (pen[:-1], np.where(np.arange(n) == 3, 0.0, pen), np.full(n, np.nan)):
        with pytest.raises(ValueError, match="penalty factor"):
            pl.set_penalty_factors(badp)
    # installing or clearing invalidates the solver; bind's default is off
    for p in (pen, None):
        pl.set_penalty_factors(p)
        with pytest.raises(N.BpglError, match=r"\(-2\): .*bpgl_panel_reset"):
            pl.duality_gap()
        pl.solver_reset(B.copy(), mu)
        assert pl.get_tuning("penalty") == int(p is not None)
    assert make(m, n, k, 1).get_tuning("penalty") == 0


# ---------------------------------------------------------------------------
# 8. the drivers
# ---------------------------------------------------------------------------
def test_lasso_path_penalty():
    m, n = 256, 512
    Ab, B, _, pen, _, _ = problem(m, n, 16)
    b = B[:, 0].copy()
    bound = 1e-4
    res = panel.lasso_path(Ab, b, n_mus=16, penalty_factors=pen, GAP_BOUND=bound, ITER_MAX=2048, check_every=64, device=0)
    nnz = (res["x"] != 0).sum(axis=0)
    print(f"lasso_path penalty: iters {res['iters']}, mu_max {res['mu_max']:.6g}, nonzeros {nnz.tolist()}, "
          f"rel gap {(res['gap'] / (0.5 * b @ b)).max():.2e}")
    assert np.all(res["reached"]) and np.all(res["gap"] <= bound * 0.5 * float(b @ b))
    mu_max = float(np.max(np.abs(Ab.T @ b) / pen))
    assert abs(res["mu_max"] - mu_max) <= 1e-12 * mu_max
    assert abs(mu_max - float(np.abs(Ab.T @ b).max())) > 1e-3 * mu_max       # not the unweighted one
    np.testing.assert_allclose(res["mus"], C.mu_grid(mu_max, 16), rtol=1e-12)
    assert nnz[0] == 1 and nnz[-1] > nnz[0]                   # 1 nonzero at the largest mu: the column that sets mu_max
    assert np.flatnonzero(res["x"][:, 0])[0] == int(np.argmax(np.abs(Ab.T @ b) / pen))
    for j in (0, 7, 15):
        cert = C.penalty_duality_gap(Ab, b, None, res["x"][:, j].copy(), res["mus"][j], pen)
        assert abs(cert["gap"] - res["gap"][j]) <= 1e-9 * cert["primal"]
    # composes with positive, fit_intercept and x0
    both = panel.lasso_path(Ab, b, mus=res["mus"], penalty_factors=pen, positive=True, fit_intercept=True, x0=res["x"],
                            GAP_BOUND=bound, ITER_MAX=2048, check_every=64, device=0)
    assert np.all(both["reached"]) and np.all(both["x"] >= 0)
    for j in (0, 15):
        cert = C.penalty_duality_gap(Ab, b, None, both["x"][:, j].copy(), res["mus"][j], pen, intercept=True, positive=True)
        assert abs(cert["gap"] - both["gap"][j]) <= 1e-9 * cert["primal"]
        assert abs(cert["intercept"] - both["intercept"][j]) <= 1e-9 * abs(cert["intercept"])


def test_lasso_path_penalty_shrink():
    Ab, b, _, _, _ = screen_instance()
    n = Ab.shape[1]
    pen = PR.factors(n)
    bound = 3e-6
    mus = C.mu_grid(float(np.max(np.abs(Ab.T @ b) / pen)), 16, 0.9, 0.1)
    kw = dict(mus=mus, GAP_BOUND=bound, ITER_MAX=4096, check_every=64, device=0, penalty_factors=pen)
    plain = panel.lasso_path(Ab, b, **kw)
    res = panel.lasso_path(Ab, b, shrink=0.75, **kw)
    rel = np.linalg.norm(res["x"] - plain["x"]) / np.linalg.norm(plain["x"])
    print(f"lasso_path penalty shrink: compactions {res['compactions']}, iters {res['iters']} (plain {plain['iters']}), "
          f"x against shrink=0 {rel:.2e}")
    assert plain["compactions"] == [] and np.all(plain["reached"])
    widths = [wd for _, wd in res["compactions"]]
    assert widths and widths[-1] < n and all(wd % 256 == 0 for wd in widths) and widths == sorted(widths, reverse=True)
    assert res["active"].size == widths[-1] and np.all(res["reached"])
    assert rel <= 1e-4
    for j in range(mus.size):
        cert = C.penalty_duality_gap(Ab, b, None, res["x"][:, j].copy(), mus[j], pen)
        assert abs(res["gap"][j] - cert["gap"]) <= 1e-9 * cert["primal"]
        assert cert["gap"] <= bound * 0.5 * float(b @ b) * (1 + 1e-9)


@pytest.mark.parametrize("fit_intercept,positive", [(False, False), (True, False), (False, True), (True, True)])
def test_lasso_cv_penalty(fit_intercept, positive):
    m, n, nf, nm = 256, 512, 4, 4
    pen = PR.factors(n)
    if fit_intercept:
        Ab, b = offset_instance(m, n)[:2]
    else:
        Ab, B, _, _, _, _ = problem(m, n, 16)
        b = B[:, 0].copy()
    res = panel.lasso_cv(Ab, b, n_folds=nf, n_mus=nm, seed=7, penalty_factors=pen, positive=positive,
                         fit_intercept=fit_intercept, return_x=True, warm_refit=True, GAP_BOUND=1e-4, ITER_MAX=2048,
                         check_every=64, device=0)
    masks, mus = res["masks"], res["mus"]
    print(f"lasso_cv penalty fit_intercept={fit_intercept} positive={positive}: iters {res['iters']}, mean mse "
          f"{res['mean_mse']}, best {res['best']}, refit iters {res['refit_iters']}")
    assert np.all(res["reached"]) and res["x"].any()
    bc = b - b.mean() if fit_intercept else b
    g0 = Ab.T @ bc
    np.testing.assert_allclose(mus, C.mu_grid(float(np.max((np.maximum(g0, 0) if positive else np.abs(g0)) / pen)), nm),
                               rtol=1e-9)
    count = (masks == 0).sum(axis=1)
    for f in range(nf):
        out = masks[f] == 0
        for j in range(nm):
            x = res["x_folds"][:, f, j]
            b0 = res["intercept_folds"][f, j] if fit_intercept else 0.0
            sse = float(np.square(Ab[out] @ x + b0 - b[out]).sum())
            assert abs(res["mse"][f, j] * count[f] - sse) <= 1e-9 * sse
            cert = C.penalty_duality_gap(Ab, b, masks[f], x.copy(), mus[j], pen, intercept=fit_intercept, positive=positive)
            assert abs(res["gap"][f, j] - cert["gap"]) <= 1e-9 * cert["primal"]
    # the refit is lasso_path(penalty_factors=) on the same grid
    path = panel.lasso_path(Ab, b, mus=mus, penalty_factors=pen, positive=positive, fit_intercept=fit_intercept,
                            GAP_BOUND=1e-4, ITER_MAX=2048, check_every=64, device=0)
    assert res["refit_iters"] <= path["iters"]
    assert np.linalg.norm(res["x"] - path["x"]) <= 1e-2 * np.linalg.norm(path["x"])
    if fit_intercept or positive:
        return
    # and the factors matter: the unweighted CV on the same folds and grid returns another x
    unw = panel.lasso_cv(Ab, b, masks=masks, mus=mus, positive=positive, fit_intercept=fit_intercept, GAP_BOUND=1e-4,
                         ITER_MAX=2048, check_every=64, device=0)
    assert np.linalg.norm(res["x"] - unw["x"]) > 1e-1 * np.linalg.norm(unw["x"])

"""The non-negative lasso of the panel path (bpgl_panel_set_positive, ABI 308), without a GPU.

(a) the ABI is there: bpgl_version() >= 308 and bpgl_panel_set_positive(NULL, 1) is BPGL_E_ARG.
(b) ``panel_positive_reference.check_step_positive`` separates right from wrong.  The "device" is ``PosModel``,
    tests/test_panel_step_host.py's numpy model of one panel iteration with the constrained shrink: the
    one-sided prox, the bf16 direction image with the towards-zero rule (``feasible_image``), the constrained
    error criterion; everything else (R -> hi + lo, the carried gradient, fp32 S per pass-2 chunk, fp32 x) as
    there.  Its own trajectories pass at each of 18 checkpoints; each of four mutants is caught at every
    checkpoint where it acts, and acts:
      nearest       the image rounded to nearest only.  Acts where the stored x leaves the feasible set; P1 fires.
      two_sided     the two-sided soft threshold.  Acts where the stored x leaves the feasible set.
      clamp_after   nearest rounding and x clamped at 0 after the update, R not.  Acts where the clamp moved x
                    by more than check A's own bound admits as rounding on some row; A fires.
      old_err       the unconstrained error criterion.  Acts where it differs from the constrained one by more
                    than twice the gradient allowance of check D.
(c) ``cpu_calculation.positive_panel_iterate`` converges to the KKT point of the constrained problem and
    ``positive_duality_gap`` is a valid certificate: weak duality at random feasible x.
(d) the one-sided gap-safe screen never drops a coordinate that is positive in the converged solution.
(e) the drivers' argument checks that need no GPU.

Measured here (18 iterations, seed 0): the clean model's worst ratio to bound over the twelve cases A 0.25, B 0.09,
C 0.98, D 0.19, the rule firing 1339 to 9463 times per case (2152 and 1339 at 256 x 512 Block 2, whose blocks are
256 wide); one bent step leaves the feasible set at 9 of 18 checkpoints with nearest rounding at 256 x 512 Block 1
(16 with Block 2, 15 at 256 x 1024) and at all 18 with the two-sided threshold; the clamp acts at 7 to 16
checkpoints, the old error formula at 3 to 18; the nearest-only trajectory holds 5778 negative entries over its 18
iterates, min x -1.27e-3.  Over 256 iterations the model's drift is 5.7e-7, 0.003 of ``drift_bound``; the clamp's
3.1e-4, 3.7 times the bound on its worst right-hand side.
"""
import numpy as np
import pytest

import panel_positive_reference as R
import panel_step_reference as P
import test_panel_step_host as H
from convex_optimization_amd import cpu_calculation as C

T_STEPS, G_REFRESH = H.T_STEPS, H.G_REFRESH


# ---------------------------------------------------------------------------
# (a) the ABI
# ---------------------------------------------------------------------------
def test_abi_308_has_set_positive():
    from convex_optimization_amd import _native as N
    from convex_optimization_amd import panel
    L = panel._lib()
    assert L.bpgl_version() >= 308
    assert "bpgl_panel_set_positive" in N.header_functions()
    assert L.bpgl_panel_set_positive(None, 1) == -1            # BPGL_E_ARG
    assert b"null" in L.bpgl_last_error()


# ---------------------------------------------------------------------------
# (b) the numpy model and its mutants
# ---------------------------------------------------------------------------
class PosModel(H.Model):
    """H.Model with the constrained shrink; ``mutant`` in (None, "nearest", "two_sided", "clamp_after", "old_err")."""

    def step(self):
        mut, mb = self.mutant, self.t % self.Block
        sl = slice(mb * self.w, (mb + 1) * self.w)
        Am = self.Ab[:, sl]
        exact = not self.carry or self.t % G_REFRESH == 0
        if exact:
            hi, lo = P.split_bf16(self.R)
            op = hi + lo
        else:
            op = self.Vh
        prod = P.f32(Am.T @ op.T)
        g = prod if exact else P.f32(self.Gc + prod)
        if self.carry:
            self.Gc = g
        xb = self.x[sl].copy()
        d = self.diag[mb][:, None]
        soft = P.soft_thr(d * xb - g, self.mu) / d
        D = (soft if mut == "two_sided" else np.maximum(soft, 0.0)) - xb
        Dp, fired = R.feasible_image(D, xb, self.d_split, nearest_only=mut in ("nearest", "clamp_after", "two_sided"))
        self.fired = int(np.count_nonzero(fired))
        err_new = float(np.max(np.abs(xb - np.maximum(xb - g - self.mu, 0.0))))
        err_old = float(np.max(np.abs(g - np.clip(g - xb, -self.mu, self.mu))))
        kc = self.w // self.kchunks
        S = sum(P.f32(Am[:, c * kc:(c + 1) * kc] @ Dp[c * kc:(c + 1) * kc]) for c in range(self.kchunks)).T
        S = np.where(self.Wk, S, 0.0)
        rs, ss = np.einsum("km,km->k", self.R, S), np.einsum("km,km->k", S, S)
        r1 = rs + self.mu * (np.abs(xb + Dp).sum(axis=0) - np.abs(xb).sum(axis=0))
        gamma = np.where(ss == 0.0, 0.0, np.clip(-r1 / np.where(ss == 0.0, 1.0, ss), 0.0, 1.0))
        xn = P.f32(xb + gamma * Dp)
        info = dict(neg=bool(np.any(xn < 0.0)), err_gap=abs(err_old - err_new), clamp=np.zeros_like(xn), Am=Am, xb=xb, xn=xn)
        if mut == "clamp_after":
            info["clamp"] = np.maximum(xn, 0.0) - xn
            xn = np.maximum(xn, 0.0)
        self.x[sl] = xn
        self.R = self.R + gamma[:, None] * S
        if self.carry:
            V = gamma[:, None] * S + (0.0 if exact else self.E)
            self.Vh = P.bf16(V)
            self.E = P.f32(V - self.Vh)
        self.t += 1
        return (err_old if mut == "old_err" else err_new), info


def problem(m, n, k, masked):
    Ab, B, mu = P.instance(m, n, k)
    return Ab, B, mu, (P.fold_mask(m, k) if masked else None)


def run_checked(m, n, Block, k, masked, d_split, carry, mutant=None, stats=None):
    """18 steps of the clean model, ``check_step_positive`` at each; a mutant bends the single step from the clean
    state at t.  Per checkpoint (violations, acted, fired)."""
    Ab, B, mu, W = problem(m, n, k, masked)
    mod = PosModel(Ab, B, mu, Block, d_split, carry, W=W)
    out, snaps = [], [mod.snap()]
    for t in range(T_STEPS):
        if mutant is not None:
            bent = mod.clone(mutant)
            err, info = bent.step()
            after = bent.snap()
            mod.step()
        else:
            err, info = mod.step()
            after = mod.snap()
        snaps.append(mod.snap())
        q = t % G_REFRESH if mod.carry else 0
        exact = not mod.carry or q == 0
        st = {}
        viol = R.check_step_positive(Ab, mod.diag, mu, W, t % Block, snaps[t], after, err, d_split, exact,
                                     None if exact else snaps[t][1] - snaps[t - 1][1], chain=mod.chain, q=q,
                                     R_ref=None if exact else snaps[t - q][1], stats=st)
        if stats is not None:
            for key in "ABCD":
                stats[key] = max(stats.get(key, 0.0), st[key])
            stats["x_min"] = min(stats.get("x_min", np.inf), st["x_min"])
        acted = False
        if mutant in ("nearest", "two_sided"):
            acted = info["neg"]
        elif mutant == "clamp_after":
            # the clamp's effect on A dx against check A's bound on some row (below it: rounding, by the check's own terms)
            Am, xb, xn = info["Am"], info["xb"], info["xn"]
            absA = np.abs(Am)
            xc = np.maximum(xn, 0.0)
            bound = P.U24 * (absA @ (np.abs(xb) + np.abs(xc))) + mod.chain * P.U24 * (absA @ np.abs(xc - xb))
            acted = bool(np.any(np.abs(Am @ info["clamp"]) > 2.0 * bound + 1e-300))
        elif mutant == "old_err":
            Am = Ab[:, (t % Block) * mod.w:(t % Block + 1) * mod.w]
            R0 = snaps[t][1]
            sig = 2.0 ** -17 * np.sqrt(np.square(Am).T @ np.square(R0).T)
            acted = exact and info["err_gap"] > 2.0 * P.C_G * float(sig.max())
        out.append((viol, acted, mod.fired))
    return out


CASES = [(256, 512, 1, 16, False), (256, 512, 2, 16, False), (256, 1024, 2, 16, False), (256, 512, 1, 16, True)]


@pytest.mark.parametrize("m,n,Block,k,masked,d_split,carry",
                         [c + (ds, cg) for c in CASES for ds in (1, 2) for cg in ((1, 0) if c[2] == 1 else (0,))])
def test_model_passes(m, n, Block, k, masked, d_split, carry):
    stats = {}
    res = run_checked(m, n, Block, k, masked, d_split, carry, stats=stats)
    fired = sum(f for _, _, f in res)
    print(f"positive model {m}x{n} B={Block} k={k} masked={masked} d_split={d_split} carry={carry}: worst ratio to bound "
          + " ".join(f"{key} {stats[key]:.3g}" for key in "ABCD") + f", rule fired {fired} times, min x {stats['x_min']}")
    for t, (viol, _, _) in enumerate(res):
        assert not viol, (t, viol)
    assert stats["x_min"] >= 0.0
    if d_split == 1 and not masked and Block == 1:
        assert fired >= 2000                       # the instance exercises the rule


MUTANT_CASES = [(256, 512, 1, 16, False, 1, 1), (256, 512, 1, 16, False, 1, 0), (256, 512, 2, 16, False, 1, 0),
                (256, 1024, 2, 16, False, 1, 0)]


@pytest.mark.parametrize("case", MUTANT_CASES)
@pytest.mark.parametrize("mutant", ["nearest", "two_sided", "clamp_after", "old_err"])
def test_mutant_is_caught(mutant, case):
    res = run_checked(*case, mutant=mutant)
    acted = [t for t, (_, a, _) in enumerate(res) if a]
    missed = [t for t, (viol, a, _) in enumerate(res) if a and not viol]
    print(f"{mutant} {case}: acts at {len(acted)} checkpoints, missed at {missed}")
    assert acted, "the mutant never acted: the case does not exercise it"
    assert not missed
    want = {"nearest": "P1", "clamp_after": "A:"}.get(mutant)
    if want:
        for t in acted:
            assert any(v.startswith(want) for v in res[t][0]), (t, res[t][0])


def test_nearest_rounding_leaves_the_feasible_set():
    """The trap itself: the unmodified nearest image, run as a trajectory (not one bent step), puts thousands of
    negative entries into the stored iterates."""
    Ab, B, mu, _ = problem(256, 512, 16, False)
    mod = PosModel(Ab, B, mu, 1, 1, 1, mutant="nearest")
    neg, xmin = 0, 0.0
    for _ in range(T_STEPS):
        mod.step()
        neg += int(np.count_nonzero(mod.x < 0.0))
        xmin = min(xmin, float(mod.x.min()))
    print(f"nearest-only trajectory: {neg} negative entries over {T_STEPS} iterates, min x {xmin:.3g}")
    assert neg >= 1000 and xmin < 0.0


def test_drift_bound_separates_the_clamp():
    """``drift_bound`` (asserted on the device by tests/test_panel_positive.py over 256 iterations) holds for the
    model with room, and the trajectory that clamps x after the update (bf16 direction) breaks it."""
    Ab, B, mu, _ = problem(256, 512, 16, False)
    ratio = {}
    for mut in (None, "clamp_after"):
        mod = PosModel(Ab, B, mu, 1, 1, 1, mutant=mut)
        xs = [mod.x.copy()]
        for _ in range(256):
            mod.step()
            xs.append(mod.x.copy())
        drift = np.abs(mod.R - (Ab @ mod.x - B).T).max(axis=1)
        ratio[mut] = drift / R.drift_bound(Ab, xs, mod.chain, np.abs(B).max())
        print(f"drift over 256 iterations, mutant {mut}: worst {drift.max():.3g}, worst ratio to bound {ratio[mut].max():.3g}")
    assert ratio[None].max() <= 1.0
    assert ratio["clamp_after"].max() > 1.0


# ---------------------------------------------------------------------------
# (c), (d) the fp64 restatements
# ---------------------------------------------------------------------------
def small(seed=5, m=64, n=32):
    rs = np.random.RandomState(seed)
    A = rs.randn(m, n)
    b = A @ (rs.randn(n) * (rs.rand(n) < 0.5)) + 0.1 * rs.randn(m)
    mu = 0.1 * float(np.max(A.T @ b))
    return A, b, mu


@pytest.mark.parametrize("intercept,masked", [(False, False), (False, True), (True, False), (True, True)])
def test_positive_iterate_converges_to_kkt(intercept, masked):
    A, b, mu = small()
    m, n = A.shape
    w = (np.arange(m) % 4 != 1).astype(np.uint8) if masked else None
    it = 0
    x0 = None
    while True:
        res = C.positive_panel_iterate(A, b, w, mu, 1, 500, x0=x0, intercept=intercept)
        it += 500
        cert = C.positive_duality_gap(A, b, w, res["x"], mu, intercept=intercept)
        if cert["gap"] <= 1e-12 * cert["primal"] or it >= 20000:
            break
        x0 = res["x"]
    x, g = res["x"], cert["g"]
    print(f"positive KKT intercept={intercept} masked={masked}: {it} iterations, gap / primal {cert['gap'] / cert['primal']:.2e}, "
          f"{int((x > 0).sum())} positive, max |g + mu| on them {np.abs(g[x > 0] + mu).max():.2e}, min g off them "
          f"{(g[x == 0] + mu).min() if (x == 0).any() else np.nan:.2e}")
    assert cert["gap"] <= 1e-12 * cert["primal"]
    assert np.all(x >= 0) and (x > 0).sum() >= 3 and (x == 0).sum() >= 3
    np.testing.assert_allclose(res["r"], cert["r"], rtol=0, atol=1e-11 * np.abs(cert["r"]).max())
    # the gap bounds the distance to the optimum: |grad + mu| on the support <= sqrt(2 gap) max |a_j|, with margin
    tol = 10.0 * np.sqrt(2.0 * max(cert["gap"], 0.0)) * np.sqrt(np.square(A).sum(axis=0).max()) + 1e-12 * mu
    assert np.all(np.abs(g[x > 0] + mu) <= tol)
    assert np.all(g[x == 0] >= -mu - tol)
    # not the unconstrained solution: that one has negative coordinates
    if not intercept:
        xu = C.masked_panel_iterate(A, b, np.ones(m) if w is None else w, mu, 1, 5000)["x"]
        assert (xu < 0).sum() >= 3
    # (d) the screen is safe at every stage of the solve
    # (while the gap is above the rounding of the primal, 1e-10 of it: once primal - dual is a difference of
    # two equal fp64 numbers the radius is 0 or noise and score = mu (1 - 1e-16) on the support)
    xs, stages, screened = np.zeros(n), 0, 0
    for _ in range(40):
        c = C.positive_duality_gap(A, b, w, xs, mu, intercept=intercept)
        assert np.array_equal(c["keep"], ~(c["score"] < mu))
        if c["gap"] <= 1e-10 * c["primal"]:
            break
        stages += 1
        screened = max(screened, int((~c["keep"]).sum()))
        assert np.all(c["keep"][x > 0]), "the screen dropped a coordinate of the solution's support"
        xs = C.positive_panel_iterate(A, b, w, mu, 1, 2, x0=xs, intercept=intercept)["x"]
    print(f"screen: {stages} stages checked, up to {screened} of {n} columns screened")
    assert stages >= 3 and screened >= 3            # and it does screen


@pytest.mark.parametrize("intercept", [False, True])
def test_weak_duality_at_random_feasible_points(intercept):
    A, b, mu = small(seed=9)
    m, n = A.shape
    w = (np.arange(m) % 5 != 2).astype(np.uint8)
    xs = C.positive_panel_iterate(A, b, w, mu, 1, 2000, intercept=intercept)["x"]
    best = C.positive_duality_gap(A, b, w, xs, mu, intercept=intercept)
    rs = np.random.RandomState(1)
    for _ in range(50):
        x = np.abs(rs.randn(n)) * (rs.rand(n) < 0.5) * rs.choice([1e-3, 1.0, 30.0])
        c = C.positive_duality_gap(A, b, w, x, mu, intercept=intercept)
        assert c["gap"] >= -1e-12 * c["primal"]
        assert c["dual"] <= best["primal"] * (1 + 1e-12)           # any dual value below the optimum
        assert 0.0 < c["scale"] <= 1.0
        assert c["gnorm_inf"] == max(0.0, float(np.max(-c["g"])))
        assert np.all(c["scale"] * (-c["g"]) <= mu * (1 + 1e-12))  # scale r is dual feasible


def test_block_cycling_and_projection_of_x0():
    A, b, mu = small(seed=3, m=64, n=64)
    one = C.positive_panel_iterate(A, b, None, mu, 1, 4000)["x"]
    two = C.positive_panel_iterate(A, b, None, mu, 2, 8000)["x"]
    np.testing.assert_allclose(one, two, atol=1e-8 * np.abs(one).max())
    x0 = np.random.RandomState(0).randn(64)
    a = C.positive_panel_iterate(A, b, None, mu, 1, 0, x0=x0)
    assert np.array_equal(a["x"], np.maximum(x0, 0.0))
    np.testing.assert_allclose(a["r"], A @ np.maximum(x0, 0.0) - b, atol=1e-12)


# ---------------------------------------------------------------------------
# (e) argument checks that need no GPU
# ---------------------------------------------------------------------------
def test_mu_max_zero_is_a_value_error():
    from convex_optimization_amd import panel
    with pytest.raises(ValueError, match="positive"):
        panel._grid_below(0.0, 4, 0.9, 0.1, True)
    g = panel._grid_below(2.0, 4, 0.9, 0.1, True)
    np.testing.assert_allclose(g, C.mu_grid(2.0, 4, 0.9, 0.1))
    np.testing.assert_allclose(panel._grid_below(2.0, 4, 0.9, 0.1, False), g)
    assert not panel._grid_below(0.0, 4, 0.9, 0.1, False).any()              # without the flag: as before
    assert np.all(np.isnan(panel._grid_below(np.nan, 4, 0.9, 0.1, True)))    # a NaN is not "no positive correlation"
    # the signatures carry the flag, default off
    import inspect
    for f in (panel.lasso_path, panel.lasso_cv):
        assert inspect.signature(f).parameters["positive"].default is False
    # checks that come before any device work still raise with the flag on
    A = np.zeros((256, 256))
    with pytest.raises(ValueError):
        panel.lasso_path(A, np.zeros(256), mus=[1.0], positive=True, check_every=0)
    with pytest.raises(ValueError):
        panel.lasso_cv(A, np.zeros(256), mus=[1.0], positive=True, shrink=1.5)

"""The penalty factors of the panel path (bpgl_panel_set_penalty, ABI 309), without a GPU.

(a) the ABI is there: bpgl_version() >= 309 (309 is this feature's number; a later ABI keeps the symbol) and
    bpgl_panel_set_penalty(NULL, .) is BPGL_E_ARG.
(b) ``panel_penalty_reference.check_step_penalty`` separates right from wrong.  The "device" is ``PenModel``,
    tests/test_panel_step_host.py's numpy model of one panel iteration (fp32 x, bf16 D', a carried fp32 G) with the
    weighted shrink: tau_j = mu p_j in the prox and in the error record, sum p |.| in the line search; with
    ``positive`` the constrained shrink of tests/test_panel_positive_host.py.  Its own trajectories pass at each of
    18 checkpoints; each of five mutants is caught at every checkpoint where it acts, and acts:
      thr        the unweighted threshold mu in the prox
      ls_norms   unweighted norms in the line search.  Acts where the step size differs from the clean one.
      shift      the factors shifted by one column
      block0     Block 2 reading block 0's factors for block 1.  Acts on the iterations of block 1.
      old_err    the unweighted error formula.  Acts where it differs from the weighted one by more than twice the
                 gradient allowance of check D.
    The sixth, the certificate's slot as max |g| without the 1 / p_j, is caught by ``check_certificate`` against
    ``penalty_duality_gap`` (test_certificate_slot_mutant).
(c) independent ground truth: ``penalty_panel_iterate`` on A is ``masked_panel_iterate`` on A diag(1 / p) with
    x = z / p, to fp64 rounding.
(d) KKT at a 64 x 32 Gaussian after convergence, weak duality at random points, a safe screen.
(e) exact scaling in the model: with power-of-two factors the model on A is the feature-off model on the rescaled
    bf16 A with z = p o x, ``==``; no subnormal occurs.  All-ones factors are the feature-off model, ``==``.
(f) the instance is informative: the weighted and the unweighted fp64 solutions differ in support on every
    right-hand side at the tests' mu.
(g) the Python argument errors that need no GPU.
"""
import numpy as np
import pytest

import panel_penalty_reference as PR
import panel_positive_reference as R
import panel_step_reference as P
import test_panel_step_host as H
from convex_optimization_amd import cpu_calculation as C

T_STEPS, G_REFRESH = H.T_STEPS, H.G_REFRESH
MUTANTS = ("thr", "ls_norms", "shift", "block0", "old_err")


# ---------------------------------------------------------------------------
# (a) the ABI
# ---------------------------------------------------------------------------
def test_abi_309_has_set_penalty():
    from convex_optimization_amd import _native as N
    from convex_optimization_amd import panel
    L = panel._lib()
    assert L.bpgl_version() >= 309
    assert "bpgl_panel_set_penalty" in N.header_functions()
    assert L.bpgl_panel_set_penalty(None, None) == -1            # BPGL_E_ARG
    assert b"null" in L.bpgl_last_error()


# ---------------------------------------------------------------------------
# (b) the numpy model and its mutants
# ---------------------------------------------------------------------------
class PenModel(H.Model):
    """H.Model with the weighted shrink; ``pen`` (n,), ``positive``; ``mutant`` in (None,) + MUTANTS."""

    def __init__(self, Ab, B, mu, Block, d_split, carry, pen, W=None, positive=False, mutant=None):
        super().__init__(Ab, B, mu, Block, d_split, carry, W=W, mutant=mutant)
        self.pen, self.positive = np.asarray(pen, dtype=np.float64), bool(positive)
        self.tiny = np.inf      # the smallest nonzero magnitude among the fp32 / bf16 quantities of the run

    def note(self, *arrays):
        for a in arrays:
            nz = np.abs(a[a != 0.0])
            if nz.size:
                self.tiny = min(self.tiny, float(nz.min()))

    def step(self):
        mut, mb = self.mutant, self.t % self.Block
        sl = slice(mb * self.w, (mb + 1) * self.w)
        Am = self.Ab[:, sl]
        exact = not self.carry or self.t % G_REFRESH == 0
        if exact:
            hi, lo = P.split_bf16(self.R)
            op = hi + lo
            self.note(hi, lo)
        else:
            op = self.Vh
        prod = P.f32(Am.T @ op.T)
        g = prod if exact else P.f32(self.Gc + prod)
        self.note(prod, g)
        if self.carry:
            self.Gc = g
        pen = np.roll(self.pen, 1) if mut == "shift" else self.pen
        p_true = self.pen[sl][:, None]
        pb = pen[slice(0, self.w) if mut == "block0" else sl][:, None]       # (w, 1)
        tau = pb * self.mu                                                      # (w, k)
        xb = self.x[sl].copy()
        d = self.diag[mb][:, None]
        soft = P.soft_thr(d * xb - g, self.mu if mut == "thr" else tau) / d
        D = (np.maximum(soft, 0.0) if self.positive else soft) - xb
        if self.positive:
            Dp, _ = R.feasible_image(D, xb, self.d_split)
        else:
            Dp = self.direction_image(D)
        self.note(Dp)
        err_new = PR.error_record(xb, g, tau, self.positive)
        err_old = PR.error_record(xb, g, self.mu + 0.0 * tau, self.positive)
        kc = self.w // self.kchunks
        S = sum(P.f32(Am[:, c * kc:(c + 1) * kc] @ Dp[c * kc:(c + 1) * kc]) for c in range(self.kchunks)).T
        S = np.where(self.Wk, S, 0.0)
        self.note(S)
        rs, ss = np.einsum("km,km->k", self.R, S), np.einsum("km,km->k", S, S)

        def line_search(wgt):
            r1 = rs + self.mu * ((wgt * np.abs(xb + Dp)).sum(axis=0) - (wgt * np.abs(xb)).sum(axis=0))
            return np.where(ss == 0.0, 0.0, np.clip(-r1 / np.where(ss == 0.0, 1.0, ss), 0.0, 1.0))

        gamma = line_search(np.ones_like(pb) if mut == "ls_norms" else pb)
        # what the clean model does from this state: where the mutant changed nothing, it did not act
        if mut is None:
            acted = False
        elif mut in ("thr", "shift", "block0"):
            soft_c = P.soft_thr(d * xb - g, p_true * self.mu) / d
            acted = bool(np.any(soft_c != soft)) or (mut != "thr" and bool(np.any(gamma != line_search(p_true))))
        elif mut == "ls_norms":
            acted = bool(np.any(gamma != line_search(p_true)))
        else:
            acted = False                                   # old_err: decided by the caller against check D's allowance
        self.x[sl] = P.f32(xb + gamma * Dp)
        self.R = self.R + gamma[:, None] * S
        self.note(self.x[sl])
        if self.carry:
            V = gamma[:, None] * S + (0.0 if exact else self.E)
            self.Vh = P.bf16(V)
            self.E = P.f32(V - self.Vh)
            self.note(self.Vh, self.E)
        self.gamma_last = gamma
        self.t += 1
        return (err_old if mut == "old_err" else err_new), dict(acted=acted, err_gap=abs(err_old - err_new))


def problem(m, n, k, masked):
    Ab, B, mu, pen, pen2 = PR.instance(m, n, k)
    return Ab, B, mu, pen, pen2, (P.fold_mask(m, k) if masked else None)


def run_checked(m, n, Block, k, masked, d_split, carry, positive, mutant=None, stats=None):
    """18 steps of the clean model, ``check_step_penalty`` at each; a mutant bends the single step from the clean
    state at t.  Per checkpoint (violations, acted)."""
    Ab, B, mu, pen, _, W = problem(m, n, k, masked)
    mod = PenModel(Ab, B, mu, Block, d_split, carry, pen, W=W, positive=positive)
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
        viol = PR.check_step_penalty(Ab, mod.diag, mu, pen, W, t % Block, snaps[t], after, err, d_split, exact,
                                     None if exact else snaps[t][1] - snaps[t - 1][1], chain=mod.chain, q=q,
                                     R_ref=None if exact else snaps[t - q][1], stats=stats, positive=positive)
        acted = info["acted"]
        if mutant == "old_err":
            Am = Ab[:, (t % Block) * mod.w:(t % Block + 1) * mod.w]
            sig = 2.0 ** -17 * np.sqrt(np.square(Am).T @ np.square(snaps[t][1]).T)
            acted = exact and info["err_gap"] > 2.0 * P.C_G * float(sig.max())
        out.append((viol, acted))
    return out


# 256 x 512, k 16: Block 1 and Block 2, masked and not
CASES = [(256, 512, 1, 16, False), (256, 512, 2, 16, False), (256, 512, 1, 16, True), (256, 512, 2, 16, True)]


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("m,n,Block,k,masked,d_split,carry",
                         [c + (ds, cg) for c in CASES for ds in (1, 2) for cg in ((1, 0) if c[2] == 1 else (0,))])
def test_model_passes(m, n, Block, k, masked, d_split, carry, positive):
    stats = {}
    res = run_checked(m, n, Block, k, masked, d_split, carry, positive, stats=stats)
    print(f"penalty model {m}x{n} B={Block} k={k} masked={masked} d_split={d_split} carry={carry} positive={positive}: "
          "worst ratio to bound " + " ".join(f"{key} {stats[key]:.3g}" for key in "ABCD"))
    for t, (viol, _) in enumerate(res):
        assert not viol, (t, viol)
    if positive:
        assert stats["x_min"] >= 0.0


MUTANT_CASES = [(256, 512, 1, 16, False, 1, 1), (256, 512, 1, 16, False, 1, 0), (256, 512, 2, 16, False, 1, 0),
                (256, 512, 2, 16, True, 2, 0)]


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("mutant,case", [(mt, c) for mt in MUTANTS for c in MUTANT_CASES if mt != "block0" or c[2] == 2])
def test_mutant_is_caught(mutant, case, positive):
    res = run_checked(*case, positive, mutant=mutant)
    acted = [t for t, (_, a) in enumerate(res) if a]
    missed = [t for t, (viol, a) in enumerate(res) if a and not viol]
    print(f"{mutant} {case} positive={positive}: acts at {len(acted)} checkpoints, missed at {missed}")
    assert acted, "the mutant never acted: the case does not exercise it"
    assert not missed
    if mutant == "block0":
        assert all(t % 2 == 1 for t in acted) and len(acted) == T_STEPS // 2
    if mutant == "old_err":
        for t in acted:
            assert any(v.startswith("D:") for v in res[t][0]), (t, res[t][0])


@pytest.mark.parametrize("positive", [False, True])
def test_certificate_slot_mutant(positive):
    """The certificate with max |g| in the slot instead of max |g_j| / p_j: ``check_certificate`` reports gnorm_inf
    (and scale, dual, gap where the scaling is active), on the model's iterate after 18 steps."""
    Ab, B, mu, pen, _, _ = problem(256, 512, 16, False)
    mod = PenModel(Ab, B, mu, 1, 1, 1, pen, positive=positive)
    for _ in range(T_STEPS):
        mod.step()
    ref = [C.penalty_duality_gap(Ab, B[:, c], None, mod.x[:, c], mu[c], pen, positive=positive) for c in range(16)]
    get = lambda key: np.array([r[key] for r in ref])  # noqa: E731
    good = {key: get(key) for key in ("primal", "dual", "gap", "scale", "gnorm_inf")}
    assert not PR.check_certificate(good, good)
    g = get("g")
    gn = (np.maximum(-g, 0.0) if positive else np.abs(g)).max(axis=1)      # the mutant's slot
    assert np.all(gn != good["gnorm_inf"])
    scale = np.where(gn > 0, np.minimum(1.0, mu / np.where(gn > 0, gn, 1.0)), 1.0)
    rr, rb = np.einsum("km,km->k", get("r"), get("r")), np.einsum("km,mk->k", get("r"), B)
    bad = dict(good, gnorm_inf=gn, scale=scale, dual=-0.5 * scale * scale * rr - scale * rb)
    bad["gap"] = bad["primal"] - bad["dual"]
    viol = PR.check_certificate(bad, good)
    assert any(v.startswith("gnorm_inf") for v in viol), viol
    # and it matters: the mutant's dual point is infeasible or needlessly small on some right-hand side
    assert np.any(np.abs(bad["gap"] - good["gap"]) > 1e-9 * good["primal"])


# ---------------------------------------------------------------------------
# (c) independent ground truth: the column-rescaled problem
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("Block,masked", [(1, False), (2, False), (1, True)])
def test_iterate_is_the_rescaled_unweighted_iterate(Block, masked):
    rs = np.random.RandomState(11)
    m, n = 64, 48
    A = rs.randn(m, n)
    b = A @ (rs.randn(n) * (rs.rand(n) < 0.4)) + 0.1 * rs.randn(m)
    p = PR.factors(n, seed=3)
    w = (np.arange(m) % 4 != 1).astype(np.uint8) if masked else np.ones(m, dtype=np.uint8)
    mu = 0.1 * float(np.max(np.abs(A.T @ b) / p))
    # the first 12 iterations, while the steps are large: ``masked_panel_iterate`` forms the line search's l1 change
    # as the difference of two sums, whose rounding (1e-14 absolute) reaches the step size once |S|^2 is small --
    # 7e-11 in x on a single step from a common state after 60 iterations -- and a difference grows by about 1.3
    # per iteration along the two trajectories; neither says anything about the maps
    for T in (1, 2, 3, 5, 8, 12):
        a = C.penalty_panel_iterate(A, b, w, mu, p, Block, T)
        z = C.masked_panel_iterate(A / p, b, w, mu, Block, T)
        np.testing.assert_allclose(a["x"], z["x"] / p, rtol=0, atol=1e-12 * np.abs(a["x"]).max() + 1e-300)
        np.testing.assert_allclose(a["r"], z["r"], rtol=0, atol=1e-12 * np.abs(b).max())
        ca = C.penalty_duality_gap(A, b, w, a["x"], mu, p)
        cz = C.masked_duality_gap(A / p, b, w, a["x"] * p, mu)
        for key in ("primal", "dual", "gap", "scale", "gnorm_inf", "holdout_sse"):
            assert abs(ca[key] - cz[key]) <= 1e-12 * max(abs(cz[key]), ca["primal"]), key
        assert np.array_equal(ca["keep"], cz["keep"]) or \
            np.all(np.abs(ca["score"] / p - cz["score"])[ca["keep"] != cz["keep"]] <= 1e-12 * mu)
    assert np.count_nonzero(a["x"]) >= 3 and np.count_nonzero(a["x"] == 0) >= 3


# ---------------------------------------------------------------------------
# (d) KKT, weak duality, the screen
# ---------------------------------------------------------------------------
def small(seed=5, m=64, n=32):
    rs = np.random.RandomState(seed)
    A = rs.randn(m, n)
    b = A @ (rs.randn(n) * (rs.rand(n) < 0.5)) + 0.1 * rs.randn(m)
    p = PR.factors(n, seed=seed + 100)
    mu = 0.1 * float(np.max(np.abs(A.T @ b) / p))
    return A, b, mu, p


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("intercept,masked", [(False, False), (False, True), (True, False), (True, True)])
def test_penalty_iterate_converges_to_kkt(intercept, masked, positive):
    A, b, mu, p = small()
    m, n = A.shape
    w = (np.arange(m) % 4 != 1).astype(np.uint8) if masked else None
    it, x0 = 0, None
    while True:       # as the non-negative lasso's host test runs it: 500 at a time to the bound, 20000 at the most
        res = C.penalty_panel_iterate(A, b, w, mu, p, 1, 500, x0=x0, intercept=intercept, positive=positive)
        it += 500
        cert = C.penalty_duality_gap(A, b, w, res["x"], mu, p, intercept=intercept, positive=positive)
        if cert["gap"] <= 1e-12 * cert["primal"] or it >= 20000:
            break
        x0 = res["x"]
    x, g = res["x"], cert["g"]
    on = x != 0
    print(f"penalty KKT intercept={intercept} masked={masked} positive={positive}: {it} iterations, gap / primal "
          f"{cert['gap'] / cert['primal']:.2e}, support {int(on.sum())}, max |g + mu p sign x| on it "
          f"{np.abs(g[on] + mu * p[on] * np.sign(x[on])).max():.2e}, max |g| / (mu p) off it "
          f"{(np.abs(g[~on]) / (mu * p[~on])).max():.4f}")
    assert cert["gap"] <= 1e-12 * cert["primal"]           # the bound of the non-negative lasso's host test
    assert on.sum() >= 3 and (~on).sum() >= 3
    np.testing.assert_allclose(res["r"], cert["r"], rtol=0, atol=1e-11 * np.abs(cert["r"]).max())
    tol = 10.0 * np.sqrt(2.0 * max(cert["gap"], 0.0)) * np.sqrt(np.square(A).sum(axis=0).max()) + 1e-12 * mu
    assert np.all(np.abs(g[on] + mu * p[on] * np.sign(x[on])) <= tol)      # equality and sign on the support
    if positive:
        assert np.all(x >= 0) and np.all(-g <= mu * p + tol)
    else:
        assert np.all(np.abs(g) <= mu * p + tol)
    # it is not the unweighted solution
    xu = (C.positive_panel_iterate(A, b, w, mu, 1, it, intercept=intercept) if positive else
          C.penalty_panel_iterate(A, b, w, mu, np.ones(n), 1, it, intercept=intercept))["x"]
    assert np.any((xu != 0) != on)
    # the screen is safe at every stage of the solve, while the gap is above the rounding of the primal
    xs, stages, screened = np.zeros(n), 0, 0
    for _ in range(40):
        c = C.penalty_duality_gap(A, b, w, xs, mu, p, intercept=intercept, positive=positive)
        assert np.array_equal(c["keep"], ~(c["score"] < mu * p))
        if c["gap"] <= 1e-10 * c["primal"]:
            break
        stages += 1
        screened = max(screened, int((~c["keep"]).sum()))
        assert np.all(c["keep"][on]), "the screen dropped a column of the converged support"
        xs = C.penalty_panel_iterate(A, b, w, mu, p, 1, 2, x0=xs, intercept=intercept, positive=positive)["x"]
    print(f"screen: {stages} stages checked, up to {screened} of {n} columns screened")
    assert stages >= 3 and screened >= 3


@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("intercept", [False, True])
def test_weak_duality_at_random_points(intercept, positive):
    A, b, mu, p = small(seed=9)
    m, n = A.shape
    w = (np.arange(m) % 5 != 2).astype(np.uint8)
    xs = C.penalty_panel_iterate(A, b, w, mu, p, 1, 2000, intercept=intercept, positive=positive)["x"]
    best = C.penalty_duality_gap(A, b, w, xs, mu, p, intercept=intercept, positive=positive)
    rs = np.random.RandomState(1)
    for _ in range(50):
        x = rs.randn(n) * (rs.rand(n) < 0.5) * rs.choice([1e-3, 1.0, 30.0])
        x = np.abs(x) if positive else x
        c = C.penalty_duality_gap(A, b, w, x, mu, p, intercept=intercept, positive=positive)
        assert c["gap"] >= -1e-12 * c["primal"]
        assert c["dual"] <= best["primal"] * (1 + 1e-12)           # any dual value below the optimum
        assert 0.0 < c["scale"] <= 1.0
        ga = np.maximum(-c["g"], 0.0) if positive else np.abs(c["g"])
        assert c["gnorm_inf"] == float(np.max(ga / p))
        assert np.all(c["scale"] * ga <= mu * p * (1 + 1e-12))     # scale r is dual feasible
    # mu_max: the x = 0 certificate's slot; just above it x = 0 is the solution, just below it is not
    c0 = C.penalty_duality_gap(A, b, w, np.zeros(n), mu, p, intercept=intercept, positive=positive)
    mu_max = c0["gnorm_inf"]
    assert not C.penalty_panel_iterate(A, b, w, mu_max * 1.001, p, 1, 5, intercept=intercept, positive=positive)["x"].any()
    assert C.penalty_panel_iterate(A, b, w, mu_max * 0.999, p, 1, 5, intercept=intercept, positive=positive)["x"].any()


def test_factor_vector_is_validated_in_the_restatement():
    A, b, mu, p = small()
    for bad in (p[:-1], np.where(np.arange(p.size) == 3, 0.0, p), -p, np.where(np.arange(p.size) == 0, np.inf, p),
                np.where(np.arange(p.size) == 5, np.nan, p)):
        with pytest.raises(ValueError):
            C.penalty_panel_iterate(A, b, None, mu, bad, 1, 1)
        with pytest.raises(ValueError):
            C.penalty_duality_gap(A, b, None, np.zeros(A.shape[1]), mu, bad)


# ---------------------------------------------------------------------------
# (e) exact scaling in the model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("Block,d_split,carry", [(1, 1, 1), (1, 1, 0), (1, 2, 1), (2, 1, 0), (2, 2, 0)])
def test_power_of_two_factors_are_an_exact_rescaling(Block, d_split, carry):
    """With p_j = 2^e_j the model on A equals, bit for bit, the feature-off model (tests/test_panel_step_host.py's
    ``Model``) on A diag(1 / p) -- exactly representable in bf16 -- with z = p o x: every product and rounding
    commutes with the scaling as long as nothing leaves the normal range, which is asserted.  With the hi + lo
    direction a coordinate that the shrink sends to zero keeps 2^-16 of itself per visit and reaches the fp32
    subnormals at the 14th iteration of this instance (there the scaling stops being exact, in the model as on any
    hardware): those cases run 10 iterations."""
    Ab, B, mu, _, p2, _ = problem(256, 512, 16, False)
    As = Ab / p2
    assert np.array_equal(P.bf16(As), As)
    on = PenModel(Ab, B, mu, Block, d_split, carry, p2)
    off = H.Model(As, B, mu, Block, d_split, carry)
    for t in range(T_STEPS if d_split == 1 else 10):
        on.step()
        off.step()
        assert np.array_equal(off.x, p2[:, None] * on.x), t
        assert np.array_equal(off.R, on.R), t
        assert np.array_equal(off.gamma_prev, on.gamma_last), t
    print(f"exact scaling B={Block} d_split={d_split} carry={carry}: smallest nonzero fp32 / bf16 magnitude {on.tiny:.3g}")
    assert on.tiny >= 4.0 * 2.0 ** -126 * 2.0 ** 8         # no subnormal, also after a scaling by 1/4 and in a bf16 lo piece
    assert on.x.any()


@pytest.mark.parametrize("Block,d_split,carry", [(1, 1, 1), (2, 2, 0)])
def test_all_ones_factors_are_the_feature_off_model(Block, d_split, carry):
    Ab, B, mu, _, _, W = problem(256, 512, 16, True)
    on = PenModel(Ab, B, mu, Block, d_split, carry, np.ones(512), W=W)
    off = H.Model(Ab, B, mu, Block, d_split, carry, W=W)
    for t in range(T_STEPS):
        e_on, _ = on.step()
        e_off, _ = off.step()
        assert np.array_equal(off.x, on.x) and np.array_equal(off.R, on.R) and e_on == e_off, t


# ---------------------------------------------------------------------------
# (f) the instance is informative
# ---------------------------------------------------------------------------
def test_instance_is_informative():
    Ab, B, mu, pen, _, _ = problem(256, 512, 16, False)
    diff, wei, unw = PR.support_difference(Ab, B, mu, pen, iters=1000)
    print(f"penalty instance 256 x 512 k 16: columns in exactly one of the two supports, per right-hand side {diff.tolist()}")
    assert np.all(diff >= 10), diff
    # and the certificate's screen has no borderline entry at this instance (the GPU test caps them at 1 %)
    for c in (0, 7, 15):
        cert = C.penalty_duality_gap(Ab, B[:, c], None, P.f32(wei[c]), mu[c], pen)
        assert not np.any(np.abs(cert["score"] - mu[c] * pen) <= 1e-9 * mu[c] * pen)


# ---------------------------------------------------------------------------
# (g) argument checks that need no GPU
# ---------------------------------------------------------------------------
def test_python_argument_errors():
    import inspect

    import torch

    from convex_optimization_amd import panel
    n = 256
    good = PR.factors(n)
    assert panel._check_penalty(None, n) is None
    assert np.array_equal(panel._check_penalty(good, n), good)
    assert np.array_equal(panel._check_penalty(torch.from_numpy(good.astype(np.float32)), n), good.astype(np.float32))
    for bad in (good[:-1], good.reshape(16, 16), np.where(np.arange(n) == 7, 0.0, good), -good,
                np.where(np.arange(n) == 0, np.inf, good), np.where(np.arange(n) == n - 1, np.nan, good)):
        with pytest.raises(ValueError, match="penalty factor"):
            panel._check_penalty(bad, n)
    for f in (panel.lasso_path, panel.lasso_cv):
        assert inspect.signature(f).parameters["penalty_factors"].default is None
    # the drivers check the vector before any device work
    A = np.zeros((256, n))
    for bad in (good[:-1], np.zeros(n), np.full(n, np.nan)):
        with pytest.raises(ValueError, match="penalty factor"):
            panel.lasso_path(A, np.zeros(256), mus=[1.0], penalty_factors=bad)
        with pytest.raises(ValueError, match="penalty factor"):
            panel.lasso_cv(A, np.zeros(256), mus=[1.0], penalty_factors=bad)
    assert hasattr(panel.PanelLasso, "set_penalty_factors")

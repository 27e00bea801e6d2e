"""Observation weights of the panel path (bpgl_panel_set_row_weights, ABI 310), without a GPU.

(1) the ABI is there: bpgl_version() >= 310 (310 is this feature's number; a later ABI keeps the symbol) and
    bpgl_panel_set_row_weights(NULL, ...) is BPGL_E_ARG.
(2) ``weighted_panel_iterate`` on (A, b, omega) is the existing plain restatement on the scaled problem
    (diag(sqrt omega) A, sqrt(omega) o b) with the SAME ``diag=`` handed to both: x to 1e-9 relative, the project's fp64
    parity bound; with ``positive`` / ``p`` against ``positive_panel_iterate`` / ``penalty_panel_iterate`` there.  With
    the intercept the scaled problem's unpenalised column is sqrt(omega), not a constant, so the plain restatement runs
    on the scaled data projected off u = sqrt(omega) / |sqrt(omega)| (profiling that column out).  With 0/1 weights it
    is ``masked_panel_iterate`` to the same bound, on the row-deleted and explicitly centred problem with the intercept.
(3) ``weighted_duality_gap`` against ``masked_duality_gap`` of the scaled (projected) problem: scalars to 1e-12 relative;
    dual <= the primal of a long fp64 run (weak duality); that run's support lies inside keep.
(4) ``panel_weight_reference.check_step_weighted`` separates right from wrong.  The "device" is ``WModel``, a numpy model
    of the weighted iteration with tests/test_panel_step_host.py's operand roundings (R^ -> hi + lo bf16, g -> fp32, the
    carried recurrence, D -> bf16 or hi + lo, s in fp32 per pass-2 chunk, x -> fp32, fp64 elsewhere).  Its own
    trajectories pass at each of 18 checkpoints; each of six mutants is caught by the check named beside it at every
    checkpoint where it acts, and acts:
      curv_sq      B   the curvature from s^ . s^
      num_sq       B   the numerator from R^ . s^
      upd_unw      A   the update with the unweighted s
      zero_row     A   a zero-weight row updated (exactly-zero part of A)
      mean_unw     A   the intercept's mean of s taken unweighted, over all rows
      centre_plain A   the centring update s - c instead of s^ - c w
    and the steps are informative on the unrounded model: the median over the right-hand sides of |dx| / |x| stays
    >= 1e-3 at every checkpoint.
(5) the Python argument errors that need no GPU.
"""
import copy

import numpy as np
import pytest

import panel_step_reference as P
import panel_weight_reference as WR
import test_panel_step_host as H
from convex_optimization_amd import cpu_calculation as C

T_STEPS, G_REFRESH = H.T_STEPS, H.G_REFRESH
REL = 1e-9


# ---------------------------------------------------------------------------
# (1) the ABI
# ---------------------------------------------------------------------------
def test_abi_310_has_set_row_weights():
    from convex_optimization_amd import _native as N
    from convex_optimization_amd import panel
    L = panel._lib()
    assert L.bpgl_version() >= 310
    assert "bpgl_panel_set_row_weights" in N.header_functions()
    assert "bpgl_panel_set_row_weights" in N._SIGS
    assert L.bpgl_panel_set_row_weights(None, None, None) == -1            # BPGL_E_ARG
    assert b"null" in L.bpgl_last_error()


# ---------------------------------------------------------------------------
# (2), (3) the restatements against the scaled problem
# ---------------------------------------------------------------------------
def small(seed=0, m=96, n=48):
    rs = np.random.RandomState(seed)
    A = rs.randn(m, n) / np.sqrt(m)
    x = rs.randn(n) * (rs.rand(n) < 0.3)
    b = A @ x + 0.05 * rs.randn(m) + 1.5
    om = 1.0 - 0.95 * rs.rand(m)
    om[rs.rand(m) < 0.125] = 0.0
    pen = np.exp(rs.uniform(-1.0, 1.0, n))
    return A, b, om, pen


def scaled(A, b, om, intercept):
    """(A~, b~): diag(sqrt om) A and sqrt(om) o b, projected off sqrt(om) with ``intercept``."""
    sq = np.sqrt(om)
    At, bt = sq[:, None] * A, sq * b
    if intercept:
        u = sq / np.linalg.norm(sq)
        At, bt = At - np.outer(u, u @ At), bt - u * (u @ bt)
    return At, bt


def plain_iterate(At, bt, mu, iters, dg, positive, pen):
    ones = np.ones(At.shape[0])
    if pen is not None:
        return C.penalty_panel_iterate(At, bt, None, mu, pen, 1, iters, diag=dg, positive=positive)
    if positive:
        return C.positive_panel_iterate(At, bt, None, mu, 1, iters, diag=dg)
    return C.masked_panel_iterate(At, bt, ones, mu, 1, iters, diag=dg)


@pytest.mark.parametrize("intercept,positive,use_p", [(False, False, False), (True, False, False), (False, True, False),
                                                      (False, False, True), (True, True, True)])
def test_restatement_is_the_scaled_problem(intercept, positive, use_p):
    A, b, om, pen = small()
    pen = pen if use_p else None
    dg = C.centred_diag(A) if intercept else np.square(A).sum(axis=0)      # the same diag to both
    At, bt = scaled(A, b, om, intercept)
    mu = 0.2 * float(np.max(np.abs(At.T @ bt) / (pen if use_p else 1.0)))
    # the first 12 iterations, as tests/test_panel_penalty_host.py (c) does and for its reason: a difference between two
    # fp64 trajectories grows by about 1.3 per iteration, which says nothing about the maps
    for iters in (1, 2, 3, 5, 8, 12):
        got = C.weighted_panel_iterate(A, b, om, mu, iters, diag=dg, intercept=intercept, positive=positive, p=pen)
        ref = plain_iterate(At, bt, mu, iters, dg, positive, pen)
        assert np.count_nonzero(ref["x"]) > 0
        np.testing.assert_allclose(got["x"], ref["x"], rtol=0, atol=REL * np.abs(ref["x"]).max())
        # the carried residual is sqrt(w) times the scaled problem's
        np.testing.assert_allclose(got["r"], np.sqrt(om) * ref["r"], rtol=0, atol=REL * np.abs(ref["r"]).max())


@pytest.mark.parametrize("intercept", [False, True])
def test_zero_one_weights_are_the_masked_restatement(intercept):
    """With the intercept ``intercept_panel_iterate`` is the same code as ``weighted_panel_iterate``, so the reference
    is ``masked_panel_iterate`` on the row-deleted, explicitly centred problem (as
    panel_intercept_instance.row_deleted_reference builds it), the centred data's own column norms handed to both."""
    A, b, om, _ = small(1)
    w = (om > 0.5).astype(np.float64)
    idx = w != 0
    mu = 0.2 * float(np.max(np.abs(A.T @ (w * b))))
    if intercept:
        Ai, bi = A[idx] - A[idx].mean(axis=0), b[idx] - b[idx].mean()
        dg = np.square(Ai).sum(axis=0)
    else:
        dg = np.square(A).sum(axis=0)
    for iters in (1, 2, 3, 5, 8, 12):
        got = C.weighted_panel_iterate(A, b, w, mu, iters, diag=dg, intercept=intercept)
        if intercept:
            sub = C.masked_panel_iterate(Ai, bi, np.ones(int(idx.sum())), mu, 1, iters, diag=dg)
            r = np.zeros(A.shape[0])                 # the held-out rows of the carried residual are 0
            r[idx] = sub["r"]
            ref = dict(x=sub["x"], r=r, intercept=float(b[idx].mean() - A[idx].mean(axis=0) @ sub["x"]))
        else:
            ref = C.masked_panel_iterate(A, b, w, mu, 1, iters, diag=dg)
        np.testing.assert_allclose(got["x"], ref["x"], rtol=0, atol=REL * np.abs(ref["x"]).max())
        np.testing.assert_allclose(got["r"], ref["r"], rtol=0, atol=REL * np.abs(ref["r"]).max())
        if intercept:
            assert abs(got["intercept"] - ref["intercept"]) <= REL * abs(ref["intercept"])
    assert np.count_nonzero(got["x"]) >= 3


def test_row_weight_errors_of_the_restatement():
    A, b, om, _ = small()
    for bad in (np.where(np.arange(om.size) == 3, 1.5, om), np.where(np.arange(om.size) == 3, -0.1, om),
                np.where(np.arange(om.size) == 3, np.nan, om), om[:-1]):
        with pytest.raises(ValueError):
            C.weighted_panel_iterate(A, b, bad, 0.1, 1)
        if bad.size == om.size:
            with pytest.raises(ValueError):
                C.weighted_duality_gap(A, b, bad, np.zeros(A.shape[1]), 0.1)


@pytest.mark.parametrize("intercept", [False, True])
def test_certificate_is_the_scaled_problems(intercept):
    A, b, om, _ = small(2)
    dg = C.centred_diag(A) if intercept else np.square(A).sum(axis=0)
    At, bt = scaled(A, b, om, intercept)
    mu = 0.15 * float(np.max(np.abs(At.T @ bt)))
    ones = np.ones(A.shape[0])
    long = C.weighted_panel_iterate(A, b, om, mu, 20000, diag=dg, intercept=intercept)
    p_star = C.weighted_duality_gap(A, b, om, long["x"], mu, diag=dg, intercept=intercept)
    assert p_star["gap"] <= 1e-10 * p_star["primal"]
    rs = np.random.RandomState(5)
    for x in (np.zeros(A.shape[1]), C.weighted_panel_iterate(A, b, om, mu, 30, diag=dg, intercept=intercept)["x"],
              long["x"], rs.randn(A.shape[1]) * 0.1):
        got = C.weighted_duality_gap(A, b, om, x, mu, diag=dg, intercept=intercept)
        ref = C.masked_duality_gap(At, bt, ones, x, mu, diag=dg)
        for key in ("primal", "dual", "scale", "gnorm_inf"):
            assert abs(got[key] - ref[key]) <= 1e-12 * abs(ref[key]), key
        assert abs(got["gap"] - ref["gap"]) <= 1e-12 * abs(ref["primal"])
        np.testing.assert_allclose(got["g"], ref["g"], rtol=0, atol=1e-12 * np.abs(ref["g"]).max())
        assert got["dual"] <= p_star["primal"] * (1 + 1e-12)                # weak duality
        assert np.all(got["keep"][long["x"] != 0.0])                        # the optimum's support is kept
        # the held-out score against its definition, default and explicit scoring weights
        e = A @ x - b + got["intercept"]
        assert abs(got["holdout_sse"] - float((om == 0) @ (e * e))) <= 1e-12 * float(e @ e)
        h = rs.rand(A.shape[0])
        sse = C.weighted_duality_gap(A, b, om, x, mu, diag=dg, intercept=intercept, hold=h)["holdout_sse"]
        assert abs(sse - float(h @ (e * e))) <= 1e-12 * float(e @ e)
        if intercept:
            nw = om.sum()
            assert abs(got["intercept"] + float(om @ (A @ x - b)) / nw) <= 1e-12 * (1 + abs(got["intercept"]))


# ---------------------------------------------------------------------------
# (4) the numpy model and its mutants
# ---------------------------------------------------------------------------
MUTANTS = {"curv_sq": "B", "num_sq": "B", "upd_unw": "A", "zero_row": "A", "mean_unw": "A", "centre_plain": "A"}
ICPT_ONLY = ("mean_unw", "centre_plain")


class WModel:
    """k right-hand sides with weights Wt (m, k), one feature block, one update per ``step``."""

    def __init__(self, Ab, B, mu, Wt, d_split, carry, intercept=False, rounding=True, mutant=None):
        self.Ab, self.mu, self.d_split, self.carry = Ab, np.asarray(mu, dtype=np.float64), d_split, bool(carry)
        self.m, self.n = Ab.shape
        self.k = B.shape[1]
        self.Wk = np.asarray(Wt, dtype=np.float64).T.copy()
        self.nw = self.Wk.sum(axis=1)
        self.icpt = bool(intercept)
        self.diag = C.centred_diag(Ab) if intercept else np.square(Ab).sum(axis=0)
        self.kchunks = H.auto_kchunks(self.m, self.n)
        self.chain = d_split * (self.n // self.kchunks)
        self.rounding, self.mutant = rounding, mutant
        self.x = np.zeros((self.n, self.k))
        Bt = B.T
        self.R = -self.Wk * (WR.wcentre(self.Wk, Bt) if intercept else Bt)
        self.t = 0
        self.Gc = self.E = self.Vh = None

    def rnd(self, f, v):
        return f(v) if self.rounding else np.asarray(v, dtype=np.float64)

    def step(self):
        """One iteration; returns (err, acted): ``acted`` is False where the mutant provably changed nothing."""
        mut, Ab, Wk = self.mutant, self.Ab, self.Wk
        exact = not self.carry or self.t % G_REFRESH == 0
        if exact:
            op = self.R
            if self.rounding:
                hi, lo = P.split_bf16(self.R)
                op = hi + lo
        else:
            op = self.Vh
        prod = self.rnd(P.f32, Ab.T @ op.T)
        g = prod if exact else self.rnd(P.f32, self.Gc + prod)
        if self.carry:
            self.Gc = g
        d = self.diag[:, None]
        x = self.x
        D = P.soft_thr(d * x - g, self.mu) / d - x
        if not self.rounding:
            Dp = D
        elif self.d_split == 1:
            Dp = P.bf16(D)
        else:
            hi, lo = P.split_bf16(D)
            Dp = hi + lo
        err = float(np.max(np.abs(g - np.clip(g - x, -self.mu, self.mu))))
        kc = self.n // self.kchunks
        S = sum(self.rnd(P.f32, Ab[:, c * kc:(c + 1) * kc] @ Dp[c * kc:(c + 1) * kc]) for c in range(self.kchunks)).T
        Wf = np.where(Wk == 0.0, 0.5, Wk) if mut == "zero_row" else Wk       # mutant: the zero-weight rows take part
        Sh = Wf * S
        l1 = lambda v: np.abs(v).sum(axis=0)      # noqa: E731
        nws = np.where(self.nw > 0, self.nw, 1.0)

        def line_search(rs, ss, c, sm):
            r1 = rs + self.mu * (l1(x + Dp) - l1(x))
            cv = ss - c * sm
            return np.where(cv <= 0.0, 0.0, np.clip(-r1 / np.where(cv <= 0.0, 1.0, cv), 0.0, 1.0))

        dot = lambda a, b: np.einsum("km,km->k", a, b)      # noqa: E731
        sm = Sh.sum(axis=1)
        c_clean = np.where(self.nw > 0, sm / nws, 0.0) if self.icpt else np.zeros(self.k)
        c = S.sum(axis=1) / self.m if mut == "mean_unw" else c_clean
        clean = line_search(dot(self.R, S), dot(S, Wk * S), c_clean, (Wk * S).sum(axis=1) if self.icpt else 0.0)
        rs = dot(self.R, Sh) if mut == "num_sq" else dot(self.R, S)
        ss = dot(Sh, Sh) if mut == "curv_sq" else dot(S, Sh)
        gamma = line_search(rs, ss, c, sm if self.icpt else 0.0)
        step = Sh - c[:, None] * Wf
        if mut == "upd_unw":
            step = S - c[:, None] * Wf
        if mut == "centre_plain":
            step = S - c[:, None]
        acted = False
        if mut in ("curv_sq", "num_sq"):
            # a step size of 0 leaves no step to check (x and R^ do not move: a stall, which the trajectory tests see)
            acted = bool(np.any((gamma != clean) & (gamma != 0.0)))
        elif mut == "mean_unw":
            acted = bool(np.any((gamma != 0.0) & (c != c_clean)))
        elif mut is not None:
            acted = bool(np.any(gamma[:, None] * (step - (Wk * S - c_clean[:, None] * Wk)) != 0.0))
        self.x = self.rnd(P.f32, x + gamma * Dp)
        self.R = self.R + gamma[:, None] * step
        if self.carry:
            V = gamma[:, None] * step + (0.0 if exact else self.E)
            self.Vh = self.rnd(P.bf16, V)
            self.E = self.rnd(P.f32, V - self.Vh)
        self.t += 1
        return err, acted

    def snap(self):
        return self.x.copy(), self.R.copy()

    def clone(self, mutant):
        c = copy.copy(self)
        c.x, c.mutant = self.x.copy(), mutant
        return c


def run_checked(m, n, k, intercept, d_split, carry, mutant=None, stats=None):
    """18 steps of the model, check_step_weighted at each; per checkpoint (violations, acted).  A mutant bends the
    single step from the clean trajectory's state at t, as in tests/test_panel_step_host.py."""
    Ab, B, mu, Wt = WR.problem(m, n, k)
    mod = WModel(Ab, B, mu, Wt, d_split, carry, intercept=intercept)
    out, snaps = [], [mod.snap()]
    for t in range(T_STEPS):
        if mutant is not None:
            bent = mod.clone(mutant)
            err, acted = bent.step()
            after = bent.snap()
            mod.step()
        else:
            err, acted = mod.step()
            after = mod.snap()
        snaps.append(mod.snap())
        q = t % G_REFRESH if mod.carry else 0
        exact = not mod.carry or q == 0
        viol = WR.check_step_weighted(Ab, mod.diag, mu, Wt, B, t, snaps[t], after, err, d_split, exact,
                                      None if exact else snaps[t][1] - snaps[t - 1][1], chain=mod.chain, q=q,
                                      R_ref=None if exact else snaps[t - q][1], stats=stats, intercept=intercept)
        out.append((viol, acted))
    return out


# (m, n, k): the smallest shapes of the two-kernel fold and of the fused form
SHAPES = [(256, 512, 16), (1024, 512, 16)]
MODEL_CASES = [s + (ic, ds, cg) for s in SHAPES for ic in (False, True) for ds, cg in ((1, 1), (2, 0))]


@pytest.mark.parametrize("m,n,k,intercept,d_split,carry", MODEL_CASES)
def test_model_passes(m, n, k, intercept, d_split, carry):
    stats = {}
    res = run_checked(m, n, k, intercept, d_split, carry, stats=stats)
    print(f"weighted model {m}x{n} k={k} intercept={intercept} d_split={d_split} carry={carry}: worst ratio to bound "
          + " ".join(f"{key} {stats[key]:.3g}" for key in "ABCD") + (f" 0' {stats['0']:.3g}" if intercept else ""))
    for t, (viol, _) in enumerate(res):
        assert not viol, (t, viol)


# the curvature mutant only ever raises the step size, and on the overdetermined 1024 x 512 shape the clean one is
# already clipped at 1: it runs on the two-kernel shape at two panel widths instead
MUTANT_SHAPES = {"curv_sq": [(256, 512, 16), (256, 512, 32)]}


@pytest.mark.parametrize("mutant,case", [(mu, s + (mu in ICPT_ONLY or ic, 1, 1)) for mu in MUTANTS
                                         for s in MUTANT_SHAPES.get(mu, SHAPES)
                                         for ic in ((True,) if mu in ICPT_ONLY else (False, True))])
def test_mutant_is_caught(mutant, case):
    res = run_checked(*case, mutant=mutant)
    tag = MUTANTS[mutant] + ":"
    acted = [t for t, (_, a) in enumerate(res) if a]
    missed = [t for t, (viol, a) in enumerate(res) if a and not any(v.startswith(tag) for v in viol)]
    print(f"{mutant} {case}: acts at {len(acted)} checkpoints, missed by check {tag[0]} at {missed}")
    assert acted, "the mutant never acted: the case does not exercise it"
    assert not missed


INFORMATIVE_STEPS = {(1024, 512): 10}    # as tests/test_panel_step_host.py: the overdetermined shape converges fast


@pytest.mark.parametrize("m,n,k", SHAPES)
@pytest.mark.parametrize("intercept", [False, True])
def test_steps_are_informative(m, n, k, intercept):
    Ab, B, mu, Wt = WR.problem(m, n, k)
    mod = WModel(Ab, B, mu, Wt, 2, 0, intercept=intercept, rounding=False)
    worst = np.inf
    for t in range(INFORMATIVE_STEPS.get((m, n), T_STEPS)):
        x0 = mod.x.copy()
        mod.step()
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.linalg.norm(mod.x - x0, axis=0) / np.linalg.norm(mod.x, axis=0)
        worst = min(worst, float(np.median(rel)))
        assert np.median(rel) >= 1e-3, (t, float(np.median(rel)))
    print(f"informativeness {m}x{n} k={k} intercept={intercept}: min over t of the median |dx|/|x| = {worst:.3g}")


@pytest.mark.parametrize("intercept", [False, True])
def test_t_ref_of_the_trajectory_instance(intercept):
    """tests/test_panel_weights.py::test_weighted_trajectory gives the device 4 T_ref iterations of ITER_MAX = 4096: the
    reference alone must meet T_ref <= ITER_MAX / 4."""
    T = WR.weighted_t_ref(256, 512, 16, intercept)
    print(f"weighted T_ref intercept={intercept}: {T}")
    assert T <= 4096 // 4


def test_weights_instance():
    for m, k in ((256, 16), (1024, 16), (4096, 128)):
        w = WR.general_weights(m, k)
        assert w.shape == (m, k) and np.all((w == 0.0) | ((w > 0.05) & (w <= 1.0)))
        assert 0.09 < np.mean(w == 0.0) < 0.16
        assert not np.array_equal(w[:, 0], w[:, 1])
        assert np.array_equal(w, WR.general_weights(m, k))                   # a fixed seed
        p4 = WR.pow4_weights(m, k)
        assert set(np.unique(p4)) == {0.0, 0.0625, 0.25, 1.0}


# ---------------------------------------------------------------------------
# (5) argument checks that need no GPU
# ---------------------------------------------------------------------------
def test_python_argument_checks():
    from convex_optimization_amd import panel
    w = np.full((8, 16), 0.5)
    assert panel._check_row_weights(None, 8, 16, "weights", 1.0) is None
    assert panel._check_row_weights(w, 8, 16, "weights", 1.0).shape == (16, 8)
    assert panel._check_row_weights(w[:, 0], 8, 16, "weights", 1.0).shape == (16, 8)
    for bad in (1.5, -0.1, np.nan, np.inf):
        v = w.copy()
        v[3, 2] = bad
        with pytest.raises(ValueError):
            panel._check_row_weights(v, 8, 16, "weights", 1.0)
    with pytest.raises(ValueError):
        panel._check_row_weights(w[:, :3], 8, 16, "weights", 1.0)
    v = w.copy()
    v[0, 0] = 7.0
    assert panel._check_row_weights(v, 8, 16, "holdout", np.inf)[0, 0] == 7.0  # scoring weights: any finite value >= 0
    for bad in (-1.0, np.nan, np.inf):
        v[0, 0] = bad
        with pytest.raises(ValueError):
            panel._check_row_weights(v, 8, 16, "holdout", np.inf)
    om = np.arange(8.0)
    assert np.array_equal(panel._check_sample_weight(om, 8, 1), om)
    for bad, blk in ((np.zeros(8), 1), (-om, 1), (np.where(om == 2, np.nan, om), 1), (om[:-1], 1), (om, 2)):
        with pytest.raises(ValueError):
            panel._check_sample_weight(bad, 8, blk)

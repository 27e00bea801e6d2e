"""The panel intercept without a GPU: the host restatements against the problem
stated the long way, the iteration counts the design quotes, and the step checker against a numpy model
of the device iteration and seven mutants of it.

* ``intercept_panel_iterate`` / ``intercept_duality_gap`` agree with ``masked_panel_iterate`` on each
  fold's row-DELETED, explicitly centred data (x, beta0 and the held-out sum of squares within 1e-6
  relative after 4096 iterations; convergence is the limit, measured 1.2e-7 on x);
* the T_ref the design quotes: 128 / 64 / 320 iterations on the three offset instances, and on
  ``big_offset_instance`` 192 with the centred diag against 1472 with ||a_j||^2;
* the gap-safe screen with the centred diag keeps the support of every row-deleted reference;
* ``centred_diag`` is exactly 0 on a constant column;
* ``check_step_intercept`` (A-D, 0') passes on ``IModel`` -- test_panel_step_host.py's ``Model`` with the
  intercept's fold, line search, update and reset -- and catches each of its mutants wherever it acts;
  the two mutants that live in the certificate are caught by ``check_certificate``.
"""
import copy
import functools

import numpy as np
import pytest

import panel_intercept_reference as Q
import panel_step_reference as P
from convex_optimization_amd import cpu_calculation as C
from panel_intercept_instance import (big_offset_instance, cv_t_ref, offset_instance, row_deleted_reference,
                                      screened_reference, sparse_offset_instance, t_ref)
from test_panel_step_host import G_REFRESH, T_STEPS, auto_kchunks

INSTANCES = [(256, 512), (1024, 512), (256, 1024)]


# --------------------------------------------------------------------------------------------------
# the restatements
# --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_runs(m, n, f):
    """Fold f at the smallest mu of the grid: (the row-deleted centred reference, the intercept iteration),
    4096 iterations each."""
    Ab, b, _, _, _, masks, mus = offset_instance(m, n)
    return row_deleted_reference(Ab, b, masks[f], mus[-1]), C.intercept_panel_iterate(Ab, b, masks[f], mus[-1], 4096)


@pytest.mark.parametrize("f", range(4))
@pytest.mark.parametrize("m,n", INSTANCES)
def test_restatement_is_the_row_deleted_centred_problem(m, n, f):
    Ab, b, _, _, _, masks, mus = offset_instance(m, n)
    ref, run = long_runs(m, n, f)
    cert = C.intercept_duality_gap(Ab, b, masks[f], run["x"], mus[-1])
    rel_x = np.linalg.norm(run["x"] - ref["x"]) / np.linalg.norm(ref["x"])
    rel_b = abs(cert["intercept"] - ref["intercept"]) / abs(ref["intercept"])
    rel_s = abs(cert["holdout_sse"] - ref["holdout_sse"]) / ref["holdout_sse"]
    print(f"{m}x{n} fold {f}: x rel {rel_x:.2e}, beta0 {cert['intercept']:.6f} rel {rel_b:.2e}, sse rel {rel_s:.2e}")
    assert ref["x"].any() and rel_x <= 1e-6 and rel_b <= 1e-6 and rel_s <= 1e-6
    assert run["intercept"] == cert["intercept"]
    # the carried residual is the centred one of the final x, and it sums to zero over the in-rows
    np.testing.assert_allclose(run["r"], cert["r"], rtol=0, atol=1e-12 * np.abs(cert["r"]).max())
    assert abs(cert["r"][masks[f] != 0].sum()) <= 1e-12 * np.abs(cert["r"]).sum() and not cert["r"][masks[f] == 0].any()
    # the same objective as the problem stated the long way
    assert abs(cert["primal"] - ref["objective"]) <= 1e-9 * ref["objective"]


@pytest.mark.parametrize("m,n,T", [(256, 512, 128), (1024, 512, 64), (256, 1024, 320)])
def test_t_ref_of_the_offset_instances(m, n, T):
    assert cv_t_ref(m, n) == T


def test_centred_diag_is_seven_times_faster_on_big_offsets():
    Ab, b, w, mu = big_offset_instance()
    tc = t_ref(Ab, b, w, mu, C.centred_diag(Ab))
    tu = t_ref(Ab, b, w, mu, np.square(Ab).sum(axis=0))
    print(f"big offsets: {tc} iterations with the centred diag, {tu} with ||a_j||^2")
    assert (tc, tu) == (192, 1472) and tu >= 7 * tc


@pytest.mark.parametrize("m,n", INSTANCES)
def test_screen_keeps_the_row_deleted_support(m, n):
    Ab, b, _, _, _, masks, mus = offset_instance(m, n)
    T = cv_t_ref(m, n)
    for f in range(4):
        ref = long_runs(m, n, f)[0]
        x = C.intercept_panel_iterate(Ab, b, masks[f], mus[-1], T)["x"].astype(np.float32).astype(np.float64)
        cert = C.intercept_duality_gap(Ab, b, masks[f], x, mus[-1])
        supp = np.abs(ref["x"]) > 2.0 ** -52 * np.abs(ref["x"]).max()
        assert supp.any() and not np.any(supp & ~cert["keep"]), f
        # and the certificate is sound for the problem stated the long way: P(x) - P* <= gap
        assert cert["primal"] - ref["objective"] <= cert["gap"] + 1e-9 * cert["primal"]


def test_reference_schedule_of_the_screened_path():
    """What tests/test_panel_intercept.py's lasso_path(fit_intercept=True, shrink=0.75) case rests on: in fp64
    the sparse offset instance compacts at the first check and stops at the second, as without compaction."""
    Ab, b, mus = sparse_offset_instance()
    ref = screened_reference(Ab, b, mus, 3e-6, 1024, 64, 0.75)
    assert ref["compactions"] == [(64, 1280)] and ref["t"] == 128 and ref["reached"].all()
    plain = screened_reference(Ab, b, mus, 3e-6, 1024, 64, 0.0)
    assert plain["compactions"] == [] and plain["t"] == 128 and plain["reached"].all()


def test_centred_diag_of_a_constant_column_is_exactly_zero():
    Ab = offset_instance(256, 512)[0].copy()
    Ab[:, 7] = Ab[0, 7]
    Ab[:, 300] = 0.0
    Ab[:, 301] = 0.1          # not a bf16 value: the sum of 256 of them is inexact, the deviations are not
    d = C.centred_diag(Ab)
    assert d[7] == 0.0 and d[300] == 0.0 and d[301] == 0.0 and np.all(np.delete(d, [7, 300, 301]) > 0)
    np.testing.assert_allclose(d, np.square(Ab - Ab.mean(axis=0)).sum(axis=0), rtol=1e-12, atol=1e-28)
    # d dominates every fold's curvature || P_w a_j ||^2
    for w in C.kfold_masks(256, 4, seed=7):
        wf = w.astype(np.float64)
        Pa = wf[:, None] * (Ab - (wf @ Ab) / wf.sum())
        # (+ 1e-28: the fold mean of the 0.1 column rounds, so its P_w a is ~1e-17, not 0)
        assert np.all(np.square(Pa).sum(axis=0) <= d * (1 + 1e-12) + 1e-28)
    # the iteration leaves the constant columns at 0 and produces no NaN
    b = offset_instance(256, 512)[1]
    run = C.intercept_panel_iterate(Ab, b, np.ones(256), 0.05, 64)
    assert np.all(np.isfinite(run["x"])) and run["x"].any() and not run["x"][[7, 300, 301]].any()


# --------------------------------------------------------------------------------------------------
# a numpy model of the device iteration with the intercept, and its mutants
# --------------------------------------------------------------------------------------------------
STEP_MUTANTS = ("c_all_rows", "c_not_in_update", "ss_uncorrected", "diag_uncentred")
RESET_MUTANTS = ("b_uncentred",)
CERT_MUTANTS = ("beta0_sign", "holdout_without_c")


class IModel:
    """k right-hand sides, one feature block, the intercept on: test_panel_step_host.py's ``Model`` (the
    same roundings in the same places) with S masked then centred by c = sum_in S / n_w, the corrected
    curvature, R and the carried operand updated with gamma (S - c), and R0 = -P_w B."""

    def __init__(self, Ab, B, mu, d_split, carry, W=None, mutant=None):
        self.Ab, self.B, self.mu, self.d_split = Ab, B, np.asarray(mu, dtype=np.float64), d_split
        self.m, self.n = Ab.shape
        self.k = B.shape[1]
        self.carry = bool(carry)
        self.Wk = Q.in_rows(W, self.k, self.m)
        self.nw = self.Wk.sum(axis=1).astype(np.float64)
        self.diag = C.centred_diag(Ab)
        self.kchunks = auto_kchunks(self.m, self.n)
        self.chain = d_split * (self.n // self.kchunks)
        self.mutant = mutant
        self.x = np.zeros((self.n, self.k))
        self.R = np.where(self.Wk, -B.T, 0.0) if mutant == "b_uncentred" else -Q.centre(self.Wk, B.T)
        self.t = 0
        self.Gc = self.E = self.Vh = None

    def direction_image(self, D):
        if self.d_split == 1:
            return P.bf16(D)
        hi, lo = P.split_bf16(D)
        return hi + lo

    def step(self):
        """One iteration; returns (err, acted): ``acted`` is False where the mutant provably changed nothing."""
        mut, Am = self.mutant, self.Ab
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
        xb = self.x
        d = (np.square(Am).sum(axis=0) if mut == "diag_uncentred" else self.diag)[:, None]
        D = P.soft_thr(d * xb - g, self.mu) / d - xb
        Dp = self.direction_image(D)
        err = float(np.max(np.abs(g - np.clip(g - xb, -self.mu, self.mu))))
        kc = self.n // self.kchunks
        S_all = sum(P.f32(Am[:, c * kc:(c + 1) * kc] @ Dp[c * kc:(c + 1) * kc]) for c in range(self.kchunks)).T
        S = np.where(self.Wk, S_all, 0.0)
        sm = S.sum(axis=1)
        c_in = sm / self.nw
        c = S_all.sum(axis=1) / self.m if mut == "c_all_rows" else c_in
        rs, ss = np.einsum("km,km->k", self.R, S), np.einsum("km,km->k", S, S)
        l1 = lambda v: np.abs(v).sum(axis=0)      # noqa: E731
        r1 = rs + self.mu * (l1(xb + Dp) - l1(xb))

        def line_search(curv):
            return np.where(curv <= 0.0, 0.0, np.clip(-r1 / np.where(curv <= 0.0, 1.0, curv), 0.0, 1.0))

        clean = line_search(ss - c_in * sm)
        gamma = line_search(ss if mut == "ss_uncorrected" else ss - c * sm)
        Sc = S if mut == "c_not_in_update" else np.where(self.Wk, S - c[:, None], 0.0)
        moving = Dp.any(axis=0) & (gamma > 0)
        # a wrong step size counts where the correct step is informative (test_panel_step_host.py's condition:
        # it moves x by >= 1e-3 of its norm); below that dx is a few fp32 ulps of x and B's own rounding
        # allowance covers either step size
        with np.errstate(divide="ignore", invalid="ignore"):
            informative = np.linalg.norm(clean * Dp, axis=0) >= 1e-3 * np.linalg.norm(xb + clean * Dp, axis=0)
        acted = {None: False, "b_uncentred": True, "diag_uncentred": bool(np.any(moving)),
                 "c_all_rows": bool(np.any(moving & (c != c_in))), "c_not_in_update": bool(np.any(moving & (c != 0))),
                 "ss_uncorrected": bool(np.any((gamma != clean) & informative))}.get(mut, False)
        self.x = P.f32(xb + gamma * Dp)
        dR = gamma[:, None] * Sc
        self.R = self.R + dR
        if self.carry:
            V = dR + (0.0 if exact else self.E)
            self.Vh = P.bf16(V)
            self.E = P.f32(V - self.Vh)
        self.t += 1
        return err, acted

    def certificate(self):
        """intercept and holdout_sse of the stored x, as the device's three certificate kernels form them"""
        e = (self.Ab @ self.x).T - self.B.T
        c = np.where(self.Wk, e, 0.0).sum(axis=1) / self.nw
        h = np.where(self.Wk, 0.0, e if self.mutant == "holdout_without_c" else e - c[:, None])
        return dict(intercept=c if self.mutant == "beta0_sign" else -c, holdout_sse=np.einsum("km,km->k", h, h))

    def snap(self):
        return self.x.copy(), self.R.copy()

    def clone(self, mutant):
        c = copy.copy(self)
        c.x, c.mutant = self.x.copy(), mutant
        return c


@functools.lru_cache(maxsize=None)
def problem(m, n, masked):
    Ab, _, B, W, mu_cols, _, _ = offset_instance(m, n)
    return Ab, B, mu_cols, (W if masked else None)


def run_checked(m, n, masked, d_split, carry, mutant=None, stats=None):
    """18 steps of the model, ``check_step_intercept`` at each; per checkpoint (violations, acted).  A step
    mutant bends the single step from the clean trajectory's state at t; the reset mutant runs throughout."""
    Ab, B, mu, W = problem(m, n, masked)
    mod = IModel(Ab, B, mu, d_split, carry, W=W, mutant=mutant if mutant in RESET_MUTANTS else None)
    out, snaps = [], [mod.snap()]
    for t in range(T_STEPS):
        if mutant in STEP_MUTANTS:
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
        viol = Q.check_step_intercept(Ab, mod.diag, mu, W, B, t, snaps[t], after, err, d_split, exact,
                                      None if exact else snaps[t][1] - snaps[t - 1][1], chain=mod.chain, q=q,
                                      R_ref=None if exact else snaps[t - q][1], stats=stats)
        out.append((viol, acted))
    return out, mod


CASES = [(256, 512, True), (256, 512, False), (1024, 512, True), (256, 1024, True)]


@pytest.mark.parametrize("m,n,masked,d_split,carry", [c + (ds, cg) for c in CASES for ds in (1, 2) for cg in (1, 0)])
def test_model_passes(m, n, masked, d_split, carry):
    stats = {}
    res, mod = run_checked(m, n, masked, d_split, carry, stats=stats)
    print(f"intercept model {m}x{n} masked={masked} d_split={d_split} carry={carry}: worst ratio to bound "
          + " ".join(f"{key} {stats[key]:.3g}" for key in ("A", "B", "C", "D", "0"))
          + f", gamma^ in [{stats['gamma_min']:.3g}, {stats['gamma_max']:.3g}]")
    for t, (viol, _) in enumerate(res):
        assert not viol, (t, viol)
    assert mod.x.any()
    # the model's certificate is the restatement's
    Ab, B, mu, W = problem(m, n, masked)
    ref = [C.intercept_duality_gap(Ab, B[:, c], mod.Wk[c], mod.x[:, c], mu[c]) for c in range(mod.k)]
    cert = mod.certificate()
    assert not Q.check_certificate(cert, {key: np.array([r[key] for r in ref]) for key in ("intercept", "holdout_sse")})


MUTANT_CASES = [(256, 512, True, 1, 1), (256, 512, True, 2, 0), (1024, 512, True, 1, 1)]


@pytest.mark.parametrize("case", MUTANT_CASES)
@pytest.mark.parametrize("mutant", STEP_MUTANTS + RESET_MUTANTS)
def test_mutant_is_caught(mutant, case):
    res, _ = run_checked(*case, mutant=mutant)
    acted = [t for t, (_, a) in enumerate(res) if a]
    missed = [t for t, (viol, a) in enumerate(res) if a and not viol]
    print(f"{mutant} {case}: acts at {len(acted)} checkpoints, missed at {missed}")
    assert acted, "the mutant never acted: the case does not exercise it"
    assert not missed


@pytest.mark.parametrize("mutant", CERT_MUTANTS)
def test_certificate_mutant_is_caught(mutant):
    m, n = 256, 512
    Ab, B, mu, W = problem(m, n, True)
    mod = IModel(Ab, B, mu, 1, 1, W=W)
    for _ in range(T_STEPS):
        mod.step()
    ref = [C.intercept_duality_gap(Ab, B[:, c], mod.Wk[c], mod.x[:, c], mu[c]) for c in range(mod.k)]
    ref = {key: np.array([r[key] for r in ref]) for key in ("intercept", "holdout_sse")}
    assert not Q.check_certificate(mod.certificate(), ref)
    assert Q.check_certificate(mod.clone(mutant).certificate(), ref)

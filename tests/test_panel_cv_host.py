"""Host side of the row masks and of K-fold cross-validation as one panel (no GPU; DESIGN.md section
11): ``kfold_masks``, ``masked_panel_iterate`` and ``masked_duality_gap`` agree with the existing
restatements and the oracle at w = 1, and the masked certificate bounds the suboptimality of the
row-deleted problem."""
import numpy as np
import pytest

from convex_optimization_amd import cpu_calculation as C
from oracle import oracle
from panel_cv_instance import cv_instance
from panel_gap_instance import instance

SCALARS = ("primal", "dual", "gap", "scale", "gnorm_inf")


@pytest.mark.parametrize("m,n_folds,seed", [(256, 4, 7), (256, 8, 0), (1024, 4, 7), (10, 3, 1), (257, 5, 2)])
def test_kfold_masks(m, n_folds, seed):
    M = C.kfold_masks(m, n_folds, seed=seed)
    assert M.shape == (n_folds, m) and M.dtype == np.uint8
    assert set(np.unique(M)) <= {0, 1}
    assert np.all((M == 0).sum(axis=0) == 1)                  # every row is held out exactly once
    held = (M == 0).sum(axis=1)
    assert held.sum() == m and held.max() - held.min() <= 1
    perm = np.random.RandomState(seed).permutation(m)
    for f in range(n_folds):
        assert np.array_equal(np.flatnonzero(M[f] == 0), np.sort(perm[f::n_folds]))
    assert np.array_equal(M, C.kfold_masks(m, n_folds, seed=seed))
    if m > 20:
        assert not np.array_equal(M, C.kfold_masks(m, n_folds, seed=seed + 1))


def test_kfold_masks_rejects_bad_fold_counts():
    with pytest.raises(ValueError):
        C.kfold_masks(16, 1)
    with pytest.raises(ValueError):
        C.kfold_masks(4, 5)


@pytest.mark.parametrize("m,n", [(256, 512), (1024, 512)])
def test_all_ones_mask_is_duality_gap(m, n):
    Ab, b, _, mus, _ = instance(m, n, 16)
    rs = np.random.RandomState(2)
    w = np.ones(m, dtype=np.uint8)
    for j in (0, 7, 15):
        x = (rs.randn(n) * (rs.rand(n) < 0.3)).astype(np.float32).astype(np.float64)
        got = C.masked_duality_gap(Ab, b, w, x, mus[j])
        ref = C.duality_gap(Ab, b, x, mus[j])
        for key in SCALARS:
            assert abs(got[key] - ref[key]) <= 1e-12 * abs(ref[key]), key
        keep, score = C.gap_safe_keep(Ab, b, x, mus[j], return_score=True)
        np.testing.assert_allclose(got["score"], score, rtol=1e-12)
        assert np.array_equal(got["keep"], keep)
        assert got["holdout_sse"] == 0.0
    zero = C.masked_duality_gap(Ab, b, w, np.zeros(n), mus[0])
    assert zero["gnorm_inf"] == pytest.approx(np.abs(Ab.T @ b).max(), rel=1e-14)


@pytest.mark.parametrize("m,n,Block", [(256, 512, 1), (1024, 512, 1), (256, 1024, 2)])
def test_all_ones_mask_is_the_numpy_oracle_bitwise(m, n, Block):
    """At w = 1 the restatement performs the operations of ``oracle.run_numpy`` (the numpy restatement the
    C oracle is cross-checked with) in its order: the same bits, on every shape and mu of the tests."""
    Ab, b, _, _, mu_max = instance(m, n, 16)
    for mu in C.mu_grid(mu_max, 4):
        got = C.masked_panel_iterate(Ab, b, np.ones(m, dtype=np.uint8), mu, Block, 200)
        assert np.array_equal(got["x"], oracle.run_numpy(Ab, b, mu, Block, 200)["x"])
        np.testing.assert_allclose(got["r"], Ab @ got["x"] - b, rtol=0, atol=1e-12)


@pytest.mark.parametrize("m,n,Block", [(1024, 512, 1), (256, 1024, 2)])
def test_all_ones_mask_is_the_oracle_iteration(m, n, Block):
    """x after 200 iterations within 1e-10 (max |.|, x is O(1)) of the C oracle, which sums in another
    order, at mu = 0.9 mu_max on two of the instances.  Measured max |x - x_oracle| for
    mu / mu_max = 0.9, 0.433, 0.208, 0.1: 1024 x 512 B1 1.2e-11, 5.2e-9, 8.7e-9, 5.0e-8; 256 x 1024 B2
    1.2e-15, 2.9e-8, 7.7e-10, 2.9e-12; 256 x 512 B1 4.4e-9, 6.4e-9, 1.2e-8, 4.9e-10.  ``oracle.run_numpy``
    is exactly as far from the C oracle (the test above: same bits as this restatement), and where the
    distance is 1e-9 to 1e-7 it is what the oracle's own error criterion has reached at iteration 200
    (3.9e-9 ... 5.5e-8): there the exact line search works on differences at the square root of the fp64
    rounding unit, so two summation orders settle that far apart.  The two cases asserted here reach their
    fixed point before that."""
    Ab, b, _, _, mu_max = instance(m, n, 16)
    mu = C.mu_grid(mu_max, 4)[0]
    got = C.masked_panel_iterate(Ab, b, np.ones(m), mu, Block, 200)
    ref = oracle.run(Ab, b, mu, Block, 200)["x"]
    err = np.abs(got["x"] - ref).max()
    print(f"{m}x{n} B{Block}: max |x - x_oracle| {err:.2e}, max |x| {np.abs(ref).max():.2e}")
    assert np.abs(ref).max() > 0
    assert err <= 1e-10
    # a given diag and a start: 100 + 100 iterations are the 200 (an even count keeps the block phase)
    half = C.masked_panel_iterate(Ab, b, np.ones(m), mu, Block, 100, diag=np.square(Ab).sum(axis=0))
    two = C.masked_panel_iterate(Ab, b, np.ones(m), mu, Block, 100, x0=half["x"])
    np.testing.assert_allclose(two["x"], got["x"], rtol=0, atol=1e-10)


@pytest.mark.parametrize("m,n,Block", [(256, 512, 1), (256, 1024, 2)])
def test_masked_gap_bounds_the_row_deleted_problem(m, n, Block):
    Ab, b, _, W, mu_cols, _, _ = cv_instance(m, n)
    for c in (1, 6, 15):
        w, mu = W[:, c], mu_cols[c]
        rows = np.flatnonzero(w)
        assert 0 < rows.size < m
        Ar, br = np.ascontiguousarray(Ab[rows]), b[rows]
        x_ref = oracle.run(Ar, br, mu, Block, 4096 * Block)["x"]
        P_ref = C.duality_gap(Ar, br, x_ref, mu)["primal"]
        diag_fold = np.square(Ar).sum(axis=0)
        assert np.all(np.square(Ab).sum(axis=0) >= diag_fold)          # the full diag dominates: the screen stays safe
        supp = np.abs(x_ref) > 2.0 ** -52 * np.abs(x_ref).max()
        prev = np.inf
        for iters in (8 * Block, 32 * Block, 128 * Block):
            x = C.masked_panel_iterate(Ab, b, w, mu, Block, iters)["x"]
            cert = C.masked_duality_gap(Ab, b, w, x, mu)
            same = C.duality_gap(Ar, br, x, mu)                        # the masked problem IS the row-deleted one
            for key in SCALARS:   # the gap is a difference of the two: its rounding scales with the primal
                assert abs(cert[key] - same[key]) <= 1e-12 * (same["primal"] if key == "gap" else abs(same[key])), key
            assert cert["dual"] <= P_ref * (1 + 1e-9)
            assert cert["primal"] - P_ref <= cert["gap"] + 1e-9 * cert["primal"]
            assert cert["primal"] <= prev * (1 + 1e-12)                # a descent method with the full diag
            prev = cert["primal"]
            assert not np.any(supp & ~cert["keep"])
            out = np.flatnonzero(w == 0)
            assert cert["holdout_sse"] == pytest.approx(float(np.square(Ab[out] @ x - b[out]).sum()), rel=1e-12)
            assert np.all(cert["r"][out] == 0.0)
        if c != 6:
            continue
        # the per-fold diag reaches the same optimum
        x_fold = C.masked_panel_iterate(Ab, b, w, mu, Block, 1024 * Block, diag=diag_fold)["x"]
        x_full = C.masked_panel_iterate(Ab, b, w, mu, Block, 1024 * Block)["x"]
        P = [C.masked_duality_gap(Ab, b, w, x, mu)["primal"] for x in (x_fold, x_full)]
        assert abs(P[0] - P_ref) <= 1e-9 * P_ref and abs(P[1] - P_ref) <= 1e-9 * P_ref


def test_degenerate_masks_on_the_host():
    Ab, b, _, mus, _ = instance(256, 512, 16)
    none = C.masked_panel_iterate(Ab, b, np.zeros(256), mus[5], 1, 10)
    assert not none["x"].any() and not none["r"].any()
    cert = C.masked_duality_gap(Ab, b, np.zeros(256), none["x"], mus[5])
    assert cert["primal"] == 0.0 and cert["dual"] == 0.0 and cert["gap"] == 0.0 and cert["scale"] == 1.0
    assert cert["holdout_sse"] == pytest.approx(float(b @ b), rel=1e-14)


def test_lasso_cv_refuses_before_it_touches_a_device():
    pytest.importorskip("torch")
    from convex_optimization_amd import panel
    A, b = np.zeros((256, 256)), np.zeros(256)
    with pytest.raises(ValueError):
        panel.lasso_cv(A, b, n_folds=9, n_mus=16)
    with pytest.raises(ValueError):
        panel.lasso_cv(A, b, n_folds=1, n_mus=4)
    with pytest.raises(ValueError):
        panel.lasso_cv(A, b, n_folds=4, mus=np.linspace(1.0, 2.0, 33))
    with pytest.raises(ValueError):
        panel.lasso_cv(A, b, masks=np.ones((4, 255), dtype=np.uint8), n_mus=4)

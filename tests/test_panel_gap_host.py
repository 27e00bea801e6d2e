"""Host side of the panel certificate and the path driver (no GPU): ``panel_duality_gap`` is the
per-column ``duality_gap`` / ``gap_safe_keep``, ``mu_grid`` is the geometric grid, and the padding
rule of ``lasso_path``."""
import numpy as np
import pytest

from convex_optimization_amd import cpu_calculation as C
from panel_gap_instance import bf16_round, instance


def test_bf16_round_is_torch_rounding():
    torch = pytest.importorskip("torch")
    A = np.random.RandomState(0).randn(64, 96) * np.logspace(-6, 6, 96)
    ref = torch.from_numpy(A.astype(np.float32)).to(torch.bfloat16).to(torch.float64).numpy()
    assert np.array_equal(bf16_round(A), ref)


@pytest.mark.parametrize("m,n,k", [(256, 512, 16), (256, 256, 128)])
def test_panel_duality_gap_is_per_column(m, n, k):
    Ab, b, B, mus, _ = instance(m, n, k)
    rs = np.random.RandomState(1)
    X = (rs.randn(n, k) * (rs.rand(n, k) < 0.3)).astype(np.float32).astype(np.float64)
    X[:, 0] = 0.0
    out = C.panel_duality_gap(Ab, B, X, mus)
    assert out["keep"].shape == (k, n) and out["keep"].dtype == bool and out["n_keep"].dtype == np.int64
    for j in range(k):
        xj = np.ascontiguousarray(X[:, j])
        ref = C.duality_gap(Ab, b, xj, mus[j])
        for key in ("primal", "dual", "gap", "scale", "gnorm_inf"):
            assert out[key][j] == ref[key], (key, j)
        keep = C.gap_safe_keep(Ab, b, xj, mus[j])
        assert np.array_equal(out["keep"][j], keep)
        assert out["n_keep"][j] == keep.sum()
    # x = 0: ||g||_inf is mu_max and the primal 1/2 ||b||^2
    assert out["gnorm_inf"][0] == pytest.approx(np.abs(Ab.T @ b).max(), rel=1e-14)
    assert out["primal"][0] == pytest.approx(0.5 * float(b @ b), rel=1e-14)
    # a scalar mu serves every column
    one = C.panel_duality_gap(Ab, B[:, :2], X[:, :2], mus[3])
    assert one["gap"][1] == C.duality_gap(Ab, b, np.ascontiguousarray(X[:, 1]), mus[3])["gap"]


def test_mu_grid_endpoints_and_monotone():
    g = C.mu_grid(3.5, 16)
    assert g.shape == (16,)
    assert g[0] == pytest.approx(0.9 * 3.5, rel=1e-15) and g[-1] == pytest.approx(0.1 * 3.5, rel=1e-15)
    assert np.all(np.diff(g) < 0)
    np.testing.assert_allclose(g[1:] / g[:-1], (0.1 / 0.9) ** (1 / 15), rtol=1e-13)   # geometric
    h = C.mu_grid(2.0, 5, hi=0.5, lo=0.01)
    assert h[0] == pytest.approx(1.0, rel=1e-15) and h[-1] == pytest.approx(0.02, rel=1e-15)
    assert C.mu_grid(2.0, 1).shape == (1,)


def test_path_padding_rule():
    pytest.importorskip("torch")
    from convex_optimization_amd import panel
    for n_given, width in [(1, 16), (13, 16), (16, 16), (17, 32), (33, 64), (65, 128), (128, 128)]:
        mus = np.random.RandomState(n_given).rand(n_given) + 0.1
        grid, n = panel.pad_mus(mus)
        assert n == n_given and grid.shape == (width,)
        assert np.array_equal(grid[:n_given], mus)
        assert np.all(grid[n_given:] == mus.max())       # duplicates of a real problem
    with pytest.raises(ValueError):
        panel.pad_mus(np.ones(129))
    with pytest.raises(ValueError):
        panel.pad_mus([])
    # the driver refuses before it touches a device
    A = np.zeros((256, 256))
    with pytest.raises(ValueError):
        panel.lasso_path(A, np.zeros(256), mus=np.linspace(1.0, 2.0, 129))
    with pytest.raises(ValueError):
        panel.lasso_path(A, np.zeros(256), n_mus=129)

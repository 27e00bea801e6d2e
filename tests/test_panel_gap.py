"""GPU tests of the panel's per-RHS duality-gap certificate (``PanelLasso.duality_gap``,
bpgl_panel_gap) and of ``panel.lasso_path``.

Instance (panel_gap_instance.py): rs = RandomState(m + n), A = randn row-normalised and bf16-rounded,
x0 = randn * (rand < 0.4), b = Ab x0 + 0.01 randn in every column of B, mus = mu_grid(||Ab^T b||_inf, k).
Shapes (m, n, Block, k[, lda]): one and several feature blocks, a row count that puts the fused
reduce + update in effect (1024), panel widths 16, 32 and 128, and a padded lda.  All
of them split the certificate's reductions into chunks (the fixed-order second stage).

The reference is numpy fp64 on the device's own x and the stored Ab; the bounds are those of
tests/test_gap_screen.py as they stand there (1e-9 relative on the scalars, 1e-9 of the primal on
the gap, rtol 1e-11 + atol 1e-12 max|.| on g and r: fp64 sums over the same numbers in another
order).  P_ref and the support come from the fp64 per-RHS oracle after 4096 Block iterations.
Measured on the MI355X over all cases and checkpoints: the scalars within 1.5e-15 relative, the gap
within 1.1e-15 of the primal, g within 1.7e-15 and r within 4.9e-16 of their largest entries, at most
one borderline mask entry (256 x 256, k = 128), drift 1e-7 to 7e-7; lasso_path stops at 192 and 256
iterations, which are also T_ref.

The oracle's support is |x_j| > 2^-52 max|x|.  A plain x_j != 0 counts rounding residue: a coordinate
the iteration drives to zero with steps gamma < 1 is left at (1 - gamma) ... x_j, which decays but need
not land on 0.0 -- at 256 x 256 the oracle's x keeps -1.7e-21 (mu index 37, column 169) and 7.3e-28
(index 45, column 190), unchanged from 4096 to 65536 iterations, both columns the rule screens
correctly with score 0.996 mu and 0.975 mu at 16 iterations.  An entry below the rounding unit of the
largest one cannot change A x in fp64, so it is not support.
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
from panel_gap_instance import instance  # noqa: E402

NT = min(16, os.cpu_count() or 1)
# (m, n, Block, k, lda)
CASES = [(256, 512, 1, 16, None), (256, 1024, 2, 16, None), (512, 768, 3, 32, None), (1024, 512, 1, 16, None),
         (256, 256, 1, 128, None), (256, 512, 1, 16, 520)]
SCALARS = ("primal", "dual", "gap", "scale", "gnorm_inf", "n_keep", "drift")


def make(m, n, B, k, lda=None):
    return PanelLasso(instance(m, n, k)[0], B, nrhs=k, device=0, lda=lda)


def snapshot(pl, t):
    """One certificate with host copies of everything the tests look at (the device buffers are reused)."""
    d = pl.duality_gap()
    k, n, m = pl.nrhs, pl.MAT_WIDTH_ALL, pl.MAT_HEIGHT
    assert d["g"].dtype == torch.float64 and tuple(d["g"].shape) == (k, n) and d["g"].is_cuda
    assert d["r"].dtype == torch.float64 and tuple(d["r"].shape) == (k, m) and d["r"].is_cuda
    assert d["keep"].dtype == torch.bool and tuple(d["keep"].shape) == (k, n) and d["keep"].is_cuda
    rec = {key: d[key] for key in SCALARS}
    rec.update(t=t, x=pl.solver_x(), g=d["g"].cpu().numpy(), r=d["r"].cpu().numpy(), keep=d["keep"].cpu().numpy(),
               drift_torch=(pl.residual_device() - d["r"]).abs().amax(dim=1).cpu().numpy())
    return rec


@functools.lru_cache(maxsize=None)
def checkpoints(m, n, B, k, lda):
    """One device run per case: a certificate right after the reset, then after 16 B, 64 B and 256 B
    iterations."""
    _, _, Bm, mus, _ = instance(m, n, k)
    pl = make(m, n, B, k, lda)
    if m == 1024:
        assert pl.get_tuning("fuse_update") == 1   # the fused reduce + update is in effect
    pl.solver_reset(Bm, mus)
    out, t = [snapshot(pl, 0)], 0
    for stop in (16 * B, 64 * B, 256 * B):
        pl.solver_step(stop - t)
        t = stop
        out.append(snapshot(pl, t))
    assert pl.solver_status()["iters"] == t
    return out


@functools.lru_cache(maxsize=None)
def oracle_opt(m, n, B, k):
    """X (n, k) of the fp64 per-RHS oracle after 4096 B iterations, and its objectives (k,)."""
    Ab, b, _, mus, _ = instance(m, n, k)
    with concurrent.futures.ThreadPoolExecutor(NT) as ex:
        cols = list(ex.map(lambda mu: oracle.run(Ab, b, mu, B, 4096 * B, nthreads=1)["x"], mus))
    X = np.stack(cols, axis=1)
    P = np.array([C.duality_gap(Ab, b, X[:, j].copy(), mus[j])["primal"] for j in range(k)])
    X.setflags(write=False)
    return X, P


# ---------------------------------------------------------------------------
# 1. parity with the numpy restatement on the device's own x
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,B,k,lda", CASES)
def test_panel_gap_matches_numpy(m, n, B, k, lda):
    Ab, b, Bm, mus, _ = instance(m, n, k)
    for rec in checkpoints(m, n, B, k, lda)[1:]:
        X = rec["x"]
        ref = C.panel_duality_gap(Ab, Bm, X, mus)
        r_ref = (Ab @ X - Bm).T
        g_ref = r_ref @ Ab
        radius = np.sqrt(2.0 * np.maximum(ref["gap"], 0.0))
        score = ref["scale"][:, None] * np.abs(g_ref) + np.sqrt(np.square(Ab).sum(axis=0))[None, :] * radius[:, None]
        rel = {key: np.max(np.abs(rec[key] - ref[key]) / np.abs(ref[key])) for key in ("primal", "dual", "scale",
                                                                                         "gnorm_inf")}
        gap_err = np.max(np.abs(rec["gap"] - ref["gap"]) / ref["primal"])
        clear = np.abs(score - mus[:, None]) > 1e-9 * mus[:, None]
        print(f"{m}x{n} B{B} k{k} lda{lda} t={rec['t']}: worst rel {rel}, gap err / primal {gap_err:.2e}, "
              f"rel gap {np.min(rec['gap'] / (0.5 * b @ b)):.2e}..{np.max(rec['gap'] / (0.5 * b @ b)):.2e}, "
              f"g err {np.abs(rec['g'] - g_ref).max() / np.abs(g_ref).max():.2e} of max, "
              f"r err {np.abs(rec['r'] - r_ref).max() / np.abs(r_ref).max():.2e} of max, "
              f"borderline {int((~clear).sum())}, n_keep {rec['n_keep'].min()}..{rec['n_keep'].max()}, "
              f"drift {rec['drift'].max():.2e}")
        for key in rel:
            assert np.all(np.abs(rec[key] - ref[key]) <= 1e-9 * np.abs(ref[key])), key
        assert np.all(np.abs(rec["gap"] - ref["gap"]) <= 1e-9 * ref["primal"])
        for j in range(k):
            np.testing.assert_allclose(rec["g"][j], g_ref[j], rtol=1e-11, atol=1e-12 * np.abs(g_ref[j]).max())
            np.testing.assert_allclose(rec["r"][j], r_ref[j], rtol=1e-11, atol=1e-12 * np.abs(r_ref[j]).max())
        # the mask: exact wherever the numpy score is farther than 1e-9 mu from mu
        assert (~clear).sum() <= 0.01 * k * n
        assert np.array_equal(rec["keep"][clear], ref["keep"][clear])
        assert rec["n_keep"].dtype == np.int64 and np.array_equal(rec["n_keep"], rec["keep"].sum(axis=1))
        # max |.| is order-independent: the device's drift is torch's on the same arrays, exactly
        assert np.array_equal(rec["drift"], rec["drift_torch"])


# ---------------------------------------------------------------------------
# 2. the certificate is sound, and the screen is safe
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,B,k,lda", CASES)
def test_panel_gap_is_sound(m, n, B, k, lda):
    Ab, b, Bm, mus, _ = instance(m, n, k)
    X_ref, P_ref = oracle_opt(m, n, B, k)
    supp = (np.abs(X_ref) > 2.0 ** -52 * np.abs(X_ref).max(axis=0, keepdims=True)).T     # (k, n)
    assert np.all(supp.sum(axis=1) > 0) and np.all(supp.sum(axis=1) < n)
    for rec in checkpoints(m, n, B, k, lda)[1:]:
        P_dev = C.panel_duality_gap(Ab, Bm, rec["x"], mus)["primal"]
        print(f"{m}x{n} B{B} k{k} t={rec['t']}: worst (P(x) - P_ref) / gap {np.max((P_dev - P_ref) / rec['gap']):.3f}, "
              f"worst dual / P_ref {np.max(rec['dual'] / P_ref):.9f}, screened {int((~rec['keep']).sum())} of {k * n}")
        assert np.all(rec["dual"] <= P_ref * (1 + 1e-9))
        assert np.all(P_dev - P_ref <= rec["gap"] + 1e-9 * rec["primal"])
        assert int((supp & ~rec["keep"]).sum()) == 0, rec["t"]


# ---------------------------------------------------------------------------
# 3. x = 0
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,B,k,lda", CASES)
def test_panel_gap_at_zero(m, n, B, k, lda):
    _, b, _, _, mu_max = instance(m, n, k)
    rec = checkpoints(m, n, B, k, lda)[0]
    assert not rec["x"].any()
    assert np.all(np.abs(rec["gnorm_inf"] - mu_max) <= 1e-9 * mu_max)
    assert np.all(np.abs(rec["primal"] - 0.5 * b @ b) <= 1e-9 * 0.5 * b @ b)
    assert np.all(rec["drift"] == 0.0)
    assert np.array_equal(rec["r"], -np.repeat(b[None, :], k, axis=0))


# ---------------------------------------------------------------------------
# 4. read-only for the solve, and deterministic
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("m,n,B,k,g_refresh", [(1024, 512, 1, 16, None), (256, 1024, 2, 16, None),
                                               (1024, 512, 1, 16, 16)])
def test_panel_gap_is_read_only_and_deterministic(m, n, B, k, g_refresh, use_graph):
    _, _, Bm, mus, _ = instance(m, n, k)

    def fresh():
        pl = make(m, n, B, k)
        if g_refresh:
            pl.set_tuning("g_refresh", g_refresh)
        pl.solver_reset(Bm, mus, use_graph=use_graph)
        return pl

    def final(pl):
        st = pl.solver_status()
        return (pl.solver_x_device().clone(), pl.residual_device().clone(), pl.stat("iters_enqueued"),
                pl.stat("exact_gradients"), st)

    pa = fresh()
    pa.solver_step(64)
    d1 = pa.duality_gap()
    h1 = {key: d1[key].clone() for key in ("g", "r", "keep")}
    d2 = pa.duality_gap()
    pa.solver_step(64)
    xa, ra, ia, ea, sa = final(pa)
    pb = fresh()
    pb.solver_step(64)
    pb.solver_step(64)
    xb, rb, ib, eb, sb = final(pb)
    assert torch.equal(xa, xb) and torch.equal(ra, rb)
    assert ia == ib == 128
    assert ea == eb == (0 if B > 1 else 128 // (g_refresh or 64))
    assert sa == sb and sa["iters"] == 128
    for key in SCALARS:
        assert np.array_equal(d1[key], d2[key]), key
    for key in ("g", "r", "keep"):
        assert torch.equal(h1[key], d2[key]), key
    assert np.all(d1["gap"] > 0)


# ---------------------------------------------------------------------------
# 5. errors (argument and state checks on the host; nothing is launched)
# ---------------------------------------------------------------------------
def test_panel_gap_errors():
    m, n, B, k = 256, 512, 1, 16
    _, _, Bm, mus, _ = instance(m, n, k)
    pl = make(m, n, B, k)
    with pytest.raises(N.BpglError, match=r"\(-2\): .*bpgl_panel_reset"):
        pl.duality_gap()
    pl.solver_reset(Bm, mus)
    L = panel._lib()
    g = torch.empty((B, k, n // B), dtype=torch.float64, device="cuda")
    r = torch.empty((k, m), dtype=torch.float64, device="cuda")
    out = (ctypes.c_double * (8 * k))()
    assert L.bpgl_panel_gap(pl._ctx, None, N.ptr(r), None, out) == -1
    assert "non-null" in L.bpgl_last_error().decode()
    assert L.bpgl_panel_gap(pl._ctx, N.ptr(g), None, None, out) == -1
    assert L.bpgl_panel_gap(pl._ctx, N.ptr(g), N.ptr(r), None, None) == -1
    assert L.bpgl_panel_gap(None, N.ptr(g), N.ptr(r), None, out) == -1
    # screen=False: no mask, every column counted
    d = pl.duality_gap(screen=False)
    assert d["keep"] is None and np.all(d["n_keep"] == n)


# ---------------------------------------------------------------------------
# 6. the path driver
# ---------------------------------------------------------------------------
def t_ref(m, n, B, k, bound):
    """The first multiple of 64 B at which the fp64 per-RHS oracle, its x rounded to fp32, meets the
    bound for every mu."""
    Ab, b, _, mus, _ = instance(m, n, k)
    target = bound * 0.5 * float(b @ b)
    X = np.zeros((n, k))

    def advance(j):
        X[:, j] = oracle.run(Ab, b, mus[j], B, 64 * B, x0=X[:, j].copy(), nthreads=1)["x"]
        x32 = X[:, j].astype(np.float32).astype(np.float64)
        return C.duality_gap(Ab, b, x32, mus[j])["gap"] <= target

    with concurrent.futures.ThreadPoolExecutor(NT) as ex:
        for t in range(64 * B, 64 * B * 64 + 1, 64 * B):
            if all(list(ex.map(advance, range(k)))):
                return t
    raise AssertionError("the oracle did not reach the bound")


@pytest.mark.parametrize("m,n,B", [(256, 512, 1), (256, 1024, 2)])
def test_lasso_path(m, n, B):
    k, bound = 16, 1e-4
    Ab, b, _, mus, mu_max = instance(m, n, k)
    T = t_ref(m, n, B, k, bound)
    res = panel.lasso_path(Ab, b, mus=mus, Block=B, GAP_BOUND=bound, ITER_MAX=4 * T, check_every=64, device=0)
    print(f"lasso_path {m}x{n} B{B}: T_ref {T}, device iters {res['iters']}, first_reached {res['first_reached']}, "
          f"rel gap {res['gap'] / (0.5 * b @ b)}")
    assert res["x"].shape == (n, k) and np.array_equal(res["mus"], mus) and res["mu_max"] is None
    assert np.all(res["reached"]) and res["iters"] <= 4 * T
    assert np.all(res["first_reached"] > 0) and res["first_reached"].max() <= res["iters"]
    assert np.all(res["first_reached"] % 64 == 0)
    target = bound * 0.5 * float(b @ b)
    for j in range(k):
        cert = C.duality_gap(Ab, b, res["x"][:, j].copy(), mus[j])
        assert abs(cert["gap"] - res["gap"][j]) <= 1e-9 * cert["primal"]
        assert cert["gap"] <= target
    # mus=None: the grid comes from the device's own ||Ab^T b||_inf
    auto = panel.lasso_path(Ab, b, n_mus=k, Block=B, GAP_BOUND=bound, ITER_MAX=4 * T, check_every=64, device=0)
    assert abs(auto["mu_max"] - mu_max) <= 1e-9 * mu_max
    np.testing.assert_allclose(auto["mus"], mus, rtol=1e-9)
    assert np.all(auto["reached"])
    # 13 given mus pad to 16: the first 13 columns of the 16-column run whose last three repeat the largest
    part = panel.lasso_path(Ab, b, mus=mus[:13], Block=B, GAP_BOUND=bound, ITER_MAX=4 * T, check_every=64, device=0)
    full = panel.lasso_path(Ab, b, mus=np.concatenate([mus[:13], np.full(3, mus[:13].max())]), Block=B,
                            GAP_BOUND=bound, ITER_MAX=4 * T, check_every=64, device=0)
    assert part["x"].shape == (n, 13) and full["x"].shape == (n, 16)
    assert part["iters"] == full["iters"]
    assert np.array_equal(part["x"], full["x"][:, :13])
    for key in SCALARS + ("reached", "first_reached", "mus"):
        assert part[key].shape == (13,) and np.array_equal(part[key], full[key][:13]), key
    with pytest.raises(ValueError):
        panel.lasso_path(Ab, b, mus=np.linspace(0.1, 1.0, 129) * mu_max, Block=B, device=0)

"""GPU tests of the duality-gap certificate, gap-safe screening, the column gather and the
screened driver (``GPU_Calculation.duality_gap`` / ``gather_columns``, ``ClassLassoScreened``).

Common instance: parameters(250, 2040, 0.05, seed=7) with A taken as the device stores it, ragged
on purpose: 250 rows are no multiple of 64, and with Block 4 the block width 510 pads to 512 for
fp32 and bf16 storage (and stays 510 for fp64).  bf16 also runs 256 x 2048 with Block 2 (the
in-place layout).  The host reference is ``cpu_calculation.duality_gap`` / ``gap_safe_keep`` in
numpy fp64, evaluated on the device's own x; x* is the numpy oracle's 8000-iteration run.

Bounds: primal and dual 1e-9 relative (the fixture-parity bound of test_gpu.py), the gap 1e-9
of the primal absolute, A^T r the bound of test_gpu.py::test_kernels_match_oracle as it stands there
(rtol 1e-11 with atol 1e-12 max|g|).  Every device value is an fp64 sum over the stored A, so it
differs from numpy by summation order only.  The atol term is that test's, not a widening: g_j is
a cancelling sum of 250 products, and a relative bound alone cannot hold for an entry that cancels
to ~1e-4 of max|g| -- measured on the MI355X: 2039 of 2040 entries within 6e-12 relative, one
entry of size 5.7e-6 off by 8.0e-17 absolute (1.4e-11 relative; fp64, Block 4, t = 768).
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from convex_optimization_amd import _native as N  # noqa: E402
from convex_optimization_amd import cpu_calculation as C  # noqa: E402
from convex_optimization_amd import lasso  # noqa: E402
from convex_optimization_amd.gpu_calculation import GPU_Calculation  # noqa: E402
from convex_optimization_amd.parameters import parameters  # noqa: E402

STORAGES = ["double", "float", "bf16"]
# (storage, rows, columns, Block)
PARITY_CASES = [(s, 250, 2040, B) for s in STORAGES for B in (1, 4)] + [("bf16", 256, 2048, 2)]


def make_cls(type_name):
    return type("GC_" + type_name, (GPU_Calculation,), {"TYPE": type_name})


def stored(A, type_name):
    """A as the device stores it, returned as fp64 (as in test_gpu.py)."""
    if type_name == "double":
        return A.astype(np.float64)
    if type_name == "float":
        return A.astype(np.float32).astype(np.float64)
    t = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float32)).to(torch.bfloat16)
    return t.to(torch.float64).numpy()


@functools.lru_cache(maxsize=None)
def instance(m, n):
    A, _, b, mu = parameters(m, n, 0.05, SILENCE=True, seed=7)
    return A, np.asarray(b).reshape(-1), float(mu)


@functools.lru_cache(maxsize=None)
def stored_instance(type_name, m, n):
    A, b, mu = instance(m, n)
    return stored(A, type_name), b, mu


def context(type_name, m, n, B):
    """250 x 2040 from the host array (the padded (Block, H, W_pad) layout); 256 x 2048 from a device
    tensor of the storage dtype, which is bound in place (lda = K, block stride = W)."""
    As = stored_instance(type_name, m, n)[0]
    if m != 256:
        return make_cls(type_name)(As, B, device=0)
    gc = make_cls(type_name)(torch.from_numpy(As).to(N.TORCH_DTYPE[N.dtype_code(type_name)]).cuda(), B, device=0)
    assert gc._A_dev.dim() == 2
    return gc


@functools.lru_cache(maxsize=None)
def x_star(type_name, m, n, B):
    As, b, mu = stored_instance(type_name, m, n)
    x = oracle.run_numpy(As, b, mu, B, 8000)["x"]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def checkpoints(type_name, m, n, B):
    """One device run per case, stopped at 64 B, 192 B and 256 B iterations; host copies of
    everything the parity and the safety tests look at."""
    _, b, mu = stored_instance(type_name, m, n)
    gc = context(type_name, m, n, B)
    gc.solver_reset(b, mu)
    out, t = [], 0
    for stop in (64 * B, 192 * B, 256 * B):
        gc.solver_step(stop - t)
        t = stop
        d = gc.duality_gap()
        rec = {k: d[k] for k in ("primal", "dual", "gap", "scale", "gnorm_inf", "n_keep")}
        rec.update(t=t, x=gc.solver_x(), g_all=d["g_all"].cpu().numpy().reshape(-1),
                   keep=d["keep"].cpu().numpy().reshape(-1), keep_raw=gc._gap_keep.cpu().numpy(),
                   onepass=gc.solver_stat("onepass"), fallbacks=gc.solver_stat("fallbacks"))
        assert d["keep"].dtype == torch.bool and tuple(d["keep"].shape) == (B, n // B) and d["keep"].is_cuda
        out.append(rec)
    return out


# ---------------------------------------------------------------------------
# 1. parity with the numpy restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("type_name,m,n,B", PARITY_CASES)
def test_gap_matches_numpy(type_name, m, n, B):
    As, b, mu = stored_instance(type_name, m, n)
    W = n // B
    for rec in checkpoints(type_name, m, n, B)[:2]:
        if B == 1:   # one feature block runs the one-pass iteration
            assert rec["onepass"] == 1
        assert rec["fallbacks"] == 0
        ref = C.duality_gap(As, b, rec["x"], mu)
        g_ref = As.T @ (As @ rec["x"] - b)
        keep_ref, score = C.gap_safe_keep(As, b, rec["x"], mu, return_score=True)
        g_rel = np.max(np.abs(rec["g_all"] - g_ref) / np.abs(g_ref))
        print(f"{type_name} {m}x{n} B{B} t={rec['t']}: primal {rec['primal']:.17g} ref {ref['primal']:.17g}, "
              f"dual {rec['dual']:.17g} ref {ref['dual']:.17g}, gap {rec['gap']:.6e} ref {ref['gap']:.6e}, "
              f"worst g rel {g_rel:.3e}, n_keep {rec['n_keep']} ref {int(keep_ref.sum())}")
        assert abs(rec["primal"] - ref["primal"]) <= 1e-9 * abs(ref["primal"])
        assert abs(rec["dual"] - ref["dual"]) <= 1e-9 * abs(ref["dual"])
        assert abs(rec["gap"] - ref["gap"]) <= 1e-9 * ref["primal"]
        assert abs(rec["scale"] - ref["scale"]) <= 1e-9 * ref["scale"]
        assert abs(rec["gnorm_inf"] - ref["gnorm_inf"]) <= 1e-9 * ref["gnorm_inf"]
        np.testing.assert_allclose(rec["g_all"], g_ref, rtol=1e-11, atol=1e-12 * np.abs(g_ref).max())
        # the mask: exact wherever the numpy score is farther than 1e-9 mu from mu
        clear = np.abs(score - mu) > 1e-9 * mu
        assert (~clear).sum() <= 0.01 * n
        assert np.array_equal(rec["keep"][clear], keep_ref[clear])
        assert rec["n_keep"] == int(rec["keep"].sum())
        raw = rec["keep_raw"]
        assert raw.dtype == np.uint8 and raw.shape[0] == B and raw.shape[1] >= W
        assert not raw[:, W:].any() and set(np.unique(raw)) <= {0, 1}
        assert np.array_equal(raw[:, :W].reshape(-1).astype(bool), rec["keep"])


# ---------------------------------------------------------------------------
# 2. read-only for the solve, and deterministic
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("B", [1, 4])
def test_gap_is_read_only_and_deterministic(B, use_graph):
    As, b, mu = stored_instance("float", 250, 2040)

    def fresh():
        gc = make_cls("float")(As, B, device=0)
        if B == 1:
            gc.set_tuning("onepass_refresh", 48)   # refreshes at 48 and 96: the gap calls fall inside a period
        gc.solver_reset(b, mu, use_graph=use_graph)
        return gc

    def final(gc):
        gc.solver_status()
        return gc.solver_x_device().clone(), gc._ctx_residual().clone(), gc.solver_stat("refreshes")

    ga = fresh()
    ga.solver_step(64)
    d1 = ga.duality_gap()
    d2 = ga.duality_gap()
    ga.solver_step(64)
    xa, ra, na = final(ga)
    gb = fresh()
    gb.solver_step(128)
    xb, rb, nb = final(gb)
    assert torch.equal(xa, xb) and torch.equal(ra, rb)
    assert na == nb == (2 if B == 1 else 0)
    assert ga.solver_stat("enqueued") == gb.solver_stat("enqueued") == 128
    for k in ("primal", "dual", "gap", "scale", "gnorm_inf", "n_keep"):
        assert d1[k] == d2[k], k
    assert torch.equal(d1["g_all"], d2["g_all"]) and torch.equal(d1["keep"], d2["keep"])
    assert d1["gap"] > 0


# ---------------------------------------------------------------------------
# 3. the rule is safe on the device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("type_name,m,n,B", PARITY_CASES)
def test_support_never_screened_on_device(type_name, m, n, B):
    supp = x_star(type_name, m, n, B) != 0
    assert 0 < supp.sum() < n
    for rec in checkpoints(type_name, m, n, B):
        assert int((supp & ~rec["keep"]).sum()) == 0, rec["t"]


# ---------------------------------------------------------------------------
# 4. gather
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("type_name", STORAGES)
@pytest.mark.parametrize("m,n,B", [(250, 2040, 4), (256, 2048, 2)])
def test_gather_columns_bitwise(type_name, m, n, B):
    gc = context(type_name, m, n, B)
    full = gc.A_b_gpu.permute(1, 0, 2).reshape(m, n)          # (H, K), the storage dtype
    as_int = {"double": torch.int64, "float": torch.int32, "bf16": torch.int16}[type_name]
    rs = np.random.RandomState(11)
    for n_out in (16, 176, 2032):
        sub = np.sort(rs.choice(n, n_out, replace=False))
        holes = sub.copy()
        holes[rs.choice(n_out, max(1, n_out // 5), replace=False)] = -1
        for cols in (sub, rs.permutation(sub), rs.permutation(holes)):
            ct = torch.from_numpy(cols.astype(np.int64)).cuda()
            want = full[:, ct.clamp(min=0)].clone()
            want[:, ct < 0] = 0
            for arg in (ct, cols.tolist()):                    # device tensor and host sequence
                got = gc.gather_columns(arg)
                assert got.dtype == full.dtype and tuple(got.shape) == (m, n_out) and got.is_contiguous()
                assert torch.equal(got.view(as_int), want.view(as_int)), (n_out, type_name)


# ---------------------------------------------------------------------------
# 5. the screened driver
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 4])
def test_screened_driver(B):
    m, n = 250, 2040
    As, b, mu = stored_instance("float", m, n)
    gc = make_cls("float")(As, B, device=0)
    drv = lasso.ClassLassoScreened(gc, gc.diag_ATA, As, b, mu, B, 4000)
    drv.run(GAP_BOUND=1e-7, SILENCE=True)
    bound = 1e-7 * 0.5 * float(b @ b)
    x = drv.x.reshape(-1)
    cert = C.duality_gap(As, b, x, mu)
    xs = x_star("float", m, n, B)
    p_star = C.duality_gap(As, b, xs, mu)["primal"]
    print(f"B{B}: iters {drv.iters}, trace n_active {[t['n_active'] for t in drv.trace]}, "
          f"gaps {[float('%.3e' % t['gap']) for t in drv.trace]}, bound {bound:.3e}, "
          f"full-A gap numpy {cert['gap']:.6e} device {drv.certificate['gap']:.6e}, "
          f"P(x) - P(x*) {cert['primal'] - p_star:.3e}")
    assert drv.stopped
    assert cert["gap"] <= bound + 1e-9 * cert["primal"]
    assert abs(drv.certificate["gap"] - cert["gap"]) <= 1e-9 * cert["primal"]
    assert cert["primal"] - p_star <= bound + 1e-9 * cert["primal"]
    off = np.ones(n, dtype=bool)
    off[drv.active] = False
    assert not x[off].any()
    assert np.isin(np.nonzero(xs)[0], drv.active).all()
    na = [t["n_active"] for t in drv.trace]
    assert all(a >= c for a, c in zip(na, na[1:])) and na[0] == n and na[-1] <= 0.25 * n
    assert drv.iters == drv.trace[-1]["t"] <= 4000


@pytest.mark.parametrize("B", [1, 4])
def test_screened_driver_without_compaction_is_the_device_loop(B):
    As, b, mu = stored_instance("float", 250, 2040)
    gc = make_cls("float")(As, B, device=0)
    drv = lasso.ClassLassoScreened(gc, gc.diag_ATA, As, b, mu, B, 4000, shrink=0)
    drv.run(GAP_BOUND=1e-7, SILENCE=True)
    assert drv.stopped and drv.active.size == 2040 and all(t["n_active"] == 2040 for t in drv.trace)
    g2 = make_cls("float")(As, B, device=0)
    dev = lasso.ClassLassoDevice(g2, g2.diag_ATA, As, b, mu, B, drv.iters)
    dev.run(SILENCE=True)
    assert dev.iters == drv.iters
    assert np.array_equal(drv.x, dev.x)


# ---------------------------------------------------------------------------
# 6. errors (argument and state checks on the host; nothing is launched)
# ---------------------------------------------------------------------------
def test_gap_state_errors():
    As, b, mu = stored_instance("float", 250, 2040)
    gc = make_cls("float")(As, 4, device=0)
    with pytest.raises(N.BpglError, match=r"\(-2\): .*bpgl_solver_reset"):
        gc.duality_gap()
    gc.solver_reset(b, mu)
    gc.set_ranks(0, 2)
    with pytest.raises(N.BpglError, match=r"\(-2\): .*single-rank"):
        gc.duality_gap()


def test_gather_argument_errors():
    As, _, _ = stored_instance("float", 250, 2040)
    gc = make_cls("float")(As, 4, device=0)
    cols = torch.arange(16, dtype=torch.int32, device="cuda")
    out = torch.empty((250, 32), dtype=torch.float32, device="cuda")
    L = N.lib()
    ctx, cp, op = gc._ctx, N.ptr(cols), N.ptr(out)
    assert L.bpgl_gather_columns(ctx, cp, 16, op, 18) == -1          # lda_out no multiple of 16 bytes
    assert "lda_out" in L.bpgl_last_error().decode()
    assert L.bpgl_gather_columns(ctx, cp, 16, op, 12) == -1          # lda_out < n_out
    assert L.bpgl_gather_columns(ctx, cp, 0, op, 16) == -1
    assert L.bpgl_gather_columns(ctx, None, 16, op, 16) == -1
    assert L.bpgl_gather_columns(ctx, cp, 16, ctypes.c_void_p(out.data_ptr() + 4), 16) == -1   # misaligned A_out
    assert L.bpgl_gather_columns(None, cp, 16, op, 16) == -1
    torch.cuda.synchronize()

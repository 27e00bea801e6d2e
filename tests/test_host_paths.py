"""The host layer's observable behaviour, pinned: what bpgl_set_tuning accepts, rejects and
invalidates for every key; which kernel kinds each form of the iteration times; and that graph
replay (graphs of 64, 4 and 2 iterations) and plain enqueueing give the same bits.

The expected tuning table below is written out from the rules of the ABI (include/bpgl.h), not read
from the library."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from convex_optimization_amd import _native as N  # noqa: E402
from convex_optimization_amd import distributed as D  # noqa: E402
from convex_optimization_amd.gpu_calculation import GPU_Calculation  # noqa: E402
from convex_optimization_amd.panel import PanelLasso  # noqa: E402

E_ARG, E_STATE = -1, -2
BIG = 1 << 40


def make_cls(type_name):
    return type("GC_" + type_name, (GPU_Calculation,), {"TYPE": type_name})


def problem(m, n, seed=0):
    rs = np.random.RandomState(seed + m + 3 * n)
    A = rs.randn(m, n) / np.sqrt(n)
    b = A @ np.where(rs.rand(n) < 0.3, rs.randn(n), 0.0) + 0.01 * rs.randn(m)
    return A, b, 0.1 * float(np.abs(A.T @ b).max())


def tune(gc, key, value):
    """(return code, last error) of bpgl_set_tuning"""
    rc = N.lib().bpgl_set_tuning(gc._ctx, key.encode(), int(value))
    return rc, N.lib().bpgl_last_error().decode(errors="replace")


def step_rc(gc, n=1):
    with gc._on_stream():
        return N.lib().bpgl_solver_step(gc._ctx, n)


# key: (smallest, largest admissible value; None = unbounded on that side), a reset must follow,
# the value that restores the default.  "cus" (before bind only) has a test of its own.
TUNING = {
    "reverse_rows": (None, None, True, 0),
    "tail_permille": (0, 1000, True, 120),
    "col_mode": (0, 2, True, 1),
    "onepass": (-1, 1, True, -1),
    "tail_row_blocks": (0, 1, False, 1),
    "onepass_cache_permille": (-1, 1000, True, -1),
    "onepass_rows": (-1, 1, True, -1),
    "onepass_sb1": (-1, 0, True, -1),
    "exchange_fp32": (-1, 1, True, 0),
    "onepass_fail_at": (None, None, True, -1),
    "onepass_refresh": (0, None, False, 256),
    "graph_max": (1, 64, True, 64),
    "nt_loads": (None, None, True, 1),
}


@pytest.fixture(scope="module")
def small():
    A, b, mu = problem(64, 256)
    return make_cls("float")(A, 1, device=0), b, mu


@pytest.mark.parametrize("key", sorted(TUNING))
def test_tuning_key(small, key):
    gc, b, mu = small
    lo, hi, invalidates, default = TUNING[key]
    try:
        for v in (lo if lo is not None else -BIG, hi if hi is not None else BIG):
            assert tune(gc, key, v)[0] == 0, (key, v)
        for v in ([] if lo is None else [lo - 1]) + ([] if hi is None else [hi + 1]):
            rc, msg = tune(gc, key, v)
            assert rc == E_ARG and key in msg, (key, v, rc, msg)
        assert tune(gc, key, default)[0] == 0
        gc.solver_reset(b, mu)
        assert step_rc(gc) == 0
        assert tune(gc, key, default)[0] == 0
        if invalidates:
            assert step_rc(gc) == E_STATE
            assert step_rc(gc) == E_STATE   # until the next reset
            gc.solver_reset(b, mu)
        assert step_rc(gc) == 0
        assert gc.solver_status()["iters"] == (1 if invalidates else 2)
    finally:
        tune(gc, key, default)


def test_tuning_rejections_and_read_back(small):
    gc, b, mu = small
    rc, msg = tune(gc, "graph_max", 3)
    assert rc == E_ARG and "graph_max" in msg
    rc, msg = tune(gc, "cus", 1)
    assert rc == E_STATE and "cus" in msg   # after bind
    rc, msg = tune(gc, "no_such_key", 0)
    assert rc == E_ARG and "no_such_key" in msg
    assert N.lib().bpgl_set_tuning(gc._ctx, None, 0) == E_ARG
    # one segment block per row: the LDS-only hand-off by default; an explicit "onepass_rows" = 1 or
    # "onepass_sb1" = 0 takes the granule form, which is interleaved only when asked for
    stats = lambda: (gc.solver_stat("onepass_rows"), gc.solver_stat("onepass_sb1"))
    try:
        gc.solver_reset(b, mu)
        assert stats() == (0, 1) and gc.solver_stat("onepass") == 1
        for rows, sb1, want in [(1, -1, (1, 0)), (0, -1, (0, 1)), (0, 0, (0, 0)), (-1, 0, (0, 0)), (1, 0, (1, 0)),
                                (-1, -1, (0, 1))]:
            assert tune(gc, "onepass_rows", rows)[0] == 0 and tune(gc, "onepass_sb1", sb1)[0] == 0
            assert stats() == want, (rows, sb1)
            gc.solver_reset(b, mu)
            assert step_rc(gc, 3) == 0 and gc.solver_status()["iters"] == 3
            assert stats() == want and gc.solver_stat("onepass") == 1
        assert gc.solver_stat("refresh_period") == 256
        for v, want in [(0, 0), (7, 7), (BIG, 1 << 30), (256, 256)]:
            assert tune(gc, "onepass_refresh", v)[0] == 0
            assert gc.solver_stat("refresh_period") == want
            assert step_rc(gc) == 0   # no reset needed
        assert tune(gc, "onepass", 0)[0] == 0
        gc.solver_reset(b, mu)
        assert gc.solver_stat("onepass") == 0 and gc.solver_stat("refresh_period") == 0
    finally:
        for key in ("onepass", "onepass_rows", "onepass_sb1"):
            tune(gc, key, -1)
        tune(gc, "onepass_refresh", 256)


def test_cus_before_bind():
    L = N.lib()
    ctx = ctypes.c_void_p()
    N.check(L.bpgl_create(ctypes.byref(ctx), 0, N.BPGL_F32, 64, 256, 1, None), "bpgl_create")
    try:
        v = ctypes.c_int64()
        N.check(L.bpgl_solver_stat(ctx, b"cus", ctypes.byref(v)), "bpgl_solver_stat")
        dev = v.value
        assert dev >= 1
        for bad in (0, dev + 1):
            assert L.bpgl_set_tuning(ctx, b"cus", bad) == E_ARG
            assert "cus" in L.bpgl_last_error().decode()
        for ok in (dev, 1):
            assert L.bpgl_set_tuning(ctx, b"cus", ok) == 0
            N.check(L.bpgl_solver_stat(ctx, b"cus", ctypes.byref(v)), "bpgl_solver_stat")
            assert v.value == ok
        N.check(L.bpgl_solver_stat(ctx, b"onepass_grid", ctypes.byref(v)), "bpgl_solver_stat")
        assert v.value == 1   # one CU: one row group of one segment block
    finally:
        L.bpgl_destroy(ctx)


TWOPASS = {"colpass", "shrink", "rowpass", "rowreduce", "update"}
# (feature blocks, RCCL communicator of one rank, shard, "onepass", "onepass_refresh", steps) -> kinds timed
TIMED = [
    (1, False, "columns", -1, 256, 3, {"onepass", "update"}),
    (1, False, "columns", 0, 256, 3, TWOPASS),
    (2, False, "columns", -1, 256, 3, TWOPASS),
    (2, True, "columns", -1, 256, 3, TWOPASS | {"allreduce", "step"}),
    (1, True, "rows", -1, 256, 3, {"onepass", "rowreduce", "allreduce", "update"}),
    (1, True, "rows", 0, 256, 3, {"colpass", "rowpass", "rowreduce", "allreduce", "update"}),
    (1, False, "columns", -1, 2, 5, {"onepass", "update", "refresh"}),
]


@pytest.mark.parametrize("blocks,comm,shard,onepass,refresh,steps,want", TIMED,
                         ids=["onepass", "onepass_off", "two_blocks", "rccl_columns", "rccl_rows", "rccl_rows_twopass",
                              "refresh"])
def test_timed_kinds(blocks, comm, shard, onepass, refresh, steps, want):
    A, b, mu = problem(64, 256)
    gc = make_cls("float")(A, blocks, device=0, comm=D.RankComm(0, 1) if comm else None, shard=shard)
    gc.set_tuning("onepass", onepass)
    gc.set_tuning("onepass_refresh", refresh)
    gc.solver_reset(b, mu, use_graph=False)
    gc.set_kernel_timing(True)
    gc.solver_step(steps)
    t, n = gc.kernel_times()
    print(f"timed kinds blocks={blocks} comm={comm} {shard} onepass={onepass}: {t}")
    assert n == steps
    assert {k for k, v in t.items() if v > 0} == want
    t2, n2 = gc.kernel_times()
    assert n2 == 0 and not any(t2.values())
    gc.set_kernel_timing(False)
    assert gc.solver_status()["iters"] == steps


@pytest.mark.parametrize("m", [256, 1024])   # 1024 rows admit the fused reduce + update, 256 do not
@pytest.mark.parametrize("fuse", [1, 0])
def test_panel_timed_kinds(m, fuse):
    n, k = 256, 16
    rs = np.random.RandomState(m + fuse)
    A = rs.randn(m, n) / np.sqrt(n)
    B = rs.randn(m, k)
    pl = PanelLasso(A, 1, nrhs=k, device=0)
    pl.set_tuning("fuse_update", fuse)
    fused = bool(pl.get_tuning("fuse_update"))
    assert fused == (fuse == 1 and m == 1024 and pl.stat("fuse_cus") >= k)
    pl.solver_reset(B, 0.1, use_graph=False)
    pl.set_kernel_timing(True)
    pl.solver_step(3)
    t, ns = pl.kernel_times()
    print(f"panel timed kinds m={m} fused={fused}: {t}")
    assert ns == 3
    # the line search runs in the reduce ("step" is never timed); the fused form has no update launch
    want = {"pass1_mfma", "pass2_mfma", "reduce"} | (set() if fused else {"update"})
    assert {key for key, v in t.items() if v > 0} == want
    t2, n2 = pl.kernel_times()
    assert n2 == 0 and not any(t2.values())
    pl.set_kernel_timing(False)


@pytest.mark.parametrize("type_name,n", [("float", 256), ("double", 256), ("bf16", 512)])
def test_graph_replay_and_enqueue_agree(type_name, n):
    """70 iterations replay the graphs of 64, 4 and 2 iterations (graph_max 64) or 70 graphs of one
    (graph_max 1); without graphs every launch is enqueued: the same bits all four ways"""
    A, b, mu = problem(64, n)
    gc = make_cls(type_name)(A, 1, device=0)
    xs = []
    for graph_max in (1, 64):
        gc.set_tuning("graph_max", graph_max)
        for use_graph in (True, False):
            res = gc.run(b, mu, 70, use_graph=use_graph)
            assert res["iters"] == 70 and gc.solver_stat("enqueued") == 70
            xs.append(res["x"])
    assert np.abs(xs[0]).max() > 0
    for x in xs[1:]:
        np.testing.assert_array_equal(x, xs[0])

"""Every iteration of the panel solver is the algorithm's step (panel_step_reference.check_step, A-D).

Reset, then ``solver_step(1)`` eighteen times with a snapshot (x, R, the error record) after each, and
``check_step`` on every pair of consecutive snapshots, every right-hand side: dR = w o (A dx) to the fp32
summation bound (A), the step an exact line search along the direction taken (B), the direction the shrink
of the exact gradient within the operand-precision allowances (C), the error record (D).  With
``g_refresh`` 8 the eighteen iterations hold the first one, carried ones, the last carried before a refresh
(t = 7, 15), the refreshes (t = 8, 16) and the first carried after each.  The checker and its bounds are
proved against a numpy model and eleven mutants of it in tests/test_panel_step_host.py.

Instance: tests/test_panel.py::instance's A and B with mu_j = ||A^T b_j||_inf * geomspace(0.3, 0.05, k)_j,
so that no two right-hand sides share b or mu.  Shapes (m, n, Block, k): the smallest at which each kernel
variant runs (the lists below), and 1024 x 1024 / 1024 x 2048 for the fused reduce + update, whose 1024 x 512 steps
fall below 1e-3 |x| after t = 9 (test_panel_step_host.py::test_steps_are_informative).

A one-iteration step launches its kernels directly whether or not the reset captured graphs (a graph holds
eight iterations), and ends with the flush of the pending x update, so the pass-1 epilogue never applies a
pending update here.  Each test therefore ends with one ``solver_step(18)`` from a fresh reset -- graphs
replayed, x deferred into the epilogues -- whose x, R and error record must equal the stepped run's bitwise.

Worst ratio to bound on the MI355X, over all 106 cases: A 0.247, B 0.114, C 0.987, D 0.235 (the numpy model
of test_panel_step_host.py: 0.25, 0.098, 0.987, 0.28).  C has no margin by construction: its u_D = 2^-8 is the
bf16 image's own rounding.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import panel_step_reference as P  # noqa: E402
from convex_optimization_amd.panel import PanelLasso  # noqa: E402
from test_panel import instance as panel_instance  # noqa: E402

T_STEPS = 18
G_REFRESH = 8

# (m, n, Block, k, masked)
TWO_KERNEL = [(256, 512, 1, 16, False), (256, 512, 1, 32, False), (256, 512, 1, 64, False)]
LDS_EPILOGUE = [(256, 256, 1, 128, False), (256, 512, 1, 128, False)]
FUSED = [(1024, 512, 1, 16, False), (1024, 512, 1, 128, False), (1024, 1024, 1, 16, False), (1024, 2048, 1, 128, False)]
MULTI_BLOCK = [(256, 1024, 2, 16, False), (256, 768, 3, 64, False)]
MASKED = [(256, 512, 1, 16, True), (1024, 512, 1, 16, True), (1024, 1024, 1, 16, True)]
ONE_BLOCK = TWO_KERNEL + LDS_EPILOGUE + FUSED + MASKED
WORST = {}


@functools.lru_cache(maxsize=None)
def problem(m, n, k, masked):
    Ab, B, mu = P.instance(m, n, k, seed=m + n + k)
    ref = panel_instance(m, n, k, seed=m + n + k)
    assert np.array_equal(Ab, ref[0]) and np.array_equal(B, ref[1])
    W = P.fold_mask(m, k) if masked else None
    for a in (Ab, B, mu) + ((W,) if masked else ()):
        a.setflags(write=False)
    return Ab, B, mu, W


def run_case(m, n, Block, k, masked, d_split, carry, defer_x, use_graph):
    Ab, B, mu, W = problem(m, n, k, masked)
    B_dev = B.copy()                                       # (torch warns about read-only arrays)
    pl = PanelLasso(Ab.copy(), Block, nrhs=k, device=0)
    pl.set_tuning("d_split", d_split)
    if Block == 1:
        pl.set_tuning("carry_g", carry)
        pl.set_tuning("g_refresh", G_REFRESH)
        pl.set_tuning("defer_x", defer_x)
    if masked:
        pl.set_row_mask(W.copy())
    carried = pl.get_tuning("carry_g") == 1
    assert carried == (Block == 1 and carry == 1)
    assert pl.get_tuning("fuse_update") == int(m % 1024 == 0 and Block == 1 and defer_x == 1)
    diag = pl.diag_ATA
    np.testing.assert_allclose(diag.reshape(-1), np.square(Ab).sum(axis=0), rtol=1e-12)   # full norms, masked or not
    chain = d_split * (n // Block // pl.kchunks)

    pl.solver_reset(B_dev, mu, record_len=T_STEPS, use_graph=use_graph)
    snaps, errs, stats, bad = [P.snapshot(pl)], [], {}, []
    assert not snaps[0][0].any() and np.array_equal(snaps[0][1], np.where(W.T != 0, -B.T, 0.0) if masked else -B.T)
    for t in range(T_STEPS):
        pl.solver_step(1)
        snaps.append(P.snapshot(pl))
        status = pl.solver_status()
        err_iter = pl._err_iter.cpu().numpy()
        errs.append(float(err_iter[t]))
        assert status["iters"] == t + 1
        assert np.array([status["err"]]).tobytes() == err_iter[t:t + 1].tobytes()   # bitwise the last record
        q = t % G_REFRESH if carried else 0
        exact = not carried or q == 0
        viol = P.check_step(Ab, diag, mu, W, t % Block, snaps[t], snaps[t + 1], errs[t], d_split, exact,
                            None if exact else snaps[t][1] - snaps[t - 1][1], chain=chain, q=q,
                            R_ref=None if exact else snaps[t - q][1], stats=stats)
        bad += [(t, v) for v in viol]
    assert pl.stat("exact_gradients") == (3 if carried else 0)
    key = (m, n, Block, k, masked)
    line = " ".join(f"{c} {stats[c]:.3g}" for c in "ABCD")
    print(f"panel step {key} d_split={d_split} carry={carry} defer_x={defer_x} graph={use_graph}: "
          f"worst ratio to bound {line}, gamma in [{stats['gamma_min']:.3g}, {stats['gamma_max']:.3g}]")
    for c in "ABCD":
        WORST[c] = max(WORST.get(c, 0.0), stats[c])
    print("  so far over all cases: " + " ".join(f"{c} {WORST[c]:.3g}" for c in "ABCD"))
    assert not bad, bad

    # the same eighteen iterations in one call: the graphs (when captured) and the deferred x update
    pl.solver_reset(B_dev, mu, record_len=T_STEPS, use_graph=use_graph)
    pl.solver_step(T_STEPS)
    x, R = P.snapshot(pl)
    assert np.array_equal(x, snaps[-1][0]) and np.array_equal(R, snaps[-1][1])
    assert pl._err_iter.cpu().numpy().tobytes() == np.array(errs).tobytes()


@pytest.mark.parametrize("defer_x", [1, 0])
@pytest.mark.parametrize("carry", [1, 0])
@pytest.mark.parametrize("d_split", [1, 2])
@pytest.mark.parametrize("m,n,Block,k,masked", ONE_BLOCK)
def test_one_block_steps(m, n, Block, k, masked, d_split, carry, defer_x):
    run_case(m, n, Block, k, masked, d_split, carry, defer_x, use_graph=True)


@pytest.mark.parametrize("d_split", [1, 2])
@pytest.mark.parametrize("m,n,Block,k,masked", MULTI_BLOCK)
def test_multi_block_steps(m, n, Block, k, masked, d_split):
    """Ax per block, the exact gradient every iteration, mb = t % Block."""
    run_case(m, n, Block, k, masked, d_split, 0, 0, use_graph=True)


@pytest.mark.parametrize("m,n,Block,k,masked", [TWO_KERNEL[0], LDS_EPILOGUE[0], FUSED[0], MULTI_BLOCK[0], MASKED[0],
                                                MASKED[1]])
def test_steps_without_graphs(m, n, Block, k, masked):
    """One case per form with no graph captured at the reset."""
    run_case(m, n, Block, k, masked, 1, 1, 1, use_graph=False)

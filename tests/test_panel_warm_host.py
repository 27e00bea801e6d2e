"""Host side of the panel warm start and gap-safe compaction, no device needed:
``cpu_calculation.compaction_columns``, the drivers' argument checks, the null-context rejections of the two
new ABI functions, and the schedule of the fp64 reference driver (panel_screen_reference.py) on the screen
instance, which pins the premises of tests/test_panel_warm.py.

Measured with the fp64 reference (256 x 2048, 16 values of mu, check_every 64), worst relative gap over
the grid / size of the union of keep:
  Block 1: 3.3e-3 / 2048 at t = 64, 1.26e-5 / 217 at 128, 9.2e-8 / 116 at 192
  Block 2: 3.6e-3 / 2048, 2.4e-5 / 275, then on the compacted problem 1.4e-6 / 140 at 192
With shrink 0.75 the reference compacts once, at t = 128: 2048 -> 256 columns (Block 1, q = 256) or 512
(Block 2, q = 512).  With GAP_BOUND 3e-6 it stops at t = 192 in both, so the check at 128 is >= 4x above the
bound and the stop >= 2x below it: the schedule does not hinge on rounding.  With GAP_BOUND 1e-6 the screened
x equals the unscreened one to 7.1e-9 (Block 1) and 2.3e-7 (Block 2) relative l2.
"""
import functools

import numpy as np
import pytest

from convex_optimization_amd import _native as N
from convex_optimization_amd import cpu_calculation as C
from convex_optimization_amd import panel
from panel_screen_reference import screen_instance, screened_reference

BOUND = 3e-6
T_REF = 192


# ---------------------------------------------------------------------------
# compaction_columns
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,q,n_keep", [(2048, 256, 217), (2048, 512, 275), (2048, 256, 256), (2048, 256, 257),
                                        (1024, 256, 0), (1024, 256, 1), (768, 256, 700)])
def test_compaction_columns(n, q, n_keep):
    rs = np.random.RandomState(n + q + n_keep)
    keep = np.zeros(n, dtype=bool)
    keep[rs.permutation(n)[:n_keep]] = True
    sel = C.compaction_columns(keep, q)
    assert sel.dtype == np.int64 and sel.ndim == 1
    assert np.all(np.diff(sel) > 0)                                   # sorted, no duplicates
    assert sel.size % q == 0 and sel.size >= q
    assert sel.size == max(q, -(-n_keep // q) * q)                    # the next multiple, no more
    assert np.all(np.isin(np.flatnonzero(keep), sel))                 # a superset of the kept set
    pads = np.setdiff1d(sel, np.flatnonzero(keep))
    assert np.array_equal(pads, np.flatnonzero(~keep)[:pads.size])    # the smallest screened indices
    assert np.array_equal(sel, C.compaction_columns(keep.astype(np.uint8), q))   # deterministic, any 0/1 type


def test_compaction_columns_all_kept_and_errors():
    assert np.array_equal(C.compaction_columns(np.ones(1024, dtype=bool), 256), np.arange(1024))
    assert np.array_equal(C.compaction_columns(np.zeros(512, dtype=bool), 256), np.arange(256))
    for q in (0, -256, 300):
        with pytest.raises(ValueError):
            C.compaction_columns(np.ones(1024, dtype=bool), q)


# ---------------------------------------------------------------------------
# argument checks that need no device
# ---------------------------------------------------------------------------
def test_driver_argument_checks():
    A = np.zeros((256, 512))
    b = np.ones(256)
    mus = np.linspace(1.0, 0.1, 16)
    with pytest.raises(ValueError, match="x0 needs mus"):
        panel.lasso_path(A, b, x0=np.zeros((512, 16)))
    for bad in (np.zeros((512, 15)), np.zeros((16, 512)), np.zeros(512)):
        with pytest.raises(ValueError, match="x0 must be"):
            panel.lasso_path(A, b, mus=mus, x0=bad)
    for shrink in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="shrink"):
            panel.lasso_path(A, b, mus=mus, shrink=shrink)
        with pytest.raises(ValueError, match="shrink"):
            panel.lasso_cv(A, b, n_folds=4, mus=mus[:4], shrink=shrink)


def test_new_abi_null_context_is_an_error_not_a_crash():
    L = panel._lib()
    assert L.bpgl_version() >= 306
    assert L.bpgl_panel_reset_x0(None, None, None, None, None, 0, 0) == -1
    assert L.bpgl_last_error().decode()
    assert L.bpgl_panel_gather_columns(None, None, 0, None, 0) == -1
    assert L.bpgl_last_error().decode()
    for name in ("bpgl_panel_reset_x0", "bpgl_panel_gather_columns"):
        assert name in N.header_functions() and name in N._SIGS


# ---------------------------------------------------------------------------
# the reference's schedule on the screen instance
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(Block, bound, shrink):
    Ab, b, _, mus, _ = screen_instance()
    return screened_reference(Ab, b, mus, Block, bound, 4 * T_REF, 64, shrink)


@pytest.mark.parametrize("Block,n_after,union_128", [(1, 256, 217), (2, 512, 275)])
def test_reference_schedule(Block, n_after, union_128):
    Ab, b, _, mus, _ = screen_instance()
    ref = reference(Block, BOUND, 0.75)
    print(f"Block {Block}: {ref['trace']}, compactions {ref['compactions']}")
    assert ref["compactions"] == [(128, n_after)]
    assert ref["t"] == T_REF and ref["reached"].all()
    (t1, g1, u1, a1), (t2, g2, u2, a2), (t3, g3, u3, a3) = ref["trace"]
    assert (t1, t2, t3) == (64, 128, 192) and (a1, a2, a3) == (2048, 2048, n_after)
    assert u1 == 2048 and u2 == union_128                 # nothing to drop at 64, most columns at 128
    assert g2 >= 4 * BOUND and g3 <= BOUND / 2            # the schedule does not hinge on rounding
    assert ref["active"].size == n_after and np.all(np.diff(ref["active"]) > 0)
    # the certificate of the scattered x on the full A meets the bound, and no dropped column carries weight
    for j in range(len(mus)):
        x32 = ref["x"][:, j].astype(np.float32).astype(np.float64)
        assert C.duality_gap(Ab, b, x32, mus[j])["gap"] <= BOUND * 0.5 * float(b @ b)
    assert not np.delete(ref["x"], ref["active"], axis=0).any()


@pytest.mark.parametrize("Block,tol", [(1, 1e-7), (2, 1e-6)])
def test_reference_screened_equals_unscreened(Block, tol):
    """GAP_BOUND 1e-6: both runs end within sqrt(2 gap) of the same optimum."""
    plain, screened = reference(Block, 1e-6, 0.0), reference(Block, 1e-6, 0.75)
    rel = np.linalg.norm(screened["x"] - plain["x"]) / np.linalg.norm(plain["x"])
    print(f"Block {Block}: screened vs unscreened {rel:.2e}, stops {screened['t']} / {plain['t']}")
    assert screened["compactions"] and not plain["compactions"]
    assert rel <= tol


def test_reference_cv_schedule():
    """The premises of test_panel_warm.py's lasso_cv tests: 4 folds (kfold_masks seed 0) x mus[0, 4, 8, 12],
    GAP_BOUND 1e-5.  Measured: relative gap 1.2e-3 / 4.0e-5 / 1.5e-6 at t = 64 / 128 / 192, union of keep
    1987 / 335 / 229; one compaction, 2048 -> 512 at t = 128; the stop at 192."""
    Ab, b, _, mus, _ = screen_instance()
    cols = np.arange(16)
    fold, jmu = cols // 4, cols % 4
    W = C.kfold_masks(Ab.shape[0], 4, 0)[fold].T
    ref = screened_reference(Ab, b, mus[[0, 4, 8, 12]][jmu], 1, 1e-5, 1024, 64, 0.75, W=W)
    print(ref["trace"], ref["compactions"])
    assert ref["compactions"] == [(128, 512)] and ref["t"] == 192 and ref["reached"].all()
    assert ref["trace"][1][1] >= 3 * 1e-5 and ref["trace"][2][1] <= 1e-5 / 4

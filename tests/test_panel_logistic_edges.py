"""GPU tests of the logistic model's kernels (csrc/bpgl_panel_glm.hip) on the states written for
the hard cases: the curvature floor, p rounded to exactly 1, the safeguards of the intercept's Newton iteration, the
one-class flag, the model without an intercept, fractional labels, and the end points of the dual sum.  Every state is
placed with ``solver_reset(B, mu, x0=X)``; every comparison is against ``cpu_calculation.logistic_model`` /
``logistic_dual`` / ``logistic_gap`` on the fp32 x read back with ``solver_x()``.  The instances, the assertions and
their tolerances are in tests/panel_logistic_instance.py (``edge_instance``, ``check_model_column``, ``check_dual``);
tests/test_panel_logistic_host.py shows on the CPU that the instances reach the branches and that the assertions
reject five mutants of the restatement.

Shapes, and product 1's split (``pgap_split(m / 64, n / 32)``: doubled while m / 64 x split < 512 and a chunk keeps two
32-deep stages):
  256 x 512,  k = 16   4 tiles, 16 stages: split 8;   1 row block per right-hand side
  768 x 256,  k = 32  12 tiles,  8 stages: split 4;   3 row blocks (m no power of two), the k = 32 product
  256 x 512,  k = 64   4 tiles, 16 stages: split 8;   the k = 64 product
  4096 x 256, k = 16  64 tiles,  8 stages: split 4 (256 blocks; 8 would leave one stage per chunk); 16 row blocks

Columns per 16: 3 saturated (planted model x 8, 40, 1: a floor share of 12 to 31 %, 56 to 83 % and 0), 9 two-cluster (sep 12 / 30 / 45 x ybar 0.2 / 0.5 / 0.9, every
other one started at 500, outside the bracket), 3 one-class, 1 of fractional labels.

Bounds.  AX, P, W, the five sums, |phi|: those of tests/test_panel_logistic.py.  W on the floor rows and where om = 0:
bitwise.  beta0 and Z on the floor rows: derived per column in ``beta_tolerance`` and ``check_model_column``, from the
stopping rule of the Newton iteration and from the division by v = 1e-5, from the restatement and the AX bound alone:
no output of the device enters a tolerance.  The step
count is exact in the columns whose count on the CPU survives 8 draws of +-1 ulp noise on sigma, +-1 elsewhere.

Measured on one MI355X (worst over the columns of the shape; `pytest -s` prints them).  Sums: relative error of the
five sums.  beta0: against the restatement's root / against the long double bisection (the latter's 4.1e-13 is the
restatement's own distance in a scale-40 column, where phi' = 1.2e-2 sum om; the phi term of its bound there is 9.6e-13).
Z: relative error on the floor rows.  Exact: the share of columns with a root whose step count must match exactly -- it
did in all.  AX was bitwise the restatement's in every column.
                        sums      beta0                Z (floor)   exact          dual / (sum om log 2)   R / bound
  256 x 512,  k = 16    4.0e-16   5.6e-17 / 4.4e-14    0           100 % of 13    0                       < 0.01
  768 x 256,  k = 32    1.4e-16   4.4e-16 / 5.0e-14    1.4e-16     100 % of 26    1.1e-16                 < 0.01
  256 x 512,  k = 64    1.7e-16   1.8e-15 / 4.1e-13    0           100 % of 52    9.0e-17                 0.09
  4096 x 256, k = 16    1.7e-16   1.1e-14 / 7.1e-14    5.4e-16     100 % of 13    2.3e-16                 0.02
Step counts taken: 2 to 11; 1 to 5 of them midpoint fallbacks in every two-cluster column.

Not reached.  ``d > 0`` false in the Newton loop: inside the bracket some row with a weight has sigma <= ybar < 1 and
some row sigma >= ybar > 0, so phi' > 0 at every point the loop can visit.  The cap of 40 steps: no instance here needs
more than 11.  p rounded to exactly 0 (eta < -745): the ``t > 0`` branch of the dual is reached through scale = 0 and a
label 0 instead.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import panel_logistic_instance as I  # noqa: E402
from convex_optimization_amd import cpu_calculation as C  # noqa: E402
from convex_optimization_amd import panel  # noqa: E402
from convex_optimization_amd.panel import PanelLasso  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = {"256x512x16": (256, 512, 16), "768x256x32": (768, 256, 32), "256x512x64": (256, 512, 64),
          "4096x256x16": (4096, 256, 16)}
MU_FRAC = 0.3
KEYS = ("AX", "P", "W", "Z", "beta0") + PanelLasso.GLM_KEYS


def dev(v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda()


def host(mod):
    """a ``glm_model`` result as numpy copies (its tensors are buffers the next call overwrites)"""
    return {key: (v.cpu().numpy().copy() if isinstance(v, torch.Tensor) else np.array(v)) for key, v in mod.items()}


def column(mod, c):
    """column c of a ``host`` result under the restatement's keys"""
    out = {key: mod[key][c] for key in PanelLasso.GLM_KEYS}
    out.update(ax=mod["AX"][c], beta0=float(mod["beta0"][c]), p=mod["P"][c], w=mod["W"][c], z=mod["Z"][c])
    return out


@pytest.fixture(scope="module", params=list(SHAPES))
def state(request):
    """One context per shape, driven once: x placed; the model (twice, then from the stored root, then without scoring
    weights); the dual sums; the model with the one-class columns relabelled, the inner reset and its certificate; the
    model without the intercept.  The tests assert on what it recorded; the references are computed here once."""
    m, n, k = SHAPES[request.param]
    inst = I.edge_instance(m, n, k)
    A, Y, Om, H, X, B0 = (inst[q] for q in ("A", "Y", "Om", "H", "X", "B0"))
    s = dict(inst=inst, m=m, n=n, k=k)
    pl = PanelLasso(A.copy(), 1, nrhs=k, device=0)
    pl.set_intercept(True)
    zeros = np.zeros((m, k))
    pl.solver_reset(zeros, 1.0, x0=X)
    s["x"] = x = pl.solver_x()
    Yd, Omd, Hd = dev(Y), dev(Om), dev(H)
    s["mod"] = host(pl.glm_model(Yd, Omd, Hd, None, dev(B0)))
    s["mod_twice"] = host(pl.glm_model(Yd, Omd, Hd, None, dev(B0)))
    s["mod_from_root"] = host(pl.glm_model(Yd, Omd, Hd, None, None))      # beta0=None: the start is the last root
    s["mod_no_hold"] = host(pl.glm_model(Yd, Omd, None, None, dev(B0)))
    s["x_after_model"] = pl.solver_x()
    s["mix"] = mix = np.resize([0.5, 1e-8, 1.0, 0.0, 0.999], k)      # another scale in every column, each value used
    s["D1"], s["D0"], s["Dmix"] = pl.glm_dual(np.ones(k)), pl.glm_dual(np.zeros(k)), pl.glm_dual(mix)

    # every column with a root: the one-class columns relabelled; then the inner reset and its certificate
    Y2, Om2, B02 = I.without_one_class(inst)
    Y2d, Om2d = dev(Y2), dev(Om2)
    mod2 = pl.glm_model(Y2d, Om2d, Hd, None, dev(B02))
    s["mod2"] = host(mod2)
    ref = [C.logistic_model(A, Y[c], Om[c], x[:, c], B0[c], True, 0, H[c]) for c in range(k)]
    ref2 = [C.logistic_model(A, Y2[c], Om2[c], x[:, c], B02[c], True, 0, H[c]) if ref[c]["flag"] else ref[c]
            for c in range(k)]
    g0 = np.array([np.abs(A.T @ (Om2[c] * (ref2[c]["p"] - Y2[c]))).max() for c in range(k)])
    s["mu"] = mu = MU_FRAC * g0
    pl.set_row_weights_device(mod2["W"], Hd)
    pl.solver_reset(mod2["Z"].t(), 4.0 * mu, x0=pl.solver_x_device())
    pl.stream.synchronize()
    s["R"] = pl.residual_device().cpu().numpy().copy()
    cert = pl.duality_gap(screen=False)
    s["cert"] = {key: (v.cpu().numpy().copy() if isinstance(v, torch.Tensor) else np.copy(v))
                 for key, v in cert.items() if v is not None}
    s["x_after_reset"] = pl.solver_x()

    # the same instances without the intercept
    pl.set_row_weights(None)
    pl.set_intercept(False)
    pl.solver_reset(zeros, 1.0, x0=X)
    s["mod_off"] = host(pl.glm_model(Yd, Omd, Hd, None, dev(B0)))
    s["x_off"] = pl.solver_x()

    s.update(ref=ref, ref2=ref2, Y2=Y2, Om2=Om2,
             ref_off=[C.logistic_model(A, Y[c], Om[c], x[:, c], B0[c], False, 0, H[c]) for c in range(k)],
             stable=[bool(r["flag"]) or I.count_is_stable(r["ax"], Y[c], Om[c], B0[c]) for c, r in enumerate(ref)],
             root=[None if r["flag"] else I.root_longdouble(r["ax"], Y[c], Om[c]) for c, r in enumerate(ref)])
    return s


def test_x_is_the_x_placed(state):
    for key in ("x", "x_after_model", "x_after_reset", "x_off"):
        assert state[key].tobytes() == state["inst"]["X"].tobytes(), key


# ---------------------------------------------------------------------------
# 2. the model at the edges
# ---------------------------------------------------------------------------
def test_model_matches_the_restatement_at_the_edges(state):
    s, inst, k = state, state["inst"], state["k"]
    worst = {}
    for c in range(k):
        try:
            err = I.check_model_column(column(s["mod"], c), s["ref"][c], inst["Y"][c], inst["Om"][c],
                                       s["stable"][c], root=s["root"][c])
        except AssertionError as e:
            raise AssertionError((c, inst["kinds"][c]) + tuple(e.args)) from e
        for key, v in err.items():
            worst[key] = max(worst.get(key, 0.0), v)
    rooted = [c for c in range(k) if not s["ref"][c]["flag"]]
    share = np.mean([s["stable"][c] for c in rooted])
    print(f"{s['m']} x {s['n']}, k = {k}: worst " + ", ".join(f"{key} {v:.1e}" for key, v in sorted(worst.items()))
          + f"; exact-count class {share:.0%} of {len(rooted)} columns; steps "
          + str(sorted({int(s['mod']['steps'][c]) for c in rooted})))
    assert share >= 0.9
    assert [c for c in range(k) if s["mod"]["flag"][c] == 1] == I.columns_of(inst, "one")
    # the instance is what it claims to be, on the x the device holds
    floor = [np.mean(s["ref"][c]["v"] == C.GLM_FLOOR) for c in range(k)]
    sat = I.columns_of(inst, "sat")
    assert all((floor[c] > 0) == (inst["kinds"][c]["scale"] != 1.0) for c in sat)     # x 8 and x 40 reach it, x 1 does not
    assert all(floor[c] < 1 for c in sat)
    assert any((s["ref"][c]["p"][inst["Om"][c] > 0] == 1.0).any() for c in I.columns_of(inst, "sat"))
    assert all(floor[c] > 0 for c in I.columns_of(inst, "two"))


def test_one_class_columns_leave_the_others_alone(state):
    """flag 1, no steps, beta0 bitwise the incoming value (asserted in ``check_model_column``); and every other column
    of the call is, byte for byte, what it is when those columns hold ordinary labels."""
    s, inst = state, state["inst"]
    one = I.columns_of(inst, "one")
    assert len(one) == 3 * (s["k"] // 16)
    for c in one:
        assert s["mod"]["flag"][c] == 1 and s["mod"]["steps"][c] == 0
        assert s["mod"]["beta0"][c] == inst["B0"][c] == I.ONE_CLASS_B0[inst["kinds"][c]["kind"]]
        assert s["mod2"]["flag"][c] == 0 and s["mod2"]["steps"][c] > 0
    rest = [c for c in range(s["k"]) if c not in one]
    for key in KEYS:
        assert s["mod"][key][rest].tobytes() == s["mod2"][key][rest].tobytes(), key
    assert s["mod"]["AX"].tobytes() == s["mod2"]["AX"].tobytes()


def test_model_without_the_intercept(state):
    s, inst, k = state, state["inst"], state["k"]
    assert (s["mod_off"]["beta0"] == 0.0).all() and (s["mod_off"]["steps"] == 0).all()
    assert (s["mod_off"]["flag"] == 0).all()
    for c in range(k):
        try:
            I.check_model_column(column(s["mod_off"], c), s["ref_off"][c], inst["Y"][c], inst["Om"][c], True,
                                 intercept=False)
        except AssertionError as e:
            raise AssertionError((c, inst["kinds"][c]) + tuple(e.args)) from e
    # |phi(0)| is not small, this is no root: in a two-cluster column phi(0) / sum om is about 1/2 - ybar
    assert all(s["ref_off"][c]["phi"] > 0.1 * inst["Om"][c].sum() for c in I.columns_of(inst, "two")
               if inst["kinds"][c]["ybar"] != 0.5)


def test_fractional_labels_and_the_miss_rule(state):
    """y = 1/2 is no class 1: the row is a miss exactly when p > 1/2.  The rows are there, carry scoring weights, and
    counting them with >= would move ``hold_miss`` by far more than the bound it is held to."""
    s, inst = state, state["inst"]
    for c in I.columns_of(inst, "frac"):
        y, h, r = inst["Y"][c], inst["H"][c], s["ref"][c]
        half = y == 0.5
        assert half.sum() == 12 and (h[half] > 0).all() and ((y > 0) & (y < 1) & ~half).sum() > s["m"] // 2
        moved = float(h[half & (r["p"] > 0.5)].sum())        # what `>=` on y would take out of the sum
        assert moved > 1e-3 * r["hold_miss"] > 0
        assert abs(s["mod"]["hold_miss"][c] - r["hold_miss"]) <= 1e-9 * r["hold_miss"]
        assert abs(s["mod_off"]["hold_miss"][c] - s["ref_off"][c]["hold_miss"]) <= 1e-9 * s["ref_off"][c]["hold_miss"]


def test_no_scoring_weights_and_the_stored_start(state):
    s, k = state, state["k"]
    assert (s["mod"]["hold_loss"] > 0).all()
    for key in ("hold_loss", "hold_miss"):
        assert (s["mod_no_hold"][key] == 0.0).all() and not np.signbit(s["mod_no_hold"][key]).any(), key
    for key in KEYS:
        if key not in ("hold_loss", "hold_miss"):
            assert s["mod_no_hold"][key].tobytes() == s["mod"][key].tobytes(), key
    # beta0=None: the Newton start is the root the last call left, so a column that met the phi bound takes no step
    met = s["mod"]["phi"] <= C.GLM_PHI_TOL * s["mod"]["sum_omega"] * (1.0 - 1e-12)
    rooted = s["mod"]["flag"] == 0
    assert (met | ~rooted).mean() >= 0.9
    assert (s["mod_from_root"]["steps"][met & rooted] == 0).all()
    assert (s["mod_from_root"]["steps"][~rooted] == 0).all()
    sel = (met & rooted) | ~rooted
    assert s["mod_from_root"]["beta0"][sel].tobytes() == s["mod"]["beta0"][sel].tobytes()
    for key in ("AX", "P", "W", "Z", "loss", "hold_loss", "hold_miss", "sum_omega", "l1", "phi", "flag"):
        assert s["mod_from_root"][key][sel].tobytes() == s["mod"][key][sel].tobytes(), key


def test_model_is_repeatable(state):
    for key in KEYS:
        assert state["mod"][key].tobytes() == state["mod_twice"][key].tobytes(), key


# ---------------------------------------------------------------------------
# 3. the dual sum at its end points
# ---------------------------------------------------------------------------
def test_dual_end_points(state):
    s, inst, k = state, state["inst"], state["k"]
    worst = 0.0
    for c in range(k):
        y, om, p = inst["Y"][c], inst["Om"][c], s["ref"][c]["p"]
        for D, sc in ((s["D1"][c], 1.0), (s["D0"][c], 0.0), (s["Dmix"][c], s["mix"][c])):
            try:
                worst = max(worst, I.check_dual(D, y, om, p, sc))
            except AssertionError as e:
                raise AssertionError((c, inst["kinds"][c]) + tuple(e.args)) from e
    print(f"{s['m']} x {s['n']}, k = {k}: glm_dual, worst error relative to sum om log 2: {worst:.1e}")
    # the end points are there: p = 1 exactly on rows with a weight at s = 1; D = 0 exactly at s = 0
    assert any((s["mod"]["P"][c][inst["Om"][c] > 0] == 1.0).any() for c in I.columns_of(inst, "sat"))
    binary = [c for c in range(k) if inst["kinds"][c]["kind"] != "frac"]
    assert (s["D0"][binary] == 0.0).all()
    assert all(s["D0"][c] > 0.1 * inst["Om"][c].sum() for c in I.columns_of(inst, "frac"))


def test_gap_at_scale_one(state):
    s, inst = state, state["inst"]
    for c in I.columns_of(inst, "sat", "frac", "two"):
        y, om, r = inst["Y"][c], inst["Om"][c], s["ref"][c]
        mu = 1.5 * C.logistic_gap(inst["A"], y, om, s["x"][:, c], 1.0, model=r)["gnorm_inf"]
        ref = C.logistic_gap(inst["A"], y, om, s["x"][:, c], mu, model=r)
        assert ref["scale"] == 1.0 and ref["gap"] >= 0.0
        P = s["mod"]["loss"][c] + mu * s["mod"]["l1"][c]
        assert abs(P - ref["primal"]) <= 1e-9 * ref["primal"]
        assert abs((P - s["D1"][c]) - ref["gap"]) <= 1e-9 * ref["primal"], (c, P - s["D1"][c], ref["gap"])
        assert P - s["D1"][c] >= 0.0


# ---------------------------------------------------------------------------
# 4. the inner reset on a saturated model
# ---------------------------------------------------------------------------
def test_inner_reset_on_a_saturated_model(state):
    """R^ = 4 om o (p - y) + 4 om v (beta_inner - beta0): the inner intercept is the W-weighted mean of Z - A x, which is
    beta0 - phi / sum om v.  Hence the second term of both bounds, computed from the restatement."""
    s, inst, A = state, state["inst"], state["inst"]["A"]
    worst = 0.0
    for c in I.columns_of(inst, "sat", "two"):
        r, om, y = s["ref2"][c], s["Om2"][c], s["Y2"][c]
        shift = r["phi"] / float(om @ r["v"])
        want = 4.0 * om * (r["p"] - y)
        bound = 1e-12 * np.abs(want).max() + 4.0 * (om * r["v"]).max() * shift
        err = np.abs(s["R"][c] - want).max()
        worst = max(worst, err / bound)
        assert err <= bound, (c, inst["kinds"][c], err, bound)
        g = A.T @ want
        gb = 1e-12 * np.abs(g).max() + (np.abs(A).T @ (4.0 * om * r["v"])).max() * shift
        assert np.abs(s["cert"]["g"][c] - g).max() <= gb, (c, inst["kinds"][c], np.abs(s["cert"]["g"][c] - g).max(), gb)
        assert abs(s["cert"]["intercept"][c] - r["beta0"]) <= 1e-9 * max(1.0, abs(r["beta0"])) + shift
    print(f"{s['m']} x {s['n']}, k = {s['k']}: inner reset, worst |R - want| / bound: {worst:.2f}")
    assert (s["cert"]["drift"] == 0.0).all()


# ---------------------------------------------------------------------------
# 5. the drivers
# ---------------------------------------------------------------------------
def test_logistic_path_without_the_intercept():
    A, y, om = I.path_instance()
    out = panel.logistic_path(A, y, n_mus=8, hi=0.9, lo=0.3, GAP_BOUND=I.GAP_BOUND, OUTER_MAX=I.OUTER_MAX,
                              sample_weight=om, fit_intercept=False, device=0)
    assert (out["intercept"] == 0.0).all()
    mm = C.logistic_gap(A, y, om, np.zeros(A.shape[1]), 1.0, intercept=False)["gnorm_inf"]
    assert abs(out["mu_max"] - mm) <= 1e-9 * mm
    I.check_path(A, y, om, out, intercept=False)


def test_a_column_on_bohnings_bound_descends():
    """``_logistic_loop``'s outer step by hand with curvature 1 in every column: wherever the fp32-rounded numpy model of
    the loop lowers P by more than 1e-6 x the null deviance, the device lowers it too."""
    m, n, k = I.BOHNING_SHAPE
    A, Y, Om = I.panel_instance(m, n, k)
    want = I.bohning_reference()
    mu = want["mu"]
    pl = PanelLasso(A.copy(), 1, nrhs=k, device=0)
    pl.set_intercept(True)
    Yd, Omd = dev(Y), dev(Om)
    curv = torch.ones(k, dtype=torch.int32, device="cuda")
    beta0 = torch.zeros(k, dtype=torch.float64, device="cuda")
    pl.set_row_weights(None)
    pl.solver_reset(np.zeros((m, k)), mu, use_graph=False)
    hist = []
    for outer in range(I.BOHNING_OUTER + 1):
        mod = pl.glm_model(Yd, Omd, None, curv, beta0)
        assert (mod["flag"] == 0).all()
        hist.append(mod["loss"] + mu * mod["l1"])
        if outer == I.BOHNING_OUTER:
            break
        assert mod["W"].cpu().numpy().tobytes() == Om.tobytes()
        pl.set_row_weights_device(mod["W"], None)
        pl.solver_reset(mod["Z"].t(), 4.0 * mu, x0=pl.solver_x_device())
        pl.duality_gap(screen=False)
        pl.solver_step(I.BOHNING_ITERS)
    hist = np.array(hist).T                                   # (k, outer + 1)
    drop = -np.diff(want["history"], axis=1)
    qualifies = drop > 1e-6 * want["null"][:, None]
    assert (qualifies.sum(axis=1) >= 4).all()
    assert (np.diff(hist, axis=1)[qualifies] < 0.0).all(), np.diff(hist, axis=1)[qualifies].max()
    assert abs(hist[:, 0] - want["history"][:, 0]).max() <= 1e-9 * want["null"].max()

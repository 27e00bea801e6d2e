"""The two-pass kernels and the certificate at the chunk geometry of the full sizes, at shapes that cost
milliseconds (csrc/bpgl_kernels.h: k_colpass, k_colreduce, k_rowpass, k_rowreduce<1|4|16>, k_shrink,
k_linesearch, fold_parts, k_update; csrc/bpgl_gap.h: k_gap_partials, k_gap_count).

Every other test of these kernels below the full sizes runs them on 16-row chunks: two trips per wave, one row
group, one batch of segments, one grid step (tests/test_twopass_host.py pins that).  ``BPGL_TARGET_BLOCKS``,
read when a context is created, sets the tile target, so a 203-row matrix gets one 208-row chunk.  The cases
live in tests/twopass_reference.py, which also restates the tiling; tests/test_twopass_host.py proves on the
CPU that each geometry below is reached and that the two product checks catch nine indexing mutants.  Every
case here first asserts ``geometry()`` against ``twopass_geometry``: no case falls back to 16-row chunks
unnoticed.

a-c. Products (test_products_at_every_knob_combination): ``diag_ATA``, ``mat_tMulVec_DiffSize`` and
   ``matMulVec_DiffSize`` of every block, at each of the 48 combinations of col_mode 0/1/2, nt_loads 0/1,
   tail_permille 0/120/500/1000 and reverse_rows 0/1; on the exact instance (integers: EQUAL to numpy's int64
   result), on the real one (within 2 gam(terms + nchunk + nseg + 4) sum |a||v|), and bitwise equal across
   the 48 combinations (the kernels' claim: results depend on neither the schedule, the load policy nor the
   row direction).  Long chunks: 203 x 1500 at target 1 (one 208-row chunk: 26/26/26/25 trips of 2 rows, 13 of
   4, last trips of 1, 2 and 3 rows) and at target 6 (ragged last chunk), 211 x 1500 (224 rows: 27/26 trips),
   3 and 2 feature blocks, 17 x 40 (R = 32), 1 x 40 (three waves own no row), 600 x 100 at target 19 (19
   chunks of 32 rows); the three storages each.  Wide rows: 24 x 70016 fp32 (69 segments: k_rowreduce<16>
   with a partial second batch), 24 x 8712 fp64 (18), 24 x 36880 bf16 (19), 40 x 6000 fp32 (6:
   k_rowreduce<4>).  Tall: 131139 x 32 in 2 blocks (2050 groups of 64 rows on 2048 reduce blocks).
d. Solver steps (test_steps_at_these_geometries): the 18-step protocol of tests/test_solver_step.py
   (``run_single_rank``: single steps, then the same run in one graphed call, bitwise equal) with
   ``check_run``'s bounds unchanged: Block 3 and 2 and ``onepass`` 0 on the long chunks for the three storages,
   each col_mode, tail_permille 500 with reverse_rows 1 on three chunks, 19 chunks (k_shrink's unrolled loop
   and its remainder), the wide fp32 shape (1094 shrink partials: fold_parts' unrolled loop), the tall shape
   (k_linesearch folding 2048 partials), and one one-pass case per storage whose refreshes at t = 8 and 16
   go through a multi-trip k_colpass.
e. The certificate (test_certificate_at_the_thresholds): ``duality_gap()`` right after the reset and after
   16 Block iterations on 24 x 70016 (274 screen blocks, a second grid step of k_gap_partials), 24 x 70006 in 2
   blocks (w 35003 padded to 35004) and 131139 x 32, against ``cpu_calculation.duality_gap`` /
   ``gap_safe_keep`` at the bounds of tests/test_gap_screen.py as they stand there.

Worst ratio to bound on the MI355X over the 54 new cases: products -- exact instance equal at every case, real
instance diag 0.076, A^T r 0.034, A d 0.0077, no knob combination differs bitwise; steps -- 0 2.2e-4, A 0.34,
B 0.0045, C 0.28, D 0.022; certificate (E) -- primal, dual, gap, scale and |g|_inf at most 3.4e-7 of their
bounds, g 2.7e-4 of its bound, every mask equal with no borderline entry.  No check is waived and no bound is
scaled.  No device bug showed: every case passed as first run.  The module takes 5 s.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

import solver_step_reference as S  # noqa: E402
import twopass_reference as TP  # noqa: E402
from convex_optimization_amd import _native as N  # noqa: E402
from convex_optimization_amd import cpu_calculation as C  # noqa: E402
from test_solver_step import make_gc, run_single_rank  # noqa: E402

WORST = {}


def note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


def so_far():
    return " ".join(f"{k} {v:.3g}" for k, v in sorted(WORST.items()))


def assert_geometry(gc, geo):
    g = gc.geometry()
    assert (g["nseg"], g["nchunk"], g["rows_per_chunk"], g["seg_width"]) == \
        (geo["nseg"], geo["nchunk"], geo["R"], geo["segw"]), (g, geo)
    assert gc.MAT_WIDTH_PAD == geo["wp"]


@functools.lru_cache(maxsize=2)
def exact_instance(m, n):
    out = TP.exact_instance(m, n, m + n)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=2)
def real_instance(m, n, ty):
    out = TP.real_instance(m, n, ty, m + n)
    for a in out:
        a.setflags(write=False)
    return out


def device_products(gc, r, d):
    """[diag | A^T r | A d] of every block as one device vector (nothing is read back here)"""
    B, W, H = gc.Block, gc.MAT_WIDTH, gc.MAT_HEIGHT
    diag = torch.empty((B, gc.MAT_WIDTH_PAD), dtype=torch.float64, device=gc.device)
    with gc._on_stream():
        N.check(N.lib().bpgl_diag_ata(gc._ctx, N.ptr(diag)), "bpgl_diag_ata")
    tmv = torch.empty((B, W), dtype=torch.float64, device=gc.device)
    mv = torch.empty((B, H), dtype=torch.float64, device=gc.device)
    for q in range(B):
        gc.mat_tMulVec_DiffSize(tmv[q], q, r)
        gc.matMulVec_DiffSize(mv[q], q, d[q * W:(q + 1) * W])
    return torch.cat([diag[:, :W].reshape(-1), tmv.reshape(-1), mv.reshape(-1)])


def split(flat, B, W, H):
    return flat[:B * W].reshape(B, W), flat[B * W:2 * B * W].reshape(B, W), flat[2 * B * W:].reshape(B, H)


def knob_sweep(c, geo, A, r, d):
    """the products at the first knob combination (host) and the combinations that differ from it bitwise"""
    B = c["Block"]
    gc = make_gc(c["ty"], A, B, target=c["target"])
    assert_geometry(gc, geo)
    assert np.array_equal(gc.A_b_gpu.to(torch.float64).cpu().numpy(), np.stack(np.hsplit(A, B)))
    rd, dd = torch.from_numpy(r.copy()).to(gc.device), torch.from_numpy(d.copy()).to(gc.device)
    first, differ = None, []
    for knobs in TP.KNOBS:
        for k, v in zip(TP.KNOB_KEYS, knobs):
            gc.set_tuning(k, v)
        out = device_products(gc, rd, dd)
        if first is None:
            first = out
        else:
            differ.append((out.view(torch.int64) != first.view(torch.int64)).sum())
    differ = torch.stack(differ).cpu().numpy()
    bad = [TP.KNOBS[k + 1] for k in np.flatnonzero(differ)]
    return split(first.cpu().numpy(), B, gc.MAT_WIDTH, gc.MAT_HEIGHT), bad


@pytest.mark.parametrize("c", TP.PRODUCT_CASES, ids=TP.pcase_id)
def test_products_at_every_knob_combination(c):
    m, n, B = c["m"], c["n"], c["Block"]
    geo = TP.pcase_geometry(c)
    names = ("diag", "A^T r", "A d")
    # integers: equal to numpy's int64 products
    A, r, d = exact_instance(m, n)
    got, differ_exact = knob_sweep(c, geo, A, r, d)
    want = TP.reference_products(A, r, d, B, exact=True)
    equal = [np.array_equal(g, w) for g, w in zip(got, want)]
    wrong = {nm: int(np.count_nonzero(g != w)) for nm, g, w in zip(names, got, want)}
    # the recipe of the step tests: within the a-priori bound
    A, r, d = real_instance(m, n, c["ty"])
    got, differ_real = knob_sweep(c, geo, A, r, d)
    want = TP.reference_products(A, r, d, B, exact=False)
    ratios = {nm: TP.worst_ratio(g, w, bd) for nm, g, w, bd in zip(names, got, want, TP.product_bounds(A, r, d, B, geo))}
    for nm, v in ratios.items():
        note("products " + nm, v)
    print(f"products {TP.pcase_id(c)} nseg {geo['nseg']} nchunk {geo['nchunk']} R {geo['R']}: exact instance "
          f"entries that differ {wrong}; real instance worst ratio to bound "
          + " ".join(f"{k} {v:.3g}" for k, v in ratios.items())
          + f"; knob combinations that differ bitwise {len(differ_exact)} + {len(differ_real)} of {len(TP.KNOBS) - 1}")
    print(f"  so far over all cases: {so_far()}")
    assert all(equal) and not any(wrong.values()), wrong
    assert all(v <= 1.0 for v in ratios.values()), ratios
    assert not differ_exact and not differ_real, (differ_exact, differ_real)


@pytest.mark.parametrize("c", TP.STEP_CASES, ids=S.case_id)
def test_steps_at_these_geometries(c):
    geo = TP.twopass_geometry(c["m"], c["n"], c["Block"], c["ty"], c["target"])
    assert c["target"] is None or geo["R"] > 16

    def merge(stats):
        for k in S.TAGS:
            note("steps " + k, stats.get(k, 0.0))

    print(f"steps {S.case_id(c)}: nseg {geo['nseg']} nchunk {geo['nchunk']} R {geo['R']} shrink partials "
          f"{geo['nparts']} reduce blocks {geo['reduce_blocks']}")
    try:
        run_single_rank(c, on_context=lambda gc: assert_geometry(gc, geo), on_report=merge)
    finally:
        print(f"  so far over the cases of this module: {so_far()}")


@functools.lru_cache(maxsize=1)
def gap_instance(m, n, ty):
    out = TP.gap_instance(m, n, ty)
    for a in out[:2]:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("m,n,ty,B", TP.GAP_CASES, ids=[f"{m}x{n}-{ty}-B{B}" for m, n, ty, B in TP.GAP_CASES])
def test_certificate_at_the_thresholds(m, n, ty, B):
    As, b, mu = gap_instance(m, n, ty)
    W = n // B
    geo = TP.twopass_geometry(m, n, B, ty)
    gc = make_gc(ty, As, B)
    assert_geometry(gc, geo)
    assert geo["gap_steps"] >= 2
    gc.solver_reset(b.copy(), mu)
    t = 0
    for stop in (0, 16 * B):
        if stop > t:
            gc.solver_step(stop - t)
        t = stop
        d = gc.duality_gap()
        x = gc.solver_x()
        g_all = d["g_all"].cpu().numpy().reshape(-1)
        keep = d["keep"].cpu().numpy().reshape(-1)
        raw = gc._gap_keep.cpu().numpy()
        assert gc.solver_stat("fallbacks") == 0 and gc.solver_stat("onepass") == int(B == 1)
        ref = C.duality_gap(As, b, x, mu)
        g_ref = As.T @ (As @ x - b)
        keep_ref, score = C.gap_safe_keep(As, b, x, mu, return_score=True)
        ratios = dict(primal=abs(d["primal"] - ref["primal"]) / (1e-9 * abs(ref["primal"])),
                      dual=abs(d["dual"] - ref["dual"]) / (1e-9 * abs(ref["dual"])),
                      gap=abs(d["gap"] - ref["gap"]) / (1e-9 * ref["primal"]),
                      scale=abs(d["scale"] - ref["scale"]) / (1e-9 * ref["scale"]),
                      gnorm=abs(d["gnorm_inf"] - ref["gnorm_inf"]) / (1e-9 * ref["gnorm_inf"]),
                      g=float(np.max(np.abs(g_all - g_ref) / (1e-12 * np.abs(g_ref).max() + 1e-11 * np.abs(g_ref)))))
        clear = np.abs(score - mu) > 1e-9 * mu
        for k, v in ratios.items():
            note("E " + k, v)
        print(f"certificate {m}x{n} {ty} B{B} t={t}: gap blocks {geo['gap_blocks']} x {geo['gap_steps']} steps, screen "
              f"blocks {geo['screen_blocks']}; primal {d['primal']:.17g} ref {ref['primal']:.17g}, gap {d['gap']:.6e} "
              f"ref {ref['gap']:.6e}, n_keep {d['n_keep']} ref {int(keep_ref.sum())}, borderline {int((~clear).sum())}; "
              "ratio to bound " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
        print(f"  so far over the cases of this module: {so_far()}")
        assert abs(d["primal"] - ref["primal"]) <= 1e-9 * abs(ref["primal"])
        assert abs(d["dual"] - ref["dual"]) <= 1e-9 * abs(ref["dual"])
        assert abs(d["gap"] - ref["gap"]) <= 1e-9 * ref["primal"]
        assert abs(d["scale"] - ref["scale"]) <= 1e-9 * ref["scale"]
        assert abs(d["gnorm_inf"] - ref["gnorm_inf"]) <= 1e-9 * ref["gnorm_inf"]
        np.testing.assert_allclose(g_all, g_ref, rtol=1e-11, atol=1e-12 * np.abs(g_ref).max())
        assert (~clear).sum() <= 0.01 * n
        assert np.array_equal(keep[clear], keep_ref[clear])
        assert d["n_keep"] == int(keep.sum())
        assert raw.dtype == np.uint8 and raw.shape[0] == B and raw.shape[1] == geo["wp"]
        assert not raw[:, W:].any() and set(np.unique(raw)) <= {0, 1}
        assert np.array_equal(raw[:, :W].reshape(-1).astype(bool), keep)
        if t == 0 and n > 65536:
            assert 0 < d["n_keep"] < n

"""The per-iteration checker of the fp64 solver (solver_step_reference.check_step) separates right from
wrong, without a GPU.

The "device" here is ``Model``, a numpy restatement of the device's iteration (csrc/bpgl_kernels.h,
bpgl_onepass.h) in its two forms: two-pass (the exact g = A^T r every iteration, any number of blocks) and
one-pass (one block; g carried as G += gamma U, U = A^T s23, an exact refresh every 8 iterations, the next
shrink in the tail).  Both products are summed the way the device partitions them -- s23 in segment-block
partials, U, g and the line search's dot products in row-group partials -- each partial a recursive fp64 sum
in a permuted order that is fixed per seed, the folds in index order; the one-pass s23 partials have their
lowest mantissa bit replaced by the launch parity (``op_stuff``); the residual is r = sum_q Ax_q - b with
Ax += gamma s23; the shrink multiplies by a rounded 1 / d.

* the model's trajectories pass 0 and A-D with ratio <= 1 at every one of 18 iterations, for the three
  storages and several summation orders, and E (test_model_passes, test_model_stops_where_the_reference_does);
* each of the twelve mutants in MUTANTS -- bugs that the trajectory tests cannot see -- is caught by the check
  named beside it, at the iteration where it first acts or the next one (test_mutant_is_caught).  "Acts" is
  decided by the model: the first iteration after which the mutant's state (x, r, the carried G), step size or
  error record differs from the clean model's;
* every case of the MI355X lists is informative (test_steps_are_informative): on the reference's own
  trajectory at least 12 of the 18 steps have gamma > 0 and max_j allow_j / d_j <= 1e-6 max_j |D_j|, so an
  fp32-sized error in g cannot hide inside the allowance; the reference passes its own checker there; and
  each stop case's bound meets E's conditions, ``oracle.run_numpy`` stopping where ``stop_bound`` says.

Worst ratio to bound of the model over test_model_passes and test_model_passes_clipped_steps: 0 0.12, A 0.24,
B 0.036, C 0.70, D 0.73 (C and D at 4 x 900 from a dense start and at 3 x 5, where an m-term sum's allowance
is a handful of roundings); the reference's own trajectories on the MI355X cases (test_steps_are_informative,
every one of them with 18 informative steps of 18): A 0.14, B 0.011, C 0.24.

What the model showed about the checks as the issue states them, each restated in solver_step_reference with
its derivation: without the shrink's own fp64 arithmetic (eps_j) the correct model exceeds C at 3 x 5 (ratio
1.05), so it is counted; several blocks need rr in terms of sum_j |a_ij| |x_j|, since a block's Ax_q is not
bounded by |r| + |b|; a refresh from a stale residual shows in B (gamma = 0 against a descent direction of the
reference) and D, not in C, whose dx = 0 = gamma D.  D holds as stated (the model reaches 0.73 of it).
"""
import functools

import numpy as np
import pytest

import solver_step_reference as S
from oracle import oracle

T = S.T_STEPS


def f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)


def op_stuff(v, bit):
    """csrc/bpgl_onepass.h op_stuff followed by op_unstuff: the lowest mantissa bit replaced, then cleared."""
    del bit   # the reader clears the tag again: whatever the parity, the value loses its lowest bit
    return (np.ascontiguousarray(v, dtype=np.float64).view(np.uint64) & ~np.uint64(1)).view(np.float64)


def seq_sum(P, axis):
    """recursive fp64 summation along ``axis`` in the order given"""
    if P.shape[axis] == 0:
        return np.zeros(np.delete(P.shape, axis))
    return np.take(np.cumsum(P, axis=axis), -1, axis=axis)


class Model:
    """One right-hand side, one block update per ``step``; ``mutant`` names one deliberate bug."""

    def __init__(self, As, b, mu, Block=1, onepass=True, bc=64, ngroups=5, seed=0, order=None, x0=None,
                 err_bound=None, mutant=None):
        self.As, self.b, self.mu, self.Block = As, np.asarray(b, dtype=np.float64), float(mu), Block
        self.m, self.n = As.shape
        self.w = self.n // Block
        self.wp = (self.w // 4 + 1) * 4                       # always at least one padding column
        self.onepass = bool(onepass) and Block == 1
        self.order, self.err_bound, self.mutant = order, err_bound, mutant
        self.diag = np.square(As).sum(axis=0).reshape(Block, self.w)
        self.rec = 1.0 / self.diag
        rs = np.random.RandomState(seed)
        # segment blocks of bc columns, row groups of R rows, each summed in a permuted order of its own
        self.SB = -(-self.w // bc)
        self.seg = [rs.permutation(np.arange(k * bc, min((k + 1) * bc, self.w))) for k in range(self.SB)]
        R = -(-self.m // max(1, min(ngroups, self.m)))
        self.ngroups = -(-self.m // R)
        self.grp = [rs.permutation(np.arange(q * R, min((q + 1) * R, self.m))) for q in range(self.ngroups)]
        self.x = np.zeros((Block, self.w)) if x0 is None else np.array(x0, dtype=np.float64).reshape(Block, self.w)
        self.Ax = np.stack([self.rows_dot(self.block(q), self.x[q], False) for q in range(Block)])
        self.r = self.residual()
        self.r_prev = self.r.copy()
        self.G = np.zeros(self.wp)
        self.s23_prev = np.zeros(self.m)
        self.D = np.zeros(self.w)
        self.parts = []
        self.t, self.done, self.t_last, self.gamma, self.err, self.cnt = 0, False, -1, 0.0, 0.0, 0
        self.err_iter = []

    def block(self, q):
        return self.As[:, q * self.w:(q + 1) * self.w]

    def mb_of(self, t):
        return int(self.order[t]) if self.order is not None else t % self.Block

    def residual(self):
        acc = self.Ax[0].copy()
        for q in range(1, self.Block):
            acc = acc + self.Ax[q]
        return acc - self.b

    def rows_dot(self, Am, v, stuff):
        """A v per row: SB segment-block partials (tagged on the one-pass path), folded in block order"""
        acc = None
        for cols in self.seg:
            p = seq_sum(Am[:, cols] * v[cols], 1)
            if stuff:
                p = op_stuff(p, self.t & 1)
            acc = p if acc is None else acc + p
        return acc

    def cols_partials(self, Am, v, drop_last_row_of=None):
        """the row groups' partials of A^T v, (ngroups, w)"""
        out = []
        for q, rows in enumerate(self.grp):
            if q == drop_last_row_of:
                rows = rows[rows != rows.max()]
            out.append(seq_sum(Am[rows] * v[rows, None], 0))
        return np.array(out)

    def fold(self, P, skip=None):
        acc = np.zeros(P.shape[1:])
        for q in range(P.shape[0]):
            if q != skip:
                acc = acc + P[q]
        return acc

    def shrink(self, mb):
        """D and the 64-column tiles' partials (sum |Bx|, sum |x|, max err) from G"""
        g, x = self.G[:self.w], self.x[mb]
        dsel = (mb + 1) % self.Block if self.mutant == "wrong_block_diag" else mb
        rx = self.diag[dsel] * x - g
        bx = self.rec[dsel] * S.soft_thr(rx, self.mu)
        self.D = bx - x
        e = np.abs(g - np.clip(g - x, -self.mu, self.mu))
        self.parts = [(np.abs(bx[j:j + 64]).sum(), np.abs(x[j:j + 64]).sum(), e[j:j + 64].max())
                      for j in range(0, self.w, 64)]

    def state(self):
        return self.x.copy(), self.r.copy(), self.G.copy(), self.gamma, self.err

    def step(self):
        if self.done:
            return
        t, mut = self.t, self.mutant
        mb = self.mb_of(t)
        Am = self.block(mb)
        if not self.onepass or t % S.REFRESH == 0:
            src = self.r_prev if (mut == "refresh_from_old_r" and t > 0) else self.r
            self.G[:self.w] = self.fold(self.cols_partials(Am, src))
            self.shrink(mb)
        D = self.D
        s23 = self.rows_dot(Am, D, self.onepass)
        if mut == "stale_s23_row" and t > 0:
            s23[self.m // 2] = self.s23_prev[self.m // 2]
        self.s23_prev = s23.copy()
        rs = sum(seq_sum(self.r[rows] * s23[rows], 0) for rows in self.grp)
        ss = sum(seq_sum(s23[rows] * s23[rows], 0) for rows in self.grp)
        parts = self.parts[:-1] if (mut == "linesearch_drops_last_partial" and len(self.parts) > 1) else self.parts
        a, bsum = sum(p[0] for p in parts), sum(p[1] for p in parts)
        eparts = self.parts[:-1] if (mut == "err_skips_last_tile" and len(self.parts) > 1) else self.parts
        err = max(p[2] for p in eparts)
        if mut == "err_counts_padding":
            gpad = 1.5 * self.mu                               # a padding column's G, x = 0 there
            err = max(err, abs(gpad - np.clip(gpad, -self.mu, self.mu)))
        r1 = rs + self.mu * (a - bsum)
        gamma = 0.0 if ss == 0.0 else -r1 / ss
        gamma = max(gamma, 0.0) if mut == "gamma_not_clipped_at_1" else min(max(gamma, 0.0), 1.0)
        self.err, self.t_last = float(err), t
        self.err_iter.append(float(err))
        if self.err_bound is not None:
            self.cnt += err < self.err_bound
            if mb == self.Block - 1:
                if self.cnt == self.Block:
                    self.done, self.gamma = True, 0.0
                    return
                self.cnt = 0
        self.gamma = float(gamma)
        self.r_prev = self.r.copy()
        rows = self.m - self.m % 256 if mut == "residual_skips_tail_rows" else self.m
        self.Ax[mb][:rows] = self.Ax[mb][:rows] + gamma * s23[:rows]
        self.r[:rows] = self.residual()[:rows]
        cols = self.w - 1 if mut == "x_update_misses_a_column" else self.w
        self.x[mb][:cols] = self.x[mb][:cols] + gamma * D[:cols]
        if self.onepass:
            P = self.cols_partials(Am, s23, drop_last_row_of=1 if mut == "U_omits_a_row" else None)
            self.G[:self.w] = self.G[:self.w] + gamma * self.fold(P, skip=2 if mut == "U_partial_left_out" else None)
            if mut == "g_rounded_to_fp32":
                self.G = f32(self.G)
            self.shrink(mb)                                    # the next iteration's, from the carried G
        self.t = t + 1


def run_model(model, iters=T):
    """(snaps, gammas, errs, states): 18 single iterations with a snapshot after each"""
    snaps, gammas, errs, states = [(model.x.reshape(-1).copy(), model.r.copy())], [], [], []
    for _ in range(iters):
        model.step()
        snaps.append((model.x.reshape(-1).copy(), model.r.copy()))
        gammas.append(model.gamma)
        errs.append(model.err)
        states.append(model.state())
    return snaps, gammas, errs, states


def check_model(model, snaps, gammas, errs, x0=None, t_stop=None, stats=None):
    return S.check_run(model.As, model.b, model.diag, model.mu, model.Block, snaps, gammas, errs, model.onepass,
                       order=model.order, x0=x0, parts=model.SB, ngroups=model.ngroups, t_stop=t_stop, stats=stats)


@functools.lru_cache(maxsize=None)
def small(m, n, ty, seed=None):
    out = S.instance(m, n, ty, m + n if seed is None else seed)
    out[0].setflags(write=False)
    return out


# (m, n, Block, onepass): tiny, several blocks with padding, ragged segment blocks, fewer rows than groups
MODEL_SHAPES = [(3, 5, 1, True), (3, 5, 1, False), (77, 120, 3, False), (129, 1002, 2, False), (300, 700, 1, True),
                (300, 700, 1, False), (4, 900, 1, True), (517, 333, 1, True)]
WORST = {}


def test_bf16_rounding_is_torch_s():
    torch = pytest.importorskip("torch")
    A = np.random.RandomState(0).randn(64, 96) / 7.0
    t = torch.from_numpy(np.ascontiguousarray(A, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()
    assert np.array_equal(S.stored(A, "bf16"), t)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("ty", ["float", "double", "bf16"])
@pytest.mark.parametrize("m,n,Block,onepass", MODEL_SHAPES)
def test_model_passes(m, n, Block, onepass, ty, seed):
    As, b, mu = small(m, n, ty)
    x0 = np.random.RandomState(seed).randn(n) if seed == 2 else None
    order = np.random.RandomState(seed).randint(0, Block, size=T) if (seed == 1 and Block > 1) else None
    model = Model(As, b, mu, Block, onepass, seed=seed, order=order, x0=x0)
    snaps, gammas, errs, _ = run_model(model)
    stats = {}
    bad = check_model(model, snaps, gammas, errs, x0=x0, stats=stats)
    for c in S.TAGS:
        WORST[c] = max(WORST.get(c, 0.0), stats.get(c, 0.0))
    print(f"model {(m, n, Block, onepass, ty, seed)}: {S.line(stats)}; so far {S.line(WORST)}")
    assert not bad, bad
    assert all(stats[c] <= 1.0 for c in S.TAGS)


@pytest.mark.parametrize("onepass", [True, False])
def test_model_passes_clipped_steps(onepass):
    """an instance whose unclipped step size exceeds 1 (nearly orthogonal columns): B's gamma = 1 branch"""
    As, b, mu = small(300, 8, "double", 5)
    model = Model(As, b, mu, 1, onepass)
    snaps, gammas, errs, _ = run_model(model)
    assert gammas.count(1.0) >= 3
    stats = {}
    bad = check_model(model, snaps, gammas, errs, stats=stats)
    print(f"clipped steps, onepass {onepass}: {gammas.count(1.0)} of {T} at gamma = 1, {S.line(stats)}")
    assert not bad, bad


# (mutant, the check expected to catch it, (m, n, type, Block, onepass), instance seed)
MUTANTS = [
    ("U_omits_a_row", "C", (300, 700, "float", 1, True), None),
    ("stale_s23_row", "A", (300, 700, "double", 1, True), None),
    ("U_partial_left_out", "C", (300, 700, "bf16", 1, True), None),
    ("residual_skips_tail_rows", "A", (300, 700, "float", 1, True), None),
    ("refresh_from_old_r", "D", (300, 700, "float", 1, True), None),
    ("g_rounded_to_fp32", "C", (517, 333, "double", 1, True), None),
    ("gamma_not_clipped_at_1", "B", (300, 8, "double", 1, False), 5),
    ("linesearch_drops_last_partial", "B", (300, 700, "float", 1, True), None),
    ("err_skips_last_tile", "D", (300, 100, "float", 1, True), None),
    ("err_counts_padding", "D", (300, 700, "float", 1, True), None),
    ("x_update_misses_a_column", "C", (300, 700, "bf16", 1, True), None),
    ("wrong_block_diag", "C", (77, 120, "float", 3, False), None),
]


@pytest.mark.parametrize("mutant,expected,shape,seed", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutant_is_caught(mutant, expected, shape, seed):
    m, n, ty, Block, onepass = shape
    As, b, mu = small(m, n, ty, seed)
    clean = run_model(Model(As, b, mu, Block, onepass))
    model = Model(As, b, mu, Block, onepass, mutant=mutant)
    snaps, gammas, errs, states = run_model(model)
    differs = [t for t in range(T) if any(np.asarray(u).tobytes() != np.asarray(v).tobytes()
                                          for u, v in zip(states[t], clean[3][t]))]
    assert differs, "the mutant never acts on this instance"
    t_act = differs[0]
    bad = check_model(model, snaps, gammas, errs)
    assert bad, "not caught"
    t_first = bad[0][0]
    tags = {v[0] for t, v in bad if t == t_first}
    print(f"{mutant}: acts at t = {t_act}, caught at t = {t_first} by {sorted(tags)}: {bad[0][1]}")
    assert t_act <= t_first <= t_act + 1, (t_act, bad[:4])
    assert expected in tags, (expected, bad[:4])


# -------------------------------------------------------------------------------------------------
# conditions on the inputs of the MI355X run (tests/test_solver_step.py), on the reference alone
# -------------------------------------------------------------------------------------------------
def problem_key(c):
    return (c["m"], c["n"], c["ty"], c["Block"], c["order_seed"], c["x0_seed"], S.case_carried(c),
            c["fail_at"], c["world"])


UNIQUE = list({problem_key(c): c for c in S.ALL_CASES}.values())
REF_WORST = {}


@pytest.mark.parametrize("c", UNIQUE, ids=S.case_id)
def test_steps_are_informative(c):
    As, b, mu, order, x0 = S.case_problem(c)
    snaps, gammas, errs = S.reference_run(As, b, mu, c["Block"], T, order=order, x0=x0)
    diag = np.square(As).sum(axis=0)
    stats = {}
    carried = S.case_carried(c)
    SB, ng, _, _ = S.onepass_geometry(c["m"], c["n"] // c["Block"], c["ty"], 256)
    bad = S.check_run(As, b, diag, mu, c["Block"], snaps, gammas, errs, carried, order=order, x0=x0, parts=SB,
                      ngroups=ng * c["world"] + c["world"], nranks=c["world"], exact_from=c["fail_at"], stats=stats)
    good = sum(1 for ga, a, dmax in stats["steps"] if ga > 0.0 and a <= 1e-6 * dmax)
    for k in S.TAGS:
        REF_WORST[k] = max(REF_WORST.get(k, 0.0), stats.get(k, 0.0))
    print(f"{S.case_id(c)}: {good} informative steps of {T}; reference against its own checker {S.line(stats)}; "
          f"so far {S.line(REF_WORST)}")
    assert not bad, bad
    assert S.informative(stats), stats["steps"]


STOPS = list({problem_key(c): c for c in S.STOP_CASES}.values())


@pytest.mark.parametrize("c", STOPS, ids=S.case_id)
def test_stop_bounds_meet_their_conditions(c):
    As, b, mu, order, x0 = S.case_problem(c)
    _, _, errs = S.reference_run(As, b, mu, c["Block"], T, order=order, x0=x0)
    picked = S.stop_bound(errs, c["Block"], order)
    assert picked is not None, errs
    bound, t_stop = picked
    assert 10 <= t_stop <= 17
    ref = oracle.run_numpy(As, b, mu, c["Block"], T, order=order, err_bound=bound)
    assert ref["t_last"] == t_stop
    ratio = ref["err_iter"][:t_stop + 1] / bound
    assert not np.any((ratio > 1.0 - 1e-3) & (ratio < 1.0 + 1e-3)), ratio
    np.testing.assert_allclose(ref["err_iter"][:t_stop + 1], errs[:t_stop + 1], rtol=1e-9)
    print(f"{S.case_id(c)}: err_bound {bound:.6g} stops the reference at t = {t_stop}; err / bound there "
          f"{ratio[t_stop]:.4f}, smallest before {ratio[:t_stop].min():.4f}")


@pytest.mark.parametrize("m,n,ty,Block,onepass", [(300, 700, "float", 1, True), (77, 120, "double", 3, False)])
def test_model_stops_where_the_reference_does(m, n, ty, Block, onepass):
    As, b, mu = small(m, n, ty)
    _, _, ref_errs = S.reference_run(As, b, mu, Block, T)
    bound, t_stop = S.stop_bound(ref_errs, Block)
    model = Model(As, b, mu, Block, onepass, err_bound=bound)
    snaps, gammas, errs, _ = run_model(model)
    assert model.done and model.t_last == t_stop and len(model.err_iter) == t_stop + 1
    bad = check_model(model, snaps, gammas, errs, t_stop=t_stop)     # the record up to t_stop, frozen after it
    assert not bad, bad

"""The per-iteration checker (panel_step_reference.check_step) separates right from wrong, without a GPU.

The "device" here is ``Model``, a numpy restatement of one panel iteration (csrc/bpgl_panel.h) that rounds
its operands where the device does and nowhere else: R -> hi + lo bf16 and g -> fp32 on an exact
iteration; the carried recurrence G += A^T bf16(V), V = gamma S + E, E = V - bf16(V) exactly as
panel_put_carry has it; D -> bf16 or hi + lo; S in fp32 per pass-2 column chunk; x -> fp32; fp64 elsewhere.

* the model's own trajectories pass A-D at each of 18 checkpoints of every case (test_model_passes);
* each of eleven mutants of the model -- bugs of the kind the trajectory tests cannot see -- gives at least
  one violation at every checkpoint where it acts (test_mutant_is_caught).  A mutant bends the single step
  from the clean trajectory's state at t, so each checkpoint sees it afresh; "acts" is decided by the model
  (``Model.step``): the mutated step size differs from the clean one, the dropped stage held a nonzero
  direction, and so on.  The dropped error feedback runs for a whole refresh period and counts from q >= 4 on,
  once the feedback dropped so far exceeds, on a coordinate that moves, the carried allowance that
  check_step must grant a correct run (below that it is rounding by the checker's own definition);
* the instance is informative: on the unrounded iteration the median over the right-hand sides of
  |dx|_2 / |x_{t+1}|_2 stays >= 1e-3 at every checkpoint (test_steps_are_informative; measured 1.2e-3 to
  3.1e-2 at the worst checkpoint of each shape; the 1024 x 512 shapes through t = 9 only, see there).

Measured here, worst over all cases and checkpoints of test_model_passes, ratio to bound: A 0.25, B 0.098,
C 0.987 (the bf16 image's own rounding, 2^-8, has no margin in C), D 0.28.  The model's gradient noise on
exact iterations (R -> hi + lo, g -> fp32) stays within 1.84 sigma_j (14 instances x 2 d_split x 18
iterations), against the allowance's C_g = 8.

What the model showed about the checks as first stated, each restated in panel_step_reference with its
derivation: a least-squares gamma^ is off by up to 2^-8 gamma with the bf16 direction, which breaks
gamma^ <= 1 + 1e-6, the clipped / unclipped split of B and B itself on coordinates shrunk to zero (ratio 11
on the correct model) -- hence ``gamma_interval``; dx == 0 does not make dR zero near convergence (the model
reaches it at t = 30 on 1024 x 512, k = 128); the carried allowance needs the refresh's own error.
"""
import functools

import numpy as np
import pytest

import panel_step_reference as P

T_STEPS = 18
G_REFRESH = 8


def auto_kchunks(m, w):
    """bpgl_panel_create's default split of a block's columns over pass-2 chunks"""
    kc = max(1, min(w // 128, 256 // (m // 256)))
    while kc > 1 and w % (kc * 128):
        kc -= 1
    return kc


class Model:
    """k right-hand sides, one block update per ``step``; ``mutant`` names one deliberate bug."""

    def __init__(self, Ab, B, mu, Block, d_split, carry, W=None, rounding=True, mutant=None):
        self.Ab, self.mu, self.Block, self.d_split = Ab, np.asarray(mu, dtype=np.float64), Block, d_split
        self.m, self.n = Ab.shape
        self.k = B.shape[1]
        self.w = self.n // Block
        self.carry = bool(carry) and Block == 1
        self.Wk = np.ones((self.k, self.m), dtype=bool) if W is None else (np.asarray(W).T != 0)
        self.diag = np.square(Ab).sum(axis=0).reshape(Block, self.w)    # the full column norms, masked or not
        self.kchunks = auto_kchunks(self.m, self.w)
        self.chain = d_split * (self.w // self.kchunks)
        self.rounding, self.mutant = rounding, mutant
        self.x = np.zeros((self.n, self.k))
        self.R = np.where(self.Wk, -B.T, 0.0)
        self.t = 0
        self.Gc = self.E = self.Vh = None
        self.gamma_prev = np.zeros(self.k)
        self.noise_over_sigma = 0.0

    def rnd(self, f, v):
        return f(v) if self.rounding else np.asarray(v, dtype=np.float64)

    def direction_image(self, D):
        if not self.rounding:
            return D
        if self.d_split == 1:
            return P.bf16(D)
        hi, lo = P.split_bf16(D)
        return hi + lo

    def step(self):
        """One iteration; returns (err, acted): ``acted`` is False where the mutant provably changed nothing."""
        mut, mb = self.mutant, self.t % self.Block
        sl = slice(mb * self.w, (mb + 1) * self.w)
        Am = self.Ab[:, sl]
        exact = not self.carry or self.t % G_REFRESH == 0
        acted = mut is not None
        if exact:
            op = self.R
            if self.rounding:
                hi, lo = P.split_bf16(self.R)
                op = hi + lo
        else:
            op = self.Vh
        if mut == "stage_g":                      # one 64-row stage missing from the A^T product
            op = op.copy()
            op[:, 64:128] = 0.0
        prod = self.rnd(P.f32, Am.T @ op.T)       # (w, k), the fp32 accumulators
        g = prod if exact else self.rnd(P.f32, self.Gc + prod)
        if exact and mut is None and self.rounding:
            sigma = 2.0 ** -17 * np.sqrt(np.square(Am).T @ np.square(self.R).T)
            self.noise_over_sigma = max(self.noise_over_sigma, float(np.max(np.abs(g - Am.T @ self.R.T) / sigma)))
        if self.carry:
            self.Gc = g
        if mut == "tile_g":                       # one 256-column tile of g zeroed
            g = g.copy()
            g[:256] = 0.0
        xb = self.x[sl]
        xb0, R_in = xb.copy(), self.R
        d = self.diag[(mb + 1) % self.Block if mut == "d_block" else mb][:, None]
        mu_s = np.roll(self.mu, -1) if mut == "mu_shrink" else self.mu
        D = P.soft_thr(d * xb - g, mu_s) / d - xb
        Dp = self.direction_image(D)
        err = float(np.max(np.abs(g - np.clip(g - xb, -self.mu, self.mu))))
        Ds = Dp
        if mut == "stage_s":                      # one 64-column stage missing from S
            Ds = Dp.copy()
            Ds[64:128] = 0.0
            acted = bool(np.any(Dp[64:128] != 0.0))
        kc = self.w // self.kchunks
        S = sum(self.rnd(P.f32, Am[:, c * kc:(c + 1) * kc] @ Ds[c * kc:(c + 1) * kc]) for c in range(self.kchunks)).T
        if mut != "mask_s":                       # mutant: a masked row's S not zeroed
            S = np.where(self.Wk, S, 0.0)
        rs, ss = np.einsum("km,km->k", self.R, S), np.einsum("km,km->k", S, S)
        l1 = lambda v: np.abs(v).sum(axis=0)      # noqa: E731

        def line_search(mu, Dl):
            r1 = rs + mu * (l1(xb + Dl) - l1(xb))
            return np.where(ss == 0.0, 0.0, np.clip(-r1 / np.where(ss == 0.0, 1.0, ss), 0.0, 1.0))

        clean = line_search(self.mu, Dp)
        gamma = line_search(np.roll(self.mu, -1) if mut == "mu_ls" else self.mu, D if mut == "ls_unrounded" else Dp)
        gamma_x = self.gamma_prev if mut == "gamma_prev" else gamma
        if mut in ("mu_ls", "ls_unrounded"):
            acted = bool(np.any(gamma != clean))
        if mut == "gamma_prev":
            acted = bool(np.any((gamma_x != gamma) & Dp.any(axis=0)))
        self.x[sl] = self.rnd(P.f32, xb + gamma_x * Dp)
        self.R = self.R + gamma[:, None] * S
        if self.carry:
            V = gamma[:, None] * S + (0.0 if exact or mut == "drop_e" else self.E)
            self.Vh = self.rnd(P.bf16, V)
            self.E = self.rnd(P.f32, V - self.Vh)
        if mut == "drop_e":
            # checked at q >= 4, where the feedback dropped so far has grown past what check_step must admit
            # as the rounding of a correct run (its carried allowance) on a coordinate that moves
            q = self.t % G_REFRESH
            if not exact:
                A2 = np.square(Am)
                admit = P.C_G * (2.0 ** -9 * np.sqrt(A2.T @ np.square(self.dR_last).T) + q * P.U24 * np.abs(g)
                                 + 2.0 ** -17 * np.sqrt(A2.T @ np.square(self.R_ref).T))
                moves = (xb0 != 0.0) | (np.abs(g) > self.mu)
                acted = q >= 4 and bool(np.any(moves & (np.abs(Am.T @ self.E_acc.T) > admit)))
            else:
                acted = False
            if exact:
                self.R_ref = R_in
            self.E_acc = (0.0 if exact else self.E_acc) + self.E
            self.dR_last = gamma[:, None] * S
        if mut == "err_after":                    # the criterion on the wrong x: after the update
            xb, g = self.x[sl], Am.T @ self.R.T
            err = float(np.max(np.abs(g - np.clip(g - xb, -self.mu, self.mu))))
        self.gamma_prev = gamma
        self.t += 1
        return err, acted

    def snap(self):
        return self.x.copy(), self.R.copy()

    def clone(self, mutant):
        """A copy of the state (the arrays are never written in place, x excepted) with ``mutant`` switched on."""
        import copy
        c = copy.copy(self)
        c.x, c.mutant = self.x.copy(), mutant
        return c


@functools.lru_cache(maxsize=None)
def problem(m, n, k, masked):
    Ab, B, mu = P.instance(m, n, k, seed=m + n + k)
    W = P.fold_mask(m, k) if masked else None
    for a in (Ab, B, mu) + ((W,) if masked else ()):
        a.setflags(write=False)
    return Ab, B, mu, W


PERSISTENT = ("drop_e",)    # mutants that need several iterations to show; the others act on one step


def run_checked(m, n, Block, k, masked, d_split, carry, mutant=None, stats=None):
    """18 steps of the model, check_step at each; per checkpoint (violations, acted).  A mutant is applied
    to the single step from the clean trajectory's state at t (so every checkpoint sees it on a state the
    bug has not yet bent), the PERSISTENT ones to the whole run."""
    Ab, B, mu, W = problem(m, n, k, masked)
    mod = Model(Ab, B, mu, Block, d_split, carry, W=W, mutant=mutant if mutant in PERSISTENT else None)
    out, snaps = [], [mod.snap()]
    for t in range(T_STEPS):
        if mutant is not None and mutant not in PERSISTENT:
            bent = mod.clone(mutant)
            err, acted = bent.step()
            after = bent.snap()
            mod.step()
        else:
            err, acted = mod.step()
            after = mod.snap()
        snaps.append(mod.snap())
        q = t % G_REFRESH if mod.carry else 0
        exact = not mod.carry or q == 0
        viol = P.check_step(Ab, mod.diag, mu, W, t % Block, snaps[t], after, err, d_split, exact,
                            None if exact else snaps[t][1] - snaps[t - 1][1], chain=mod.chain, q=q,
                            R_ref=None if exact else snaps[t - q][1], stats=stats)
        out.append((viol, acted))
    if stats is not None:
        stats["noise"] = max(stats.get("noise", 0.0), mod.noise_over_sigma)
    return out


# (m, n, Block, k, masked): the shapes of tests/test_panel_step.py
CASES = [(256, 512, 1, 16, False), (256, 512, 1, 32, False), (256, 512, 1, 64, False), (256, 256, 1, 128, False),
         (256, 512, 1, 128, False), (1024, 512, 1, 16, False), (1024, 512, 1, 128, False), (256, 1024, 2, 16, False),
         (256, 768, 3, 64, False), (256, 512, 1, 16, True), (1024, 512, 1, 16, True),
         (1024, 1024, 1, 16, False), (1024, 2048, 1, 128, False), (1024, 1024, 1, 16, True)]


def test_bf16_helpers_match_torch_and_the_device_split():
    """Round to nearest even, ties included, as torch's CPU bfloat16 (and the compiler's float -> __bf16)."""
    torch = pytest.importorskip("torch")
    rs = np.random.RandomState(0)
    v = np.concatenate([rs.randn(4096) * np.exp(rs.uniform(-30, 30, 4096)), [0.0, -0.0, 1.0, 1.00390625, 1.01171875,
                        -1.00390625, 3.0 * 2.0 ** -130, 2.0 ** -126]])
    ref = torch.from_numpy(v.astype(np.float32)).to(torch.bfloat16).to(torch.float64).numpy()
    np.testing.assert_array_equal(P.bf16(v), ref)
    assert P.bf16(1.00390625) == 1.0 and P.bf16(1.01171875) == 1.015625     # ties go to the even mantissa
    hi, lo = P.split_bf16(v)
    np.testing.assert_array_equal(hi, ref)
    np.testing.assert_array_equal(lo, torch.from_numpy((v - hi).astype(np.float32)).to(torch.bfloat16)
                                  .to(torch.float64).numpy())
    big = np.abs(v) > 2.0 ** -100
    assert np.all(np.abs(v - hi - lo)[big] <= 2.0 ** -16 * np.abs(v)[big])


@pytest.mark.parametrize("m,n,Block,k,masked,d_split,carry",
                         [c + (ds, cg) for c in CASES for ds in (1, 2) for cg in ((1, 0) if c[2] == 1 else (0,))])
def test_model_passes(m, n, Block, k, masked, d_split, carry):
    stats = {}
    res = run_checked(m, n, Block, k, masked, d_split, carry, stats=stats)
    print(f"model {m}x{n} B={Block} k={k} masked={masked} d_split={d_split} carry={carry}: worst ratio to bound "
          + " ".join(f"{key} {stats[key]:.3g}" for key in "ABCD")
          + f", gradient noise / sigma {stats['noise']:.3g}, gamma^ in [{stats['gamma_min']:.3g}, "
          f"{stats['gamma_max']:.3g}] +- {stats['dgamma']:.2g}")
    for t, (viol, _) in enumerate(res):
        assert not viol, (t, viol)
    assert stats["noise"] <= P.C_G


# mutant -> the cases (m, n, Block, k, masked, d_split, carry) it runs on
ONE = [(256, 512, 1, 16, False, 1, 1), (256, 512, 1, 16, False, 2, 0), (1024, 2048, 1, 128, False, 1, 1)]
MULTI = [(256, 1024, 2, 16, False, 1, 0), (256, 768, 3, 64, False, 2, 0)]
MUTANTS = {
    "mu_shrink": ONE + MULTI,
    "mu_ls": ONE + MULTI,
    "gamma_prev": ONE + MULTI,
    "tile_g": ONE + MULTI,
    "stage_g": ONE + MULTI,
    "stage_s": ONE + MULTI,
    "drop_e": [(256, 512, 1, 16, False, 1, 1), (256, 512, 1, 16, False, 2, 1), (1024, 2048, 1, 128, False, 1, 1)],
    "ls_unrounded": [(256, 512, 1, 16, False, 1, 1), (256, 512, 1, 16, False, 1, 0), (256, 1024, 2, 16, False, 1, 0)],
    "err_after": ONE + MULTI,
    "d_block": MULTI,
    "mask_s": [(256, 512, 1, 16, True, 1, 1), (1024, 512, 1, 16, True, 2, 0)],
}


@pytest.mark.parametrize("mutant,case", [(mu, c) for mu, cs in MUTANTS.items() for c in cs])
def test_mutant_is_caught(mutant, case):
    res = run_checked(*case, mutant=mutant)
    acted = [t for t, (_, a) in enumerate(res) if a]
    missed = [t for t, (viol, a) in enumerate(res) if a and not viol]
    print(f"{mutant} {case}: acts at {len(acted)} checkpoints, missed at {missed}")
    assert acted, "the mutant never acted: the case does not exercise it"
    assert not missed


# The 1024 x 512 shapes (the smallest at which the fused reduce + update runs) are overdetermined and
# converge about three times faster than the others: the condition holds there through t = 9 (the first
# iteration, the carried ones, the refresh at t = 8 and the first carried one after it).  The 1024 x 1024
# and 1024 x 2048 shapes carry the same kernels through t = 17.
INFORMATIVE_STEPS = {(1024, 512): 10}


@pytest.mark.parametrize("m,n,Block,k,masked", CASES)
def test_steps_are_informative(m, n, Block, k, masked):
    """A condition on the instance, not a measurement of the device: on the unrounded iteration every
    checkpoint still moves x by >= 1e-3 of its norm in the median right-hand side, so that a wrong step
    is large against the allowances."""
    Ab, B, mu, W = problem(m, n, k, masked)
    mod = Model(Ab, B, mu, Block, 2, 0, W=W, rounding=False)
    worst = np.inf
    for t in range(INFORMATIVE_STEPS.get((m, n), T_STEPS)):
        x0 = mod.x.copy()
        mod.step()
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.linalg.norm(mod.x - x0, axis=0) / np.linalg.norm(mod.x, axis=0)
        worst = min(worst, float(np.median(rel)))
        assert np.median(rel) >= 1e-3, (t, float(np.median(rel)))
    print(f"informativeness {m}x{n} B={Block} k={k} masked={masked}: min over t of the median |dx|/|x| = {worst:.3g}")

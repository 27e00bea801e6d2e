#!/usr/bin/env python
"""Cost of the panel's penalty factors.

At the configs[4] shape by default (8192 x 65536 bf16, k = 128, one feature block, `device_instance`;
mu = mu_max * geomspace(0.9, 0.1, 128) with mu_max taken with the factors on; p_j = exp(u_j), u uniform in
[-1, 1], seed 0): ms per iteration of ONE context with the factors off, all ones (the PF kernels on the same
iterates bit for bit) and on, each without and with x >= 0,
alternating `--rounds` times: per run set_penalty_factors / set_positive, a reset with hipGraph replay, 64
untimed iterations, then `--windows` windows of `--iters` iterations each (host clock, synchronised at both
ends), of which the median is the run's figure, then `--kernel-iters` eager iterations with HIP events around every
kernel (the average per kernel kind: where a difference sits).
Writes profiles/panel_penalty.json and prints it.  Reads nothing from the oracle or the reference.

    python tools/panel_penalty_time.py [--m 8192 --n 65536 --k 128 --iters 400 --windows 5 --rounds 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--den", type=float, default=0.4)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--kernel-iters", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panel_penalty.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from convex_optimization_amd import panel
    from convex_optimization_amd.cpu_calculation import mu_grid
    from convex_optimization_amd.parameters import device_instance

    if not torch.cuda.is_available():
        raise SystemExit("panel_penalty_time.py needs a GPU: there is no other path")
    torch.cuda.set_device(0)
    gc, b, _, _ = device_instance(args.m, args.n, args.den, 1, TYPE="bf16", seed=0, device=0)
    A = gc._A_dev
    assert A.dim() == 2 and A.dtype == torch.bfloat16
    k = args.k
    B = b.reshape(-1, 1).expand(args.m, k)
    pen = np.exp(np.random.RandomState(0).uniform(-1.0, 1.0, args.n))
    pl = panel.PanelLasso(A, 1, nrhs=k, device=0)
    pl.set_penalty_factors(pen)
    pl.solver_reset(B, 1.0)
    mu_max = float(pl.duality_gap(screen=False)["gnorm_inf"][0])
    mus = mu_grid(mu_max, k)

    def run(fac, positive):
        pl.set_positive(positive)
        pl.set_penalty_factors(fac)
        pl.solver_reset(B, mus)
        pl.solver_step(64)
        wins = []
        for _ in range(args.windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pl.solver_step(args.iters)
            torch.cuda.synchronize()
            wins.append(1e3 * (time.perf_counter() - t0) / args.iters)
        pl.set_kernel_timing(True)                       # eager, HIP events around every kernel: where a difference sits
        pl.solver_step(args.kernel_iters)
        kms, _ = pl.kernel_times()
        pl.set_kernel_timing(False)
        return statistics.median(wins), wins, kms

    # "ones": the PF kernels on the feature-off problem (bitwise the same iterates: the kernels' own cost); "on": the
    # weighted problem, whose iterates -- and with them the X tiles that pass 1 skips -- differ
    ones = np.ones(args.n)
    forms = (("off", None, False), ("ones", ones, False), ("on", pen, False),
             ("off_positive", None, True), ("ones_positive", ones, True), ("on_positive", pen, True))
    for _, on, pos in forms:                              # untimed
        run(on, pos)
    res = {name: [] for name, _, _ in forms}
    for _ in range(args.rounds):                         # alternate the forms
        for name, on, pos in forms:
            med, wins, kms = run(on, pos)
            res[name].append(dict(ms_median=med, ms_windows=wins, kernel_ms=kms))
    out = dict(shape=dict(m=args.m, n=args.n, k=k, block=1), device=torch.cuda.get_device_name(0), mu_max=mu_max,
               iters_per_window=args.iters, windows=args.windows, fuse_update=int(pl.get_tuning("fuse_update")),
               d_split=int(pl.get_tuning("d_split")), carry_g=int(pl.get_tuning("carry_g")), iteration_ms=res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

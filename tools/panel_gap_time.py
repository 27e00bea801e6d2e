#!/usr/bin/env python
"""Cost of the panel certificate, and a regularization path as one panel against the single-RHS run.

At the configs[4] shape by default (8192 x 65536 bf16, k = 128, one feature block, `device_instance`):
  gap       : after 64 iterations, one untimed PanelLasso.duality_gap() and five timed ones (host
              clock around the call, which ends in a synchronise), with the two products' device
              times (stats gap_prod1_ns / gap_prod2_ns);
  iteration : 256 iterations of the same context (host clock, synchronised at both ends);
  ratio and the smallest multiple of 64 iterations at which one certificate costs at most 10 % of
  that many iterations;
  path      : panel.lasso_path with 128 mu (mu_max * geomspace(0.9, 0.1)) to the gap bound, one
              untimed run and `--repeats` timed ones (the wall clock includes building the context:
              bind, the tiled copies of A, graph capture);
  single    : the single-RHS bf16 device loop with a duality_gap() every 64 iterations
              (ClassLassoScreened, shrink = 0: ClassLassoDevice's loop bit for bit) to the same bound
              for the smallest mu of that grid -- the slowest one.
Writes profiles/panel_gap.json and prints it.  Reads nothing from the oracle or the reference.

    python tools/panel_gap_time.py [--m 8192 --n 65536 --k 128 --gap 1e-4 --repeats 3]
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--den", type=float, default=0.4)
    ap.add_argument("--gap", type=float, default=1e-4)
    ap.add_argument("--iter-max", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panel_gap.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from convex_optimization_amd import lasso, panel
    from convex_optimization_amd.cpu_calculation import mu_grid
    from convex_optimization_amd.parameters import device_instance

    if not torch.cuda.is_available():
        raise SystemExit("panel_gap_time.py needs a GPU: there is no other path")
    torch.cuda.set_device(0)
    gc, b, _, _ = device_instance(args.m, args.n, args.den, 1, TYPE="bf16", seed=0, device=0)
    A = gc._A_dev
    assert A.dim() == 2 and A.dtype == torch.bfloat16
    b_host = b.cpu().numpy()
    half_bb = 0.5 * float(b_host @ b_host)
    B = b.reshape(-1, 1).expand(args.m, args.k)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    # --- the certificate against the iteration --------------------------------------------------
    pl = panel.PanelLasso(A, 1, nrhs=args.k, device=0)
    pl.solver_reset(B, 1.0)
    mu_max = float(pl.duality_gap(screen=False)["gnorm_inf"][0])
    mus = mu_grid(mu_max, args.k)
    pl.solver_reset(B, mus)
    pl.solver_step(64)
    pl.duality_gap()                                    # untimed
    gap_s, p1, p2 = [], [], []
    for _ in range(5):
        dt, cert = clock(pl.duality_gap)
        gap_s.append(dt)
        p1.append(pl.stat("gap_prod1_ns") * 1e-9)
        p2.append(pl.stat("gap_prod2_ns") * 1e-9)
    it_s = clock(lambda: pl.solver_step(256))[0] / 256
    gap_med = statistics.median(gap_s)
    ratio = gap_med / it_s
    check_every = 64 * max(1, -(-ratio // (0.10 * 64)))   # gap <= 0.10 * check_every iterations
    fma = float(args.m) * args.n * args.k
    out = dict(shape=dict(m=args.m, n=args.n, k=args.k, block=1), device=torch.cuda.get_device_name(0), mu_max=mu_max,
               gap_call=dict(seconds_median=gap_med, seconds_all=gap_s,
                             product1_seconds_median=statistics.median(p1), product2_seconds_median=statistics.median(p2),
                             product1_tflops=2 * fma / statistics.median(p1) * 1e-12,
                             product2_tflops=2 * fma / statistics.median(p2) * 1e-12,
                             drift_max=float(cert["drift"].max()),
                             rel_gap_after_64=[float(cert["gap"].min() / half_bb), float(cert["gap"].max() / half_bb)]),
               iteration=dict(seconds=it_s, iterations_timed=256),
               gap_over_iteration=ratio, check_every_at_10_percent=int(check_every),
               check_every_default=panel.PATH_CHECK_EVERY)
    del pl
    torch.cuda.empty_cache()

    # --- the path as one panel against the slowest single-RHS run -------------------------------
    def path():
        return panel.lasso_path(A, b_host, mus=mus, GAP_BOUND=args.gap, ITER_MAX=args.iter_max, device=0)

    d_ata = np.ones((1, args.n, 1))   # the device drivers read the context's own diag

    def single():
        drv = lasso.ClassLassoScreened(gc, d_ata, types.SimpleNamespace(shape=(args.m, args.n)), b_host, float(mus[-1]),
                                       1, args.iter_max * 8, check_every=64, shrink=0.0)
        drv.run(GAP_BOUND=args.gap, SILENCE=True)
        gc.solver_x()
        return drv

    path(), single()                                    # untimed
    ps, ss = [], []
    for _ in range(args.repeats):                       # alternate the two
        dt, res = clock(path)
        ps.append(dt)
        dt, drv = clock(single)
        ss.append(dt)
    setup_s = clock(lambda: panel.PanelLasso(A, 1, nrhs=args.k, device=0))[0]
    out["path"] = dict(n_mus=int(mus.size), rel_gap_target=args.gap, seconds_median=statistics.median(ps), seconds_all=ps,
                       context_setup_seconds=setup_s, iterations=int(res["iters"]), reached=bool(res["reached"].all()),
                       first_reached=[int(v) for v in res["first_reached"]],
                       rel_gap_last=[float(res["gap"].min() / half_bb), float(res["gap"].max() / half_bb)],
                       check_every=panel.PATH_CHECK_EVERY)
    out["single_rhs_smallest_mu"] = dict(mu=float(mus[-1]), seconds_median=statistics.median(ss), seconds_all=ss,
                                         iterations=int(drv.iters), stopped=bool(drv.stopped), check_every=64,
                                         rel_gap_last=drv.trace[-1]["gap"] / half_bb)
    out["path_seconds_per_mu"] = out["path"]["seconds_median"] / mus.size
    out["single_over_path_per_mu"] = out["single_rhs_smallest_mu"]["seconds_median"] / out["path_seconds_per_mu"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Does gap-safe compaction pay on the panel path, and what does a warm reset cost?

At the configs[4] shape by default (8192 x 65536 bf16, k = 128, one feature block, `device_instance`
seed 0, mu = mu_max * geomspace(0.9, 0.1)):
  path  : panel.lasso_path with shrink 0 against shrink 0.75, at GAP_BOUND 1e-4 and 1e-6: one untimed run
          of each, then `--repeats` timed runs alternating (host clock, synchronised at both ends; the
          wall clock includes building the contexts: bind, the tiled copies of A, graph capture);
  reset : on one context after 64 iterations, solver_reset(x0 = the stored x) against the plain
          solver_reset, one untimed and five timed each, alternating, with and without graph capture
          (the difference is one product 1 of the certificate plus the copy of x).
Writes profiles/panel_screen.json and prints it.  Reads nothing from the oracle or the reference.

    python tools/panel_screen_time.py [--m 8192 --n 65536 --k 128 --repeats 3]
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
    ap.add_argument("--gaps", type=float, nargs="+", default=[1e-4, 1e-6])
    ap.add_argument("--shrink", type=float, default=0.75)
    ap.add_argument("--iter-max", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panel_screen.json"))
    args = ap.parse_args()

    import torch
    from convex_optimization_amd import panel
    from convex_optimization_amd.cpu_calculation import mu_grid
    from convex_optimization_amd.parameters import device_instance

    if not torch.cuda.is_available():
        raise SystemExit("panel_screen_time.py needs a GPU: there is no other path")
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

    # --- a warm reset against a plain one -------------------------------------------------------
    pl = panel.PanelLasso(A, 1, nrhs=args.k, device=0)
    pl.solver_reset(B, 1.0)
    mu_max = float(pl.duality_gap(screen=False)["gnorm_inf"][0])
    mus = mu_grid(mu_max, args.k)
    pl.solver_reset(B, mus)
    pl.solver_step(64)
    x = pl.solver_x_device().clone()                    # (k, n) fp32: the copy form, not the aliasing one
    out = dict(shape=dict(m=args.m, n=args.n, k=args.k, block=1), device=torch.cuda.get_device_name(0), mu_max=mu_max,
               reset={})
    for graph in (True, False):
        def plain():
            pl.solver_reset(B, mus, use_graph=graph)

        def warm():
            pl.solver_reset(B, mus, use_graph=graph, x0=x)

        plain(), warm()                                 # untimed
        ps, ws = [], []
        for _ in range(5):
            ps.append(clock(plain)[0])
            ws.append(clock(warm)[0])
        drift = float(pl.duality_gap(screen=False)["drift"].max())
        out["reset"]["graph" if graph else "no_graph"] = dict(
            plain_seconds_median=statistics.median(ps), warm_seconds_median=statistics.median(ws),
            plain_seconds_all=ps, warm_seconds_all=ws, warm_minus_plain=statistics.median(ws) - statistics.median(ps),
            drift_after_warm=drift)
    pl.solver_reset(B, mus)
    it_s = clock(lambda: pl.solver_step(256))[0] / 256
    out["iteration_seconds"] = it_s
    out["warm_minus_plain_in_iterations"] = out["reset"]["no_graph"]["warm_minus_plain"] / it_s
    del pl, x
    torch.cuda.empty_cache()

    # --- the path with and without compaction ---------------------------------------------------
    out["path"] = []
    for gap in args.gaps:
        def path(shrink):
            return panel.lasso_path(A, b_host, mus=mus, GAP_BOUND=gap, ITER_MAX=args.iter_max, device=0, shrink=shrink)

        path(0.0), path(args.shrink)                    # untimed
        secs, last = {0.0: [], args.shrink: []}, {}
        for _ in range(args.repeats):                   # alternate the two
            for s in (0.0, args.shrink):
                dt, last[s] = clock(lambda: path(s))
                secs[s].append(dt)
        rec = dict(rel_gap_target=gap, check_every=panel.PATH_CHECK_EVERY)
        for s, name in ((0.0, "shrink_0"), (args.shrink, "shrink")):
            r = last[s]
            rec[name] = dict(shrink=s, seconds_median=statistics.median(secs[s]), seconds_all=secs[s],
                             iterations=int(r["iters"]), reached=bool(r["reached"].all()),
                             n_reached=int(r["reached"].sum()), compactions=[list(c) for c in r["compactions"]],
                             compact_seconds=float(r["compact_seconds"]), n_active=int(r["active"].size),
                             n_keep_last=[int(r["n_keep"].min()), int(r["n_keep"].max())],
                             rel_gap_last=[float(r["gap"].min() / half_bb), float(r["gap"].max() / half_bb)])
        rec["shrink_over_shrink_0"] = rec["shrink"]["seconds_median"] / rec["shrink_0"]["seconds_median"]
        out["path"].append(rec)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

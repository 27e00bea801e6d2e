#!/usr/bin/env python
"""Wall clock to a relative duality gap, with and without gap-safe screening.

At the configs[1] shape by default (8192 x 65536 fp32, one feature block, `device_instance`):
  plain    : the ClassLassoDevice loop, stepped 64 iterations at a time with a duality_gap()
             after each (no compaction) -- ClassLassoScreened with shrink=0, which is that loop
             bit for bit;
  screened : ClassLassoScreened with its defaults.
Each is run once untimed (code objects, graph captures, allocator) and then `--repeats` times,
alternating the two; every timed run ends in a device synchronise (solver_x).  Writes
profiles/screening.json and prints it.  Reads nothing from the oracle or the reference.

    python tools/screen_time.py [--m 8192 --n 65536 --den 0.4 --gap 1e-6 --iter-max 20000 --repeats 3]
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
    ap.add_argument("--den", type=float, default=0.4)
    ap.add_argument("--block", type=int, default=1)
    ap.add_argument("--type", default="float")
    ap.add_argument("--gap", type=float, default=1e-6)
    ap.add_argument("--iter-max", type=int, default=20000)
    ap.add_argument("--check-every", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "screening.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from convex_optimization_amd import lasso
    from convex_optimization_amd.parameters import device_instance

    if not torch.cuda.is_available():
        raise SystemExit("screen_time.py needs a GPU: there is no other path")
    torch.cuda.set_device(0)
    gc, b, mu, _ = device_instance(args.m, args.n, args.den, args.block, TYPE=args.type, seed=0, device=0)
    b_host = b.cpu().numpy()
    d_ata = np.ones((args.block, args.n // args.block, 1))   # the device drivers read the context's own diag

    def one(shrink):
        drv = lasso.ClassLassoScreened(gc, d_ata, types.SimpleNamespace(shape=(args.m, args.n)), b_host, mu,
                                       args.block, args.iter_max, check_every=args.check_every, shrink=shrink)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        drv.run(GAP_BOUND=args.gap, SILENCE=True)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        half_bb = 0.5 * float(b_host @ b_host)
        return dict(seconds=wall, iterations=int(drv.iters), stopped=bool(drv.stopped),
                    gather_seconds=drv.gather_seconds, compact_seconds=drv.compact_seconds,
                    n_active=[t["n_active"] for t in drv.trace][:: max(1, len(drv.trace) // 64)],
                    n_active_final=int(drv.active.size),
                    rel_gap_last=drv.trace[-1]["gap"] / half_bb,
                    rel_gap_full_A=drv.certificate["gap"] / half_bb,
                    primal=drv.certificate["primal"], nnz=int(np.count_nonzero(drv.x)))

    runs = {"plain": [], "screened": []}
    one(0.0), one(0.75)                     # warm-up of both paths
    for _ in range(args.repeats):           # alternate the two
        runs["plain"].append(one(0.0))
        runs["screened"].append(one(0.75))
    out = dict(shape=dict(m=args.m, n=args.n, den=args.den, block=args.block, type=args.type), mu=mu,
               rel_gap_target=args.gap, iter_max=args.iter_max, check_every=args.check_every,
               device=torch.cuda.get_device_name(0))
    for k, rs in runs.items():
        secs = [r["seconds"] for r in rs]
        out[k] = dict(seconds_median=statistics.median(secs), seconds_all=secs, **{
            f: rs[-1][f] for f in ("iterations", "stopped", "gather_seconds", "compact_seconds", "n_active", "n_active_final",
                                   "rel_gap_last", "rel_gap_full_A", "primal", "nnz")})
    out["speedup_median"] = out["plain"]["seconds_median"] / out["screened"]["seconds_median"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

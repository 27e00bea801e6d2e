#!/usr/bin/env python
"""Cost of the panel's observation weights against the row mask and the plain iteration.

At the configs[4] shape by default (8192 x 65536 bf16, k = 128 = 8 folds x 16 mu, one feature block,
`device_instance`; mu = mu_max * geomspace(0.9, 0.1, 16)), tools/panel_cv_time.py's protocol on one context:
  iteration : ms per iteration with general weights (uniform in (0.05, 1], about one row in eight exactly 0, different
              per column, seed 0), with the 0/1 row mask `kfold_masks(m, 8, seed=0)` and with neither: one untimed run
              of each (install, reset, 64 + 256 iterations), then `--repeats` timed ones of each, alternating (host
              clock around 256 iterations, synchronised at both ends).  Then the same for the weighted two-kernel form
              (the tuning key fuse_update = 0), which is what the library falls back to when the fused variant does not
              fit;
  gap       : one PanelLasso.duality_gap() with weights, with the mask and with neither after those iterations: one
              untimed call and five timed ones each.
Writes profiles/panel_weights.json and prints it.  Reads nothing from the oracle or the reference.

    python tools/panel_weights_time.py [--m 8192 --n 65536 --folds 8 --mus 16 --repeats 3]
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
    ap.add_argument("--folds", type=int, default=8)
    ap.add_argument("--mus", type=int, default=16)
    ap.add_argument("--den", type=float, default=0.4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panel_weights.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from convex_optimization_amd import panel
    from convex_optimization_amd.cpu_calculation import kfold_masks, mu_grid
    from convex_optimization_amd.parameters import device_instance

    if not torch.cuda.is_available():
        raise SystemExit("panel_weights_time.py needs a GPU: there is no other path")
    torch.cuda.set_device(0)
    gc, b, _, _ = device_instance(args.m, args.n, args.den, 1, TYPE="bf16", seed=0, device=0)
    A = gc._A_dev
    assert A.dim() == 2 and A.dtype == torch.bfloat16
    k = args.folds * args.mus
    assert k in panel.PANEL_NRHS, "folds x mus must fill a panel width"
    B = b.reshape(-1, 1).expand(args.m, k)
    masks = kfold_masks(args.m, args.folds, seed=0)
    cols = np.arange(k)
    W = torch.from_numpy(np.ascontiguousarray(masks[cols // args.mus].T)).to("cuda")
    rs = np.random.RandomState(0)
    Wt = 1.0 - 0.95 * rs.rand(args.m, k)
    Wt[rs.rand(args.m, k) < 0.125] = 0.0

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    pl = panel.PanelLasso(A, 1, nrhs=k, device=0)
    pl.solver_reset(B, 1.0)
    mu_max = float(pl.duality_gap(screen=False)["gnorm_inf"][0])
    mu_cols = mu_grid(mu_max, args.mus)[cols % args.mus]
    fused = {}

    def install(mode):
        if mode == "weighted":
            pl.set_row_weights(Wt)
        elif mode == "masked":
            pl.set_row_mask(W)
        else:
            pl.set_row_weights(None)
        fused[mode] = int(pl.get_tuning("fuse_update"))

    def iterations(mode):
        install(mode)
        pl.solver_reset(B, mu_cols)
        pl.solver_step(64)
        return clock(lambda: pl.solver_step(256))[0] / 256

    def gap_calls(mode):
        iterations(mode)
        pl.duality_gap()                                # untimed
        return [clock(pl.duality_gap)[0] for _ in range(5)]

    def alternate(modes):
        for mode in modes:                              # untimed
            iterations(mode)
        it = {mode: [] for mode in modes}
        for _ in range(args.repeats):
            for mode in modes:
                it[mode].append(1e3 * iterations(mode))
        return {mode: dict(ms_all=v, ms_median=statistics.median(v), ms_min=min(v), ms_max=max(v), fuse_update=fused[mode])
                for mode, v in it.items()}

    modes = ("weighted", "masked", "plain")
    out = dict(shape=dict(m=args.m, n=args.n, k=k, block=1), device=torch.cuda.get_device_name(0), mu_max=mu_max,
               iterations_timed=256, iteration=alternate(modes))
    out["gap_call_seconds"] = {mode: dict(all=v, median=statistics.median(v))
                               for mode, v in ((mode, gap_calls(mode)) for mode in modes)}
    pl.set_tuning("fuse_update", 0)
    out["iteration_two_kernel"] = alternate(("weighted", "masked"))
    it = out["iteration"]
    out["weighted_over_masked"] = it["weighted"]["ms_median"] / it["masked"]["ms_median"]
    out["weighted_over_plain"] = it["weighted"]["ms_median"] / it["plain"]["ms_median"]
    out["weighted_two_kernel_over_fused"] = out["iteration_two_kernel"]["weighted"]["ms_median"] / it["weighted"]["ms_median"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

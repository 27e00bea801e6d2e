#!/usr/bin/env python
"""Cost of the logistic lasso's outer step and of ``logistic_cv``.

At the configs[4] shape by default (8192 x 65536 bf16, k = 128 = 8 folds x 16 mu, one feature block,
`device_instance`; labels y = [b > median b], prior weights uniform in (0.05, 1] with about one row in sixteen exactly 0,
the folds of `kfold_masks(m, 8, seed=0)`; mu = mu_max * geomspace(0.9, 0.1, 16)), on one context, after one outer step
and 64 iterations so that x is not 0:
  calls      : one `glm_model`, one `glm_dual` and one `duality_gap()` each -- one untimed call, five timed (host clock,
               synchronised at both ends);
  outer_step : the pieces of one outer step, timed the same way: model, `set_row_weights_device`, the inner reset with
               graph capture on and off, the certificate, the dual, and `inner_iters` = 64 iterations;
  cv         : `logistic_cv` (8 x 16, refit off, GAP_BOUND 1e-4) for inner_iters 32 / 64 / 128 with graph capture on and
               off: seconds, outer steps, inner iterations, columns reached.  `--cv-repeats` timed runs of each after
               one untimed run of the first.
Writes profiles/panel_logistic.json and prints it.  Reads nothing from the oracle or the reference.

    python tools/panel_logistic_time.py [--m 8192 --n 65536 --folds 8 --mus 16]
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
    ap.add_argument("--outer-max", type=int, default=64)
    ap.add_argument("--cv-repeats", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panel_logistic.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from convex_optimization_amd import panel
    from convex_optimization_amd.cpu_calculation import kfold_masks, mu_grid
    from convex_optimization_amd.parameters import device_instance

    if not torch.cuda.is_available():
        raise SystemExit("panel_logistic_time.py needs a GPU: there is no other path")
    torch.cuda.set_device(0)
    gc, b, _, _ = device_instance(args.m, args.n, args.den, 1, TYPE="bf16", seed=0, device=0)
    A = gc._A_dev
    assert A.dim() == 2 and A.dtype == torch.bfloat16
    k = args.folds * args.mus
    assert k in panel.PANEL_NRHS, "folds x mus must fill a panel width"
    bh = b.detach().cpu().numpy().reshape(-1).astype(np.float64)
    y = (bh > np.median(bh)).astype(np.float64)
    rs = np.random.RandomState(0)
    omega = 1.0 - 0.95 * rs.rand(args.m)
    omega[rs.rand(args.m) < 1.0 / 16] = 0.0
    masks = kfold_masks(args.m, args.folds, seed=0)
    cols = np.arange(k)
    fold = cols // args.mus

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def timed(fn, n=5):
        fn()                                            # untimed
        v = [1e3 * clock(fn)[0] for _ in range(n)]
        return dict(ms_all=v, ms_median=statistics.median(v))

    pl = panel.PanelLasso(A, 1, nrhs=k, device=0)
    pl.set_intercept(True)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).cuda()   # noqa: E731
    Yd = dev(np.repeat(y[None, :], k, axis=0))
    Omd = dev((masks * omega)[fold])
    Hd = dev(((1.0 - masks) * omega)[fold])
    mu_max = panel._logistic_mu_max(pl, Yd, dev(np.repeat(omega[None, :], k, axis=0)))
    mu = mu_grid(mu_max, args.mus)[cols % args.mus]

    # one outer step and 64 iterations, so that the timed calls see a non-zero x
    pl.set_row_weights(None)
    pl.solver_reset(np.zeros((args.m, k)), mu)
    mod = pl.glm_model(Yd, Omd, Hd)
    pl.set_row_weights_device(mod["W"], Hd)
    pl.solver_reset(mod["Z"].t(), 4.0 * mu, x0=pl.solver_x_device())
    pl.solver_step(64)
    scale = pl.duality_gap(screen=False)["scale"]

    def reset(use_graph):
        return lambda: pl.solver_reset(mod["Z"].t(), 4.0 * mu, use_graph=use_graph, x0=pl.solver_x_device())

    out = dict(shape=dict(m=args.m, n=args.n, k=k, block=1), device=torch.cuda.get_device_name(0), mu_max=mu_max)
    step = dict(model=timed(lambda: pl.glm_model(Yd, Omd, Hd)),
                set_row_weights=timed(lambda: pl.set_row_weights_device(mod["W"], Hd)))
    step["reset_graph"] = timed(reset(True), 3)
    step["reset_no_graph"] = timed(reset(False), 3)
    step["certificate"] = timed(lambda: pl.duality_gap(screen=False))
    step["dual"] = timed(lambda: pl.glm_dual(scale))
    pl.solver_reset(mod["Z"].t(), 4.0 * mu, x0=pl.solver_x_device())
    step["iterations_64_graph"] = timed(lambda: pl.solver_step(64), 3)
    pl.solver_reset(mod["Z"].t(), 4.0 * mu, use_graph=False, x0=pl.solver_x_device())
    step["iterations_64_no_graph"] = timed(lambda: pl.solver_step(64), 3)
    out["outer_step"] = step
    out["calls"] = dict(glm_model_ms=step["model"]["ms_median"], glm_dual_ms=step["dual"]["ms_median"],
                        duality_gap_ms=timed(lambda: pl.duality_gap(screen=True))["ms_median"],
                        gap_prod1_ms=pl.stat("gap_prod1_ns") / 1e6, gap_prod2_ms=pl.stat("gap_prod2_ns") / 1e6)
    del pl

    def cv(inner, graph):
        return panel.logistic_cv(A, y, n_folds=args.folds, mus=mu_grid(mu_max, args.mus), masks=masks,
                                 sample_weight=omega, GAP_BOUND=1e-4, OUTER_MAX=args.outer_max, inner_iters=inner,
                                 use_graph=graph, refit=False, device=0)
    cv(32, True)                                        # untimed
    runs = []
    for inner in (32, 64, 128):
        for graph in (True, False):
            for _ in range(args.cv_repeats):
                sec, r = clock(lambda: cv(inner, graph))
                runs.append(dict(inner_iters=inner, use_graph=graph, seconds=sec, outer_steps=int(r["outer_iters"].max()),
                                 iters=int(r["iters"]), reached=int(r["reached"].sum()), columns=int(r["reached"].size),
                                 fell_back=int(r["curvature"].sum()), best=int(r["best"])))
    out["cv"] = runs
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

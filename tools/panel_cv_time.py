#!/usr/bin/env python
"""Cost of the panel's row mask, and K-fold cross-validation as one panel against K row-deleted paths.

At the configs[4] shape by default (8192 x 65536 bf16, k = 128 = 8 folds x 16 mu, one feature block,
`device_instance`; masks `kfold_masks(m, 8, seed=0)`, mu = mu_max * geomspace(0.9, 0.1, 16)):
  iteration : ms per iteration of one context, masked against unmasked: one untimed run of each
              (set_row_mask, reset, 64 + 256 iterations), then `--repeats` timed ones of each,
              alternating (host clock around 256 iterations, synchronised at both ends);
  gap       : one PanelLasso.duality_gap() with and without the mask after those iterations: one
              untimed call and five timed ones each;
  cv        : panel.lasso_cv(refit=False) to the gap bound against what a user could do before:
              for each of the 8 folds an index_select of its 7168 training rows (torch) and a
              panel.lasso_path of the 16 mu on them.  One untimed run of each, then `--repeats` timed
              ones, alternating; the wall clocks include building the contexts (bind, the tiled copies
              of A, graph capture).
Writes profiles/panel_cv.json and prints it.  Reads nothing from the oracle or the reference.

    python tools/panel_cv_time.py [--m 8192 --n 65536 --folds 8 --mus 16 --gap 1e-4 --repeats 3]
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
    ap.add_argument("--gap", type=float, default=1e-4)
    ap.add_argument("--iter-max", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "panel_cv.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    from convex_optimization_amd import panel
    from convex_optimization_amd.cpu_calculation import kfold_masks, mu_grid
    from convex_optimization_amd.parameters import device_instance

    if not torch.cuda.is_available():
        raise SystemExit("panel_cv_time.py needs a GPU: there is no other path")
    torch.cuda.set_device(0)
    gc, b, _, _ = device_instance(args.m, args.n, args.den, 1, TYPE="bf16", seed=0, device=0)
    A = gc._A_dev
    assert A.dim() == 2 and A.dtype == torch.bfloat16
    b_host = b.cpu().numpy()
    k = args.folds * args.mus
    assert k in panel.PANEL_NRHS, "folds x mus must fill a panel width"
    B = b.reshape(-1, 1).expand(args.m, k)
    masks = kfold_masks(args.m, args.folds, seed=0)
    cols = np.arange(k)
    W = torch.from_numpy(np.ascontiguousarray(masks[cols // args.mus].T)).to("cuda")

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    # --- the masked iteration and certificate against the unmasked ones, on one context -----------
    pl = panel.PanelLasso(A, 1, nrhs=k, device=0)
    pl.solver_reset(B, 1.0)
    mu_max = float(pl.duality_gap(screen=False)["gnorm_inf"][0])
    mus = mu_grid(mu_max, args.mus)
    mu_cols = mus[cols % args.mus]

    def iterations(masked):
        pl.set_row_mask(W if masked else None)
        pl.solver_reset(B, mu_cols)
        pl.solver_step(64)
        return clock(lambda: pl.solver_step(256))[0] / 256

    def gap_calls():
        pl.duality_gap()                                # untimed
        return [clock(pl.duality_gap)[0] for _ in range(5)]

    iterations(True), iterations(False)                 # untimed
    it = {True: [], False: []}
    for _ in range(args.repeats):                       # alternate the two
        for masked in (True, False):
            it[masked].append(iterations(masked))
    gap_plain = gap_calls()                             # the context is unmasked after the loop
    iterations(True)
    gap_masked = gap_calls()
    cert = pl.duality_gap()
    out = dict(shape=dict(m=args.m, n=args.n, k=k, block=1, folds=args.folds, mus=args.mus),
               device=torch.cuda.get_device_name(0), mu_max=mu_max, fuse_update=int(pl.get_tuning("fuse_update")),
               iteration=dict(iterations_timed=256, masked_ms_all=[1e3 * v for v in it[True]],
                              unmasked_ms_all=[1e3 * v for v in it[False]],
                              masked_ms_median=1e3 * statistics.median(it[True]),
                              unmasked_ms_median=1e3 * statistics.median(it[False])),
               gap_call=dict(masked_seconds_all=gap_masked, unmasked_seconds_all=gap_plain,
                             masked_seconds_median=statistics.median(gap_masked),
                             unmasked_seconds_median=statistics.median(gap_plain),
                             holdout_mse_after_320=[float(v) for v in
                                                    (cert["holdout_sse"] / (masks == 0).sum(axis=1)[cols // args.mus])[::args.mus]]))
    out["iteration"]["masked_over_unmasked"] = out["iteration"]["masked_ms_median"] / out["iteration"]["unmasked_ms_median"]
    del pl
    torch.cuda.empty_cache()

    # --- cross-validation as one panel against one row-deleted path per fold ----------------------
    kw = dict(GAP_BOUND=args.gap, ITER_MAX=args.iter_max, device=0)

    def cv():
        return panel.lasso_cv(A, b_host, mus=mus, masks=masks, refit=False, **kw)

    def per_fold():
        res = []
        for f in range(args.folds):
            rows = torch.from_numpy(np.flatnonzero(masks[f])).to("cuda")
            res.append(panel.lasso_path(torch.index_select(A, 0, rows), b_host[masks[f] != 0], mus=mus, **kw))
        return res

    trainable = all(int(masks[f].sum()) % 256 == 0 for f in range(args.folds))   # the panel's row contract
    cv()
    if trainable:
        per_fold()
    cs, fs = [], []
    for _ in range(args.repeats):                       # alternate the two
        dt, res = clock(cv)
        cs.append(dt)
        if trainable:
            dt, paths = clock(per_fold)
            fs.append(dt)
    out["cv"] = dict(rel_gap_target=args.gap, check_every=panel.PATH_CHECK_EVERY, seconds_median=statistics.median(cs),
                     seconds_all=cs, iterations=int(res["iters"]), reached=bool(res["reached"].all()),
                     mean_mse=[float(v) for v in res["mean_mse"]], se_mse=[float(v) for v in res["se_mse"]],
                     best=res["best"], best_1se=res["best_1se"])
    if trainable:
        out["per_fold_paths"] = dict(seconds_median=statistics.median(fs), seconds_all=fs,
                                     iterations=[int(p["iters"]) for p in paths],
                                     reached=bool(all(p["reached"].all() for p in paths)),
                                     training_rows=[int(masks[f].sum()) for f in range(args.folds)])
        out["per_fold_over_cv"] = out["per_fold_paths"]["seconds_median"] / out["cv"]["seconds_median"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

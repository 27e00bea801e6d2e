"""Offline generator of tests/golden/panel/panel_restatement.npz (TEST INFRASTRUCTURE; no GPU, no compiled library).

The fixture freezes what the per-mode fp64 restatements of ``cpu_calculation`` computed BEFORE they were folded into
one iteration core and one certificate core ("one fp64 restatement"): it was written from the commit
"Panel observation weights: per-row weights in solver, gap, path, CV", where ``masked_*``, ``intercept_*``,
``positive_*``, ``penalty_*`` and ``weighted_*`` were five separate statements.  Run from a later tree it records
that tree's own output, which pins nothing: do not regenerate it.  tests/test_panel_restatement_host.py never does.

Per case of tests/panel_restatement_cases.py: mu = 0.3 of the case's own mu_max, x, r (and the intercept) after 18
iterations, and the certificate at that x (the scalars, keep, g), one array per key with a row per case, in the order
of ``tags``; the instance is rebuilt by the test and its arrays are kept here too, so a changed instance is seen before
anything is compared.

usage: python tests/golden/make_panel_restatement.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import panel_restatement_cases as RC  # noqa: E402
from convex_optimization_amd import cpu_calculation as C  # noqa: E402


def main():
    inst = RC.instance()
    out = {f"instance_{key}": np.asarray(val) for key, val in inst.items()}
    recs = []
    for case in RC.CASES:
        mu = 0.3 * RC.mu_max(C, inst, case)
        recs.append(dict(RC.run(C, inst, case, mu), mu=np.float64(mu)))
        assert np.count_nonzero(recs[-1]["x"]) >= 1, case[0]
    out["tags"] = np.array([case[0] for case in RC.CASES])
    # one array per key, a row per case; NaN where the parent's dict had no such key
    for key in ("mu", "x", "r", "g", "keep", "x_intercept") + RC.SCALARS:
        out[key] = np.stack([np.asarray(rec.get(key, np.nan)) for rec in recs])
    path = os.path.join(HERE, "panel", "panel_restatement.npz")
    np.savez_compressed(path, **out)
    print(f"{len(RC.CASES)} cases -> {path}, {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()

"""convex_optimization_amd -- MI355X-native block best-response lasso hot path.

Drop-in modules for the reference's call surface:
  ``cpu_calculation``  host helpers (numpy), same names and shapes
  ``gpu_calculation``  ``GPU_Calculation`` over hand-written gfx950 HIP kernels
                       (``_lib/libbpgl.so``, C ABI in ``include/bpgl.h``)
  ``panel``            ``PanelLasso`` (k right-hand sides on bf16 A, MFMA), its per-RHS certificate
                       ``PanelLasso.duality_gap`` and ``lasso_path`` (a grid of mu as one panel)
  ``lasso``            drivers: ClassLasso / ClassLassoR / ClassLassoDevice, and
                       ``ClassLassoScreened`` (duality-gap stopping rule + gap-safe screening)
  ``parameters``       problem instances (reference recipe + in-HBM generator)
  ``distributed``      column-sharded multi-GPU path (RCCL all-reduce)
"""
__version__ = "0.1.0"

from .lasso import ClassLassoScreened  # noqa: E402  (numpy only: torch is imported when it runs)

from .cpu_calculation import mu_grid, panel_duality_gap  # noqa: E402


def __getattr__(name):
    # PanelLasso and lasso_path need torch: imported on first use
    if name in ("PanelLasso", "lasso_path"):
        from . import panel
        return getattr(panel, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["cpu_calculation", "gpu_calculation", "lasso", "panel", "parameters", "distributed", "ClassLassoScreened",
           "mu_grid", "panel_duality_gap", "PanelLasso", "lasso_path"]

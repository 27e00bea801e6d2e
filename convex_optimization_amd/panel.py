"""k right-hand sides at once with bf16 A on CDNA4 MFMA (BASELINE configs[4]).

The reference solves one lasso problem per run (lasso.py:102-157).  The panel
path runs k in {16, 32, 64, 128} of them together on one matrix: each block
update computes G = A_m^T R and S = A_m D as MFMA panel products instead of
GEMVs, then applies the reference's shrink, exact line search and update to
every right-hand side (cyclic block order, fixed iteration count).

Numerics (stated tolerance): A is stored as bf16 (the problem is defined by the
bf16-rounded A); fp32 accumulation per block tile, fp64 after that.  The default
path (one feature block) is:

* the direction enters the A D pass as its bf16 rounding (d_split = 1; 2 = a
  hi + lo bf16 pair), and the line search is exact along the direction the MFMA
  saw, so every step is an exact line search (monotone objective);
* the gradient is carried (carry_g = 1): G_t = G_{t-1} + gamma A^T bf16(V) in
  fp32, with V = gamma S + the previous rounding (error feedback), and computed
  exactly from the residual's hi + lo bf16 pair every g_refresh = 64 iterations;
* x += gamma D' is applied by the next pass-1 epilogue (defer_x = 1; bitwise the
  same x).

Against the fp64 oracle on the same bf16 A: after the reference's 1000
iterations at the full configs[4] shape, x within 1e-4 relative l2 (measured
3.6-4.1e-6 for the default, 1.7-2.2e-5 for the exact-gradient forms) and the
objective within 1e-5 (measured ~1e-12) (tests/test_longrun.py).  Over short
runs the forms follow different trajectories to the same fixed point: x within
1e-2 and the objective within 1e-4 on the default path (tests/test_panel.py;
1e-5 for the exact-gradient hi + lo form).

``PanelLasso.duality_gap`` certifies the stored fp32 x of every right-hand side (fp64 products on
the bf16 A), and ``lasso_path`` runs one b against a grid of mu as one panel
with that certificate as its stopping rule.  ``PanelLasso.set_row_mask`` gives every right-hand side
0/1 row weights, and ``lasso_cv`` uses them to run K-fold cross-validation over a grid of mu as one
panel (K folds x J values of mu = K J columns on one bound A).
``PanelLasso.solver_reset(x0=...)`` starts the panel at a given x and ``gather_columns`` compacts the
bound A; ``lasso_path`` and ``lasso_cv`` use them, opt-in, to warm-start and to drop columns the
gap-safe screen proves zero for every right-hand side.
``PanelLasso.set_intercept`` gives every right-hand side an unpenalised intercept, centred over that
right-hand side's own in-rows inside the fold, and ``lasso_path`` / ``lasso_cv`` take ``fit_intercept``
(DESIGN.md section 13).
``PanelLasso.set_positive`` adds the sign constraint x >= 0 (scikit-learn's ``positive=True``, glmnet's
``lower.limits = 0``) to every right-hand side -- every stored iterate is then >= 0 -- and ``lasso_path`` /
``lasso_cv`` take ``positive``.
``PanelLasso.set_penalty_factors`` gives column j the l1 weight p_j > 0 (glmnet's ``penalty.factor``, the adaptive
lasso's weights; used as given, not renormalised), one vector for all right-hand sides on the A that is bound,
and ``lasso_path`` / ``lasso_cv`` take ``penalty_factors``.
``PanelLasso.set_row_weights`` gives every right-hand side observation weights w_i in [0, 1] (glmnet's ``weights``,
scikit-learn's ``sample_weight``) and scoring weights for the held-out score, on the A that is bound -- no row-rescaled
copy -- and ``lasso_path`` / ``lasso_cv`` take ``sample_weight`` (any scale, used as given).

``PanelLasso.glm_model`` / ``glm_dual`` are the piece between two inner solves of an IRLS loop for the L1-penalised
logistic regression (glmnet's ``family = "binomial"``), and ``logistic_path`` / ``logistic_cv`` the drivers on top: the
inner solves are the weighted lasso above, unchanged.

All compute goes through libbpgl.so (bpgl_panel_* in include/bpgl.h).
"""
import contextlib
import ctypes
import time

import numpy as np
import torch

from . import _native as N

_p = ctypes.c_void_p
_i64 = ctypes.c_int64
_i32 = ctypes.c_int32
_PANEL_SIGS = {
    "bpgl_panel_create": (ctypes.c_int, [ctypes.POINTER(_p), ctypes.c_int, _i64, _i64, _i32, _i32, _i32, _p]),
    "bpgl_panel_destroy": (None, [_p]),
    "bpgl_panel_scratch_bytes": (_i64, [_p]),
    "bpgl_panel_bind": (ctypes.c_int, [_p, _p, _i64, _p, _i64]),
    "bpgl_panel_diag": (ctypes.c_int, [_p, _p]),
    "bpgl_panel_mtm": (ctypes.c_int, [_p, _i32, _p, _p]),
    "bpgl_panel_mm": (ctypes.c_int, [_p, _i32, _p, _p]),
    "bpgl_panel_reset": (ctypes.c_int, [_p, _p, _p, _p, _i64, ctypes.c_int]),
    "bpgl_panel_step": (ctypes.c_int, [_p, _i64]),
    "bpgl_panel_status": (ctypes.c_int, [_p, ctypes.POINTER(_i64), ctypes.POINTER(ctypes.c_double)]),
    "bpgl_panel_x": (_p, [_p]),
    "bpgl_panel_set_kernel_timing": (ctypes.c_int, [_p, ctypes.c_int]),
    "bpgl_panel_kernel_times": (ctypes.c_int, [_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_i64)]),
    "bpgl_panel_geometry": (ctypes.c_int, [_p, ctypes.POINTER(_i32)]),
    "bpgl_panel_set_tuning": (ctypes.c_int, [_p, ctypes.c_char_p, _i64]),
    "bpgl_panel_get_tuning": (ctypes.c_int, [_p, ctypes.c_char_p, ctypes.POINTER(_i64)]),
    "bpgl_panel_stat": (ctypes.c_int, [_p, ctypes.c_char_p, ctypes.POINTER(_i64)]),
    "bpgl_panel_residual": (_p, [_p]),
    "bpgl_panel_gap": (ctypes.c_int, [_p, _p, _p, _p, ctypes.POINTER(ctypes.c_double)]),
    "bpgl_panel_set_row_mask": (ctypes.c_int, [_p, _p]),
    "bpgl_panel_reset_x0": (ctypes.c_int, [_p, _p, _p, _p, _p, _i64, ctypes.c_int]),
    "bpgl_panel_gather_columns": (ctypes.c_int, [_p, _p, _i64, _p, _i64]),
    "bpgl_panel_set_intercept": (ctypes.c_int, [_p, ctypes.c_int]),
    "bpgl_panel_intercept": (ctypes.c_int, [_p, ctypes.POINTER(ctypes.c_double)]),
    "bpgl_panel_set_positive": (ctypes.c_int, [_p, ctypes.c_int]),
    "bpgl_panel_set_penalty": (ctypes.c_int, [_p, _p]),
    "bpgl_panel_set_row_weights": (ctypes.c_int, [_p, _p, _p]),
    "bpgl_panel_glm_model": (ctypes.c_int, [_p, ctypes.c_int, _p, _p, _p, _p, _p, _p, _p, _p,
                                            ctypes.POINTER(ctypes.c_double)]),
    "bpgl_panel_glm_dual": (ctypes.c_int, [_p, _p, _p, _p, ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_double)]),
}
N._SIGS.update(_PANEL_SIGS)


def _lib():
    L = N.lib()
    for name, (res, args) in _PANEL_SIGS.items():
        f = getattr(L, name)
        f.restype, f.argtypes = res, args
    return L


class PanelLasso:
    """k lasso problems sharing A (m x n, bf16), one block update per iteration for all of them."""

    KERNEL_KINDS = ("pass1_mfma", "pass2_mfma", "reduce", "step", "update")

    def __init__(self, A, Block=1, nrhs=128, device=None, kchunks=0, cu_mask=None, lda=None):
        """cu_mask: CU mask words (bit i = CU i) -> the solver runs on a CU-masked stream of its own
        (bpgl_stream_create; the fused reduce + update is admitted only if it fits those CUs).
        lda: row stride of the stored bf16 A (>= n, a multiple of 8; default n), the padding zeroed."""
        L = _lib()
        self.Block = int(Block)
        self.nrhs = int(nrhs)
        H, K = int(A.shape[0]), int(A.shape[1])
        if K % self.Block:
            raise ValueError("array split does not result in an equal division")
        self.MAT_HEIGHT, self.MAT_WIDTH, self.MAT_WIDTH_ALL = H, K // self.Block, K
        if device is None:
            device = A.device if isinstance(A, torch.Tensor) and A.is_cuda else torch.cuda.current_device()
        self.device = torch.device("cuda", torch.device(device).index if not isinstance(device, int) else device)
        torch.cuda.set_device(self.device)
        if cu_mask is not None:
            from .gpu_calculation import _masked_stream
            self.stream = _masked_stream(self.device, list(cu_mask))
        else:
            self.stream = torch.cuda.Stream(device=self.device)
        ctx = ctypes.c_void_p()
        N.check(L.bpgl_panel_create(ctypes.byref(ctx), self.device.index, H, K, self.Block, self.nrhs,
                                    int(kchunks), ctypes.c_void_p(self.stream.cuda_stream)), "bpgl_panel_create")
        self._ctx = ctx
        lda = K if lda is None else int(lda)
        self.lda = lda
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.stream):
            A_src = A if isinstance(A, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(A))
            A_src = A_src.to(device=self.device, dtype=torch.bfloat16)
            if lda == K:
                self._A = A_src.contiguous()                                                # [m][n]
            else:                                                                           # [m][lda]
                self._A_store = torch.zeros(H, lda, dtype=torch.bfloat16, device=self.device)
                self._A_store[:, :K] = A_src
                self._A = self._A_store[:, :K]
            nbytes = int(L.bpgl_panel_scratch_bytes(ctx))
            self._scratch = torch.empty(nbytes // 8 + 64, dtype=torch.float64, device=self.device)
            base = (self._scratch.data_ptr() + 255) // 256 * 256
            N.check(L.bpgl_panel_bind(ctx, ctypes.c_void_p(self._A.data_ptr()), lda, ctypes.c_void_p(base), nbytes),
                    "bpgl_panel_bind")
            self._diag = torch.empty(K, dtype=torch.float64, device=self.device)
            N.check(L.bpgl_panel_diag(ctx, N.ptr(self._diag)), "bpgl_panel_diag")
        self.stream.synchronize()
        kc = ctypes.c_int32()
        N.check(L.bpgl_panel_geometry(ctx, ctypes.byref(kc)), "bpgl_panel_geometry")
        self.kchunks = kc.value

    def __del__(self):
        try:
            if self._ctx is not None and N._lib is not None:
                self.stream.synchronize()
                N.lib().bpgl_panel_destroy(self._ctx)
                self._ctx = None
        except Exception:
            pass

    @contextlib.contextmanager
    def _on_stream(self):
        cur = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            yield
        cur.wait_stream(self.stream)

    @property
    def A_bf16(self):
        """A copy of the stored A (m x n, bf16) -- the matrix the problems are defined by.  A copy:
        bind took the passes' tiled images of A (include/bpgl.h), so writing into the stored A
        would change bpgl_panel_diag's input but not the solver's."""
        return self._A.clone()

    @property
    def diag_ATA(self):
        self.stream.synchronize()
        return self._diag.cpu().numpy().reshape(self.Block, self.MAT_WIDTH, 1)

    def _dev(self, v, shape):
        t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))
        return t.to(device=self.device, dtype=torch.float64).reshape(shape)

    def mat_tMulMat(self, R, block=0):
        """G = A_block^T R for R (m, k) -> (w, k) fp64 (split-bf16 MFMA)."""
        with self._on_stream():
            Rt = self._dev(R, (self.MAT_HEIGHT, self.nrhs)).t().contiguous()
            G = torch.empty((self.nrhs, self.MAT_WIDTH), dtype=torch.float64, device=self.device)
            N.check(_lib().bpgl_panel_mtm(self._ctx, int(block), N.ptr(Rt), N.ptr(G)), "bpgl_panel_mtm")
            out = G.t().contiguous()
        return out

    def matMulMat(self, D, block=0):
        """S = A_block D for D (w, k) -> (m, k) fp64."""
        with self._on_stream():
            Dt = self._dev(D, (self.MAT_WIDTH, self.nrhs)).t().contiguous()
            S = torch.empty((self.nrhs, self.MAT_HEIGHT), dtype=torch.float64, device=self.device)
            N.check(_lib().bpgl_panel_mm(self._ctx, int(block), N.ptr(Dt), N.ptr(S)), "bpgl_panel_mm")
            out = S.t().contiguous()
        return out

    def _x0_layout(self, x0):
        """x0, (n, k) or the (k, n) of ``solver_x_device`` -> (device fp32 tensor [nblock][k][w], its address);
        the stored iterate itself (one feature block: ``solver_x_device()`` is a view of it) is passed on
        as it is, and bpgl_panel_reset_x0 then copies nothing."""
        k, n = self.nrhs, self.MAT_WIDTH_ALL
        t = x0 if isinstance(x0, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x0))
        if tuple(t.shape) == (n, k):
            t = t.t()
        elif tuple(t.shape) != (k, n):
            raise ValueError(f"x0 must be (n, k) = ({n}, {k}), got {tuple(t.shape)}")
        if t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and self.Block == 1 \
                and t.data_ptr() == _lib().bpgl_panel_x(self._ctx):
            return t, t.data_ptr()
        t = t.to(device=self.device, dtype=torch.float32)
        t = t.reshape(k, self.Block, self.MAT_WIDTH).permute(1, 0, 2).contiguous()
        return t, t.data_ptr()

    def solver_reset(self, B, mu, record_len=0, use_graph=True, x0=None):
        """B (m, k) right-hand sides, mu scalar or (k,).  ``x0``: None starts at x = 0 (bpgl_panel_reset);
        an (n, k) array or tensor (or the (k, n) of ``solver_x_device``) starts at its fp32 rounding
        (bpgl_panel_reset_x0: R = A x0 - B from the certificate's fp64 product; include/bpgl.h).
        ``solver_x_device()`` of this context (one feature block) restarts from the stored iterate
        without a copy."""
        with self._on_stream():
            self._Bt = self._dev(B, (self.MAT_HEIGHT, self.nrhs)).t().contiguous()
            mu_v = np.broadcast_to(np.asarray(mu, dtype=np.float64), (self.nrhs,)).copy()
            self._mu = torch.from_numpy(mu_v).to(self.device)
            self._err_iter = torch.zeros(max(1, record_len), dtype=torch.float64, device=self.device) \
                if record_len else None
            if x0 is None:
                N.check(_lib().bpgl_panel_reset(self._ctx, N.ptr(self._Bt), N.ptr(self._mu), N.ptr(self._err_iter),
                                                int(record_len), int(bool(use_graph))), "bpgl_panel_reset")
            else:
                self._x0, addr = self._x0_layout(x0)   # kept: the copy is enqueued, not done
                N.check(_lib().bpgl_panel_reset_x0(self._ctx, N.ptr(self._Bt), N.ptr(self._mu), ctypes.c_void_p(addr),
                                                   N.ptr(self._err_iter), int(record_len), int(bool(use_graph))),
                        "bpgl_panel_reset_x0")

    def gather_columns(self, cols):
        """(m, lda_out) bf16 device tensor with column c = column cols[c] of the stored A
        (bpgl_panel_gather_columns): ``cols`` int array or tensor in any order, an index outside [0, n)
        gives a zero column; lda_out = len(cols) rounded up to 8, the pad columns zero."""
        with self._on_stream():
            t = cols if isinstance(cols, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(cols))
            t = t.reshape(-1).to(device=self.device, dtype=torch.int32).contiguous()
            n_out = int(t.numel())
            lda_out = -(-n_out // 8) * 8
            out = torch.empty((self.MAT_HEIGHT, lda_out), dtype=torch.bfloat16, device=self.device)
            N.check(_lib().bpgl_panel_gather_columns(self._ctx, N.ptr(t), n_out, N.ptr(out), lda_out),
                    "bpgl_panel_gather_columns")
        return out

    def set_row_mask(self, mask):
        """0/1 row weights per right-hand side: ``mask`` (m, k) bool / uint8 array or tensor, nonzero =
        the row is in that column's objective, zero = held out; None clears it.  A ``solver_reset``
        (with the full B) must follow.  The solver then minimises 1/2 ||w o (A x - b)||^2 + mu ||x||_1
        per column, ``residual_device`` is the masked residual and ``duality_gap`` certifies the masked
        problems and reports each column's held-out sum of squares (include/bpgl.h)."""
        with self._on_stream():
            if mask is None:
                self._mask = None
            else:
                t = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mask))
                if tuple(t.shape) != (self.MAT_HEIGHT, self.nrhs):
                    raise ValueError(f"mask must be (m, k) = ({self.MAT_HEIGHT}, {self.nrhs}), got {tuple(t.shape)}")
                self._mask = (t.to(self.device) != 0).to(torch.uint8).t().contiguous()   # [k][m]
            N.check(_lib().bpgl_panel_set_row_mask(self._ctx, N.ptr(self._mask)), "bpgl_panel_set_row_mask")

    def set_intercept(self, on):
        """An unpenalised intercept per right-hand side (bpgl_panel_set_intercept; one feature block):
        every column minimises 1/2 ||w o (A x + beta0 - b)||^2 + mu ||x||_1 over x and beta0, beta0
        profiled out over the column's in-rows (all rows without a row mask).  A ``solver_reset`` (with the
        full B) must follow.  ``diag_ATA`` is then the centred column norms sum_i (a_ij - mean_j)^2,
        ``residual_device`` the centred residual, and ``duality_gap`` certifies the profiled problems and
        reports ``intercept``.  ``set_intercept(False)`` restores the plain solver bitwise."""
        with self._on_stream():
            N.check(_lib().bpgl_panel_set_intercept(self._ctx, int(bool(on))), "bpgl_panel_set_intercept")
            N.check(_lib().bpgl_panel_diag(self._ctx, N.ptr(self._diag)), "bpgl_panel_diag")   # the diag in effect
        self._intercept = bool(on)

    def set_positive(self, on):
        """The sign constraint x >= 0 on every right-hand side (bpgl_panel_set_positive): each column minimises
        1/2 ||w o (A x - b)||^2 + mu sum x subject to x >= 0 (with the row mask and the intercept when those are
        on).  A ``solver_reset`` must follow; with ``x0`` it starts at max(x0, 0).  Every stored iterate is
        >= 0, ``duality_gap`` certifies the constrained problem (gnorm_inf is then max_j (-g_j)+ and the screen
        one-sided), and ``set_positive(False)`` restores the plain solver bitwise."""
        N.check(_lib().bpgl_panel_set_positive(self._ctx, int(bool(on))), "bpgl_panel_set_positive")

    def set_penalty_factors(self, p):
        """Per-column l1 weights (bpgl_panel_set_penalty): every right-hand side minimises
        1/2 ||w o (A x - b)||^2 + mu sum_j p_j |x_j| (with the row mask, the intercept and x >= 0 when those are
        on).  ``p``: a numpy array or torch tensor of length n, every entry finite and > 0 (ValueError otherwise,
        before any device work), or None to switch it off.  The factors are used as given -- no renormalisation
        to sum p = n as glmnet applies.  A ``solver_reset`` must follow.  ``duality_gap`` then certifies the
        weighted problem: gnorm_inf is max_j |g_j| / p_j (at x = 0: mu_max) and the screen compares with mu p_j.
        A vector of ones, and ``set_penalty_factors(None)``, give the plain solver bitwise."""
        pen = _check_penalty(p, self.MAT_WIDTH_ALL)
        with self._on_stream():
            self._pen = None if pen is None else torch.from_numpy(pen).to(self.device)
            N.check(_lib().bpgl_panel_set_penalty(self._ctx, N.ptr(self._pen)), "bpgl_panel_set_penalty")
        self.stream.synchronize()

    def set_row_weights(self, weights, holdout=None):
        """Observation weights per right-hand side (bpgl_panel_set_row_weights; one feature block): column k
        minimises 1/2 sum_i w_ik (a_i . x - b_ik)^2 + mu sum_j p_j |x_j| (with the intercept -- then profiled over the
        weighted mean --, x >= 0 and the penalty factors when those are on).  ``weights``: an (m, k) or (m,) array or
        tensor (one vector serves every column), every entry finite and in [0, 1] (ValueError otherwise, before any
        device work; scale larger weights by their maximum c and pass mu / c), or None to clear them.  ``holdout``:
        the scoring weights h >= 0 of ``duality_gap()['holdout_sse']`` = sum_i h_ik (a_i . x + beta0 - b_ik)^2, same
        shapes; None scores the zero-weight rows with weight 1, the row mask's rule.  Weights and a row mask are
        alternatives: the last call wins.  A ``solver_reset`` (with the full B) must follow.  ``residual_device`` is
        then w o (A x - b) and ``duality_gap`` certifies the weighted problems with its usual keys.  0/1 weights compute
        what ``set_row_mask`` computes, and ``set_row_weights(None)`` restores the plain solver bitwise."""
        wt = _check_row_weights(weights, self.MAT_HEIGHT, self.nrhs, "weights", 1.0)
        hd = None if wt is None else _check_row_weights(holdout, self.MAT_HEIGHT, self.nrhs, "holdout", np.inf)
        with self._on_stream():
            self._wt = None if wt is None else torch.from_numpy(wt).to(self.device)   # [k][m]
            self._hd = None if hd is None else torch.from_numpy(hd).to(self.device)
            N.check(_lib().bpgl_panel_set_row_weights(self._ctx, N.ptr(self._wt), N.ptr(self._hd)),
                    "bpgl_panel_set_row_weights")
        self.stream.synchronize()

    def set_row_weights_device(self, W, H=None):
        """``set_row_weights`` with device fp64 tensors [k][m] (``H`` None: the row mask's rule) straight to
        bpgl_panel_set_row_weights, which validates them on the device: no host round trip."""
        for t in (W, H):
            if t is not None and not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
                                      and tuple(t.shape) == (self.nrhs, self.MAT_HEIGHT)):
                raise ValueError(f"device weights must be contiguous fp64 [k][m] = [{self.nrhs}][{self.MAT_HEIGHT}]")
        with self._on_stream():
            self._wt, self._hd = W, H
            N.check(_lib().bpgl_panel_set_row_weights(self._ctx, N.ptr(W), N.ptr(H)), "bpgl_panel_set_row_weights")
        self.stream.synchronize()

    GLM_KEYS = ("loss", "hold_loss", "hold_miss", "sum_omega", "l1", "phi", "steps", "flag")

    def glm_model(self, Y, omega, holdout=None, curvature=None, beta0=None):
        """One outer step of the logistic IRLS at the stored x (bpgl_panel_glm_model; one feature block, after a
        ``solver_reset``): ``Y``, ``omega`` device fp64 [k][m] (labels in [0, 1], prior weights in [0, 1]), ``holdout``
        the scoring weights h >= 0 or None, ``curvature`` a device int32 [k] tensor (1: Boehning's 1/4) or None,
        ``beta0`` a device fp64 [k] tensor -- the Newton start, overwritten with the root; None uses the one of the last
        call (zeros at first).  The intercept is the context's own switch (``set_intercept``).  Returns a dict of (k,)
        numpy arrays loss = sum om l, hold_loss = sum h l, hold_miss = sum h [(p > 1/2) != (y > 1/2)], sum_omega,
        l1 = sum p_j |x_j|, phi = the final |phi|, steps, flag (1: no finite intercept), and the device tensors W, Z, P
        [k][m], beta0 [k] and AX [k][m] (buffers the next call overwrites).  Read-only for the solve and bitwise
        repeatable."""
        k, m = self.nrhs, self.MAT_HEIGHT
        if getattr(self, "_glm_W", None) is None:
            self._glm_W, self._glm_Z, self._glm_P = (torch.empty((k, m), dtype=torch.float64, device=self.device)
                                                     for _ in range(3))
            self._glm_b0 = torch.zeros(k, dtype=torch.float64, device=self.device)
            self._glm_out = (ctypes.c_double * (8 * k))()
        if beta0 is not None:
            self._glm_b0 = beta0
        self._glm_Y, self._glm_Om = Y, omega
        with self._on_stream():
            N.check(_lib().bpgl_panel_glm_model(self._ctx, 1, N.ptr(Y), N.ptr(omega), N.ptr(holdout), N.ptr(curvature),
                                                N.ptr(self._glm_b0), N.ptr(self._glm_W), N.ptr(self._glm_Z),
                                                N.ptr(self._glm_P), self._glm_out), "bpgl_panel_glm_model")
        out = np.array(self._glm_out, dtype=np.float64).reshape(k, 8)
        res = {key: out[:, i].copy() for i, key in enumerate(self.GLM_KEYS)}
        off = self.stat("glm_ax_offset") + (self._scratch.data_ptr() + 255) // 256 * 256 - self._scratch.data_ptr()
        res.update(W=self._glm_W, Z=self._glm_Z, P=self._glm_P, beta0=self._glm_b0,
                   AX=self._scratch[off // 8: off // 8 + k * m].view(k, m))
        return res

    def glm_dual(self, scale):
        """(k,) D = -sum om Nh(s p + (1 - s) y) of the last ``glm_model``'s p, labels and weights at the dual scaling
        ``scale`` (k,) -- ``duality_gap()['scale']`` right after the inner reset (bpgl_panel_glm_dual)."""
        k = self.nrhs
        sc = (ctypes.c_double * k)(*np.broadcast_to(np.asarray(scale, dtype=np.float64), (k,)))
        out = (ctypes.c_double * k)()
        with self._on_stream():
            N.check(_lib().bpgl_panel_glm_dual(self._ctx, N.ptr(self._glm_P), N.ptr(self._glm_Y), N.ptr(self._glm_Om),
                                               sc, out), "bpgl_panel_glm_dual")
        return np.array(out, dtype=np.float64)

    def solver_step(self, n_iter):
        with self._on_stream():
            N.check(_lib().bpgl_panel_step(self._ctx, int(n_iter)), "bpgl_panel_step")

    def solver_status(self):
        it, err = ctypes.c_int64(), ctypes.c_double()
        N.check(_lib().bpgl_panel_status(self._ctx, ctypes.byref(it), ctypes.byref(err)), "bpgl_panel_status")
        return dict(iters=it.value, err=err.value)

    def solver_x_device(self):
        """(k, n) fp32 view of the iterates (row j = right-hand side j)."""
        addr = _lib().bpgl_panel_x(self._ctx)
        off = (addr - self._scratch.data_ptr())
        assert off % 4 == 0
        flat = self._scratch.view(torch.float32)[off // 4: off // 4 + self.Block * self.nrhs * self.MAT_WIDTH]
        return flat.view(self.Block, self.nrhs, self.MAT_WIDTH).permute(1, 0, 2).reshape(self.nrhs, -1)

    def solver_x(self):
        self.stream.synchronize()
        return self.solver_x_device().to(torch.float64).cpu().numpy().T.copy()   # (n, k)

    def set_tuning(self, key, value):
        """Speed-only knobs (bitwise-identical results): 'interleave1' / 'interleave2' / 'interleave'
        0-2 (the mainloop form; default: the measured best per pass); 'defer_x' 0 / 1 (default 1, one
        block: where x += gamma D' is applied; a reset must follow).

        Knobs that change the arithmetic (each an exact line search along the direction taken; the
        accuracy of each against the oracle is in the module docstring): 'd_split' 1 (default) / 2 --
        the direction as its bf16 rounding or a hi + lo pair; 'carry_g' 1 (default, one block) / 0 --
        the carried fp32 gradient or the exact A^T R product every iteration; 'g_refresh' (default 64,
        a multiple of 8) -- the carried gradient's exact recompute period (include/bpgl.h)."""
        N.check(_lib().bpgl_panel_set_tuning(self._ctx, key.encode(), int(value)), "bpgl_panel_set_tuning")

    def get_tuning(self, key):
        v = ctypes.c_int64()
        N.check(_lib().bpgl_panel_get_tuning(self._ctx, key.encode(), ctypes.byref(v)), "bpgl_panel_get_tuning")
        return v.value

    def stat(self, key):
        """Counter since the last reset: "iters_enqueued", "exact_gradients"; of the last duality_gap,
        its two products' device times: "gap_prod1_ns", "gap_prod2_ns"."""
        v = ctypes.c_int64()
        N.check(_lib().bpgl_panel_stat(self._ctx, key.encode(), ctypes.byref(v)), "bpgl_panel_stat")
        return v.value

    def residual_device(self):
        """(k, m) fp64 device view of the solver's residual R = A X - B (drain the stream first)."""
        addr = _lib().bpgl_panel_residual(self._ctx)
        off = addr - self._scratch.data_ptr()
        assert off % 8 == 0
        return self._scratch[off // 8: off // 8 + self.nrhs * self.MAT_HEIGHT].view(self.nrhs, self.MAT_HEIGHT)

    GAP_KEYS = ("primal", "dual", "gap", "scale", "gnorm_inf", "n_keep", "drift")

    def duality_gap(self, screen=True):
        """Per-RHS optimality certificate of the stored fp32 x (include/bpgl.h bpgl_panel_gap): a dict of
        (k,) numpy arrays primal, dual, gap, scale, gnorm_inf, n_keep (int64), drift, and the device
        tensors g (k, n) fp64 = A^T r, r (k, m) fp64 = A x - b recomputed from x, keep (k, n) bool
        (None when ``screen`` is false; n_keep is then n).  drift is max |solver residual - r| per RHS.
        Also holdout_sse (k,): with a row mask the sum of squared errors over each column's held-out
        rows (everything else then describes the masked problem), zero without one; and intercept (k,):
        with ``set_intercept`` each column's beta0 = -mean over its in-rows of (A x - b) (everything else
        then describes the profiled problem, holdout_sse includes beta0), zero without it.
        Read-only for the solve and bitwise repeatable.  The tensors are views of buffers the next call
        overwrites (g is a copy when there is more than one feature block)."""
        k, n, m = self.nrhs, self.MAT_WIDTH_ALL, self.MAT_HEIGHT
        if getattr(self, "_gap_g", None) is None:
            self._gap_g = torch.empty((self.Block, k, self.MAT_WIDTH), dtype=torch.float64, device=self.device)
            self._gap_r = torch.empty((k, m), dtype=torch.float64, device=self.device)
            self._gap_keep = torch.empty((k, n), dtype=torch.uint8, device=self.device)
            self._gap_out = (ctypes.c_double * (8 * k))()
        with self._on_stream():
            N.check(_lib().bpgl_panel_gap(self._ctx, N.ptr(self._gap_g), N.ptr(self._gap_r),
                                          N.ptr(self._gap_keep) if screen else None, self._gap_out),
                    "bpgl_panel_gap")
        out = np.array(self._gap_out, dtype=np.float64).reshape(k, 8)
        res = {key: out[:, i].copy() for i, key in enumerate(self.GAP_KEYS)}
        res["n_keep"] = res["n_keep"].astype(np.int64)
        res["holdout_sse"] = out[:, 7].copy()
        b0 = (ctypes.c_double * k)()
        N.check(_lib().bpgl_panel_intercept(self._ctx, b0), "bpgl_panel_intercept")
        res["intercept"] = np.array(b0, dtype=np.float64)
        res["g"] = self._gap_g.permute(1, 0, 2).reshape(k, n)
        res["r"] = self._gap_r
        res["keep"] = self._gap_keep.view(torch.bool) if screen else None
        return res

    def set_kernel_timing(self, enable):
        N.check(_lib().bpgl_panel_set_kernel_timing(self._ctx, int(bool(enable))), "bpgl_panel_set_kernel_timing")

    def kernel_times(self):
        arr = (ctypes.c_double * 5)()
        ns = ctypes.c_int64()
        N.check(_lib().bpgl_panel_kernel_times(self._ctx, arr, ctypes.byref(ns)), "bpgl_panel_kernel_times")
        return dict(zip(self.KERNEL_KINDS, list(arr))), ns.value

    def run(self, B, mu, iters, record=False, use_graph=True):
        """Returns dict(x (n, k) fp64 copy of the fp32 iterates, iters, err[, err_iter])."""
        self.solver_reset(B, mu, record_len=int(iters) if record else 0, use_graph=use_graph)
        self.solver_step(int(iters))
        out = self.solver_status()
        out["x"] = self.solver_x()
        if record:
            self.stream.synchronize()
            out["err_iter"] = self._err_iter.cpu().numpy().copy()
        return out


PANEL_NRHS = (16, 32, 64, 128)
# the certificate's outputs that scale with the objective (``sample_weight``: the library solves the problem / max omega)
_SCALED_KEYS = ("primal", "dual", "gap", "gnorm_inf")
# lasso_path's default: the smallest multiple of 64 iterations at which one certificate costs at most
# 10 % of the iterations between two of them, measured at 8192 x 65536, k = 128
PATH_CHECK_EVERY = 192


def pad_mus(mus):
    """(padded grid, number given): 1 <= len(mus) <= 128 values of mu padded to the next panel width
    (16, 32, 64 or 128) by repeating the largest given one, so the pad columns are duplicates of a
    real problem.  More than 128 raise ValueError."""
    mus = np.asarray(mus, dtype=np.float64).reshape(-1)
    if not 1 <= mus.size <= PANEL_NRHS[-1]:
        raise ValueError(f"lasso_path takes 1 to {PANEL_NRHS[-1]} values of mu (got {mus.size})")
    k = next(v for v in PANEL_NRHS if v >= mus.size)
    return np.concatenate([mus, np.full(k - mus.size, mus.max())]), int(mus.size)


def _check_loop(pl, target, ITER_MAX, check_every):
    """The drivers' loop on a freshly reset ``pl``: ``check_every`` iterations, then a certificate, until
    every column has gap <= target (a scalar or one per column) or ITER_MAX iterations have run.
    Returns (iterations run, the last certificate, per column the iteration of the first check at
    which it met its target, else -1)."""
    first = np.full(pl.nrhs, -1, dtype=np.int64)
    t, cert = 0, None
    while t < int(ITER_MAX):
        step = min(int(check_every), int(ITER_MAX) - t)
        pl.solver_step(step)
        t += step
        cert = pl.duality_gap(screen=True)
        ok = cert["gap"] <= target
        first[ok & (first < 0)] = t
        if ok.all():
            break
    if cert is None:
        cert = pl.duality_gap(screen=True)
    return t, cert, first


def _check_penalty(p, n):
    """``p`` as a contiguous fp64 numpy vector of length ``n``, every entry finite and > 0 (ValueError otherwise);
    None stays None.  Needs no GPU."""
    if p is None:
        return None
    pen = np.array(p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else p, dtype=np.float64)   # a copy
    if pen.ndim != 1 or pen.size != int(n):
        raise ValueError(f"penalty factors must be a vector of length n = {int(n)}, got shape {pen.shape}")
    if not np.all(np.isfinite(pen) & (pen > 0.0)):
        raise ValueError("every penalty factor must be finite and > 0 (an unpenalised or an excluded column is "
                         "not a penalty factor: DESIGN.md section 15)")
    return pen


def _check_row_weights(v, m, k, what, upper):
    """``v``, (m, k) or (m,), as a contiguous fp64 numpy array [k][m], every entry finite and in [0, ``upper``]
    (ValueError otherwise); None stays None.  Needs no GPU."""
    if v is None:
        return None
    a = np.array(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64)   # a copy
    if a.shape == (int(m),):
        a = np.repeat(a[:, None], int(k), axis=1)
    if a.shape != (int(m), int(k)):
        raise ValueError(f"{what} must be (m, k) = ({int(m)}, {int(k)}) or (m,), got {a.shape}")
    if not np.all(np.isfinite(a) & (a >= 0.0) & (a <= upper)):
        raise ValueError(f"every entry of {what} must be finite and " + ("in [0, 1]" if upper == 1.0 else ">= 0"))
    return np.ascontiguousarray(a.T)


def _check_sample_weight(sw, m, Block):
    """``sample_weight`` of the drivers as an fp64 vector (m,): finite, >= 0, not all zero, and Block = 1
    (ValueError otherwise); None stays None."""
    if sw is None:
        return None
    om = np.array(sw.detach().cpu().numpy() if isinstance(sw, torch.Tensor) else sw, dtype=np.float64).reshape(-1)
    if om.size != int(m):
        raise ValueError(f"sample_weight must have m = {int(m)} entries, got {om.size}")
    if not np.all(np.isfinite(om) & (om >= 0.0)) or not np.any(om > 0.0):
        raise ValueError("every sample weight must be finite and >= 0, and not all of them zero")
    if int(Block) != 1:
        raise ValueError("sample_weight needs Block = 1")
    return om


def _check_shrink(shrink):
    if not 0.0 <= float(shrink) < 1.0:
        raise ValueError("shrink must lie in [0, 1)")
    return float(shrink)


def _grid_below(mu_max, n_mus, hi, lo, positive):
    """``mu_grid`` below the mu_max read off the x = 0 certificate, for every path and CV run.  With ``positive``
    mu_max is max_j (a_j . b)+, and 0 means that no column correlates positively with b: x = 0 solves every
    mu > 0, and a grid of zeros would be built -- ValueError instead.  (A NaN mu_max is passed on, as without the
    flag: it is not this condition.)"""
    from .cpu_calculation import mu_grid
    if positive and float(mu_max) <= 0.0:
        raise ValueError("positive=True: no column of A correlates positively with b (mu_max = 0); "
                         "x = 0 is the solution for every mu")
    return mu_grid(float(mu_max), n_mus, hi, lo)


def _screened_loop(pl, B, mu, target, ITER_MAX, check_every, shrink, mask=None, intercept=False, positive=False,
                   penalty=None, weights=None):
    """``_check_loop`` on a freshly reset ``pl`` (reset with ``B``, ``mu``; ``mask``: the (m, k) row mask
    installed on it, or None) with gap-safe compaction, ``ClassLassoScreened``'s rule on a panel: after
    a check that did not stop the loop, the union over the panel's columns of the screen's keep goes
    through ``cpu_calculation.compaction_columns`` with q = Block * 256; when that leaves at most
    ``shrink`` times the active columns, they are gathered (``gather_columns``), a new ``PanelLasso`` of
    the same Block and width is built over them, the mask (and, with ``intercept`` / ``positive``, the
    intercept / the sign constraint, which ``pl`` then has on too) installed there, and the solve continues
    from ``solver_reset(B, mu, x0=X[sel])``.  ``pl`` stays alive; an earlier narrow context is dropped.
    ``penalty``: the (n,) penalty factors installed on ``pl`` (or None); a narrower context gets them gathered with
    the same columns.  ``weights``: the (weights, holdout) pair installed on ``pl`` with ``set_row_weights`` (or None;
    never with ``mask``); a narrower context gets the same pair.

    Returns dict(t, cert, first, reached, x (n, k), active, compactions [(t, n_active after)],
    compact_seconds).  ``reached`` is the loop's own verdict.  After a compaction ``cert`` is one
    ``duality_gap(screen=False)`` on ``pl`` itself, reset (mask still installed) at x scattered back
    to (n, k) with zeros outside ``active``: the dropped columns need not be dual-feasible for the
    compacted problem's dual point.  ``shrink=0`` is ``_check_loop`` and ``pl.solver_x()``, nothing else."""
    from .cpu_calculation import compaction_columns
    n, k = pl.MAT_WIDTH_ALL, pl.nrhs
    active = np.arange(n, dtype=np.int64)
    if shrink == 0.0:
        t, cert, first = _check_loop(pl, target, ITER_MAX, check_every)
        return dict(t=t, cert=cert, first=first, reached=cert["gap"] <= target, x=pl.solver_x(), active=active,
                    compactions=[], compact_seconds=0.0)
    q = pl.Block * 256
    first = np.full(k, -1, dtype=np.int64)
    cur, t, cert, compactions, seconds = pl, 0, None, [], 0.0
    while t < int(ITER_MAX):
        step = min(int(check_every), int(ITER_MAX) - t)
        cur.solver_step(step)
        t += step
        cert = cur.duality_gap(screen=True)
        ok = cert["gap"] <= target
        first[ok & (first < 0)] = t
        if ok.all() or t >= int(ITER_MAX):
            break
        sel = compaction_columns(cert["keep"].any(dim=0).cpu().numpy(), q)
        if sel.size <= shrink * active.size:
            t0 = time.time()
            sel_d = torch.from_numpy(sel).to(cur.device)
            x0 = cur.solver_x_device()[:, sel_d].clone()          # (k, n_new) fp32
            nxt = PanelLasso(cur.gather_columns(sel_d), pl.Block, nrhs=k, device=pl.device)
            if intercept:
                nxt.set_intercept(True)
            if positive:
                nxt.set_positive(True)
            if penalty is not None:
                nxt.set_penalty_factors(penalty[active[sel]])
            if mask is not None:
                nxt.set_row_mask(mask)
            if weights is not None:
                nxt.set_row_weights(*weights)
            nxt.solver_reset(B, mu, x0=x0)
            nxt.stream.synchronize()
            cur, active = nxt, active[sel]                        # a narrow `cur` is released here
            compactions.append((t, int(active.size)))
            seconds += time.time() - t0
    if cert is None:
        cert = cur.duality_gap(screen=True)
    reached = cert["gap"] <= target
    x = cur.solver_x()
    if compactions:
        x_full = np.zeros((n, k))
        x_full[active] = x
        x = x_full
        del cur
        pl.solver_reset(B, mu, use_graph=False, x0=x)
        cert = pl.duality_gap(screen=False)
    return dict(t=t, cert=cert, first=first, reached=reached, x=x, active=active, compactions=compactions,
                compact_seconds=seconds)


def lasso_path(A, b, mus=None, n_mus=16, hi=0.9, lo=0.1, Block=1, GAP_BOUND=1e-4, ITER_MAX=4096,
               check_every=PATH_CHECK_EVERY, device=None, x0=None, shrink=0.0, fit_intercept=False, positive=False,
               penalty_factors=None, sample_weight=None):
    """A regularization path as ONE panel: min 1/2 ||A x - b||^2 + mu ||x||_1 for every mu of a grid,
    on the bf16-stored A, every column of the panel holding the same b.

    ``mus``: 1 to 128 values (ValueError above that), padded to the next panel width by repeating the
    largest; the pad columns are dropped from every output.  ``mus=None``: mu_max = ||A^T b||_inf for
    the stored bf16 A, read off a certificate taken right after a reset (x = 0, so gnorm_inf is
    mu_max), then ``cpu_calculation.mu_grid(mu_max, n_mus, hi, lo)`` and a second reset.

    The loop runs ``check_every`` iterations (block updates), then ``PanelLasso.duality_gap``; it
    stops at the first check where every mu has gap <= GAP_BOUND * 1/2 ||b||^2 (ClassLassoScreened's
    criterion), or after ITER_MAX iterations; all mu run until the slowest is done.  GAP_BOUND below
    about 1e-6 is out of reach of the fp32 x.

    By default every mu starts at x = 0 and the panel keeps its width.  Opt-in:
    ``x0``, an (n, len(mus)) array, starts every mu at the given point (only with ``mus`` given,
    ValueError otherwise; the pad columns take the column of the largest mu).  ``shrink`` in [0, 1)
    (ValueError outside) compacts the panel as it runs (``_screened_loop``); 0 disables it.

    Returns a dict: x (n, len(mus)), mus, mu_max (None when mus was given), iters, reached (bool per
    mu), first_reached (the iteration of the first check at which that mu met the bound, else -1), and
    the last certificate's primal, dual, gap, scale, gnorm_inf, n_keep, drift per mu (after a
    compaction: of the final x on the full A, n_keep = n); active (the original indices still active
    at the end, arange(n) without compaction), compactions (a list of (t, n_active after)) and
    compact_seconds (gather, the new context, its reset and graph capture).

    ``fit_intercept`` (``Block`` must be 1, ValueError otherwise): every mu solves
    min over x, beta0 of 1/2 ||A x + beta0 - b||^2 + mu ||x||_1 (``PanelLasso.set_intercept``, also on
    every narrower context of ``shrink``).  mu_max is then ||A^T (b - mean b)||_inf, the bound
    GAP_BOUND * 1/2 ||b - mean b||^2, and ``intercept`` (len(mus),) is returned (zeros without it).

    ``positive``: every mu solves the problem subject to x >= 0
    (``PanelLasso.set_positive``, also on every narrower context of ``shrink``); the returned x is >= 0
    elementwise, an ``x0`` is projected to max(x0, 0), and with ``mus=None`` mu_max is max_j (a_j . b)+
    (ValueError when that is 0: no column correlates positively with b).

    ``penalty_factors``: an (n,) vector p, every entry finite and > 0 (ValueError
    otherwise); every mu solves min 1/2 ||A x - b||^2 + mu sum_j p_j |x_j| (``PanelLasso.set_penalty_factors``,
    on every narrower context of ``shrink`` gathered with its columns).  Used as given, not renormalised.  With
    ``mus=None`` mu_max is max_j |a_j . b| / p_j.

    ``sample_weight`` (``Block`` must be 1): an (m,) vector omega, every entry finite and >= 0
    and not all zero (ValueError otherwise); every mu solves min 1/2 sum_i omega_i e_i^2 + mu sum_j p_j |x_j| with
    e_i = a_i . x - b_i (+ beta0 with ``fit_intercept``, then profiled over the weighted mean).  omega is used as
    given -- no renormalisation to sum omega = m.  Internally c = max omega, w = omega / c and mu / c go to
    ``PanelLasso.set_row_weights`` (also on every narrower context of ``shrink``); ``mus``, mu_max, primal, dual, gap,
    gnorm_inf and the bound GAP_BOUND * 1/2 sum omega b^2 (b centred over the weighted mean with ``fit_intercept``)
    are in the caller's scale."""
    penalty = _check_penalty(penalty_factors, int(A.shape[1]))
    omega = _check_sample_weight(sample_weight, int(A.shape[0]), Block)
    if int(check_every) <= 0:
        raise ValueError("check_every must be > 0")
    shrink = _check_shrink(shrink)
    if fit_intercept and int(Block) != 1:
        raise ValueError("fit_intercept needs Block = 1")
    if x0 is not None and mus is None:
        raise ValueError("x0 needs mus: the grid the columns of x0 belong to")
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float64).reshape(-1)
    if x0 is not None:
        x0 = np.asarray(x0.detach().cpu() if isinstance(x0, torch.Tensor) else x0, dtype=np.float64)
        want = (int(A.shape[1]), int(np.asarray(mus).size))
        if x0.shape != want:
            raise ValueError(f"x0 must be (n, len(mus)) = {want}, got {x0.shape}")
    if mus is None:
        if not 1 <= int(n_mus) <= PANEL_NRHS[-1]:
            raise ValueError(f"lasso_path takes 1 to {PANEL_NRHS[-1]} values of mu (got {n_mus})")
        grid, n_given = None, int(n_mus)
        k = next(v for v in PANEL_NRHS if v >= n_given)
    else:
        grid, n_given = pad_mus(mus)
        k = grid.size
    pl = PanelLasso(A, Block, nrhs=k, device=device)
    if fit_intercept:
        pl.set_intercept(True)
    if positive:
        pl.set_positive(True)
    if penalty is not None:
        pl.set_penalty_factors(penalty)
    # sample weights: the library solves the problem divided by c = max omega (w = omega / c in [0, 1], mu / c); `grid`
    # and every returned scalar stay in the caller's scale
    cw = 1.0 if omega is None else float(omega.max())
    weights = None if omega is None else (omega / cw, None)
    if weights is not None:
        pl.set_row_weights(*weights)
    B = np.repeat(b[:, None], k, axis=1)
    mu_max = None
    if grid is None:
        pl.solver_reset(B, 1.0)
        mu_max = cw * float(pl.duality_gap(screen=False)["gnorm_inf"][0])
        grid, _ = pad_mus(_grid_below(mu_max, n_given, hi, lo, positive))
    if x0 is None:
        pl.solver_reset(B, grid / cw)
    else:
        pad = np.repeat(x0[:, [int(np.argmax(grid[:n_given]))]], k - n_given, axis=1)
        pl.solver_reset(B, grid / cw, x0=np.concatenate([x0, pad], axis=1))
    if omega is None:
        bc = b - b.mean() if fit_intercept else b
        target = float(GAP_BOUND) * 0.5 * float(bc @ bc)
    else:
        bc = b - float(omega @ b) / float(omega.sum()) if fit_intercept else b
        target = float(GAP_BOUND) * 0.5 * float(omega @ (bc * bc))
    run = _screened_loop(pl, B, grid / cw, target / cw, ITER_MAX, check_every, shrink, intercept=bool(fit_intercept),
                         positive=bool(positive), penalty=penalty, weights=weights)
    cert = run["cert"]
    out = dict(x=run["x"][:, :n_given], mus=grid[:n_given].copy(), mu_max=mu_max, iters=run["t"],
               reached=run["reached"][:n_given], first_reached=run["first"][:n_given])
    for key in PanelLasso.GAP_KEYS:
        out[key] = cert[key][:n_given] * cw if key in _SCALED_KEYS else cert[key][:n_given]
    out["intercept"] = cert["intercept"][:n_given]
    out.update(active=run["active"], compactions=run["compactions"], compact_seconds=run["compact_seconds"])
    return out


def lasso_cv(A, b, n_folds=8, mus=None, n_mus=16, hi=0.9, lo=0.1, Block=1, GAP_BOUND=1e-4, ITER_MAX=4096,
             check_every=PATH_CHECK_EVERY, seed=0, masks=None, refit=True, return_x=False, device=None,
             shrink=0.0, warm_refit=False, fit_intercept=False, positive=False, penalty_factors=None,
             sample_weight=None):
    """K-fold cross-validation over a grid of mu as ONE panel on one bound A: column c = f * n_mus + j
    solves fold f (the rows of ``masks[f]``) at ``mus[j]``, min 1/2 ||w_f o (A x - b)||^2 + mu_j ||x||_1,
    through ``PanelLasso.set_row_mask``.  n_folds * n_mus <= 128 and n_folds >= 2 (ValueError
    otherwise); the panel is padded to the next width (16, 32, 64, 128) with copies of column 0, which
    are dropped from every output.

    ``masks``: (n_folds, m) 0/1, 0 = held out (default ``cpu_calculation.kfold_masks(m, n_folds, seed)``;
    when given, n_folds is its row count).  One grid serves all folds: ``mus``, or with ``mus=None``
    ``mu_grid(mu_max, n_mus, hi, lo)`` with mu_max = ||A^T b||_inf of the full data, read off an unmasked
    certificate at x = 0 as ``lasso_path`` does.

    The loop is ``lasso_path``'s: ``check_every`` iterations, then a certificate; it stops when every
    column has gap <= GAP_BOUND * 1/2 ||w_f o b||^2, or after ITER_MAX iterations.

    Returns a dict: mus; mse (n_folds, n_mus) = held-out sum of squares / held-out count; mean_mse and
    se_mse (n_mus,), the mean over folds and its standard error; best = argmin mean_mse; best_1se = the
    index of the largest mu whose mean_mse is <= the minimum + its standard error; iters; reached, gap
    and n_keep (n_folds, n_mus) from the last certificate; masks.  ``return_x``: also x_folds
    (n, n_folds, n_mus).  ``refit``: the mask is cleared on the SAME context (A stays bound) and the
    full-data path on the grid is solved by the same loop, as ``lasso_path`` pads and stops it: x
    (n, n_mus), refit_gap (n_mus,) and refit_iters.

    Opt-in: ``shrink`` in [0, 1) compacts the panel as ``lasso_path`` does, in the
    fold solve and in the refit, the mask installed on every narrower context; mse, gap and n_keep then
    come from the certificate of the final x on the full A.  Also returned: active, compactions,
    compact_seconds of the fold solve (and refit_compactions).  ``warm_refit``: the refit starts each mu
    from the mean over folds of that mu's fold solutions instead of from 0.

    ``fit_intercept`` (``Block`` must be 1, ValueError otherwise): every column also
    fits an unpenalised intercept, centred over the training rows of ITS fold inside the panel
    (``PanelLasso.set_intercept``); the refit and every narrower context of ``shrink`` get it too.  mu_max
    is then ||A^T (b - mean b)||_inf, the bound GAP_BOUND * 1/2 ||P_w b||^2 (b centred over the fold's
    training rows), mse scores a_i . x + beta0 against b_i, and ``intercept_folds`` (n_folds, n_mus) and,
    with ``refit``, ``intercept`` (n_mus,) are returned.

    ``positive``: every column solves its fold subject to x >= 0
    (``PanelLasso.set_positive``); the refit and every narrower context of ``shrink`` get it too, the
    ``warm_refit`` start (a mean of non-negative solutions) is non-negative, and with ``mus=None`` mu_max is
    max_j (a_j . b)+ (ValueError when that is 0).

    ``penalty_factors``: an (n,) vector p, every entry finite and > 0 (ValueError
    otherwise), shared by every fold: each column solves its fold with the penalty mu sum_j p_j |x_j|
    (``PanelLasso.set_penalty_factors``); the refit and every narrower context of ``shrink`` get it too.  Used as
    given, not renormalised.  With ``mus=None`` mu_max is max_j |a_j . b| / p_j.

    ``sample_weight`` (``Block`` must be 1): an (m,) vector omega, finite, >= 0, not all zero
    (ValueError otherwise), used as given.  Column (f, j) solves min 1/2 sum_i fold_f(i) omega_i e_i^2 + mu_j sum p |x|
    through ``PanelLasso.set_row_weights`` -- weights fold_f(i) omega_i / c with c = max omega and mu_j / c, scoring
    weights (1 - fold_f(i)) omega_i -- instead of the row mask; mse is sum h e^2 / sum h per fold, the bound
    GAP_BOUND * 1/2 sum fold_f omega b^2 (b centred over the fold's weighted mean with ``fit_intercept``), and
    ``mus``, mu_max and gap are in the caller's scale.  The refit runs with the weights omega / c and no mask."""
    from .cpu_calculation import kfold_masks
    penalty = _check_penalty(penalty_factors, int(A.shape[1]))
    omega = _check_sample_weight(sample_weight, int(A.shape[0]), Block)
    if int(check_every) <= 0:
        raise ValueError("check_every must be > 0")
    shrink = _check_shrink(shrink)
    if fit_intercept and int(Block) != 1:
        raise ValueError("fit_intercept needs Block = 1")
    fit_intercept = bool(fit_intercept)
    b = np.asarray(b.detach().cpu() if isinstance(b, torch.Tensor) else b, dtype=np.float64).reshape(-1)
    m = b.size
    if masks is not None:
        masks = (np.asarray(masks.detach().cpu() if isinstance(masks, torch.Tensor) else masks) != 0).astype(np.uint8)
        if masks.ndim != 2 or masks.shape[1] != m:
            raise ValueError(f"masks must be (n_folds, m = {m})")
        n_folds = masks.shape[0]
    n_folds = int(n_folds)
    if n_folds < 2:
        raise ValueError(f"lasso_cv needs n_folds >= 2 (got {n_folds})")
    if mus is not None:
        mus = np.asarray(mus, dtype=np.float64).reshape(-1).copy()
        n_mus = mus.size
    n_mus = int(n_mus)
    ncol = n_folds * n_mus
    if n_mus < 1 or ncol > PANEL_NRHS[-1]:
        raise ValueError(f"lasso_cv takes n_folds * n_mus between 2 and {PANEL_NRHS[-1]} (got {n_folds} x {n_mus})")
    if masks is None:
        masks = kfold_masks(m, n_folds, seed)
    k = next(v for v in PANEL_NRHS if v >= ncol)
    pl = PanelLasso(A, Block, nrhs=k, device=device)
    if fit_intercept:
        pl.set_intercept(True)
    positive = bool(positive)
    if positive:
        pl.set_positive(True)
    if penalty is not None:
        pl.set_penalty_factors(penalty)
    B = np.repeat(b[:, None], k, axis=1)
    # sample weights: the library solves every column divided by c = max omega; `mus` stays in the caller's scale
    cw = 1.0 if omega is None else float(omega.max())
    if omega is not None:
        pl.set_row_weights(omega / cw)
    if mus is None:
        pl.solver_reset(B, 1.0)
        mus = _grid_below(cw * float(pl.duality_gap(screen=False)["gnorm_inf"][0]), n_mus, hi, lo, positive)
    cols = np.concatenate([np.arange(ncol), np.zeros(k - ncol, dtype=np.int64)])   # the pad: copies of column 0
    fold, jmu = cols // n_mus, cols % n_mus
    if omega is None:
        weights = None
        pl.set_row_mask(masks[fold].T)
        def centred(wf, v):   # w o v, or P_w v with the intercept
            return wf * (v - (wf @ v) / wf.sum()) if fit_intercept else wf * v
        bb = np.array([float(centred(masks[f].astype(np.float64), b) @ centred(masks[f].astype(np.float64), b))
                       for f in range(n_folds)])
        count = (masks == 0).sum(axis=1).astype(np.float64)
    else:
        wf = masks.astype(np.float64) * omega                     # (n_folds, m): the fold's training weights
        hf = (1.0 - masks.astype(np.float64)) * omega             # ... and its scoring weights
        if not np.all(wf.sum(axis=1) > 0.0):
            raise ValueError("sample_weight leaves a fold without a training row of positive weight")
        weights = (np.ascontiguousarray((wf / cw)[fold].T), np.ascontiguousarray(hf[fold].T))
        pl.set_row_weights(*weights)
        def wss(wv, v):   # sum w v^2, v centred over the weighted mean with the intercept
            vc = v - (wv @ v) / wv.sum() if fit_intercept else v
            return float(wv @ (vc * vc))
        bb = np.array([wss(wf[f], b) for f in range(n_folds)])
        count = hf.sum(axis=1)
    pl.solver_reset(B, mus[jmu] / cw)
    run = _screened_loop(pl, B, mus[jmu] / cw, float(GAP_BOUND) * 0.5 * bb[fold] / cw, ITER_MAX, check_every, shrink,
                         mask=None if omega is not None else masks[fold].T, intercept=fit_intercept, positive=positive,
                         penalty=penalty, weights=weights)
    t, cert = run["t"], run["cert"]
    shape = (n_folds, n_mus)
    mse = cert["holdout_sse"][:ncol].reshape(shape) / count[:, None]
    mean_mse = mse.mean(axis=0)
    se_mse = mse.std(axis=0, ddof=1) / np.sqrt(n_folds)
    best = int(np.argmin(mean_mse))
    within = np.flatnonzero(mean_mse <= mean_mse[best] + se_mse[best])
    out = dict(mus=mus.copy(), mse=mse, mean_mse=mean_mse, se_mse=se_mse, best=best,
               best_1se=int(within[np.argmax(mus[within])]), iters=t,
               reached=run["reached"][:ncol].reshape(shape),
               gap=cert["gap"][:ncol].reshape(shape) * cw, n_keep=cert["n_keep"][:ncol].reshape(shape), masks=masks,
               active=run["active"], compactions=run["compactions"], compact_seconds=run["compact_seconds"])
    if fit_intercept:
        out["intercept_folds"] = cert["intercept"][:ncol].reshape(shape)
    if return_x:
        out["x_folds"] = run["x"][:, :ncol].reshape(-1, n_folds, n_mus)
    if refit:
        grid = np.concatenate([mus, np.full(k - n_mus, mus.max())])   # pad_mus' layout at this panel's width
        if omega is None:
            pl.set_row_mask(None)
            rweights = None
        else:   # the full-data weights, no mask
            rweights = (omega / cw, None)
            pl.set_row_weights(*rweights)
        if warm_refit:   # each mu from the mean of its fold solutions; the pad takes the largest mu's column
            xm = run["x"][:, :ncol].reshape(-1, n_folds, n_mus).mean(axis=1)
            xm = np.concatenate([xm, np.repeat(xm[:, [int(np.argmax(mus))]], k - n_mus, axis=1)], axis=1)
            pl.solver_reset(B, grid / cw, x0=xm)
        else:
            pl.solver_reset(B, grid / cw)
        if omega is None:
            bc = b - b.mean() if fit_intercept else b
            rtarget = float(GAP_BOUND) * 0.5 * float(bc @ bc)
        else:
            bc = b - float(omega @ b) / float(omega.sum()) if fit_intercept else b
            rtarget = float(GAP_BOUND) * 0.5 * float(omega @ (bc * bc))
        rrun = _screened_loop(pl, B, grid / cw, rtarget / cw, ITER_MAX, check_every, shrink,
                              intercept=fit_intercept, positive=positive, penalty=penalty, weights=rweights)
        out.update(x=rrun["x"][:, :n_mus], refit_gap=rrun["cert"]["gap"][:n_mus] * cw, refit_iters=rrun["t"],
                   refit_compactions=rrun["compactions"])
        if fit_intercept:
            out["intercept"] = rrun["cert"]["intercept"][:n_mus]
    return out


# ---------------------------------------------------------------------------
# Logistic lasso: IRLS on the weighted panel.  The outer step is PanelLasso.glm_model, the inner
# solve the weighted lasso of section 16 on the working weights and response, the stopping rule the logistic
# certificate (PanelLasso.glm_dual at the inner certificate's scale).
# ---------------------------------------------------------------------------
# defaults of the drivers: `inner_iters` iterations between two outer steps, the inner reset with graph capture
LOGISTIC_INNER_ITERS = 64
LOGISTIC_USE_GRAPH = True
LOGISTIC_OUTER_MAX = 256


def _check_labels(y, m):
    """``y`` as an fp64 vector (m,), every entry in [0, 1] (ValueError otherwise).  Needs no GPU."""
    yv = np.array(y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else y, dtype=np.float64).reshape(-1)
    if yv.size != int(m):
        raise ValueError(f"y must have m = {int(m)} entries, got {yv.size}")
    if not np.all(np.isfinite(yv) & (yv >= 0.0) & (yv <= 1.0)):
        raise ValueError("every label must lie in [0, 1]")
    return yv


def _check_two_classes(w, yv, what):
    """ValueError when the weighted labels of ``w`` (n_sets, m) are all one class in a set: sum w y = 0 or = sum w, so
    the intercept has no finite root (and without it nothing can be learnt from that set)."""
    sy, sw = w @ yv, w.sum(axis=1)
    bad = np.flatnonzero(~((sy > 0.0) & (sy < sw)))
    if bad.size:
        raise ValueError(f"{what} {int(bad[0])}: the weighted labels are all one class (sum w y = {sy[bad[0]]:g}, "
                         f"sum w = {sw[bad[0]]:g})")


def _logistic_setup(A, y, Block, penalty_factors, sample_weight):
    """The drivers' host-side checks, before any device work: (penalty, labels, omega or ones)."""
    m, n = int(A.shape[0]), int(A.shape[1])
    if int(Block) != 1:
        raise ValueError("the logistic drivers need Block = 1")
    penalty = _check_penalty(penalty_factors, n)
    yv = _check_labels(y, m)
    omega = _check_sample_weight(sample_weight, m, 1)
    return penalty, yv, np.ones(m) if omega is None else omega


def _logistic_context(A, k, device, fit_intercept, positive, penalty):
    pl = PanelLasso(A, 1, nrhs=k, device=device)
    if fit_intercept:
        pl.set_intercept(True)
    if positive:
        pl.set_positive(True)
    if penalty is not None:
        pl.set_penalty_factors(penalty)
    return pl


def _rows_device(pl, v):
    """(k, m) numpy -> contiguous device fp64 [k][m]."""
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(pl.device)


def _logistic_mu_max(pl, Yd, Omd):
    """mu_max of column 0, read off the x = 0 model: right after the inner reset the certificate's g is 4 A^T (om o (p -
    y)), so gnorm_inf / 4 is max_j |a_j . (om o (p - y))| / p_j (one-sided with ``positive``)."""
    pl.set_row_weights(None)
    pl.solver_reset(np.zeros((pl.MAT_HEIGHT, pl.nrhs)), 1.0, use_graph=False)
    mod = pl.glm_model(Yd, Omd)
    pl.set_row_weights_device(mod["W"])
    pl.solver_reset(mod["Z"].t(), 1.0, use_graph=False, x0=pl.solver_x_device())
    return float(pl.duality_gap(screen=False)["gnorm_inf"][0]) / 4.0


def _logistic_loop(pl, Yd, Omd, Hdd, mu, target, OUTER_MAX, inner_iters, use_graph, x0=None):
    """The IRLS loop on ``pl`` (intercept, sign constraint and factors installed): from x = 0 (or ``x0`` (n, k)) an outer
    step -- ``glm_model`` at the stored x; P = loss + mu l1, and a column whose P rose gets curvature 1 from then on (the
    model is formed again); the working weights installed from the device; the inner reset at B = Z, 4 mu and the stored x,
    no copy; the inner certificate, whose scale gives ``glm_dual``; gap = P - D -- then ``inner_iters`` iterations, until
    every column has gap <= target or OUTER_MAX outer steps have run.  ``mu``, ``target``: (k,), in the library's scale.
    Returns dict(x (n, k), intercept, model (the last outer step's scalars), primal, dual, gap, scale, reached, first,
    outer_iters, iters, curvature)."""
    k, m = pl.nrhs, pl.MAT_HEIGHT
    mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), (k,)).copy()
    curv_h = np.zeros(k, dtype=np.int32)
    curv = torch.zeros(k, dtype=torch.int32, device=pl.device)
    beta0 = torch.zeros(k, dtype=torch.float64, device=pl.device)
    pl.set_row_weights(None)
    pl.solver_reset(np.zeros((m, k)), mu, use_graph=False, x0=x0)
    first = np.full(k, -1, dtype=np.int64)
    P_prev, outer, iters = None, 0, 0
    while True:
        mod = pl.glm_model(Yd, Omd, Hdd, curv, beta0)
        if mod["flag"].any():
            raise ValueError(f"column {int(np.flatnonzero(mod['flag'])[0])}: the weighted labels are all one class")
        P = mod["loss"] + mu * mod["l1"]
        rose = np.zeros(k, dtype=bool) if P_prev is None else (P > P_prev) & (curv_h == 0)
        if rose.any():   # Boehning's bound from here on: every decrease of the model is a decrease of P
            curv_h[rose] = 1
            curv.copy_(torch.from_numpy(curv_h))
            mod = pl.glm_model(Yd, Omd, Hdd, curv, beta0)
        P_prev = P
        pl.set_row_weights_device(mod["W"], Hdd)
        pl.solver_reset(mod["Z"].t(), 4.0 * mu, use_graph=use_graph, x0=pl.solver_x_device())
        cert = pl.duality_gap(screen=False)
        D = pl.glm_dual(cert["scale"])
        gap = P - D
        ok = gap <= target
        first[ok & (first < 0)] = outer
        if ok.all() or outer >= int(OUTER_MAX):
            break
        pl.solver_step(int(inner_iters))
        iters += int(inner_iters)
        outer += 1
    pl.stream.synchronize()
    return dict(x=pl.solver_x(), intercept=mod["beta0"].cpu().numpy().copy(), model=mod, primal=P, dual=D, gap=gap,
                scale=cert["scale"], reached=ok, first=first, outer_iters=outer, iters=iters, curvature=curv_h.copy())


def logistic_path(A, y, mus=None, n_mus=16, hi=0.9, lo=0.1, GAP_BOUND=1e-4, OUTER_MAX=LOGISTIC_OUTER_MAX,
                  inner_iters=LOGISTIC_INNER_ITERS, fit_intercept=True, positive=False, penalty_factors=None,
                  sample_weight=None, x0=None, Block=1, device=None, use_graph=LOGISTIC_USE_GRAPH):
    """An L1-penalised logistic regression path as ONE panel (glmnet's ``family = "binomial"``): for every mu of a grid
      min over x, beta0 of sum_i omega_i l(a_i . x + beta0; y_i) + mu sum_j p_j |x_j|,   l(eta; y) = log(1 + e^eta) - y eta
    on the bf16-stored A, by IRLS on the weighted panel: every column holds the same labels, and
    every column has its own working weights on the one bound A.

    ``y``: (m,) labels in [0, 1] (ValueError outside).  ``mus``: 1 to 128 values, padded as ``lasso_path`` pads them;
    None: mu_max = max_j |a_j . (omega o (p0 - y))| / p_j, read off the x = 0 model, then ``mu_grid(mu_max, n_mus, hi,
    lo)``.  ``fit_intercept`` (default on, as glmnet and scikit-learn have it): beta0 is profiled out of the logistic
    loss at every outer step.  ``positive``, ``penalty_factors``, ``sample_weight`` (omega, any scale, used as given) as
    in ``lasso_path``.  ``x0``: (n, len(mus)) start (needs ``mus``).  ``Block`` must be 1 (ValueError otherwise).  A
    data set whose weighted labels are all one class is refused (ValueError) before any device work.  ``shrink`` is not
    offered: the inner screen is safe for the quadratic model only.

    The loop: an outer step (the model at the stored x, the logistic certificate), then ``inner_iters`` iterations of the
    weighted lasso on the working response; it stops when every mu has gap <= GAP_BOUND x the null deviance (sum omega l
    at x = 0 and its own beta0: the analogue of 1/2 ||b||^2), or after OUTER_MAX outer steps.  A column whose objective
    rose between two outer steps runs with Boehning's curvature bound from then on and is monotone from there.

    Returns a dict: x (n, len(mus)), intercept, mus, mu_max (None when mus was given), deviance (sum omega l at the
    returned point), null_deviance, primal, dual, gap, reached, outer_iters (the outer step at which that mu first met the
    bound, else -1), iters (inner iterations run), curvature (1 where the column fell back)."""
    penalty, yv, omega = _logistic_setup(A, y, Block, penalty_factors, sample_weight)
    _check_two_classes(omega[None, :], yv, "data set")
    if x0 is not None and mus is None:
        raise ValueError("x0 needs mus: the grid the columns of x0 belong to")
    if int(inner_iters) <= 0:
        raise ValueError("inner_iters must be > 0")
    if x0 is not None:
        x0 = np.asarray(x0.detach().cpu() if isinstance(x0, torch.Tensor) else x0, dtype=np.float64)
        want = (int(A.shape[1]), int(np.asarray(mus).size))
        if x0.shape != want:
            raise ValueError(f"x0 must be (n, len(mus)) = {want}, got {x0.shape}")
    if mus is None:
        if not 1 <= int(n_mus) <= PANEL_NRHS[-1]:
            raise ValueError(f"logistic_path takes 1 to {PANEL_NRHS[-1]} values of mu (got {n_mus})")
        grid, n_given = None, int(n_mus)
        k = next(v for v in PANEL_NRHS if v >= n_given)
    else:
        grid, n_given = pad_mus(mus)
        k = grid.size
    from .cpu_calculation import logistic_null_deviance
    pl = _logistic_context(A, k, device, fit_intercept, positive, penalty)
    cw = float(omega.max())
    Yd = _rows_device(pl, np.repeat(yv[None, :], k, axis=0))
    Omd = _rows_device(pl, np.repeat((omega / cw)[None, :], k, axis=0))
    null = logistic_null_deviance(yv, omega, bool(fit_intercept))
    mu_max = None
    if grid is None:
        mu_max = cw * _logistic_mu_max(pl, Yd, Omd)
        grid, _ = pad_mus(_grid_below(mu_max, n_given, hi, lo, positive))
    if x0 is not None:
        x0 = np.concatenate([x0, np.repeat(x0[:, [int(np.argmax(grid[:n_given]))]], k - n_given, axis=1)], axis=1)
    run = _logistic_loop(pl, Yd, Omd, None, grid / cw, float(GAP_BOUND) * null / cw, OUTER_MAX, inner_iters, use_graph,
                         x0=x0)
    g = slice(0, n_given)
    return dict(x=run["x"][:, g], intercept=run["intercept"][g], mus=grid[g].copy(), mu_max=mu_max,
                deviance=run["model"]["loss"][g] * cw, null_deviance=null, primal=run["primal"][g] * cw,
                dual=run["dual"][g] * cw, gap=run["gap"][g] * cw, reached=run["reached"][g],
                outer_iters=run["first"][g], iters=run["iters"], curvature=run["curvature"][g])


def logistic_cv(A, y, n_folds=8, mus=None, n_mus=16, hi=0.9, lo=0.1, GAP_BOUND=1e-4, OUTER_MAX=LOGISTIC_OUTER_MAX,
                inner_iters=LOGISTIC_INNER_ITERS, seed=0, masks=None, fit_intercept=True, positive=False,
                penalty_factors=None, sample_weight=None, refit=True, return_x=False, Block=1, device=None,
                use_graph=LOGISTIC_USE_GRAPH):
    """K-fold cross-validation of the L1-penalised logistic regression over a grid of mu as ONE panel, with
    ``lasso_cv``'s layout and padding: column c = f * n_mus + j solves fold f at ``mus[j]`` with the prior weights
    fold_f o omega and is scored on the held-out rows with the weights h = (1 - fold_f) o omega.  K folds x J values of mu
    have K J different sets of working weights on one bound A.

    Arguments as ``logistic_path`` and ``lasso_cv`` (``masks``: (n_folds, m) 0/1, 0 = held out).  One grid serves all
    folds; with ``mus=None`` mu_max is that of the full data.  ValueError before any device work for labels outside
    [0, 1], ``Block`` != 1, and a fold (or the full data) whose weighted training labels are all one class.

    Returns a dict: mus; deviance (n_folds, n_mus) = 2 sum h l / sum h and error (n_folds, n_mus) = the weighted
    misclassification rate sum h [(p > 1/2) != (y > 1/2)] / sum h of the held-out rows; for each of the two scores s:
    mean_s, se_s, best_s, best_1se_s (``lasso_cv``'s rules); best / best_1se (those of the deviance); reached, gap,
    outer_iters, curvature (n_folds, n_mus); intercept_folds; iters; masks.  ``return_x``: x_folds (n, n_folds, n_mus).
    ``refit``: the full-data path on the grid on the SAME context: x (n, n_mus), intercept, refit_gap, refit_reached."""
    from .cpu_calculation import kfold_masks, logistic_null_deviance
    penalty, yv, omega = _logistic_setup(A, y, Block, penalty_factors, sample_weight)
    m = yv.size
    if masks is not None:
        masks = (np.asarray(masks.detach().cpu() if isinstance(masks, torch.Tensor) else masks) != 0).astype(np.uint8)
        if masks.ndim != 2 or masks.shape[1] != m:
            raise ValueError(f"masks must be (n_folds, m = {m})")
        n_folds = masks.shape[0]
    n_folds = int(n_folds)
    if n_folds < 2:
        raise ValueError(f"logistic_cv needs n_folds >= 2 (got {n_folds})")
    if mus is not None:
        mus = np.asarray(mus, dtype=np.float64).reshape(-1).copy()
        n_mus = mus.size
    n_mus = int(n_mus)
    ncol = n_folds * n_mus
    if n_mus < 1 or ncol > PANEL_NRHS[-1]:
        raise ValueError(f"logistic_cv takes n_folds * n_mus between 2 and {PANEL_NRHS[-1]} (got {n_folds} x {n_mus})")
    if int(inner_iters) <= 0:
        raise ValueError("inner_iters must be > 0")
    if masks is None:
        masks = kfold_masks(m, n_folds, seed)
    wf = masks.astype(np.float64) * omega                     # (n_folds, m): the fold's prior weights
    hf = (1.0 - masks.astype(np.float64)) * omega             # ... and its scoring weights
    _check_two_classes(omega[None, :], yv, "data set")
    _check_two_classes(wf, yv, "fold")
    if not np.all(hf.sum(axis=1) > 0.0):
        raise ValueError("a fold has no held-out row of positive weight")
    fit_intercept = bool(fit_intercept)
    k = next(v for v in PANEL_NRHS if v >= ncol)
    pl = _logistic_context(A, k, device, fit_intercept, positive, penalty)
    cw = float(omega.max())
    if mus is None:
        mu_max = cw * _logistic_mu_max(pl, _rows_device(pl, np.repeat(yv[None, :], k, axis=0)),
                                       _rows_device(pl, np.repeat((omega / cw)[None, :], k, axis=0)))
        mus = _grid_below(mu_max, n_mus, hi, lo, positive)
    cols = np.concatenate([np.arange(ncol), np.zeros(k - ncol, dtype=np.int64)])   # the pad: copies of column 0
    fold, jmu = cols // n_mus, cols % n_mus
    Yd = _rows_device(pl, np.repeat(yv[None, :], k, axis=0))
    null = np.array([logistic_null_deviance(yv, wf[f], fit_intercept) for f in range(n_folds)])
    run = _logistic_loop(pl, Yd, _rows_device(pl, (wf / cw)[fold]), _rows_device(pl, hf[fold]), mus[jmu] / cw,
                         float(GAP_BOUND) * null[fold] / cw, OUTER_MAX, inner_iters, use_graph)
    shape = (n_folds, n_mus)
    hsum = hf.sum(axis=1)[:, None]
    scores = dict(deviance=2.0 * run["model"]["hold_loss"][:ncol].reshape(shape) / hsum,
                  error=run["model"]["hold_miss"][:ncol].reshape(shape) / hsum)
    out = dict(mus=mus.copy(), iters=run["iters"], reached=run["reached"][:ncol].reshape(shape),
               gap=run["gap"][:ncol].reshape(shape) * cw, outer_iters=run["first"][:ncol].reshape(shape),
               curvature=run["curvature"][:ncol].reshape(shape),
               intercept_folds=run["intercept"][:ncol].reshape(shape), masks=masks)
    for name, sc in scores.items():
        mean = sc.mean(axis=0)
        se = sc.std(axis=0, ddof=1) / np.sqrt(n_folds)
        best = int(np.argmin(mean))
        within = np.flatnonzero(mean <= mean[best] + se[best])
        out.update({name: sc, "mean_" + name: mean, "se_" + name: se, "best_" + name: best,
                    "best_1se_" + name: int(within[np.argmax(mus[within])])})
    out.update(best=out["best_deviance"], best_1se=out["best_1se_deviance"])
    if return_x:
        out["x_folds"] = run["x"][:, :ncol].reshape(-1, n_folds, n_mus)
    if refit:
        grid = np.concatenate([mus, np.full(k - n_mus, mus.max())])   # pad_mus' layout at this panel's width
        rnull = logistic_null_deviance(yv, omega, fit_intercept)
        rrun = _logistic_loop(pl, Yd, _rows_device(pl, np.repeat((omega / cw)[None, :], k, axis=0)), None, grid / cw,
                              float(GAP_BOUND) * rnull / cw, OUTER_MAX, inner_iters, use_graph)
        out.update(x=rrun["x"][:, :n_mus], intercept=rrun["intercept"][:n_mus], refit_gap=rrun["gap"][:n_mus] * cw,
                   refit_reached=rrun["reached"][:n_mus], refit_iters=rrun["iters"])
    return out

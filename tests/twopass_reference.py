"""The tiling of the two-pass kernels (csrc/bpgl_kernels.h, bpgl_gap.h) restated in numpy, and the cases
that reach the parts of it which the 16-row chunks of every other test leave idle.

``twopass_geometry`` restates ``geometry()``, ``rowreduce_blocks()`` and the grids of ``bpgl_solver_gap`` in
csrc/bpgl.hip; the MI355X tests assert it against ``GPU_Calculation.geometry()``.  ``trip_model`` restates how
one chunk's rows fall on the four waves of a ``k_colpass`` block (RPT rows per trip, the non-temporal /
allocating split ``isplit``, the two exits and the reload branch of the pipelined loop) and on the 16-row
groups of ``k_rowpass`` (``glate``).  ``model_tmv`` / ``model_mv`` are the tiled products themselves -- chunks
x segments x waves x trips, then ``k_colreduce`` and ``k_rowreduce<BATCH>`` -- with nine deliberate indexing
bugs (``MUTANTS``) that tests/test_twopass_host.py holds the two checks below to.

Two instances per shape:

* exact: every entry of A in +-{1, 2, 3, 4} (exact in bf16, fp32 and fp64), the vectors integers in
  +-{1..8}, nothing zero.  Every product and partial sum is an integer below 2^27 (131139 rows x 4 x 8; the
  diagonal 131139 x 16), so A^T r, A d and the column sums of squares are exact on the device in any order
  and must EQUAL numpy's int64 result.  A dropped, doubled or mis-weighted row, column, segment or chunk
  moves the result by a non-zero integer.
* real: ``solver_step_reference.instance``'s recipe, r = its b and d = randn(w).  The bound is a-priori:
  |dev - ref| <= 2 gam(terms + nchunk + nseg + 4) sum |a_ij| |v|, terms = m for A^T r and the diagonal and w
  for A d: a ``terms``-term fp64 sum in any order, fused or not, the folds over chunks or segments and over
  the four waves, once more for numpy's own sum.
"""
import functools
import itertools

import numpy as np

import solver_step_reference as S

KW = 4                    # waves per block (kWaves)
KU = 4                    # 16-byte loads per lane and row (kU)
VEC = {"float": 4, "double": 2, "bf16": 8}
STORAGES = ("double", "float", "bf16")
COL_RPT = {0: 2, 1: 4, 2: 2}          # col_mode -> rows per trip; col_mode 2 is the pipelined loop
ROWS_PER_REDUCE, MAX_REDUCE_BLOCKS, GAP_BLOCKS, THREADS, SHRINK_COLS = 64, 2048, 256, 256, 64


def cdiv(a, b):
    return -(-a // b)


def up(a, b):
    return cdiv(a, b) * b


def twopass_geometry(m, n, Block, type_name, target=None):
    """geometry() for one context: nseg, nchunk, R, segw, wp, nparts (shrink partials), reduce_blocks
    (k_rowreduce's grid), and the certificate's grids: gap_blocks with gap_steps grid-stride steps, and
    screen_blocks (k_gap_count loops when there are more than 256).  ``target``: BPGL_TARGET_BLOCKS."""
    V = VEC[type_name]
    w = n // Block
    segw = 64 * V * KU
    wp = up(w, V)
    nseg = cdiv(wp, segw)
    if target is None:
        target = 1024 if type_name == "float" else 512
    nchunk = max(1, cdiv(max(1, int(target)), nseg))
    nchunk = min(nchunk, cdiv(m, 16))
    R = up(cdiv(m, nchunk), 16)
    nchunk = cdiv(m, R)
    gap_work = cdiv(max(m, Block * wp), THREADS)
    gap_blocks = min(gap_work, GAP_BLOCKS)
    return dict(nseg=nseg, nchunk=nchunk, R=R, segw=segw, wp=wp, w=w, nparts=cdiv(wp, SHRINK_COLS),
                reduce_blocks=min(cdiv(m, ROWS_PER_REDUCE), MAX_REDUCE_BLOCKS),
                reduce_steps=cdiv(cdiv(m, ROWS_PER_REDUCE), MAX_REDUCE_BLOCKS),
                reduce_batch=1 if nseg <= 4 else 4 if nseg <= 16 else 16,
                gap_blocks=gap_blocks, gap_steps=cdiv(gap_work, gap_blocks), screen_blocks=cdiv(Block * wp, THREADS))


def chunk_rows(m, geo):
    """rows of each chunk"""
    return [min(geo["R"], m - c * geo["R"]) for c in range(geo["nchunk"])]


def wave_trips(rows, q, RPT, isplit=None):
    """The trips of wave q over a chunk of ``rows`` rows as colpass_span walks them (row offsets from the
    chunk's start): [(span, first row, valid rows)].  span 0 runs up to ``isplit`` with non-temporal loads,
    span 1 to the chunk's end; a trip is the rows i, i + 4, ..., i + 4 (RPT - 1), those past the chunk's end
    clamped to i with weight 0."""
    step = RPT * KW
    out, i = [], q
    for span, istop in ((0, isplit), (1, rows)):
        if istop is None:
            continue
        while i < istop:
            out.append((span, i, sum(1 for k in range(RPT) if i + KW * k < rows)))
            i += step
    return out


def trip_model(rows_in_chunk, RPT, tail_permille=None):
    """One chunk of ``rows_in_chunk`` rows.  ``trips`` / ``last``: per wave the trip count and the valid rows
    of its last trip (0, 0: the wave owns no row).  With ``tail_permille`` (non-temporal loads): ``isplit``,
    ``span_trips`` (per wave the trips before and after it: in the pipelined loop an odd count leaves by the
    first exit, an even one by the second, three or more pass the reload branch) and ``straddle`` (isplit
    lies strictly inside the chunk and off a trip boundary, so a trip that began before it ends after it);
    ``groups`` / ``glate``: k_rowpass's 16-row groups and how many of them are read non-temporally."""
    rows = rows_in_chunk
    step = RPT * KW
    isplit = None if tail_permille is None else rows - rows * tail_permille // 1000
    trips, last, spans = [], [], []
    for q in range(KW):
        tr = wave_trips(rows, q, RPT, isplit)
        trips.append(len(tr))
        last.append(tr[-1][2] if tr else 0)
        spans.append((sum(1 for t in tr if t[0] == 0), sum(1 for t in tr if t[0] == 1)))
    groups = cdiv(rows, 4 * KW)
    return dict(trips=trips, last=last, isplit=isplit, span_trips=spans,
                straddle=isplit is not None and 0 < isplit < rows and isplit % step != 0,
                groups=groups, glate=0 if tail_permille is None else groups - groups * tail_permille // 1000)


# --------------------------------------------------------------------------------------------------
# instances
# --------------------------------------------------------------------------------------------------
def exact_instance(m, n, seed):
    """(A, r, d): A (m, n) in +-{1..4}, r (m,) and d (n,) in +-{1..8}, as fp64 holding integers"""
    rs = np.random.RandomState(seed)
    A = rs.randint(1, 5, size=(m, n)) * rs.choice([-1, 1], size=(m, n))
    r = rs.randint(1, 9, size=m) * rs.choice([-1, 1], size=m)
    d = rs.randint(1, 9, size=n) * rs.choice([-1, 1], size=n)
    return A.astype(np.float64), r.astype(np.float64), d.astype(np.float64)


def real_instance(m, n, type_name, seed):
    """(A as stored, r, d): solver_step_reference.instance's A and b, and a dense d"""
    As, b, _ = S.instance(m, n, type_name, seed)
    return As, b, np.random.RandomState(seed + 1).randn(n)


def reference_products(A, r, d, Block, exact):
    """(diag, tmv, mv): (Block, w), (Block, w), (Block, m) -- int64 arithmetic for the exact instance"""
    m, n = A.shape
    w = n // Block
    if exact:
        A, r, d = (np.rint(v).astype(np.int64) for v in (A, r, d))
    Ab = [A[:, q * w:(q + 1) * w] for q in range(Block)]
    return (np.stack([(a * a).sum(axis=0) for a in Ab]), np.stack([a.T @ r for a in Ab]),
            np.stack([a @ d[q * w:(q + 1) * w] for q, a in enumerate(Ab)]))


def product_bounds(A, r, d, Block, geo):
    """the real instance's a-priori bounds, shaped as reference_products' results"""
    m, n = A.shape
    w = n // Block
    absA = np.abs(A)
    Ab = [absA[:, q * w:(q + 1) * w] for q in range(Block)]
    extra = geo["nchunk"] + geo["nseg"] + 4
    gm, gw = 2.0 * S.gam(m + extra), 2.0 * S.gam(w + extra)
    return (np.stack([gm * (a * a).sum(axis=0) for a in Ab]), np.stack([gm * (a.T @ np.abs(r)) for a in Ab]),
            np.stack([gw * (a @ np.abs(d[q * w:(q + 1) * w])) for q, a in enumerate(Ab)]))


def worst_ratio(dev, ref, bound):
    dev_err = np.abs(np.asarray(dev, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, dev_err / bound, np.where(dev_err > 0, np.inf, 0.0))
    return float(np.max(np.where(np.isnan(r), np.inf, r)))


# --------------------------------------------------------------------------------------------------
# the tiled products
# --------------------------------------------------------------------------------------------------
MUTANTS = ("last_partial_trip_dropped", "clamped_row_weighted", "isplit_row_twice", "isplit_row_skipped",
           "ragged_columns_dropped", "chunk_left_out", "second_batch_skipped", "second_grid_step_skipped",
           "reverse_one_group_short")


@functools.lru_cache(maxsize=64)
def colpass_counts(rows, RPT, isplit, mutant=None):
    """how often the walk of one chunk counts each of its rows (all ones when the kernel is right)"""
    cnt = np.zeros(rows, dtype=np.int64)
    for q in range(KW):
        for _, i, valid in wave_trips(rows, q, RPT, isplit):
            if mutant == "last_partial_trip_dropped" and valid < RPT:
                continue
            cnt[i + KW * np.arange(valid)] += 1
            if mutant == "clamped_row_weighted":
                cnt[i] += RPT - valid                          # the clamped copies of row i keep their weight
    if isplit is not None and 0 < isplit < rows:
        cnt[isplit] += {"isplit_row_twice": 1, "isplit_row_skipped": -1}.get(mutant, 0)
    return cnt


def model_tmv(Ab, vec, geo, col_mode=1, nt=1, tail=120, mutant=None):
    """k_colpass + k_colreduce on one block ``Ab`` (m, w): A^T vec, or the column sums of squares when
    ``vec`` is None (that launch is always 2 rows per trip with plain loads)."""
    m, w = Ab.shape
    RPT, nt = (COL_RPT[col_mode], nt) if vec is not None else (2, 0)
    slab = np.zeros((geo["nchunk"], w))
    for c, rows in enumerate(chunk_rows(m, geo)):
        i0 = c * geo["R"]
        isplit = rows - rows * tail // 1000 if nt else None
        wgt = colpass_counts(rows, RPT, isplit, mutant).astype(np.float64)
        blk = Ab[i0:i0 + rows]
        P = blk * (wgt * vec[i0:i0 + rows])[:, None] if vec is not None else blk * blk * wgt[:, None]
        waves = [P[q::KW].sum(axis=0) for q in range(KW)]      # wave q: rows q, q + 4, ... in increasing order
        slab[c] = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    if mutant == "ragged_columns_dropped" and geo["wp"] % geo["segw"]:
        slab[:, (geo["nseg"] - 1) * geo["segw"]:] = 0.0
    out = np.zeros(w)
    for c in range(geo["nchunk"]):
        if not (mutant == "chunk_left_out" and c == geo["nchunk"] // 2):
            out = out + slab[c]
    return out


def model_mv(Ab, d, geo, reverse=0, mutant=None):
    """k_rowpass + k_rowreduce<BATCH> (mode 0) on one block: A d.  Rows that no group or grid step writes
    stay 0."""
    m, w = Ab.shape
    nseg, segw = geo["nseg"], geo["segw"]
    written = np.zeros(m, dtype=bool)
    for c, rows in enumerate(chunk_rows(m, geo)):
        i0 = c * geo["R"]
        groups = cdiv(rows, 4 * KW)
        walk = [groups - 1 - gi if reverse else gi for gi in range(groups)]
        if mutant == "reverse_one_group_short" and reverse:
            walk = walk[:-1]
        for grp in walk:
            written[i0 + grp * 16:min(i0 + grp * 16 + 16, i0 + rows)] = True
    slab = np.zeros((nseg, m))
    for q in range(nseg):
        lo, hi = q * segw, min((q + 1) * segw, w)
        if mutant == "ragged_columns_dropped" and q == nseg - 1 and geo["wp"] % segw:
            continue
        slab[q] = np.where(written, Ab[:, lo:hi] @ d[lo:hi], 0.0)
    batch = geo["reduce_batch"]
    waves = []
    for q in range(KW):
        acc = np.zeros(m)
        for q0 in range(q, nseg, batch * KW):
            for k in range(batch):
                if q0 + k * KW < nseg:
                    acc = acc + slab[q0 + k * KW]
            if mutant == "second_batch_skipped":
                break
        waves.append(acc)
    out = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    if mutant == "second_grid_step_skipped":
        out[geo["reduce_blocks"] * ROWS_PER_REDUCE:] = 0.0
    return out


def model_products(A, r, d, Block, geo, knobs=(1, 1, 120, 0), mutant=None):
    """(diag, tmv, mv) of the tiled model for ``knobs`` = (col_mode, nt_loads, tail_permille, reverse_rows)"""
    col_mode, nt, tail, reverse = knobs
    w = A.shape[1] // Block
    Ab = [A[:, q * w:(q + 1) * w] for q in range(Block)]
    return (np.stack([model_tmv(a, None, geo, mutant=mutant) for a in Ab]),
            np.stack([model_tmv(a, r, geo, col_mode, nt, tail, mutant) for a in Ab]),
            np.stack([model_mv(a, d[q * w:(q + 1) * w], geo, reverse, mutant) for q, a in enumerate(Ab)]))


# --------------------------------------------------------------------------------------------------
# the cases (tests/test_twopass_geometry.py on the MI355X, tests/test_twopass_host.py on the CPU)
# --------------------------------------------------------------------------------------------------
# (col_mode, nt_loads, tail_permille, reverse_rows)
KNOBS = list(itertools.product((0, 1, 2), (0, 1), (0, 120, 500, 1000), (0, 1)))
KNOB_KEYS = ("col_mode", "nt_loads", "tail_permille", "reverse_rows")


def pcase(m, n, ty, Block=1, target=None):
    return dict(m=m, n=n, ty=ty, Block=Block, target=target)


def pcase_id(c):
    return (f"{c['m']}x{c['n']}-{c['ty']}" + (f"-B{c['Block']}" if c["Block"] > 1 else "")
            + (f"-target{c['target']}" if c["target"] is not None else ""))


def pcase_geometry(c):
    return twopass_geometry(c["m"], c["n"], c["Block"], c["ty"], c["target"])


# a. long chunks (m, n, Block, BPGL_TARGET_BLOCKS): one 208-row chunk with 26/26/26/25 and 13 trips per wave;
# one 224-row chunk with 27/26 trips; three chunks for fp32 with a ragged last one; 3 and 2 feature blocks; a
# 32-row chunk of 17 rows; one row (three waves own none); 19 chunks of 32 rows (k_shrink's unrolled loop
# and its remainder of 3)
LONG_SHAPES = [(203, 1500, 1, 1), (211, 1500, 1, 1), (203, 1500, 1, 6), (203, 1500, 3, 1), (211, 2000, 2, 1),
               (17, 40, 1, 1), (1, 40, 1, 1), (600, 100, 1, 19)]
LONG_CASES = [pcase(m, n, ty, B, t) for (m, n, B, t) in LONG_SHAPES for ty in STORAGES]
# b. wide rows: nseg 69 (k_rowreduce<16>, a partial second batch), 18 and 19 (k_rowreduce<16>), 6 (k_rowreduce<4>)
WIDE_CASES = [pcase(24, 70016, "float"), pcase(24, 8712, "double"), pcase(24, 36880, "bf16"),
              pcase(40, 6000, "float")]
# c. tall: 2050 groups of 64 rows on 2048 reduce blocks
TALL_CASES = [pcase(131139, 32, ty, 2) for ty in ("float", "double", "bf16")]
PRODUCT_CASES = LONG_CASES + WIDE_CASES + TALL_CASES

# d. solver steps (solver_step_reference.case, the 18-step protocol of tests/test_solver_step.py)
_c = S.case
STEP_CASES = (
    [_c(203, 1500, ty, Block=3, target=1) for ty in STORAGES]
    + [_c(211, 2000, ty, Block=2, target=1) for ty in STORAGES]
    + [_c(203, 1500, ty, knobs=[("onepass", 0)], target=1) for ty in STORAGES]
    + [_c(211, 1500, "float", knobs=[("onepass", 0), ("col_mode", v)], target=1) for v in (0, 1, 2)]
    + [_c(203, 1500, "float", Block=3, knobs=[("tail_permille", 500), ("reverse_rows", 1)], target=6),
       _c(211, 2000, "bf16", Block=2, x0_seed=5, target=1),       # a dense start: check 0 through k_rowpass

       _c(600, 100, "float", knobs=[("onepass", 0)], target=19),
       _c(24, 70016, "float", knobs=[("onepass", 0)]),
       _c(131139, 32, "float", Block=2, knobs=[("onepass", 0)])]
    + [_c(203, 1500, ty, target=1) for ty in STORAGES])
del _c

# e. the certificate at its thresholds: (m, n, storage, Block); mu = GAP_MU_SCALE |A^T b|_inf
GAP_CASES = [(24, 70016, "float", 1), (24, 70006, "float", 2), (131139, 32, "float", 2)]
GAP_MU_SCALE = 0.5


def gap_instance(m, n, ty):
    return S.instance(m, n, ty, m + n, mu_scale=GAP_MU_SCALE)

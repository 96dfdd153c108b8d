"""Sparse X.W with W's column slices resident in LDS (csrc/xw_sparse_lds.hip): the deterministic inputs its arm tests run
on, the float64 restatement with derived bounds (the functions of _spmm_acc_ref), the arm selection of the launch
restated, and the tables of cases.  Plain numpy; nothing here touches the GPU.

The kernel's constants the inputs are built around: a wavefront owns WINDOWS of 64 consecutive rows; with LPR lanes per row
(2, 4, 8, 16) a window is 64 / LPR rows at a time, a SUB-TILE, the rows dealt to the sub-tiles by length, longest first; a
step sums EPS = min(LPR, 4) entries of every row of the sub-tile and a UNIT is D = 8 steps, i.e. 32 entries (16 at LPR 2);
a sub-tile runs its LONGEST row's steps, the shorter rows' slots past their end hold the entries that follow in memory -- the
next rows' -- and are selected to (zero row of W, value 0) when used.

Inputs: values and weights of magnitude in [1/4, 1] with a random sign, rounded to the storage type, so every term of a sum
is at least 1/16 in magnitude: one term lost or gained moves a sum by 2^-4, against a bound of (n + 2) 2^-24 scale + one
store rounding (~5e-3 at fp16 for the longest rows).  tests/test_xw_sparse_ref_cpu.py shows each mutation the kernel could
suffer lands outside the bound in every row it touches.
"""
import collections
import functools

import numpy as np

import _spmm_acc_ref as R

D_STEPS = 8                       # kDepth
LDS_BUDGET = 160 * 1024           # kLdsBudget
WAVES = 16                        # kWaves: wavefronts of a workgroup, one window each
PLAN_CUT = 512                    # the plan's cut (long_threshold) from 2^20 to under 2^22 entries


def eps(lpr):
    return min(lpr, 4)


def unit(lpr):
    """entries of one unit of work"""
    return D_STEPS * eps(lpr)


# ---- the arm selection of the launch, restated (sgx_xw_sparse_form is what the GPU tests assert on; this chooses the
# shapes and cross-checks it) ---------------------------------------------------------------------------------------------

Arm = collections.namedtuple("Arm", "lpr n_split full w_vec wgs_per_cu streams")


def per16(dt):
    return 8 if dt == "f16" else 4


def choose_lpr(dt, M, P, lpr_cap=0):
    need = 1
    while need < (P + per16(dt) - 1) // per16(dt):
        need *= 2
    lpr = min(need, 16)
    while lpr >= 1 and (M + 1) * lpr * 16 > LDS_BUDGET:
        lpr //= 2
    if 0 < lpr_cap < lpr:
        lpr = lpr_cap
    return lpr if lpr >= 2 else 0


def arm(dt, n_rows, M, P, nnz, max_degree, w_aligned=True, ldw=None, h_aligned=True, ldh=None, lpr_cap=0, streams_cap=0,
        cus=256):
    """The arm sgx_xw_sparse takes, or None for the gather kernel.  w_aligned / h_aligned: the pointer is 16-byte aligned;
    ldw / ldh in elements (default: P)."""
    es = 2 if dt == "f16" else 4
    ldw = P if ldw is None else ldw
    ldh = P if ldh is None else ldh
    if nnz < 1 << 20 or nnz >= (1 << 30) - 65536 or n_rows < 4096 or max_degree > PLAN_CUT:
        return None
    if n_rows * ldh * es >= 0xFFF00000 or M * ldw * es > 0xFFF00000:
        return None
    lpr = choose_lpr(dt, M, P, lpr_cap)
    if lpr < 2:
        return None
    cp = lpr * per16(dt)
    n_split = (P + cp - 1) // cp
    if n_split > 4:
        return None
    full = P % cp == 0 and h_aligned and (ldh * es) % 16 == 0
    w_vec = w_aligned and (ldw * es) % 16 == 0
    wgs = 2 if (M + 1) * lpr * 16 * 2 <= LDS_BUDGET else 1
    grid = cus // 8 * 8 * wgs
    tiles = (n_rows + 64 * WAVES - 1) // (64 * WAVES)
    grid = min(grid, (tiles + 7) // 8 * 8 * n_split)
    if streams_cap > 0:
        grid = min(grid, max(8, streams_cap // 8 * 8) * n_split)
    grid = max(grid, 8 * n_split)
    return Arm(lpr, n_split, full, w_vec, wgs, grid // 8 // n_split * 8)


def windows_per_wavefront(n_rows, streams):
    """how many windows each of the grid's streams x 16 wavefronts walks: window w belongs to wavefront w mod that count"""
    n_windows = (n_rows + 63) // 64
    step = streams * WAVES
    return [len(range(w, n_windows, step)) for w in range(step)]


def win_order(deg):
    """the plan's order of every window's rows: by length, longest first, ties in row order (rank -> row inside the window)"""
    deg = np.asarray(deg)
    out = []
    for b in range(0, len(deg), 64):
        d = deg[b:b + 64]
        out.append(np.argsort(-d, kind="stable"))
    return out


# ---- inputs -------------------------------------------------------------------------------------------------------------

def _signed(rng, shape):
    return (0.25 + 0.75 * rng.random(shape)) * np.where(rng.random(shape) < 0.5, -1.0, 1.0)


def csr_from_degrees(deg, M, seed, col_lo=0):
    """(rowptr, columns, float64 values not yet rounded): deg[i] distinct sorted columns in [col_lo, M) per row"""
    deg = np.asarray(deg, np.int64)
    rng = np.random.default_rng(seed)
    n, width = len(deg), M - col_lo
    assert deg.max() <= width
    keys = rng.random((n, width))
    cut = np.sort(keys, axis=1)[np.arange(n), np.maximum(deg, 1) - 1]
    rows, cols = np.nonzero(keys <= np.where(deg > 0, cut, -1.0)[:, None])         # row-major: sorted inside a row
    assert np.array_equal(np.bincount(rows, minlength=n), deg)
    rp = np.zeros(n + 1, np.int32)
    rp[1:] = np.cumsum(deg)
    return rp, (cols + col_lo).astype(np.int32), _signed(rng, len(cols))


DEEP_M, DEEP_ROWS = 600, 64 * 72 + 37
_EDGE_DEGREES = [d for u in (16, 32) for d in (u - 1, u, u + 1, 2 * u - 1, 2 * u, 2 * u + 1, 3 * u, 3 * u + 1)] + [1, 2, 3, 4, 5, 7, 8, 9]
# the whole windows `deep` starts with, in this order
DEEP_WINDOWS = [
    [0] * 64,                                             # a window without an entry
    [0] * 63 + [PLAN_CUT],                                # one row at the plan's cut: 16 units (32 at LPR 2) beside empty groups
    [32] * 64,                                            # exactly one unit of EPS = 4 (two at LPR 2), in every sub-tile
    list(range(64)),                                      # every length from 0 to 63
    _EDGE_DEGREES + [0] * (64 - len(_EDGE_DEGREES)),      # around one, two and three units of 16 and of 32 entries; one step +- 1
    [40] * 60 + [0] * 4,                                  # the last sub-tile all empty at LPR 16 ...
    [40] * 48 + [0] * 16,                                 # ... at LPR 4 (and 8, 16) ...
    [40] * 32 + [0] * 32,                                 # ... at LPR 2 (and every other), the sub-tiles before it with steps
]


def deep_degrees():
    rng = np.random.default_rng(20)
    special = np.concatenate([np.array(w, np.int64) for w in DEEP_WINDOWS])
    fill = rng.integers(250, 271, DEEP_ROWS - len(special) - 2)
    deg = np.concatenate([special, fill, [0, 6]])         # the last row but one empty, the last row ends the arrays
    if deg.sum() % 2 == 0:
        deg[-1] += 1                                      # an odd entry count: the fp16 values end inside a dword
    return deg


WIDE_M, WIDE_ROWS = 200, 64 * (3 * 128 + 5) - 27


def wide_degrees():
    rng = np.random.default_rng(21)
    deg = rng.integers(20, 71, WIDE_ROWS)
    deg[rng.random(WIDE_ROWS) < 0.05] = 0
    deg[::97] = rng.integers(129, 201, len(deg[::97]))
    return deg


# hostile: the rows of `deep` (all among its filler rows, in different windows) whose FIRST entry is made hostile, the
# length each is cut to, and the length of the CSR row before it -- odd, so that its last step has slots past its end
# at EPS = 4 and at EPS = 2, and those hold the hostile entry.  One row starts a window: the row before it is the last of
# the window before.
HOSTILE_VALUE_ROWS = {64 * 12 + 1: (6, 1, np.inf), 64 * 20: (9, 3, -np.inf), 64 * 31 + 40: (13, 5, np.nan)}
HOSTILE_COLUMN_ROWS = {64 * 15 + 63: (7, 1, 0), 64 * 27: (10, 3, 1), 64 * 44 + 17: (11, 5, 2)}
HOSTILE_W = {0: np.inf, 1: np.nan, 2: -np.inf}            # rows of W; no other row of X refers to these columns


def hostile_degrees():
    deg = deep_degrees()
    for r, (own, before, _) in {**HOSTILE_VALUE_ROWS, **HOSTILE_COLUMN_ROWS}.items():
        deg[r], deg[r - 1] = own, before
    deg[-2] = 1                                           # the last row is over-read by a one-entry row, and ends the arrays
    return deg


def hostile_rows():
    """(chosen rows, the CSR rows before them -- the ones a missing select poisons)"""
    chosen = sorted({**HOSTILE_VALUE_ROWS, **HOSTILE_COLUMN_ROWS})
    return chosen, [r - 1 for r in chosen]


@functools.lru_cache(maxsize=None)
def structure(name):
    """(rowptr, columns, unrounded float64 values, M_fea) of a fixture"""
    if name == "deep":
        return csr_from_degrees(deep_degrees(), DEEP_M, 200) + (DEEP_M,)
    if name == "wide":
        return csr_from_degrees(wide_degrees(), WIDE_M, 201) + (WIDE_M,)
    assert name == "hostile"
    rp, ci, va = csr_from_degrees(hostile_degrees(), DEEP_M, 200, col_lo=len(HOSTILE_W))
    ci, va = ci.copy(), va.copy()
    for r, (_, _, v) in HOSTILE_VALUE_ROWS.items():
        va[rp[r]] = v
    for r, (_, _, c) in HOSTILE_COLUMN_ROWS.items():
        ci[rp[r]] = c                                     # below every other column: the row stays sorted
    return rp, ci, va, DEEP_M


@functools.lru_cache(maxsize=None)
def matrix(name, dt):
    """(rowptr, columns, values the storage type holds exactly)"""
    rp, ci, va, _ = structure(name)
    return rp, ci, R.rounded(va, dt)


def n_cols(name):
    return structure(name)[3]


@functools.lru_cache(maxsize=None)
def weights(name, P, dt):
    M = n_cols(name)
    W = R.rounded(_signed(np.random.default_rng(3000 + P), (M, P)), dt)
    if name == "hostile":
        for r, v in HOSTILE_W.items():
            W[r] = v * np.sign(W[r])                      # (the infinite rows keep their elements' signs: both infinities in a row)
    return W


@functools.lru_cache(maxsize=8)
def sums(name, dt, P):
    """(X @ W, |X| @ |W|, entries per row) in float64; hostile: of the operands with the non-finite ones zeroed"""
    rp, ci, va = matrix(name, dt)
    W = weights(name, P, dt)
    return R.one_pass((rp, ci, np.where(np.isfinite(va), va, 0.0)), np.where(np.isfinite(W), W, 0.0))


@functools.lru_cache(maxsize=8)
def reference(name, dt, P):
    """(want, bound, entries per row) of the stored X @ W: the float64 sum and (n + 2) 2^-24 (|X| @ |W|) plus one store
    rounding.  hostile: the chosen rows' sums hold their one non-finite term (every other row refers to finite operands
    only, so the dense products run on the operands with the non-finite ones zeroed)."""
    s, scale, n = sums(name, dt, P)
    want, bound = R.finished(s, R.partial_bound(n, scale), dt, relu=False)
    if name != "hostile":
        return want, bound, n
    rp, ci, va = matrix(name, dt)
    W = weights(name, P, dt)
    want = want.copy()
    with np.errstate(invalid="ignore"):
        for r in hostile_rows()[0]:
            e = slice(rp[r], rp[r + 1])
            want[r] = (va[e, None] * W[ci[e]]).sum(0)
    return want, bound, n


# ---- the cases of tests/test_gpu_xw_sparse_arms.py (checked against the restatement in test_xw_sparse_ref_cpu.py) ----------

# lane splits and slices on `deep`: (dtype, P, SGX_XW_SPARSE_LPR or None, lpr, n_split, full)
DEEP_CASES = [
    ("f16", 16, None, 2, 1, True), ("f16", 12, None, 2, 1, False), ("f16", 24, 2, 2, 2, False), ("f16", 48, 2, 2, 3, True),
    ("f16", 64, 2, 2, 4, True),
    ("f16", 32, None, 4, 1, True), ("f16", 64, 4, 4, 2, True), ("f16", 70, 4, 4, 3, False), ("f16", 100, 4, 4, 4, False),
    ("f16", 64, None, 8, 1, True), ("f16", 47, None, 8, 1, False), ("f16", 128, 8, 8, 2, True), ("f16", 200, 8, 8, 4, False),
    ("f16", 128, None, 16, 1, True), ("f16", 200, None, 16, 2, False), ("f16", 384, None, 16, 3, True),
    ("f32", 8, None, 2, 1, True), ("f32", 16, 2, 2, 2, True), ("f32", 21, 2, 2, 3, False), ("f32", 32, 2, 2, 4, True),
    ("f32", 16, None, 4, 1, True), ("f32", 41, 4, 4, 3, False), ("f32", 64, 4, 4, 4, True),
    ("f32", 32, None, 8, 1, True), ("f32", 50, 8, 8, 2, False), ("f32", 64, 8, 8, 2, True),
    ("f32", 64, None, 16, 1, True), ("f32", 100, None, 16, 2, False), ("f32", 192, None, 16, 3, True), ("f32", 256, None, 16, 4, True),
]

# the window walk on `wide`: (dtype, P, lpr, n_split, full)
WIDE_CASES = [("f16", 16, 2, 1, True), ("f16", 64, 8, 1, True), ("f32", 16, 4, 1, True), ("f32", 100, 16, 2, False)]

# hostile neighbours: (dtype, P, lpr) -- an EPS = 4 split and LPR 2 per dtype
HOSTILE_CASES = [("f16", 64, 8), ("f16", 16, 2), ("f32", 64, 16), ("f32", 8, 2)]

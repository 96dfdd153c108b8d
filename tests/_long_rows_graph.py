"""The graph of tests/test_gpu_long_rows.py: 150 rows (no multiple of 8 or of 64, so the last window of the long-row walk,
csrc/long_rows.h, is partial in every kernel that uses it) with long rows -- over 256 entries -- at the walk's edges, among
short rows of 0 to 12 entries.  Scores of order 1, 5 % of the entries masked, 50 neighbour-only columns."""
import numpy as np

import _gat_ref as R

N_ROWS, N_COLS, CUT = 150, 200, 256
# row: (degree, every entry masked)
NAMED = {
    0: ("long_first_of_window_0", 300, False),
    1: ("long_257_next_to_a_long_row", 257, False),         # rows 0 and 1: two long rows inside one window of 8
    2: ("short_256", 256, False),                           # exactly the cut: not long
    64: ("long_first_of_a_window_of_64", 600, False),
    65: ("empty_between_long_rows", 0, False),
    66: ("long_after_an_empty_row", 400, False),
    70: ("long_dead", 300, True),
    149: ("long_last_row", 500, False),
}


def graph(dt, heads, f_head, seed=0):
    """dict(rowptr, col, val, Wh, att, names, n_rows, n_cols) of float64 stored values, as tests/_gat_ref.py's graphs."""
    rng = np.random.default_rng([seed, heads, f_head])
    F = heads * f_head
    deg = rng.integers(0, 13, N_ROWS)
    for r, (_name, d, _masked) in NAMED.items():
        deg[r] = d
    rowptr = np.zeros(N_ROWS + 1, np.int64)
    rowptr[1:] = np.cumsum(deg)
    nnz = int(rowptr[-1])
    col = rng.integers(0, N_COLS, nnz)
    val = rng.uniform(0.05, 1.0, nnz)
    val[rng.random(nnz) < 0.05] = -0.25
    for r, (_name, _d, masked) in NAMED.items():
        if masked:
            val[rowptr[r]:rowptr[r + 1]] = -0.25
    Wh = R._round(rng.standard_normal((N_COLS, F)) * 0.6, dt)
    att = R._round(rng.standard_normal(2 * F) / np.sqrt(f_head), dt)
    return dict(rowptr=rowptr, col=col, val=R._round(val, dt), Wh=Wh, att=att, names={r: v[0] for r, v in NAMED.items()},
                n_rows=N_ROWS, n_cols=N_COLS)

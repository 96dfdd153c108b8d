"""Small graphs at the edges of the plan's row schedule (csrc/row_schedule.h), with degrees chosen, not drawn: rows of one
8-entry step (0 to 8 entries: empty rows and exactly-8 rows among them) that the degree order ends with, rows of 9 to 40
entries ahead of them, and rows above the cut of a small matrix (64 entries) that become tasks.  The tail of one-step rows is
taken from 4096 rows on.  Used by tests/test_gpu_row_schedule.py and tools/agg_digest.py."""
import numpy as np

TAIL_GATE = 4096          # one-step rows from which the schedule gives the tail its own workgroups
SMALL_CUT = 64            # the cut of a matrix under 2^20 entries: longer rows are tasks

# name: (one-step rows, rows of 9..40 entries, entries of the long rows)
CASES = {
    "tail_4096": (TAIL_GATE, 600, (100, 200)),           # (a) the tail is taken
    "tail_4095": (TAIL_GATE - 1, 600, (100, 200)),       # (b) one row short: not taken
    "tail_only": (TAIL_GATE, 0, (100, 200)),             # (c) no row of two steps and more outside the tasks: no row blocks
    "no_long": (TAIL_GATE, 600, ()),                     # (d) as (a) without tasks: split_blocks = 0
}


def degrees(case):
    n_one, n_mid, long_rows = CASES[case]
    deg = np.concatenate([np.arange(n_one) % 9, 9 + np.arange(n_mid) % 32, np.asarray(long_rows, np.int64)]).astype(np.int64)
    n = len(deg)
    # the kinds interleaved: row i takes the degree at i * 1237 mod n (1237 is prime and divides none of the sizes)
    assert n % 1237 != 0
    return deg[(np.arange(n) * 1237) % n]


def graph(case, dt):
    """dict of numpy arrays: rowptr, col (int32), val (float64 holding values of type dt: a third of them <= 0, which the
    GAT mask drops), n = rows = columns"""
    deg = degrees(case)
    n = len(deg)
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(deg)
    row = np.repeat(np.arange(n), deg)
    k = np.arange(rowptr[-1]) - rowptr[row]
    col = (row * 31 + k * 97 + 1) % n
    val = ((row * 3 + k * 5) % 11 - 3) / 8.0                     # -0.375 .. 0.875 in eighths: exact in fp16
    return dict(rowptr=rowptr.astype(np.int32), col=col.astype(np.int32), val=val, n=n, deg=deg)


def table(n, width, seed, scale=1.0):
    """[n, width] float64 of multiples of 1/64 in (-scale, scale): exact in fp16 and fp32"""
    rng = np.random.default_rng(seed)
    return np.round(rng.uniform(-scale, scale, (n, width)) * 64) / 64


def tail_rows(deg):
    """(rows of two steps and more that are no tasks, one-step rows): what row_order[0, n_multi) and the rest hold"""
    short = deg <= SMALL_CUT
    return int(np.sum(short & (deg > 8))), int(np.sum(deg <= 8))

"""Small adversarial CSR graphs for the kernels of the attention layer's backward, with named rows (numpy only).

The kernels and what picks their arm:

  edge pass (csrc/gat_bwd.hip)          gat_bwd_dots_kernel<LPR>: LPR = next power of two >= ceil(F / 16), at most 64; a lane
                                        group covers TILE = 4 LPR columns per pass.  16-byte loads of G where G and its pitch
                                        are on 16 bytes (g_vec), element loads else.  Rows: 8 lanes per row up to
                                        LONG_ROW_CUT = 256 entries, a workgroup of 1024 threads per longer row, found window
                                        by window of 64 rows.  The dots grid is persistent: 8 workgroups of 256 entries per CU.
  attention gradient, row form          attention_grad_slices_kernel<LPR, VEC>: LPR = next power of two >= ceil(F / 4), at
  (csrc/layer_bwd.hip)                  most 64; WORKERS = 4 * 64 / LPR lane groups per workgroup.  A workgroup owns a run of
                                        rps = ceil(n_rows / min(1024, ceil(n_rows / 64))) rows and walks the run's long rows
                                        window after window of 64 rows; a long row goes in chunks of 256 entries, WORKERS
                                        chunks to a round.
  attention gradient, entry-split form  attention_grad_flat_kernel<LPR, VEC>: the same lane rule as the row form.
  (csrc/gat_attention_grad_flat.hip)

Scores.  The backward takes its E and S from the forward, and neither depends on the Wh and G of the backward's own
products.  The graphs therefore carry the scores directly: E_e = LeakyReLU(score_row[i] + score_col[c]).  score_row holds
multiples of 1/4 and score_col odd multiples of 1/8, so a score is an odd multiple of 1/8, exact in fp32 and never within
rounding of the LeakyReLU's step.  The exceptions are deliberate (zero_scores=True): two neighbour-only columns score
+1e-60 and -1e-60 and are stored only in rows that score 0, which gives live entries whose fp32 E is exactly +0.0 and -0.0.
score_graph() turns a graph into the input of _gat_ref.forward that has these scores."""
import numpy as np

import _gat_ref as R

LONG_ROW_CUT = 256                    # kLongRowCut (csrc/long_rows.h): rows over this many entries take a whole workgroup
ROW_LANES = 8                         # lanes per short row in the edge pass
LONG_THREADS = 1024                   # threads of the workgroup that takes a long row in the edge pass
WINDOW = 64                           # rows one ballot of the long-row walk looks at
DOT_BLOCK = 256                       # stored entries per workgroup pass of the dots kernel ...
DOT_BLOCKS_PER_CU = 8                 # ... and workgroups per CU of its persistent grid
AG_MAX_SLICES = 1024

EDGE_WIDTHS = [1, 7, 16, 17, 32, 33, 64, 100, 129, 257, 513, 1030]
ATTENTION_WIDTHS = [1, 4, 5, 8, 9, 20, 33, 64, 65, 129, 257, 300, 513]
ROW_LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]
TINY_SCORE = 1e-60                    # rounds to +0.0 / -0.0 in fp32


def next_pow2(n):
    p = 1
    while p < n:
        p *= 2
    return p


def edge_lanes(F):
    """LPR of gat_bwd_dots_kernel"""
    return min(next_pow2(-(-F // 16)), 64)


def attention_lanes(F):
    """LPR of attention_grad_slices_kernel and attention_grad_flat_kernel"""
    return min(next_pow2(-(-F // 4)), 64)


def attention_workers(F):
    return 4 * 64 // attention_lanes(F)


def attention_slices(n_rows):
    return max(1, min(AG_MAX_SLICES, -(-n_rows // 64)))


def rows_per_slice(n_rows):
    """rps: the run of rows one workgroup of the row form owns"""
    return -(-n_rows // attention_slices(n_rows)) if n_rows > 0 else 1


def _finish(lens, names, ents, n_extra_cols, rng, dt, tail, score_row, special=None):
    """CSR arrays from per-row lengths.  ents: row -> list of (column or None, value or None) for the rows that are set
    by hand; everything else gets random columns and live values with a tenth of the entries masked."""
    n_rows = len(lens)
    n_cols = n_rows + n_extra_cols
    n_plain = n_cols - (2 if special else 0)                 # the special columns are stored only where asked for
    rowptr = np.zeros(n_rows + 1, np.int64)
    rowptr[1:] = np.cumsum(lens)
    nnz = int(rowptr[-1])
    col = rng.integers(0, n_plain, nnz)
    val = rng.uniform(0.1, 1.0, nnz)
    val[rng.random(nnz) < 0.1] = -0.25
    for r, e in ents.items():
        assert len(e) == lens[r], (names.get(r), len(e), lens[r])
        for k, (c, v) in enumerate(e):
            if c is not None:
                col[rowptr[r] + k] = c
            val[rowptr[r] + k] = rng.uniform(0.1, 1.0) if v is None else v
    val = R._round(val, dt)
    score_col = (rng.integers(-12, 12, n_cols) * 2 + 1) / 8.0
    if special:
        score_col[n_cols - 2], score_col[n_cols - 1] = TINY_SCORE, -TINY_SCORE
    col_cap = np.concatenate([col, np.full(tail, 1 << 30, np.int64)])
    val_cap = np.concatenate([val, np.full(tail, np.nan)])
    return dict(rowptr=rowptr, col=col, val=val, col_cap=col_cap, val_cap=val_cap, nnz=nnz, capacity=nnz + tail,
                n_rows=n_rows, n_cols=n_cols, names=names, score_row=np.asarray(score_row, np.float64), score_col=score_col,
                zero_cols=(n_cols - 2, n_cols - 1) if special else None)


def adversarial(dt, zero_scores=True, seed=0, n_filler=1500, tail=37):
    """The main graph.  Named rows, in order: three empty rows; one row of each length in ROW_LENGTHS (all in the first
    64-row window, which so holds five rows over the cut); a run of empty rows; the mask's edge values; a dead short
    and a dead long row; two rows that score 0 with entries on the +-1e-60 columns (zero_scores; a short one and one over
    the cut); short filler rows of 0..8 entries; then a long row a few rows before the end and a long row as the very
    last, both in a last window of fewer than 64 rows.  col_cap / val_cap are col / val with `tail` more entries behind
    rowptr[n_rows]: columns far outside the table and NaN values."""
    rng = np.random.default_rng([seed, 11])
    neg_tiny = -R.F16_SUB if dt == "f16" else -R.F32_SUB
    lens, names, ents = [], {}, {}

    def add(name, n, e=None):
        names[len(lens)] = name
        if e is not None:
            ents[len(lens)] = e
        lens.append(n)

    for k in range(3):
        add(f"empty_first_{k}", 0)
    for n in ROW_LENGTHS:
        add(f"len{n}", n)
    for k in range(5):
        add(f"empty_run_{k}", 0)
    add("mask_edge_values", 7, [(None, None), (None, 0.0), (None, -0.0), (None, neg_tiny), (None, -0.25), (None, None),
                                (None, None)])
    add("dead_short", 4, [(None, -0.25), (None, 0.0), (None, -0.0), (None, neg_tiny)])
    add("dead_long", 300, [(None, -0.25)] * 300)
    zero_rows = [len(lens), len(lens) + 1]
    add("zero_scores", 9)
    add("zero_scores_long", 300)
    n_named = len(lens)
    for _ in range(n_filler):
        lens.append(int(rng.integers(0, 9)))
    while (len(lens) + 7) % WINDOW < 8:                              # the last window is ragged and holds the two long rows
        lens.append(2)
    lens.append(0)
    add("long_in_last_window", 400)
    lens.extend([3, 0, 0, 5])
    add("long_last_row", 258)
    filler = n_named + 1
    while sum(lens) % 64 == 0:                                       # an entry count that is no multiple of 64 (or 256)
        lens[filler] += 1
    n_rows = len(lens)
    score_row = rng.integers(-8, 9, n_rows) / 4.0
    n_extra = 16
    if zero_scores:
        plus, minus = n_rows + n_extra - 2, n_rows + n_extra - 1
        for r in zero_rows:
            score_row[r] = 0.0
            e = [(None, None)] * lens[r]
            for k, c in ((1, plus), (2, minus), (4, plus), (lens[r] - 1, minus), (lens[r] - 2, plus)):
                e[k] = (c, None)
            ents[r] = e
    g = _finish(lens, names, ents, n_extra, rng, dt, tail, score_row, special=zero_scores)
    g["zero_rows"] = zero_rows if zero_scores else []
    return g


def tiny(dt, tail=5):
    """fewer than 64 stored entries; empty rows first, in a run and last"""
    rng = np.random.default_rng(5)
    lens = [0, 0, 3, 0, 7, 1, 0, 0, 9, 0, 0]
    names = {0: "empty_first", 2: "len3", 4: "len7", 5: "len1", 8: "len9", 10: "empty_last"}
    ents = {2: [(None, None), (None, -0.0), (None, None)]}
    return _finish(lens, names, ents, 3, rng, dt, tail, rng.integers(-8, 9, len(lens)) / 4.0)


def no_entries(dt, tail=4):
    """rows, and not one stored entry"""
    rng = np.random.default_rng(6)
    return _finish([0] * 5, {0: "empty_first", 4: "empty_last"}, {}, 2, rng, dt, tail, np.zeros(5))


def many_entries(cu_count, dt="f32", tail=3):
    """Degree 9 and more entries than one sweep of the dots kernel's persistent grid covers."""
    rng = np.random.default_rng(7)
    n_rows = DOT_BLOCK * DOT_BLOCKS_PER_CU * cu_count // 9 + 301
    return _finish([9] * n_rows, {0: "first", n_rows - 1: "last"}, {}, 0, rng, dt, tail, rng.integers(-8, 9, n_rows) / 4.0)


def score_graph(g):
    """The input of _gat_ref.forward (one head, two columns) whose scores are g's: Wh_i = [score_row_i or 0, score_col_i],
    attention = [1, 0 ; 0, 1]."""
    Wh = np.zeros((g["n_cols"], 2))
    Wh[:g["n_rows"], 0] = g["score_row"]
    Wh[:, 1] = g["score_col"]
    return dict(rowptr=g["rowptr"], col=g["col"], val=g["val"], Wh=Wh, att=np.array([1.0, 0.0, 0.0, 1.0]))


def forward_ref(g, rule="zero"):
    """_gat_ref.forward on g's scores: E, S, their bounds, live, dead, row"""
    return R.forward(score_graph(g), 1, dead_rule=rule, out="f32")


def edge_tables(g, F):
    """(Wh [n_cols, F], G [n_rows, F]) of the backward's own products: fp32 values as float64"""
    rng = np.random.default_rng([F, 17])
    return R._round(rng.uniform(-1, 1, (g["n_cols"], F)), "f32"), R._round(rng.standard_normal((g["n_rows"], F)), "f32")


def row_statistics(g, ref):
    """(row_max, row_sum) of sgx_gat_stats in float64 from the forward restatement: the maximum of a row's live scores and
    the sum of exp(E - max) over them, both 0 on a row without a live entry."""
    x = np.where(ref["live"], ref["E"], -np.inf)
    m = R._seg(np.maximum, x, g["rowptr"], -np.inf)
    m = np.where(np.isfinite(m), m, 0.0)
    p = np.where(ref["live"], np.exp(np.where(ref["live"], ref["E"] - m[ref["row"]], 0.0)), 0.0)
    return m, R._seg(np.add, p, g["rowptr"], 0.0)


# ---- graphs for the attention gradient: (rowptr, col, sg, g1) with arbitrary sg and g1 ----------------------------------

def attention_inputs(rowptr, col_cap, nnz, seed):
    """sg [capacity] (NaN behind nnz) and g1 [n_rows] in (-1, 1); g1 is NOT the row sums of sg.  The entries of rows over
    the cut are 8 times as large, so that one such row left out of 70 001 rows' sum stands well clear of the bound."""
    rng = np.random.default_rng([seed, 3])
    sg = np.full(len(col_cap), np.nan, np.float32)
    sg[:nnz] = (rng.random(nnz) * 2 - 1).astype(np.float32)
    sg[:nnz] *= np.where(np.repeat(np.diff(rowptr), np.diff(rowptr)) > LONG_ROW_CUT, np.float32(8), np.float32(1))
    g1 = (rng.random(len(rowptr) - 1) * 2 - 1).astype(np.float32)
    return sg, g1


MANY_ROWS = 70_001


def many_rows(tail=9):
    """70 001 rows and columns, degree 0..3 almost everywhere.  rps = 69 here, so a workgroup's run is a window of 64 rows
    and a last window of 5 -- there is no window between them at this row count.  Long rows, by run:
      run 3      257 entries on the run's first row, 1 025 on the last row of its first window, 300 on the first row of
                 its last window: three long rows found through the same LDS mask word, two of them in one window;
      run 500    300 entries on the run's last row (the last window's last row);
      last run   257 entries on the matrix's very last row (the run is cut short by n_rows: 35 rows).
    Returns the dict of _finish plus `placed`: name -> (row, entries)."""
    n = MANY_ROWS
    rps = rows_per_slice(n)
    rng = np.random.default_rng(8)
    lens = rng.integers(0, 4, n).tolist()
    placed = {"run3_first_row": (3 * rps, 257), "run3_first_window_last_row": (3 * rps + 63, 1025),
              "run3_last_window_first_row": (3 * rps + 64, 300), "run500_last_row": (500 * rps + rps - 1, 300),
              "last_row": (n - 1, 257)}
    names = {}
    for name, (r, k) in placed.items():
        lens[r], names[r] = k, name
    g = _finish(lens, names, {}, 0, rng, "f32", tail, np.zeros(n))
    g["placed"] = placed
    return g


def hub(n_cols, tail=6):
    """Rows of exactly WORKERS x 256 and WORKERS x 256 + 1 entries for 16 workers (LPR 16), and one of 65 537 entries: 257
    chunks, the second round of the chunk loop even with the 256 workers of LPR 1.  (The main graph's len1024 / len1025
    are the pair for the 4 workers of LPR 64.)"""
    rng = np.random.default_rng(9)
    lens = [2, 0, 4096, 5, 4097, 0, 1, 65537, 3] + [int(d) for d in rng.integers(0, 5, 120)]
    names = {2: "len4096", 4: "len4097", 7: "len65537"}
    assert n_cols >= len(lens)
    return _finish(lens, names, {}, n_cols - len(lens), rng, "f32", tail, np.zeros(len(lens)))


def attention_depth(F, rowptr):
    """The longest addition chain of an element of sgx_gat_attention_grad's two halves, from its summation order:
      rows' half     one fma per row of a worker's share of the run, the WORKERS partials, the slices;
      entries' half  an fma chain of at most 256 per row or chunk, then either the rows of a worker's share and the WORKERS
                     partials, or the chunks of a long row in chunk order; one addition per long row of the run; the slices.
    Returns (d_rows, d_entries)."""
    n = len(rowptr) - 1
    deg = np.diff(rowptr)
    W, n_slices, rps = attention_workers(F), attention_slices(n), rows_per_slice(n)
    share = -(-rps // W)
    long_rows = deg > LONG_ROW_CUT
    chunks = int(-(-deg.max() // LONG_ROW_CUT)) if long_rows.any() else 0
    per_run = int(np.add.reduceat(long_rows.astype(np.int64), np.arange(0, n, rps)).max()) if n else 0
    d_rows = share + W + n_slices
    d_ent = min(int(deg.max()) if n else 0, LONG_ROW_CUT) + max(share + W, chunks) + per_run + n_slices
    return d_rows, d_ent


def attention_bound(F, rowptr, magnitude):
    """(d + 2) 2^-24 sum |term| per element of [Wh^T g1 ; Wh^T colsum(sg)], d from attention_depth"""
    d_rows, d_ent = attention_depth(F, rowptr)
    d = np.concatenate([np.full(F, d_rows + 2.0), np.full(F, d_ent + 2.0)])
    return d * 2.0 ** -24 * magnitude

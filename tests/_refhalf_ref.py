"""SGX_ACC_REF_HALF restated in numpy float16, and the inputs the exact-mode arm tests run it on.  Plain numpy; nothing
here touches the GPU or oracle/sgx_oracle.c.

The mode (csrc/refhalf.hip): every product and every add is rounded to binary16; an output element keeps four partial
sums; entry i of its row goes to partial (phase + i) mod 4; the partials are folded ((p0 + p1) + p2) + p3; the ReLU is
v > 0 ? v : +0.  numpy's float16 `*` and `+` compute in float32 and round once to half: a product of two halves is exact in
float32 and a float32 sum of two halves rounds to the correctly rounded half sum (24 >= 2 * 11 + 2), so each numpy
operation below is one operation of the mode.

phase: the reference streams SPMM_BLOCK consecutive rows (an sblock) as one sequence and each of its threads owns a
contiguous block of n_rows // threads rows, the last one the remainder as well; sblocks restart at a thread's first row.
The phase of row r is the number of stream positions of its sblock before it, mod 4: stored entries for a CSR stream,
M per row for the dense stream (zeros take part).

Two facts about values that the tests rely on:
  * a sum is never -0.  Every partial starts at +0 and in round-to-nearest x + y is -0 only when x and y both are, so a
    partial, and with it the fold, is +0 where all products are -0.  "negzero" below is such a row: its products are -0,
    its sum must be +0 with and without the ReLU -- a kernel that started a partial from its first product would store
    0x8000.  The only zeros the ReLU ever sees are therefore +0; what it does turn into +0 are NaN and negative values.
  * the NaN of inf - inf.  IEEE 754 leaves its sign and payload open; the x86 adders numpy and the oracle run on and the
    GPU's half adders all produce the negative quiet NaN, 0xfe00 as a half, and later adds pass it on unchanged.  The
    comparisons therefore hold NaNs to their bit patterns like every other value.
"""
import numpy as np

LAT = 4
H = np.float16
_QUIET = dict(over="ignore", invalid="ignore", under="ignore")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float16).view(np.uint16)


def first_row(r, n_rows, spmm_block, threads):
    """First row of the sblock that holds row r (r may be an array)."""
    r = np.asarray(r, np.int64)
    blk = n_rows // threads
    t = np.minimum(r // blk, threads - 1) if blk > 0 else np.full_like(r, threads - 1)
    first = t * blk
    return first + (r - first) // spmm_block * spmm_block


def mac(p, v, t):
    """p + v * t: the product rounded to half, then the sum rounded to half"""
    return p + v * t


def fold(p):
    return ((p[0] + p[1]) + p[2]) + p[3]


def relu_exact(v):
    return np.where(v > 0, v, H(0))


def csr_stage(rowptr, col, val, table, spmm_block=1, threads=1, relu=False, _first_row=first_row, _mac=mac, _fold=fold):
    """out[r, :] = sum over row r of val[e] * table[col[e], :] in the mode's arithmetic.  The _hooks replace one piece
    of the arithmetic each; the sensitivity tests use them, nothing else does."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    val = np.asarray(val, H)
    table = np.asarray(table, H)
    n = len(rowptr) - 1
    rows = np.arange(n)
    phase = (rowptr[:-1] - rowptr[_first_row(rows, n, spmm_block, threads)]) % LAT
    deg = np.diff(rowptr)
    p = np.zeros((LAT, n, table.shape[1]), H)
    with np.errstate(**_QUIET):
        for i in range(int(deg.max()) if n else 0):              # entry i of every row that has one
            has = deg > i
            for ph in range(LAT):
                r = np.nonzero(has & (phase == ph))[0]
                if len(r):
                    e = rowptr[r] + i
                    l = (ph + i) % LAT
                    p[l, r] = _mac(p[l, r], val[e, None], table[col[e]])
        out = _fold(p)
        return relu_exact(out) if relu else out


def dense_stage(X, Wt, spmm_block=1, threads=1, _first_row=first_row):
    """out[r, j] = sum_k X[r, k] * Wt[j, k] with the dense stream's rule: position k of row r goes to partial
    (phase + k) mod 4, zeros included.  A loop over k with all rows at once, the rows sorted by phase so that each of the
    four groups is a slice."""
    X = np.asarray(X, H)
    W = np.ascontiguousarray(np.asarray(Wt, H).T)                # [M, P]
    n, M = X.shape
    rows = np.arange(n)
    phase = ((rows - _first_row(rows, n, spmm_block, threads)) * M) % LAT
    order = np.argsort(phase, kind="stable")
    cut = np.searchsorted(phase[order], np.arange(LAT + 1))
    Xs = X[order]
    p = np.zeros((LAT, n, W.shape[1]), H)
    with np.errstate(**_QUIET):
        for k in range(M):
            for ph in range(LAT):
                a, b = cut[ph], cut[ph + 1]
                if b > a:
                    l = (ph + k) % LAT
                    p[l, a:b] = mac(p[l, a:b], Xs[a:b, k, None], W[k])
        out = np.empty((n, W.shape[1]), H)
        out[order] = fold(p)
    return out


def layer(adj, fea, Wt, relu=False, spmm_block=1, fea_threads=1, adj_threads=1):
    """(D, H) of one layer D = act(A . (X . W)): fea a CSR triple (sparse features) or a dense [M_adj, M_fea] array."""
    Wt = np.asarray(Wt, H)
    if isinstance(fea, tuple):
        Hm = csr_stage(fea[0], fea[1], fea[2], np.ascontiguousarray(Wt.T), spmm_block, fea_threads)
    else:
        Hm = dense_stage(fea, Wt, spmm_block, fea_threads)
    return csr_stage(adj[0], adj[1], adj[2], Hm, spmm_block, adj_threads, relu), Hm


# ---- inputs -------------------------------------------------------------------------------------------------------------

N_GRAPH = 598                    # ordinary rows; 603 with the hostile rows: neither a multiple of 4, 16 or 64
N_COLS = 601                     # table rows; ordinary rows gather from [0, N_ORD), the hostile table rows lie behind
N_ORD = 590
T_BIG, T_ONE, T_NEGZ, T_SUB, T_NEG = 590, 591, 592, 593, 594
_FORCED = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 31, 7: 32, 8: 33, 9: 63, 10: 64, 11: 65, 12: 300,
           21: 0, 22: 0}       # rows 21 and 22: two empty rows inside one sblock of 3 (21..23) and of 4 (20..23)


def _csr_of(rng, deg, n_cols, scale):
    deg = np.asarray(deg, np.int64)
    rp = np.zeros(len(deg) + 1, np.int32)
    rp[1:] = np.cumsum(deg)
    ci = np.concatenate([np.sort(rng.choice(n_cols, int(d), replace=False)) for d in deg] + [np.zeros(0, np.int64)])
    va = ((rng.random(int(rp[-1])) - 0.3) * scale).astype(H)
    va[va == 0] = H(0.25)
    return rp, ci.astype(np.int32), va


def adj_graph():
    """598 x 601 CSR: row lengths 0..5, one either side of every lane-group piece (31..33, 63..65), one row of 300, two
    consecutive empty rows, the rest Poisson around 6 (capped at 40)."""
    rng = np.random.default_rng(598)
    deg = np.minimum(rng.poisson(6.0, N_GRAPH), 40)
    for r, d in _FORCED.items():
        deg[r] = d
    return _csr_of(rng, deg, N_ORD, 1.2)


def table(P, seed=0):
    """[601, P] half table: N(0, 0.5) with about a tenth zeros of either sign; the rows the hostile rows gather from
    hold one value in every column: 60000, 1, -0, 3 * 2^-24 (subnormal) and -2^-20 (subnormal)."""
    rng = np.random.default_rng(1000 + P + seed)
    t = (rng.standard_normal((N_COLS, P)) * 0.5).astype(H)
    z = rng.random((N_COLS, P))
    t[z < 0.05] = H(0.0)
    t[z > 0.95] = H(-0.0)
    t[T_BIG], t[T_ONE], t[T_NEGZ] = H(60000.0), H(1.0), H(-0.0)
    t[T_SUB], t[T_NEG] = H(3 * 2.0 ** -24), H(-2.0 ** -20)
    return t


def hostile_rows(csr):
    """(csr with five rows appended, {name: row index}).  Entries i and i + 4 of a row share a partial whatever the phase:
      inf        60000 + 60000 in one partial: +inf, in the sum and not in any operand
      nan        +inf in one partial, -inf in the next: the fold forms inf - inf
      negzero    every product is 1 * -0 = -0; the sum is +0 (see the module docstring)
      subnormal  0.5 * (3 * 2^-24) is a tie and rounds to 2^-23; three of them: 6 * 2^-24, a positive subnormal
      negsub     five times 1 * -2^-20: a negative subnormal, +0 after the ReLU"""
    rp, ci, va = csr
    new = {
        "inf": [(T_BIG, 1.0), (T_ONE, 1.0), (T_ONE, 0.5), (T_ONE, -1.0), (T_BIG, 1.0)],
        "nan": [(T_BIG, 1.0), (T_BIG, -1.0), (T_ONE, 1.0), (T_ONE, 1.0), (T_BIG, 1.0), (T_BIG, -1.0)],
        "negzero": [(T_NEGZ, 1.0)] * 5,
        "subnormal": [(T_SUB, 0.5)] * 3,
        "negsub": [(T_NEG, 1.0)] * 5,
    }
    names, rp, ci, va = {}, list(rp), list(ci), list(va)
    for name, entries in new.items():
        names[name] = len(rp) - 1
        ci += [c for c, _ in entries]
        va += [H(v) for _, v in entries]
        rp.append(len(ci))
    return (np.array(rp, np.int32), np.array(ci, np.int32), np.array(va, H)), names


def hostile_graph():
    return hostile_rows(adj_graph())


def dense_case(n, M, P):
    """(X [n, M], Wt [P, M]) for the dense stage: about 30 % of X is zero.  Columns 0 and 4 of W are +1 and columns 1 and
    5 are -1 in every output; row 1 of X holds 60000 at k = 0, 4 (a partial overflows to +inf), row 2 at k = 0, 1, 4, 5
    (+inf and -inf: NaN in the fold) -- DENSE_INF_ROW, DENSE_NAN_ROW."""
    rng = np.random.default_rng(n * 31 + M * 7 + P)
    x = (rng.standard_normal((n, M)) * (rng.random((n, M)) < 0.7)).astype(H)
    wt = (rng.standard_normal((P, M)) * (1.0 / np.sqrt(M))).astype(H)
    wt[:, [0, 4]] = H(1.0)
    wt[:, [1, 5]] = H(-1.0)
    x[DENSE_INF_ROW, :8] = H(0.5)
    x[DENSE_INF_ROW, [0, 4]] = H(60000.0)
    x[DENSE_NAN_ROW, :8] = H(0.5)
    x[DENSE_NAN_ROW, [0, 1, 4, 5]] = H(60000.0)
    return x, wt


DENSE_INF_ROW, DENSE_NAN_ROW = 1, 2


def layer_case(n, M, P, sparse):
    """(adj [n, n] CSR, features, Wt [P, M]): features a CSR triple (sparse) or a dense array with 30 % zeros."""
    rng = np.random.default_rng(n * 13 + M * 5 + P + int(sparse))
    adj = _csr_of(rng, np.minimum(rng.poisson(5.0, n), min(n, 30)), n, 0.8)
    wt = (rng.standard_normal((P, M)) * (1.0 / np.sqrt(M))).astype(H)
    if sparse:
        fea = _csr_of(rng, np.minimum(rng.poisson(7.0, n), M), M, 1.5)
    else:
        fea = (rng.standard_normal((n, M)) * (rng.random((n, M)) < 0.7)).astype(H)
    return adj, fea, wt


# ---- the cases of tests/test_gpu_refhalf_arms.py; test_refhalf_ref_cpu.py holds the restatement to the oracle on each ----
AH_WIDTHS = (21, 24, 40, 41, 64, 100, 129, 256, 300, 512, 520, 1000)
AH_BLOCKS = (1, 3, 4)
DENSE_CASES = ((1100, 70, 100), (1100, 71, 100), (1100, 130, 300), (1100, 67, 300), (1100, 40, 300), (1100, 33, 600),
               (1000, 33, 100), (8192 + 23, 40, 300))
DENSE_BLOCKS = (1, 3)
# (n, M, P, sparse features, spmm_block, fea_threads, adj_threads); at 1101 rows no thread's block (367 / 275, 220 / 550,
# 275 / 220 rows) is a multiple of its spmm_block, so every split moves sblock boundaries
LAYER_CASES = tuple((1101, M, P, sparse, sb, ft, at)
                    for (M, P, sparse) in ((64, 129, True), (40, 100, False), (41, 100, False))
                    for (sb, ft, at) in ((4, 3, 4), (3, 5, 2), (3, 4, 5))) + (
    (3, 64, 129, True, 4, 4, 4), (3, 40, 100, False, 4, 4, 4), (3, 41, 100, False, 2, 4, 4),
    (1023, 40, 100, False, 3, 2, 1), (1023, 41, 100, False, 3, 2, 1))

"""The two-pass aggregation (sgx_spmm_csr_acc) restated in float64, with its derived error bounds, and the CSR inputs the
acc-arm and partition tests run it on.  Plain numpy; nothing here touches the GPU.

One pass over an edge subset S of A adds  sum_{e in S, row(e) = i} A_e H[col_e, j]  to an fp32 accumulator that starts at
acc_in[i, j] (or 0).  The restatement is the dense product of the subset in float64 and, beside it, scale = |A| @ |H| and
the number of terms n_i of every row.

Bounds (U = 2^-24, the fp32 unit roundoff), derived and not tuned:

    partial   |got - want| <= (n_i + 2) U scale_ij
              An fp32 fma adds one rounding per term; n terms summed in ANY order (the edge-order chain of the row kernels,
              the lane-group fold and the chunk-order sum of the split path) are off by at most gamma_n = nU / (1 - nU)
              times the sum of the terms' magnitudes, and (n + 2) U >= gamma_n for every n used here.
    final     one more rounding, to the storage type:  2^-11 |want| + 2^-25 for fp16 (the second term is half the spacing
              of fp16 subnormals), 2^-24 |want| for fp32.  The ReLU is 1-Lipschitz and adds nothing.
    2nd pass  checked against float64(acc_in AS THE GPU PRODUCED IT) + the float64 sum of pass 2, so its error is one
              pass's: acc_in is one more term of magnitude |acc_in|, scale = |acc_in| + scale_2, n = n_2.

With values of magnitude ~1/2 a ten-edge row has scale ~2.5 and a partial bound of 12 U 2.5 ~ 2e-6, a final fp16 bound of
~5e-4 |want|; dropping or doubling one of its edges moves the sum by ~0.25, five and three orders of magnitude outside.
"""
import numpy as np

U = 2.0 ** -24
NP_DTYPE = {"f16": np.float16, "f32": np.float32}


def rounded(a, dt):
    """float64 array of values that the storage type `dt` holds exactly"""
    return np.asarray(a, np.float64).astype(NP_DTYPE[dt]).astype(np.float64)


def rows_of(rp):
    return np.repeat(np.arange(len(rp) - 1), np.diff(rp))


def subset(csr, mask):
    """The CSR of the edges where mask holds (edge order inside a row kept)."""
    rp, ci, va = csr
    n = len(rp) - 1
    out = np.zeros(n + 1, np.int32)
    out[1:] = np.cumsum(np.bincount(rows_of(rp)[mask], minlength=n))
    return out, ci[mask].astype(np.int32), va[mask]


def empty_like(csr):
    rp = csr[0]
    return np.zeros_like(rp), np.zeros(0, np.int32), np.zeros(0, np.float64)


def merge(a, b):
    """Row-wise concatenation [row of a | row of b] of two CSRs with the same number of rows."""
    (rpa, cia, vaa), (rpb, cib, vab) = a, b
    n = len(rpa) - 1
    rp = (rpa.astype(np.int64) + rpb).astype(np.int32)
    key = np.concatenate([rows_of(rpa) * 2, rows_of(rpb) * 2 + 1])
    order = np.argsort(key, kind="stable")
    assert len(rp) == n + 1
    return rp, np.concatenate([cia, cib])[order].astype(np.int32), np.concatenate([vaa, vab])[order]


def dense(csr, n_cols):
    rp, ci, va = csr
    out = np.zeros((len(rp) - 1, n_cols), np.float64)
    np.add.at(out, (rows_of(rp), ci.astype(np.int64)), np.asarray(va, np.float64))       # (duplicates add up)
    return out


def one_pass(csr, H):
    """(sum, scale, n_terms) of one pass in float64: A @ H, |A| @ |H|, entries per row."""
    rp, ci, va = csr
    H = np.asarray(H, np.float64)
    n_cols = H.shape[0]
    rows = rows_of(rp)
    absA = np.zeros((len(rp) - 1, n_cols), np.float64)
    np.add.at(absA, (rows, ci.astype(np.int64)), np.abs(np.asarray(va, np.float64)))
    return dense(csr, n_cols) @ H, absA @ np.abs(H), np.diff(rp).astype(np.float64)


def partial_bound(n_terms, scale):
    return (np.asarray(n_terms, np.float64)[:, None] + 2.0) * U * scale


def store_bound(want, dt):
    return (2.0 ** -11 * np.abs(want) + 2.0 ** -25) if dt == "f16" else U * np.abs(want)


def second_pass(acc_in, csr, H):
    """(want, bound) of the fp32 sums acc_in + A @ H given the acc_in that was actually fed in."""
    s, scale, n = one_pass(csr, H)
    acc = np.asarray(acc_in, np.float64)
    return acc + s, partial_bound(n, np.abs(acc) + scale)


def finished(want, bound, dt, relu):
    """(want, bound) of the stored result act(sums) in the storage type."""
    want = np.maximum(want, 0.0) if relu else want
    return want, bound + store_bound(want, dt)


def assert_within(what, got, want, bound):
    got = np.asarray(got, np.float64)
    bad = ~(np.abs(got - want) <= bound)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        worst = float(np.max(np.abs(got - want) / np.maximum(bound, 1e-300)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the bound in {len(set(np.argwhere(bad)[:, 0]))} "
                             f"rows, worst |err| / bound = {worst:.3g}; first at {i}: got {got[i]!r}, want {want[i]!r}, "
                             f"bound {bound[i]!r}")


def fma_chain_f32(csr, H, acc_in=None):
    """fp32 fma chain in edge order, per output element: acc = fl32(acc + a_e * h_e).  The product of two fp16 or fp32
    values is exact in float64 and the sum of it and an fp32 is rounded once to float64 and once to fp32 -- the fused
    operation up to a double rounding, which stays inside one fp32 rounding's bound."""
    rp, ci, va = csr
    H = np.asarray(H, np.float64)
    n = len(rp) - 1
    acc = np.zeros((n, H.shape[1]), np.float32) if acc_in is None else np.array(acc_in, np.float32)
    deg = np.diff(rp)
    for k in range(int(deg.max()) if n else 0):                  # the k-th edge of every row that has one
        r = np.nonzero(deg > k)[0]
        e = rp[r] + k
        acc[r] = (acc[r].astype(np.float64) + np.asarray(va, np.float64)[e, None] * H[ci[e]]).astype(np.float32)
    return acc


# ---- inputs -------------------------------------------------------------------------------------------------------------

def table(rng, n, P, dt):
    return rounded(rng.random((n, P)) - 0.4, dt)


def random_rows(rng, deg, lo, hi, dt):
    """A CSR with deg[i] distinct sorted columns in [lo, hi) per row, values in (-0.7, 1.3) of the storage type."""
    deg = np.asarray(deg, np.int64)
    rp = np.zeros(len(deg) + 1, np.int32)
    rp[1:] = np.cumsum(deg)
    ci = np.empty(int(rp[-1]), np.int32)
    for i in np.nonzero(deg)[0]:
        ci[rp[i]:rp[i + 1]] = lo + np.sort(rng.choice(hi - lo, int(deg[i]), replace=False))
    va = rng.random(int(rp[-1])) * 2.0 - 0.7
    va[va == 0] = 0.5
    return rp, ci, rounded(va, dt)


def two_pass_graph(seed, n_rows, n_cols, dt, mean1=6.0, mean2=6.0, p_empty=0.3, long1=(), long2=(), deg1=None, deg2=None):
    """(A, A1, A2): A1 holds columns below n_cols / 2, A2 the others, A both (row-wise [A1 | A2], columns sorted).  A row is
    empty in either pass with probability p_empty, so many rows are empty in one pass only and some in both.
    long1 / long2: (row, edges) pairs forced in pass 1 / pass 2."""
    rng = np.random.default_rng(seed)
    half = n_cols // 2
    degs = []
    for mean, forced, given in ((mean1, long1, deg1), (mean2, long2, deg2)):
        d = rng.poisson(mean, n_rows) if given is None else np.array(given, np.int64)
        if given is None:
            d = np.minimum(d, 40)
            d[rng.random(n_rows) < p_empty] = 0
        for r, k in forced:
            d[r] = k
        degs.append(d)
    A1 = random_rows(rng, degs[0], 0, half, dt)
    A2 = random_rows(rng, degs[1], half, n_cols, dt)
    return merge(A1, A2), A1, A2


# ---- the graphs of the acc-arm tests (tests/test_gpu_spmm_acc_arms.py on the kernels, test_spmm_acc_ref_cpu.py on the
# restatement): name -> (A, A1, A2).  The long rows of "split": in pass 1 only, in pass 2 only, in both.
_LONG1 = [(10, 65), (11, 513), (12, 1400), (20, 65), (21, 513), (22, 1400), (30, 0), (31, 0), (32, 0)]
_LONG2 = [(10, 0), (11, 0), (12, 0), (20, 65), (21, 513), (22, 1400), (30, 65), (31, 513), (32, 1400)]


def _tail_degrees(seed, n):
    """most rows of at most 8 entries, the others of 9..60, in random order: a plan orders them by degree"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(n) < 0.6, rng.integers(0, 9, n), rng.integers(9, 61, n))


GRAPHS = {
    "base": lambda dt: two_pass_graph(1, 1000, 800, dt, long1=[(5, 300), (7, 90)], long2=[(6, 200), (7, 90)]),
    "split": lambda dt: two_pass_graph(2, 1000, 3000, dt, long1=_LONG1, long2=_LONG2),
    "tail": lambda dt: two_pass_graph(3, 9000, 1200, dt, deg1=_tail_degrees(31, 9000), deg2=_tail_degrees(32, 9000),
                                      long1=[(100, 513), (102, 70)], long2=[(101, 200), (102, 70)]),
}
N_COLS = {"base": 800, "split": 3000, "tail": 1200}


def graph_table(name, P, dt):
    """the table the tests gather from for graph `name` at width P"""
    return table(np.random.default_rng(1000 + P), N_COLS[name], P, dt)

"""The ownership rule of the entry-split aggregation (sgx_spmm_csr_flat; "entry-split aggregation" in include/sgx.h)
restated in numpy, and the smallest graphs at which it can fail.  Plain numpy; nothing here touches the GPU.

With T = sgx_spmm_flat_chunk() and end = rowPtr[n_rows]: the stored entries are cut into chunks of T, chunk c = entries
[cT, min((c+1)T, end)).  A chunk owns the rows that start inside it; a row inside one chunk is stored by it in launch 1; a
row that crosses a chunk end leaves one fp32 partial per chunk it touches -- in the tail slot (2c + 1) of the chunk c it
starts in, its leader, and in the head slot (2k) of every later chunk k -- and is stored in launch 2 by the leader, which
adds the slots in chunk order.  An empty row starts at entry rowPtr[r] like any other: it belongs to the chunk that holds
that index, to the last live chunk when the index is `end`, to the single degenerate chunk 0 when end == 0.  The host may
pass a capacity above `end`: the chunks behind the end do nothing.

schedule() lists what every chunk does; the float64 value and the error bound of the result are tests/_spmm_acc_ref.py's
(one_pass, partial_bound, finished): the order of a row's sum is the rule's business, the bound holds for any order."""
import collections

import numpy as np

Schedule = collections.namedtuple("Schedule", "n_chunks stores reads partials sums")


def n_chunks(nnz, T):
    return max(1, -(-int(nnz) // T))


def schedule(rp, T, capacity=None):
    """stores: (row, chunk, launch) -- launch 1 = the chunk's own wavefront, 2 = the second launch on behalf of the leader;
    reads: (chunk, row, e0, e1) -- entries [e0, e1) of that row read by that chunk; partials: (slot, row) written in launch
    1; sums: row -> the slots launch 2 adds, in order."""
    rp = np.asarray(rp, np.int64)
    n, end = len(rp) - 1, int(rp[-1])
    chunks = n_chunks(end if capacity is None else capacity, T)
    stores, reads, partials, sums = [], [], [], {}
    for c in range(chunks):
        lo = c * T
        if lo >= end and not (c == 0 and end == 0):
            continue                                            # a chunk of the capacity behind the end
        last = lo + T >= end
        hi = end if last else lo + T
        r_a = int(np.searchsorted(rp[:n], lo, "left"))
        r_b = n if last else int(np.searchsorted(rp[:n], hi, "left"))
        if r_a > 0 and rp[r_a] > lo and hi > lo:                # entry lo lies in a row that started earlier
            reads.append((c, r_a - 1, lo, int(min(rp[r_a], hi))))
            partials.append((2 * c, r_a - 1))
        for r in range(r_a, r_b):
            e0, e1 = int(rp[r]), int(rp[r + 1])
            if e1 > hi:                                         # starts here, ends later: this chunk leads it
                partials.append((2 * c + 1, r))
                sums[r] = [2 * c + 1] + [2 * k for k in range(c + 1, (e1 - 1) // T + 1)]
                stores.append((r, c, 2))
            else:
                stores.append((r, c, 1))
            if min(e1, hi) > e0:
                reads.append((c, r, e0, min(e1, hi)))
    return Schedule(chunks, stores, reads, partials, sums)


# ---- the graphs: name -> (degrees, capacity above the real count or 0), as functions of T ---------------------------------

def _fill(total, k=7):
    """rows of k entries (the last one shorter) that hold `total` entries in all"""
    return [k] * (total // k) + ([total % k] if total % k else [])


def degree_cases(T):
    return {
        "nnz_0": ([0] * 5, 0),
        "nnz_1": ([0, 1, 0], 0),
        "nnz_T-1": (_fill(T - 1), 0),
        "nnz_T": (_fill(T), 0),
        "nnz_T+1": (_fill(T + 1), 0),
        "long_leading": ([5 * T + 3, 4, 9, 0, 2], 0),                           # a leader that adds six partials
        "long_middle": ([3, 10, 5 * T + 3, 7, 1], 0),                           # and seven, starting inside a chunk
        "ends_on_chunk_end": ([T - 10, 10, 0, T + 50, 5], 0),                   # row 1 ends at T, row 2 is empty, row 3 crosses
        "empty_first_last": ([0, 0, 0] + _fill(T + 40, 9) + [0, 0], 0),
        "empty_run": ([100, T - 100] + [0] * 70 + [30, 0, 0], 0),               # 70 empty rows at index T, after a row ending there
        "empty_run_exact_end": (_fill(2 * T, 8) + [0] * 70, 0),                 # index = end = 2T: the last chunk's
        "one_row_short": ([3], 0),
        "one_row_long": ([T + 7], 0),
        "begins_on_last_entry": ([T - 1, 20, 4], 0),                            # row 1 begins on chunk 0's last entry
        "capacity": ([3, 10, 2 * T + 3, 7, 0, 1], 3 * T),
        "capacity_nnz_0": ([0] * 4, 3 * T),
        "capacity_exact_end": (_fill(T, 8) + [0, 0], 3 * T),
        "mixed": (list(np.random.default_rng(7).poisson(6.0, 200)) + [T // 2 + 3] * 5, 0),
    }


def build(deg, n_cols, dt, seed=0):
    """(rowptr, col, val) with deg[i] distinct columns per row where n_cols allows, any columns otherwise; values in
    (-0.7, 1.3) that the storage type `dt` holds exactly"""
    from _spmm_acc_ref import rounded
    rng = np.random.default_rng(seed)
    deg = np.asarray(deg, np.int64)
    rp = np.zeros(len(deg) + 1, np.int32)
    rp[1:] = np.cumsum(deg)
    ci = np.empty(int(rp[-1]), np.int32)
    for i in np.nonzero(deg)[0]:
        k = int(deg[i])
        ci[rp[i]:rp[i + 1]] = np.sort(rng.choice(n_cols, k, replace=False)) if k <= n_cols else rng.integers(0, n_cols, k)
    va = rng.random(int(rp[-1])) * 2.0 - 0.7
    va[va == 0] = 0.5
    return rp, ci, rounded(va, dt)

"""The rule of sgx_csr_transpose (include/sgx.h) restated in numpy: the stable sort of the stored positions by column."""
import numpy as np


def transpose(rowptr, col, val, n_cols):
    """-> (rowptr_t [n_cols + 1], col_t [nnz], val_t [nnz] or None, order [nnz]) of the CSR (rowptr, col, val)."""
    rowptr = np.asarray(rowptr, np.int64)
    nnz = int(rowptr[-1]) if len(rowptr) > 1 else 0
    col = np.asarray(col)[:nnz].astype(np.int64)
    row = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    order = np.argsort(col, kind="stable")
    rowptr_t = np.zeros(n_cols + 1, np.int64)
    rowptr_t[1:] = np.cumsum(np.bincount(col, minlength=n_cols)[:n_cols]) if n_cols else 0
    val_t = None if val is None else np.asarray(val)[:nnz][order]
    return rowptr_t.astype(np.int32), row[order].astype(np.int32), val_t, order.astype(np.int32)


def random_csr(rng, n_rows, n_cols, nnz, dtype=np.float32, unique=False):
    """A random CSR with nnz stored entries, ascending columns inside a row (repeats allowed unless unique)."""
    if unique:
        flat = np.sort(rng.choice(n_rows * n_cols, size=min(nnz, n_rows * n_cols), replace=False))
        row, col = flat // n_cols, flat % n_cols
    else:
        row = np.sort(rng.integers(0, n_rows, nnz))
        col = rng.integers(0, n_cols, nnz)
        o = np.lexsort((col, row))
        row, col = row[o], col[o]
    rowptr = np.zeros(n_rows + 1, np.int32)
    rowptr[1:] = np.cumsum(np.bincount(row, minlength=n_rows))
    val = (rng.standard_normal(len(col)) + 3.0).astype(dtype)
    return rowptr, col.astype(np.int32), val

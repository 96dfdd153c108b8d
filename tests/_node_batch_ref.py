"""Restatement of the two rules of "layer-ready node batches" (include/sgx.h) in numpy, for the node-batch tests: the
symmetric normalisation of a sampled CSR with its self loops, and the row gather of a feature CSR.  fp32 arithmetic with
numpy's correctly rounded float32 sqrt, division and products, in the order the header states."""
import numpy as np

F32 = np.float32


def sym_norm2_csr(rowptr, col, weights=None, fill=0.0, store=np.float32):
    """rowptr [n+1], col [E] (row i = the neighbours of node i, local ids), weights [E] or None (= 1), fill.
    -> rowptr_out [n+1] int64, col_out int64, val (`store`), dead bool [n], has_dead, max_row."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    n = len(rowptr) - 1
    w_in = np.ones(len(col), F32) if weights is None else np.asarray(weights, F32)
    out_ptr = np.zeros(n + 1, np.int64)
    cols, ws = [], []
    deg = np.zeros(n, F32)
    for r in range(n):
        c = col[rowptr[r]:rowptr[r + 1]]
        w = w_in[rowptr[r]:rowptr[r + 1]]
        if not (c == r).any():                              # the added loop: last in sampled order
            c = np.concatenate([c, [r]])
            w = np.concatenate([w, np.asarray([fill], F32)])
        order = np.argsort(c, kind="stable")                # by column; equal columns keep their order
        c, w = c[order], w[order].astype(F32)
        cols.append(c)
        ws.append(w)
        out_ptr[r + 1] = out_ptr[r] + len(c)
        deg[r] = np.cumsum(w, dtype=F32)[-1] if len(w) else F32(0)     # one by one, in stored order
    with np.errstate(divide="ignore"):
        dis = np.where(deg > 0, F32(1) / np.sqrt(deg, dtype=F32), F32(0)).astype(F32)
    col_out = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    w_out = np.concatenate(ws).astype(F32) if ws else np.zeros(0, F32)
    row = np.repeat(np.arange(n), np.diff(out_ptr))
    val = ((dis[row] * w_out).astype(F32) * dis[col_out]).astype(F32).astype(store)
    live = np.zeros(n, np.int64)
    np.add.at(live, row, (val.astype(F32) > 0).astype(np.int64))
    dead = live == 0
    max_row = int(np.diff(out_ptr).max()) if n else 0
    return out_ptr, col_out, val, dead, bool(dead.any()), max_row


def sym_norm2_f64(rowptr, col, weights=None, fill=0.0):
    """The same matrix's values evaluated in float64 (structure as sym_norm2_csr): w / sqrt(deg_r deg_c)."""
    out_ptr, col_out, _, _, _, _ = sym_norm2_csr(rowptr, col, weights, fill)
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    n = len(rowptr) - 1
    w_in = np.ones(len(col), np.float64) if weights is None else np.asarray(weights, np.float64)
    ws = []
    deg = np.zeros(n)
    for r in range(n):
        c = col[rowptr[r]:rowptr[r + 1]]
        w = w_in[rowptr[r]:rowptr[r + 1]]
        if not (c == r).any():
            c = np.concatenate([c, [r]])
            w = np.concatenate([w, [float(fill)]])
        w = w[np.argsort(c, kind="stable")]
        ws.append(w)
        deg[r] = w.sum()
    with np.errstate(divide="ignore"):
        dis = np.where(deg > 0, 1.0 / np.sqrt(deg), 0.0)
    w_out = np.concatenate(ws) if ws else np.zeros(0)
    row = np.repeat(np.arange(n), np.diff(out_ptr))
    return dis[row] * w_out * dis[col_out]


def gather_csr(rowptr, col, val, index, store=np.float32):
    """Rows `index` of the CSR (rowptr, col, val), in that order -> rowptr_out, col_out, val_out."""
    rowptr = np.asarray(rowptr, np.int64)
    index = np.asarray(index, np.int64)
    lens = rowptr[index + 1] - rowptr[index]
    out_ptr = np.zeros(len(index) + 1, np.int64)
    np.cumsum(lens, out=out_ptr[1:])
    take = np.concatenate([np.arange(rowptr[v], rowptr[v + 1]) for v in index]) if len(index) else np.zeros(0, np.int64)
    take = take.astype(np.int64)
    return out_ptr, np.asarray(col, np.int64)[take], np.asarray(val, F32)[take].astype(store)


def dense_to_csr(x):
    """The CSR of a dense matrix, zeros dropped, row-major -- what torch's to_sparse_csr gives."""
    x = np.asarray(x)
    r, c = np.nonzero(x)
    rowptr = np.zeros(x.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=x.shape[0]), out=rowptr[1:])
    return rowptr, c.astype(np.int64), x[r, c]

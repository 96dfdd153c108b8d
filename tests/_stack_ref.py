"""Float64 restatement of sgx_stack_forward (include/sgx.h, "a batch of small graphs"): the GCN chain of MOL cells
15-18 on a CSR adjacency, with an element-wise magnitude bound for what the device's rounding may change."""
import numpy as np


def csr_matmul(rowptr, col, val, H):
    """A @ H for a CSR A (numpy, float64)."""
    rowptr, col = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    row = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    out = np.zeros((len(rowptr) - 1, H.shape[1]), np.float64)
    np.add.at(out, row, np.asarray(val, np.float64)[:, None] * H[col])
    return out


def stack_f64(adj, x, weights, relus, graph_ptr, head_w=None, head_b=None):
    """adj = (rowptr, col, val); x dense [N, M] (a CSR feature matrix densified); weights W_l [M_l, P_l] (not
    transposed); relus per layer; graph_ptr [G+1].  Returns (layer outputs, pooled, logits or None), all float64:
        H_l = X_l W_l,  D_l = act(A H_l),  pooled[g] = mean of D_last over graph g,  logits = pooled W_head^T + b."""
    X = np.asarray(x, np.float64)
    outs = []
    for W, relu in zip(weights, relus):
        D = csr_matmul(*adj, X @ np.asarray(W, np.float64))
        X = np.maximum(D, 0.0) if relu else D
        outs.append(X)
    ptr = np.asarray(graph_ptr, np.int64)
    pooled = np.stack([X[a:b].mean(0) if b > a else np.zeros(X.shape[1]) for a, b in zip(ptr[:-1], ptr[1:])]) \
        if len(ptr) > 1 else np.zeros((0, X.shape[1]))
    logits = None
    if head_w is not None:
        logits = pooled @ np.asarray(head_w, np.float64).T
        if head_b is not None:
            logits = logits + np.asarray(head_b, np.float64)
    return outs, pooled, logits


def stack_bound(adj, x, weights, relus, graph_ptr, head_w, head_b, unit):
    """Element-wise bound on |device logits - stack_f64 logits| when every stage rounds to a format of unit roundoff
    `unit` and sums in fp32: the same chain on absolute values (the magnitude every error is relative to), times the
    roundings a value passes through -- two per layer (H and D), one per sum of fp32 terms counted by its length."""
    rowptr, col, val = adj
    deg = int(np.diff(np.asarray(rowptr)).max()) if len(rowptr) > 1 else 0
    absadj = (rowptr, col, np.abs(np.asarray(val, np.float64)))
    mags = stack_f64(absadj, np.abs(np.asarray(x, np.float64)), [np.abs(np.asarray(W, np.float64)) for W in weights],
                     [False] * len(weights), graph_ptr, np.abs(np.asarray(head_w, np.float64)),
                     None if head_b is None else np.abs(np.asarray(head_b, np.float64)))
    ptr = np.asarray(graph_ptr, np.int64)
    biggest = int(np.diff(ptr).max()) if len(ptr) > 1 else 0
    u32 = 2.0 ** -24
    steps = sum(2 * unit + (np.asarray(W).shape[0] + deg) * u32 for W in weights) + (biggest + np.asarray(head_w).shape[1] + 8) * u32
    return 2.0 * steps * mags[2] + 1e-30

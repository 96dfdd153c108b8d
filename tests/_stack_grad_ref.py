"""Float64 restatement of sgx_stack_backward (include/sgx.h, "training: the backward of that stack"): the weight
gradients of the GCN stack as the model's layer-by-layer backward forms them (FPYNQ / RPYNQ / ReadoutMean of
sgracex1_amd/molecule_gcn.py), without the roundings to dtype, and an element-wise magnitude bound for them."""
import numpy as np

from _stack_ref import csr_matmul, stack_f64


def _graph_of_rows(graph_ptr, n_rows):
    ptr = np.asarray(graph_ptr, np.int64)
    return np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))[:n_rows], np.diff(ptr)


def stack_grad_f64(adj, x, weights, relus, graph_ptr, grad_pooled, outs=None):
    """adj = (rowptr, col, val); x dense [N, M]; weights W_l [M_l, P_l]; relus per layer; graph_ptr [G+1];
    grad_pooled [G, P_last].  outs: the forward's layer outputs D_l (their zeros are the ReLU masks, D_{l-1} is X_l);
    computed with stack_f64 when None.  Returns (dW list, G list), float64:
        g_{L-1}[r] = grad_pooled[graph(r)] / n_graph;  per layer from the top: g_l = 0 where relu_l and D_l == 0,
        G_l = A g_l,  dW_l = X_l^T G_l,  g_{l-1} = G_l W_l^T."""
    x = np.asarray(x, np.float64)
    if outs is None:
        outs, _, _ = stack_f64(adj, x, weights, relus, graph_ptr)
    outs = [np.asarray(D, np.float64) for D in outs]
    N = x.shape[0]
    rows_g, sizes = _graph_of_rows(graph_ptr, N)
    gp = np.asarray(grad_pooled, np.float64)
    g = gp[rows_g] / np.maximum(sizes[rows_g], 1)[:, None] if N else np.zeros((0, gp.shape[1]))
    L = len(weights)
    dWs, Gs = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        if relus[l]:
            g = np.where(outs[l] == 0, 0.0, g)
        G = csr_matmul(*adj, g)
        X = x if l == 0 else outs[l - 1]
        dWs[l] = X.T @ G
        Gs[l] = G
        if l > 0:
            g = G @ np.asarray(weights[l], np.float64).T
    return dWs, Gs


def stack_grad_bound(adj, x, weights, graph_ptr, grad_pooled, outs, unit):
    """Element-wise bound on |device dW_l - stack_grad_f64 dW_l| (with the device's D_l as outs): the same chain on
    absolute values and without masks (the magnitude every error is relative to), times the roundings a value passes
    through -- one to the storage format (unit) per gradient handed down, one per fp32 term of every sum it passes
    (degree, width, the batch's rows for dW) -- twice, for first-order slack."""
    rowptr, col, val = adj
    deg = int(np.diff(np.asarray(rowptr)).max()) if len(rowptr) > 1 else 0
    absadj = (rowptr, col, np.abs(np.asarray(val, np.float64)))
    x = np.abs(np.asarray(x, np.float64))
    absw = [np.abs(np.asarray(W, np.float64)) for W in weights]
    L = len(weights)
    dWs, _ = stack_grad_f64(absadj, x, absw, [False] * L, graph_ptr, np.abs(np.asarray(grad_pooled, np.float64)),
                            outs=[np.abs(np.asarray(D, np.float64)) for D in outs])
    u32 = 2.0 ** -24
    n = x.shape[0]
    bounds = []
    for l in range(L):
        steps = unit + (deg + n + 2) * u32
        for j in range(l + 1, L):
            steps += unit + (deg + np.asarray(weights[j]).shape[1] + 2) * u32
        bounds.append(2.0 * steps * dWs[l] + 1e-30)
    return bounds

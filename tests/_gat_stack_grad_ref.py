"""Float64 restatement of sgx_gat_stack_backward (include/sgx.h, "training the GAT stack"), with element-wise magnitude
bounds and the tolerance that goes with them.

The chain is tests/_stack_grad_ref.stack_grad_f64's with a per-layer choice of P in G_l = P g_l: the adjacency (a GCN
layer, the same three lines) or the layer's edge softmax S (a GAT layer), where the gradients of the layer are
tests/_layer_grad_ref.edges' -- FPYNQ_GAT.backward on the edge list -- called with no dead row, so that a row without a
live entry keeps S = 0 on its stored entries (the stack's zero rule) and contributes nothing:

    g_{L-1}[r] = grad_pooled[graph(r)] / n_graph;  per layer from the top: g_l = 0 where relu_l and D_l == 0
    GCN   G_l = A g_l
    GAT   Wh = X_l W_l;  E, S = the edge softmax of tests/_gat_ref.forward on Wh (dead_rule "zero")
          G_l = S g_l;  grad_attention_l = edges(...)["grad_attention"]     (slope from the device's E when given)
    dW_l = X_l^T G_l;  g_{l-1} = G_l W_l^T

It takes the device's D_l as X_{l+1} and as the ReLU masks, and the device's E, when given, for the LeakyReLU slope, so
that a score whose sign differs between fp32 and float64 cannot turn the comparison into a jump.

Bounds: the same chain on absolute values without masks and with + for the softmax backward's - (as both references it
is built on do); every error is measured in units of that magnitude.  The tolerance in those units counts roundings, with
unit = the unit roundoff of the storage type, U = 2^-24, deg the longest row, n the batch's rows, K_l / P_l a layer's
widths, and rel_l the relative error of a GAT layer's S:

    rel_l     = max over live entries of (bS_e - 2^-126) / S_e from _gat_ref.forward (the fp32 softmax on a given Wh)
                + 2 max_e (bWh_i . |a1| + bWh_c . |a2|),  bWh = (K_l + 2) U |X_l| |W_l|: the device forms Wh again in
                fp32, which moves a score by that much and a weight by twice the row's largest move
    pass_j    = unit + (deg + P_j + 2) U + rel_j (GAT)      what layer j adds to a gradient handed down through it: the
                rounding of g_j to the storage type, the sums of P g_j and of G_j W_j^T, and S itself
    G_l       : unit + (deg + 2) U + rel_l (GAT) + sum_{j > l} pass_j
    dW_l      : that + n U                                   (the batch's rows of X_l^T G_l)
    grad_attention_l : unit + sum_{j > l} pass_j             (g_l as handed down)
                + 3 rel_l                                    (S in dx, in S rs, and in rs)
                + (P_l + 2 K_l + 3 deg + n + 16) U           (d_e: a dot over P_l on a Wh off by (K_l + 2) U; rs, g1 and T:
                                                             three row sums; sg: a few operations; the batch's rows; Wh
                                                             again in sum_i g1_i Wh_i)
    all times 2, for first-order slack, as stack_grad_bound does.

A rounding to the storage type is off by unit |v| only above the type's subnormal range; below it the error is up to half
the subnormal spacing, sub (2^-25 for fp16, 2^-150 for fp32: _gat_ref.OUT_SUB).  Every gradient that is rounded -- g_{L-1}
and each one handed down -- therefore enters the chain of magnitudes as |g| + sub / unit, so that unit times the magnitude
covers unit |g| + sub.  (A batch of thousands of graphs draws pooled gradients below fp16's 6e-5 often enough to show it.)
"""
import numpy as np
import torch

import _gat_ref as R
import _layer_grad_ref as LG
from _stack_grad_ref import _graph_of_rows
from _stack_ref import csr_matmul

U = 2.0 ** -24


def _t(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype)


def gat_stack_grad_f64(adj, x, weights, atts, relus, graph_ptr, grad_pooled, outs, alpha=0.2, E_dev=None, unit=U, sub=0.0):
    """adj = (rowptr, col, val); x dense [N, M]; weights W_l [M_l, P_l]; atts[l] = attention [2 P_l] or None (a GCN
    layer); relus per layer; graph_ptr [G+1]; grad_pooled [G, P_last]; outs: the forward's D_l (D_{l-1} is X_l, their
    zeros are the ReLU masks; an entry the chain never reads may be None); E_dev[l]: the device's E of a GAT layer, for
    the LeakyReLU slope (None: the restatement's own); unit, sub: the storage type's unit roundoff and half its subnormal
    spacing.
    Returns a dict of per-layer lists: dW, dA (None for a GCN layer), G, E, S, bE, bS (GAT layers; bounds on the device's
    E and S with Wh formed again in fp32), dead, the magnitudes mW, mA, mG and the tolerances tW, tA, tG in units of
    them, so that |device - reference| <= t * m + 1e-30 element-wise."""
    rowptr, col, val = (np.asarray(a) for a in adj)
    rowptr, col = rowptr.astype(np.int64), col.astype(np.int64)
    nnz = int(rowptr[-1]) if len(rowptr) else 0
    col, val = col[:nnz], val.astype(np.float64)[:nnz]
    x = np.asarray(x, np.float64)
    N = x.shape[0]
    L = len(weights)
    Ws = [np.asarray(W, np.float64) for W in weights]
    Xs = [x] + [None if D is None else np.asarray(D, np.float64) for D in outs[:-1]]
    rows_g, sizes = _graph_of_rows(graph_ptr, N)
    gp = np.asarray(grad_pooled, np.float64)
    size = np.maximum(sizes[rows_g], 1)[:, None]
    g = gp[rows_g] / size if N else np.zeros((0, gp.shape[1]))
    ga = np.abs(gp)[rows_g] / size if N else np.zeros((0, gp.shape[1]))     # the chain on absolute values
    ga = ga + sub / unit
    deg = int(np.diff(rowptr).max()) if len(rowptr) > 1 else 0
    tr, tc = _t(rowptr, torch.int64), _t(col, torch.int64)
    res = {k: [None] * L for k in ("dW", "dA", "G", "E", "S", "bE", "bS", "dead", "mW", "mA", "mG", "tW", "tA", "tG")}
    above = 0.0                                                       # sum of pass_j over the layers above
    for l in range(L - 1, -1, -1):
        W, X = Ws[l], Xs[l]
        K, P = W.shape
        if relus[l]:
            g = np.where(np.asarray(outs[l], np.float64) == 0, 0.0, g)
        rel = 0.0
        if atts[l] is None:
            G = csr_matmul(rowptr, col, val, g)
            Ga = csr_matmul(rowptr, col, np.abs(val), ga)
        else:
            att = np.asarray(atts[l], np.float64).reshape(-1)
            Wh, Wha = X @ W, np.abs(X) @ np.abs(W)
            r = R.forward(dict(rowptr=rowptr, col=col, val=val, Wh=Wh, att=att), 1, alpha=alpha, relu=False,
                          dead_rule="zero", out="f32")
            row, live = r["row"], r["live"]
            bWh = (K + 2) * U * Wha
            extra = (bWh @ np.abs(att[:P]))[row] + (bWh @ np.abs(att[P:]))[col]
            mx = R._seg(np.maximum, np.where(live, extra, 0.0), rowptr, 0.0)
            S_, bS = r["S"], r["bS"] + 2 * r["S"] * mx[row]
            pos = live & (S_ > 0)
            rel = float(((bS[pos] - R.TINY32) / S_[pos]).max()) if pos.any() else 0.0
            E_slope = r["E"] if E_dev is None or E_dev[l] is None else np.asarray(E_dev[l], np.float64)[:nnz]
            no_dead = torch.zeros(N, dtype=torch.bool)
            kw = dict(gat=True, E=_t(E_slope), S=_t(S_), dead=no_dead, alpha=float(np.float32(alpha)))
            grads, _ = LG.edges(tr, tc, _t(val), _t(X), _t(W), _t(g), **kw)
            _, mags = LG.edges(tr, tc, _t(val), _t(X), _t(W), _t(ga), **kw)
            G = csr_matmul(rowptr, col, S_, g)
            Ga = csr_matmul(rowptr, col, S_, ga)
            res["dA"][l] = grads["grad_attention"].numpy().reshape(-1)
            res["mA"][l] = mags["grad_attention"].numpy().reshape(-1)
            res["tA"][l] = 2.0 * (unit + above + 3 * rel + (P + 2 * K + 3 * deg + N + 16) * U)
            res["E"][l], res["S"][l], res["bE"][l], res["bS"][l] = r["E"], S_, r["bE"] + extra, bS
            res["dead"][l] = r["dead"]
        res["G"][l], res["mG"][l] = G, Ga
        res["dW"][l], res["mW"][l] = X.T @ G, np.abs(X).T @ Ga
        res["tG"][l] = 2.0 * (unit + (deg + 2) * U + rel + above)
        res["tW"][l] = res["tG"][l] + 2.0 * N * U
        above += unit + (deg + P + 2) * U + rel
        if l > 0:
            g, ga = G @ W.T, Ga @ np.abs(W).T + sub / unit
    return res


def top_layer_g(grad_pooled, graph_ptr, n_rows, D_top, relu, dt):
    """g_{L-1} exactly as the kernel forms it: fp32(grad_pooled) * fp32(1 / n_graph) in fp32, rounded to the storage type
    dt ("f16" / "f32"), 0 where relu and D_top == 0."""
    rows_g, sizes = _graph_of_rows(graph_ptr, n_rows)
    gp = np.asarray(grad_pooled, np.float32)
    inv = (np.float32(1.0) / np.maximum(sizes, 1).astype(np.float32)).astype(np.float32)
    g = (gp[rows_g] * inv[rows_g][:, None]).astype(np.float32)
    g = g.astype(np.float16 if dt == "f16" else np.float32).astype(np.float64)
    return np.where(np.asarray(D_top, np.float64) == 0, 0.0, g) if relu else g


def top_attention_grad_f64(adj, X, W, E_dev, S_dev, g, alpha=0.2):
    """grad_attention of the top layer from the device's own E and S and the exact g_{L-1} (top_layer_g): what is left to
    differ is the arithmetic behind S -- Wh = X W formed again in fp32, d_e, rs, sg, g1, T and the sums over the batch's
    rows -- so the tolerance has neither the storage type's unit nor the softmax's relative error in it:
        t = 2 (P + 2 K + 3 deg + n + 16) U      in units of the magnitude (the same formulas on absolute values, + for -)
    Small graphs, scores of order 1 and a g that varies within a graph make the gradient itself many times that, so a
    wrong slope, a dropped term, a sign or swapped halves leave the bound.  -> (dA [2 P], magnitude [2 P], t)"""
    rowptr, col, val = (np.asarray(a) for a in adj)
    rowptr, col = rowptr.astype(np.int64), col.astype(np.int64)
    nnz = int(rowptr[-1])
    col, val = col[:nnz], val.astype(np.float64)[:nnz]
    X, W, g = np.asarray(X, np.float64), np.asarray(W, np.float64), np.asarray(g, np.float64)
    K, P = W.shape
    N = X.shape[0]
    deg = int(np.diff(rowptr).max()) if N else 0
    kw = dict(gat=True, E=_t(np.asarray(E_dev, np.float64)[:nnz]), S=_t(np.asarray(S_dev, np.float64)[:nnz]),
              dead=torch.zeros(N, dtype=torch.bool), alpha=float(np.float32(alpha)))
    tr, tc = _t(rowptr, torch.int64), _t(col, torch.int64)
    grads, _ = LG.edges(tr, tc, _t(val), _t(X), _t(W), _t(g), **kw)
    _, mags = LG.edges(tr, tc, _t(val), _t(X), _t(W), _t(np.abs(g)), **kw)
    return (grads["grad_attention"].numpy().reshape(-1), mags["grad_attention"].numpy().reshape(-1),
            2.0 * (P + 2 * K + 3 * deg + N + 16) * U)


def within(got, want, mag, tol):
    """(ok, worst ratio): |got - want| <= tol * mag + 1e-30 element-wise, the worst error in units of tol * mag."""
    got = np.asarray(got, np.float64).reshape(np.shape(want))
    err = np.abs(got - want)
    bound = tol * mag + 1e-30
    ratio = float((err / bound).max()) if err.size else 0.0
    return bool(np.isfinite(got).all() and (err <= bound).all()), ratio

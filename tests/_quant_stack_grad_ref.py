"""Float64 restatement of sgx_quant_stack_backward (include/sgx.h, "training the quantised stack"):
tests/_gat_stack_grad_ref.gat_stack_grad_f64 with a per-layer quantiser, by FPYNQ_GAT.backward's rule under fake
quantisation -- the attention matrix is the QUANTISED forward's, everything a gradient multiplies with is unquantised.

    g_{L-1}, the ReLU masks (D_l is the quantised forward's output, deq_factor in it) and the chain: gat_stack_grad_f64's
    GCN layer, quantised or not      G_l = A g_l on the UNQUANTISED adjacency (the same three lines)
    GAT layer, quants[l] = None      gat_stack_grad_f64's layer
    GAT layer, quants[l] = c         H_q = _quant_ref.stage1(X_l, W_l, c)            requant(X_q . W_q), exact
                                     E, S = _quant_ref.stage2_gat on H_q, the attention vector on the signed grid and
                                     live = (A_q > 0), dead rule "zero"              the quantised forward's steps 1 and 2
                                     G_l = S g_l;  grad_attention_l = _layer_grad_ref.edges on the UNQUANTISED X_l, W_l
                                     (so Wh = X_l W_l) with that E and S
    dW_l = X_l^T G_l;  g_{l-1} = G_l W_l^T                                           (deq_factor reaches no gradient)

Tolerances are gat_stack_grad_f64's (its docstring derives them), with one change for a quantised GAT layer: rel_l drops
the 2 max(bWh . |a|) term.  That term paid for the device forming Wh again in fp32 before the scores; here the scores are
formed from H_q, which is EXACT on the device wherever the sums of code products stay below 2^24 (stage1 returns the
largest, and this module asserts it per layer), the grid values and the re-quantisation being the same fp32 statements.
So for such a layer

    rel_l = max over live entries of (bS_e - 2^-126) / S_e from _gat_ref.forward on H_q      (the fp32 softmax alone)
    bE_e  = _gat_ref.forward's bound on E alone

and the count of roundings behind S is the softmax's own: the two score dots over P_l (fma chains of 8 lanes and a
3-step tree), the sum s1_i + s2_c, the slope, x - m, the product with log2 e, exp2, the row sum over deg entries, the
reciprocal and the final product -- what _gat_ref.forward's bS counts.  The unquantised Wh of d_e, T and sum g1 Wh is
formed in fp32 as before, so the term (P_l + 2 K_l + 3 deg + n + 16) U of grad_attention stays:

    G_l              : unit + (deg + 2) U + rel_l + sum_{j > l} pass_j
    dW_l             : that + n U
    grad_attention_l : unit + sum_{j > l} pass_j + 3 rel_l + (P_l + 2 K_l + 3 deg + n + 16) U
    pass_j           = unit + (deg + P_j + 2) U + rel_j (GAT)
    all times 2, for first-order slack.

unit = U = 2^-24 always: a quantiser takes float32 only.

Mutants (for tests/test_quant_stack_train_cpu.py: each must leave the tolerance somewhere):
    "scores_unquantised_wh"   E and S from Wh = X_l W_l instead of H_q
    "d_from_hq"               d_e, T and sum g1 Wh from H_q instead of the unquantised Wh
    "mask_unquantised"        live = (A > 0) on the unquantised values
"""
import numpy as np
import torch

import _gat_ref as R
import _layer_grad_ref as LG
import _quant_ref as Q
from _gat_stack_grad_ref import U, _t, gat_stack_grad_f64, within  # noqa: F401  (within: re-exported for the tests)
from _stack_grad_ref import _graph_of_rows
from _stack_ref import csr_matmul


def quant_stack_grad_f64(adj, x, weights, atts, relus, graph_ptr, grad_pooled, outs, quants, adj_q=None, alpha=0.2,
                         E_dev=None, mutant=None):
    """gat_stack_grad_f64's arguments (adj's values UNQUANTISED, everything float32-representable) plus quants[l] =
    QuantConstants or None and adj_q = the quantised adjacency values as stored (None: quantised here with the layer's
    constants).  Returns gat_stack_grad_f64's dict and `magnitude` (per quantised GAT layer, the largest sum of
    |code_x| |code_w|, asserted below 2^24)."""
    if all(q is None for q in quants) and mutant is None:
        r = gat_stack_grad_f64(adj, x, weights, atts, relus, graph_ptr, grad_pooled, outs, alpha=alpha, E_dev=E_dev,
                               sub=R.OUT_SUB["f32"])
        r["magnitude"] = [None] * len(weights)
        return r
    rowptr, col, val = (np.asarray(a) for a in adj)
    rowptr, col = rowptr.astype(np.int64), col.astype(np.int64)
    nnz = int(rowptr[-1]) if len(rowptr) else 0
    col, val = col[:nnz], val.astype(np.float64)[:nnz]
    x = np.asarray(x, np.float64)
    N = x.shape[0]
    L = len(weights)
    unit = U
    Ws = [np.asarray(W, np.float64) for W in weights]
    Xs = [x] + [None if D is None else np.asarray(D, np.float64) for D in outs[:-1]]
    rows_g, sizes = _graph_of_rows(graph_ptr, N)
    gp = np.asarray(grad_pooled, np.float64)
    size = np.maximum(sizes[rows_g], 1)[:, None]
    g = gp[rows_g] / size if N else np.zeros((0, gp.shape[1]))
    ga = np.abs(gp)[rows_g] / size if N else np.zeros((0, gp.shape[1]))
    sub = R.OUT_SUB["f32"]
    ga = ga + sub / unit
    deg = int(np.diff(rowptr).max()) if len(rowptr) > 1 else 0
    tr, tc = _t(rowptr, torch.int64), _t(col, torch.int64)
    res = {k: [None] * L for k in ("dW", "dA", "G", "E", "S", "bE", "bS", "dead", "mW", "mA", "mG", "tW", "tA", "tG",
                                   "magnitude")}
    above = 0.0
    for l in range(L - 1, -1, -1):
        W, X = Ws[l], Xs[l]
        K, P = W.shape
        c = quants[l]
        if relus[l]:
            g = np.where(np.asarray(outs[l], np.float64) == 0, 0.0, g)
        rel = 0.0
        if atts[l] is None:
            G = csr_matmul(rowptr, col, val, g)
            Ga = csr_matmul(rowptr, col, np.abs(val), ga)
        else:
            att = np.asarray(atts[l], np.float64).reshape(-1)
            Wh, Wha = X @ W, np.abs(X) @ np.abs(W)
            extra = 0.0
            if c is None:
                r = R.forward(dict(rowptr=rowptr, col=col, val=val, Wh=Wh, att=att), 1, alpha=alpha, relu=False,
                              dead_rule="zero", out="f32")
                bWh = (K + 2) * U * Wha
                extra = (bWh @ np.abs(att[:P]))[r["row"]] + (bWh @ np.abs(att[P:]))[col]
                Hq = None
            else:
                Hq, magnitude, _facts = Q.stage1(X.astype(np.float32), W.astype(np.float32), c)
                assert magnitude < Q.EXACT_BELOW, f"layer {l}: sum |code_x| |code_w| = {magnitude} reaches 2^24: H_q is not exact"
                res["magnitude"][l] = magnitude
                aq = Q.quantise_adj(val.astype(np.float32), c) if adj_q is None else np.asarray(adj_q, np.float32)[:nnz]
                if mutant == "mask_unquantised":
                    aq = val.astype(np.float32)
                att_q, _ = Q.quantise(att.astype(np.float32), 1, c)
                H_scores = Wh if mutant == "scores_unquantised_wh" else Hq
                _D, _b, r = Q.stage2_gat((rowptr, col), aq, H_scores, att_q, c, False, "zero", alpha=alpha)
            row, live = r["row"], r["live"]
            mx = R._seg(np.maximum, np.where(live, extra, 0.0), rowptr, 0.0) if c is None else np.zeros(len(rowptr) - 1)
            S_, bS = r["S"], r["bS"] + 2 * r["S"] * mx[row]
            pos = live & (S_ > 0)
            rel = float(((bS[pos] - R.TINY32) / S_[pos]).max()) if pos.any() else 0.0
            E_slope = r["E"] if E_dev is None or E_dev[l] is None else np.asarray(E_dev[l], np.float64)[:nnz]
            no_dead = torch.zeros(N, dtype=torch.bool)
            # (edges masks sg with val > 0: an entry the quantiser killed has S = 0, so sg = 0 under either mask)
            kw = dict(gat=True, E=_t(E_slope), S=_t(S_), dead=no_dead, alpha=float(np.float32(alpha)))
            if mutant == "d_from_hq" and c is not None:
                eX, eW, eXa, eWa = Hq.astype(np.float64), np.eye(P), np.abs(Hq).astype(np.float64), np.eye(P)
            else:
                eX, eW, eXa, eWa = X, W, X, W
            grads, _ = LG.edges(tr, tc, _t(val), _t(eX), _t(eW), _t(g), **kw)
            _, mags = LG.edges(tr, tc, _t(val), _t(eXa), _t(eWa), _t(ga), **kw)
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

"""sgx_quant_stack_forward (include/sgx.h, "quantised layers in the small-graph stack") restated as a float32 chain, from
the pieces the quantised layer's tests already use: per layer tests/_quant_ref.py's stage1 (H = requant(X_q . W_q), exact
while the code sums stay below 2^24), then stage2_gcn or stage2_gat with the zero dead-row rule (float64 on the given fp32
H, with the derived element-wise bound), D rounded to float32 as the next layer's input; then _gat_stack_ref.readout_f64.

layer_ref() is one stage on a GIVEN input -- what the GPU tests call with the device's own D_{l-1}, so that no grid step
flipped by a last-ulp difference propagates and no tolerance has to be invented.  chain() strings the stages together on
the reference's own float32 D_l; tests/test_quant_stack_cpu.py pins it, stage by stage, to the dense emulation in
sgracex1_amd/sgrace.py (config.acc = 0), this project's restatement of the reference.

Parity of the quantised layer is unpinned: the reference records no quantised output.
"""
import numpy as np

import _quant_ref as Q
from _gat_stack_ref import readout_f64


def layer_ref(adj, a_val, X, W, att, c, relu, adj_quantised=False, alpha=0.2):
    """One layer with quantiser constants c on input X (dense [n, M] or a CSR triple): adj = (rowptr, col), a_val its
    values (taken as stored with adj_quantised), W [M, P], att [2 P] or None (GCN).
    Returns dict(H, magnitude, facts, D float64, bound, aq, dead)."""
    H, magnitude, facts = Q.stage1(X, W, c)
    aq = np.asarray(a_val, np.float32) if adj_quantised else Q.quantise_adj(a_val, c)
    if att is None:
        D, bound = Q.stage2_gcn(adj, aq, H, c, relu)
        dead = None
    else:
        att_q, _ = Q.quantise(np.asarray(att, np.float32).reshape(-1), 1, c)
        D, bound, ref = Q.stage2_gat(adj, aq, H, att_q, c, relu, "zero", alpha=alpha)
        dead = ref["dead"]
    return dict(H=H, magnitude=magnitude, facts=facts, D=D, bound=bound, aq=aq, dead=dead)


def chain(adj, a_val, x, weights, atts, relus, graph_ptr, quants, head_w=None, head_b=None, adj_quantised=False, alpha=0.2):
    """The whole call: weights W_l [M_l, P_l], atts[l] = attention [2 P_l] or None, quants[l] = QuantConstants (every
    layer quantised).  Returns dict(layers = [layer_ref results], outs = [float32 D_l], pooled, logits, b_pooled,
    b_logits) -- the readout and its bounds on the chain's own last D."""
    X = x
    layers, outs = [], []
    for W, att, relu, c in zip(weights, atts, relus, quants):
        r = layer_ref(adj, a_val, X, W, att, c, relu, adj_quantised, alpha)
        layers.append(r)
        X = r["D"].astype(np.float32)
        outs.append(X)
    pooled, logits, bP, bL = readout_f64(X, graph_ptr, head_w, head_b)
    return dict(layers=layers, outs=outs, pooled=pooled, logits=logits, b_pooled=bP, b_logits=bL)

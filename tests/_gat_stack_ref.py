"""sgx_gat_stack_forward (include/sgx.h, "GAT layers in the small-graph stack") restated in float64, and the block-diagonal
batch its tests run on.

The chain: per layer H_l = X_l W_l, then D_l = act(A H_l) (gat_mode 0, as tests/_stack_ref.py) or the edge softmax of
tests/_gat_ref.py on H_l (gat_mode 1: forward(dead_rule="zero", out=dtype), one head), then the per-graph mean and the
head.  chain_f64(..., dt=...) also carries an element-wise bound from stage to stage, for comparing two device paths end
to end (the GPU tests check single stages with _gat_ref's own bound instead).  With bX the bound on a stage's input
(0 for the features), U = 2^-24, u = the unit roundoff of dt and s its half subnormal spacing:

    H        bH = bX |W| + (K + 2) U |X| |W|, then the rounding to dt: + u (|H| + bH) + s
    GCN      bD = |A| bH + (deg + 2) U |A| |H|, then the rounding
    GAT      a score moves by at most be_e = bH_i.|a1| + bH_c.|a2| (LeakyReLU is 1-Lipschitz), so a weight by the factor
             exp(+-2 max_row be):  dS_e = S_e expm1(2 max_row be);  the sum over the row moves by
             sum_e dS_e (|H_c| + bH_c) + S_e bH_c, to which _gat_ref's bD (the fp32 evaluation on a given H) is added,
             then the rounding.  The mask does not depend on H; a dead row is 0 on every path.
    ReLU     1-Lipschitz: bD unchanged
    readout  pooled: mean of bD over the graph + 2 (n + 2) U mean|D|;  logits: bP |Wh|^T + 2 (F + 8) U (|P| |Wh|^T + |b|)

_gat_ref's bD is evaluated at the float64 H, not at the device's; the difference is of second order in the bounds.
"""
import numpy as np

import _gat_ref as R
from _stack_ref import csr_matmul

U = R.U


def _rows_sum(rowptr, a):
    return R._seg(np.add, a, np.asarray(rowptr, np.int64), 0.0)


def readout_f64(D, graph_ptr, head_w=None, head_b=None):
    """(pooled, logits or None, bound on pooled, bound on logits or None) for a given last-layer output D: what an fp32
    readout in any order may differ by (the readout term of _stack_ref.stack_bound, per element)."""
    D = np.asarray(D, np.float64)
    ptr = np.asarray(graph_ptr, np.int64)
    F = D.shape[1]
    pooled = np.stack([D[a:b].mean(0) if b > a else np.zeros(F) for a, b in zip(ptr[:-1], ptr[1:])]) if len(ptr) > 1 \
        else np.zeros((0, F))
    mag = np.stack([np.abs(D[a:b]).mean(0) if b > a else np.zeros(F) for a, b in zip(ptr[:-1], ptr[1:])]) if len(ptr) > 1 \
        else np.zeros((0, F))
    n = np.diff(ptr)[:, None] if len(ptr) > 1 else np.zeros((0, 1))
    bP = 2 * (n + 2) * U * mag + 1e-37
    if head_w is None:
        return pooled, None, bP, None
    W = np.asarray(head_w, np.float64)
    b = np.zeros(W.shape[0]) if head_b is None else np.asarray(head_b, np.float64)
    logits = pooled @ W.T + b
    bL = bP @ np.abs(W).T + 2 * (F + 8) * U * (np.abs(pooled) @ np.abs(W).T + np.abs(b)) + 1e-37
    return pooled, logits, bP, bL


def chain_f64(adj, x, weights, atts, relus, graph_ptr, head_w=None, head_b=None, alpha=0.2, dt=None):
    """adj = (rowptr, col, val); x dense [N, M]; weights W_l [M_l, P_l]; atts[l] = attention [2 P_l] or None (GCN layer);
    relus per layer.  Returns dict(outs, pooled, logits, refs) -- refs[l] the _gat_ref.forward result of a GAT layer --
    and with dt ("f16" / "f32") also b_outs, b_pooled, b_logits: the bounds of the module docstring."""
    rowptr, col, val = (np.asarray(a) for a in adj)
    val = val.astype(np.float64)
    deg = np.diff(rowptr.astype(np.int64))[:, None]
    X = np.asarray(x, np.float64)
    bX = np.zeros_like(X)
    u, s = (R.OUT_U[dt], R.OUT_SUB[dt]) if dt else (0.0, 0.0)
    outs, b_outs, refs = [], [], []
    for W, att, relu in zip(weights, atts, relus):
        W = np.asarray(W, np.float64)
        H = X @ W
        bH = bX @ np.abs(W) + (W.shape[0] + 2) * U * (np.abs(X) @ np.abs(W))
        bH = bH + u * (np.abs(H) + bH) + s
        if att is None:
            D = csr_matmul(rowptr, col, val, H)
            bD = csr_matmul(rowptr, col, np.abs(val), bH) + (deg + 2) * U * csr_matmul(rowptr, col, np.abs(val), np.abs(H))
            bD = bD + u * (np.abs(D) + bD) + s
            refs.append(None)
        else:
            att = np.asarray(att, np.float64).reshape(-1)
            P = H.shape[1]
            g = dict(rowptr=rowptr, col=col, val=val, Wh=H, att=att)
            r = R.forward(g, 1, alpha=alpha, relu=False, dead_rule="zero", out=dt or "f32")
            D = r["D"]
            c = col.astype(np.int64)[:len(r["row"])]
            be = (bH @ np.abs(att[:P]))[r["row"]] + (bH @ np.abs(att[P:]))[c]
            mb = R._seg(np.maximum, np.where(r["live"], be, 0.0), rowptr.astype(np.int64), 0.0)
            dS = r["S"] * np.expm1(2 * mb[r["row"]])
            prop = _rows_sum(rowptr, dS[:, None] * (np.abs(H[c]) + bH[c]) + r["S"][:, None] * bH[c])
            bD = prop * (1 + u) + r["bD"]
            bD[r["dead"]] = 0.0
            refs.append(r)
        if relu:
            D = np.maximum(D, 0.0)
        outs.append(D)
        b_outs.append(bD)
        X, bX = D, bD
    pooled, logits, bP, bL = readout_f64(X, graph_ptr, head_w, head_b)
    res = dict(outs=outs, pooled=pooled, logits=logits, refs=refs)
    if dt:
        ptr = np.asarray(graph_ptr, np.int64)
        mean_b = np.stack([bX[a:b].mean(0) if b > a else np.zeros(X.shape[1]) for a, b in zip(ptr[:-1], ptr[1:])]) \
            if len(ptr) > 1 else np.zeros((0, X.shape[1]))
        res.update(b_outs=b_outs, b_pooled=bP + mean_b)
        if logits is not None:
            res["b_logits"] = bL + mean_b @ np.abs(np.asarray(head_w, np.float64)).T
    return res


# ---- the batch ----------------------------------------------------------------------------------------------------------

POOL_T = [0, 16, 32, 64, 120, 160, 240, -400]        # neighbour score shares of the special graph's nodes 8 .. 15
SPECIAL = 16                                          # rows of the special graph (the smallest row budget of a plan)


def special_rows(dt):
    """The named rows of the special graph: name -> [(pool node's T, value; None = a random live value)], in column
    order.  A row's score with the neighbour of share T is LeakyReLU(T) (x SCALE / 1024)."""
    neg_tiny = -R.F16_SUB if dt == "f16" else -R.F32_SUB
    L = None
    return [
        ("no_stored_entry", []),
        ("all_masked_plus0_minus0_negative", [(0, 0.0), (16, neg_tiny), (160, -0.0), (240, -0.25)]),
        ("one_live_among_masked", [(0, L), (120, -0.25), (160, -0.25), (240, -0.25)]),
        ("max_on_last_entry", [(0, L), (16, L), (32, L), (240, L)]),
        ("spread_240_underflows", [(0, L), (120, L), (240, L)]),
        ("live_f16_subnormal", [(0, L), (16, L), (160, R.F16_SUB)]),
        ("masked_max", [(0, L), (32, L), (240, -0.25)]),
        ("spread_144_through_leaky", [(64, L), (-400, L)]),
    ]


def build_batch(dt, budget, m_in, seed=0, n_graphs=14, filler=(1, 12)):
    """A block-diagonal batch for a plan of row budget `budget` (>= 16): graph 0 is the special graph (16 rows: the named
    rows 0 .. 7 of special_rows, then eight neighbour nodes), then graphs of 1, 2, 15, 16 and 17 rows (a size over the
    budget is cut to it), an empty graph, one of exactly `budget` rows, and random ones of filler[0] .. filler[1] rows up to n_graphs.  With the
    budget-sized graph in it the plan takes every graph with a first row of its own as a group.
    Features [N, m_in] (m_in >= 2): column 0 holds a node's own score share (0 here), column 1 its share as a neighbour,
    T / SCALE; first_layer(P) gives the W_0 and attention that turn them into the designed scores.
    Returns dict(rowptr, col, val, x, graph_ptr, sizes, names, n_rows) of float64 stored values (val, x rounded to dt)."""
    assert budget >= SPECIAL and m_in >= 2 and 12 <= n_graphs <= 20
    rng = np.random.default_rng(seed)
    sizes = [SPECIAL] + [min(n, budget) for n in (1, 2, 15, 16, 17)] + [0, budget]
    while len(sizes) < n_graphs:
        sizes.append(int(rng.integers(min(budget, filler[0]), min(budget, filler[1]) + 1)))
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(ptr[-1])
    rows = [[] for _ in range(N)]                          # per row: [(col, value)]
    names = {}
    node_of = {t: 8 + k for k, t in enumerate(POOL_T)}
    for i, (name, ents) in enumerate(special_rows(dt)):
        names[i] = name
        rows[i] = [(node_of[t], rng.uniform(0.1, 1.0) if v is None else v) for t, v in ents]
    for k in range(8, SPECIAL):                             # the neighbour nodes: a self loop and two named rows
        rows[k] = sorted({(int(c), float(rng.uniform(0.1, 1.0))) for c in rng.choice(8, 2, replace=False)} | {(k, 0.5)})
    for g in range(1, len(sizes)):
        a, n = int(ptr[g]), sizes[g]
        for i in range(n):
            d = int(rng.integers(0, min(n, 6) + 1)) if g % 3 else min(n, 3)
            cs = np.sort(rng.choice(n, d, replace=False)) if d else []
            rows[a + i] = [(a + int(c), -0.25 if rng.random() < 0.15 else float(rng.uniform(0.1, 1.0))) for c in cs]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.array([c for r in rows for c, _ in r], np.int64)
    val = R._round(np.array([v for r in rows for _, v in r], np.float64), dt)
    if dt == "f16":
        val[np.signbit(val) & (val == 0)] = -0.0
    x = rng.standard_normal((N, m_in)) * 0.5
    x[rng.random((N, m_in)) < 0.5] = 0.0
    x[:, 0] = 0.0
    x[:, 1] = 0.0
    for t, k in node_of.items():
        x[k, 1] = t / R.SCALE
    return dict(rowptr=rowptr, col=col, val=val, x=R._round(x, dt), graph_ptr=ptr, sizes=sizes, names=names, n_rows=N)


def first_layer(dt, m_in, P, seed=0):
    """(W_0 [m_in, P], attention [2 P]) for build_batch's features: H's column 0 copies feature column 0 and column 1
    feature column 1 (one column carries their sum when P == 1), and the attention entries that read them are SCALE, as
    _gat_ref's adversarial graph scales its designed scores; the other entries are of order 1 / sqrt(P)."""
    rng = np.random.default_rng([seed, m_in, P])
    W = rng.standard_normal((m_in, P)) / np.sqrt(m_in)
    att = rng.standard_normal((2, P)) * (0.3 / np.sqrt(P))
    W[:2, :] = 0.0
    if P == 1:
        W /= R.SCALE                                   # (the other features move a score by order 1)
        W[0, 0] = W[1, 0] = 1.0
        att[0, 0] = att[1, 0] = R.SCALE
    else:
        W[:, :2] = 0.0
        W[0, 0] = W[1, 1] = 1.0
        att[0, 0], att[0, 1], att[1, 0], att[1, 1] = R.SCALE, 0.0, 0.0, R.SCALE
    return R._round(W, dt), R._round(att.reshape(-1), dt)


def plain_layer(dt, m_in, P, seed=0):
    """(W [m_in, P], attention [2 P]) with scores of order 1, for the layers behind the first."""
    rng = np.random.default_rng([seed, 1, m_in, P])
    return (R._round(rng.standard_normal((m_in, P)) / np.sqrt(m_in), dt),
            R._round(rng.standard_normal(2 * P) / np.sqrt(P), dt))


def rows_budget(dt, max_width, backward=False):
    """The plan's row budget as include/sgx.h states it: two tiles (backward: one of dt and two of fp32) of rows of
    max_width elements plus 16 bytes in 64 KiB, whole 16-row tiles, at most 128."""
    def pitch_bytes(es):
        per16 = 16 // es
        return ((max_width + per16 - 1) // per16 * per16 + per16) * es
    es = 2 if dt == "f16" else 4
    row = pitch_bytes(es) + 2 * pitch_bytes(4) if backward else 2 * pitch_bytes(es)
    return min(65536 // row // 16 * 16, 128)

"""The entry-split GAT aggregate (sgx_gat_aggregate_flat; "entry-split GAT aggregate" in include/sgx.h): the graphs at which it
can fail, its float64 reference, and an fp32 numpy emulation of the rule.  Plain numpy; nothing here touches the GPU.

Graphs: the degree patterns of _spmm_flat_ref.degree_cases(T) (capacity cases, empty runs, rows that end on, begin on and
cross chunk ends) plus "masked_chunks" (two crossing rows, one over five chunks, and rows inside a chunk), each crossed with a
value mask:
    "live"    all entries live;
    "third"   a third of the entries masked, +0.0, -0.0 and negative values mixed, positive subnormals among the live ones;
    "chunks"  every even chunk wholly masked and every row r with r % 4 == 3 wholly masked: crossing rows whose leader piece,
              head pieces and middle chunks hold no live entry, a crossing row dead over all its chunks ("masked_chunks"
              row 3), rows inside a chunk that are dead;
    "ascend" / "descend"   all live, chunk k's scores in about [4k, 4k + 1] (descend: chunk k takes the scores of chunk
              K - 1 - k): every merge of a crossing row rescales, and in the descending case the leader holds the maximum.
Row r of the matrix is node r of Wh; N_COLS >= every row count.

Reference: _gat_ref.forward in float64 with its bound, unchanged.  Its constant C = 8 budgets, per weight, the exponential
(2 roundings), the division (2) and "a running state and one merge of partial states" (4).  The rule's operation count per
weight: the exponential against the running maximum, the rescales of the running state -- one product per step of the walk
at which the piece's maximum moves: on the scores of these graphs (independent draws inside a piece) that happens at a few
steps, each factor exp(m_old - m_new) weighting the moved terms down --, no rescale when the lane groups of a long piece
are folded (one maximum over the wavefront), and ONE product with exp(m_k - M) in the leader's merge.  That is the running
state plus one merge the constant names; emulate() below evaluates exactly this in fp32 and test_gat_flat_cpu.py shows it
inside the bound on every case, at T = 256 and T = 128.  No term is added.

Statistics: score_row / score_col bit-equal to sgx_gat_aggregate_stats's (no plan) on the same inputs; row_max bit-equal to
the maximum of the E_e the statistics expression forms; row_sum within l rel_max, rel_max the row's largest rel_e of
_gat_ref (rel_of below restates the docstring's formula on forward()'s outputs)."""
import numpy as np

import _gat_ref as G
import _spmm_flat_ref as F

N_COLS = 211
K_CLASSES = 7                     # score classes of the ascend / descend masks: one per chunk of the longest graphs (6 T + ...)
MASKS = ("live", "third", "chunks", "ascend", "descend")
ALPHA = 0.2


def degree_cases(T):
    cases = dict(F.degree_cases(T))
    # row 0 inside chunk 0; row 1: 0.5 T .. 3.5 T, chunks 0 (leader) .. 3 -- under "chunks" its leader piece and the middle
    # chunk 2 are masked; row 2 inside chunk 3; row 3: 3.5 T + 6 .. 6 T + 6, chunks 3 (leader) .. 6 -- wholly masked under
    # "chunks"; rows 4.. inside the last chunk
    cases["masked_chunks"] = ([T // 2, 3 * T, 6, 2 * T + T // 2, 9, 11, 0, 5], 0)
    return cases


def _round(a, dt):
    return np.asarray(a, np.float64).astype(np.float16 if dt == "f16" else np.float32).astype(np.float64)


def graph(name, mask, n_feat, dt, T):
    """dict(rowptr, col, val, Wh, att, n_rows, n_cols, capacity) of float64 stored values; capacity = the entries the
    device arrays hold (those behind rowptr[-1] are never read)."""
    deg, extra = degree_cases(T)[name]
    seed = [len(name), MASKS.index(mask), n_feat]
    rng = np.random.default_rng(seed)
    deg = np.asarray(deg, np.int64)
    n = len(deg)
    assert n <= N_COLS
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum(deg)
    nnz = int(rp[-1])
    chunk_of = np.arange(nnz) // T
    row_of = G.rows_of(rp)
    Wh = rng.standard_normal((N_COLS, n_feat)) * 0.6
    att = rng.standard_normal(2 * n_feat) / np.sqrt(n_feat)
    col = rng.integers(0, N_COLS, nnz)
    val = rng.uniform(0.1, 1.0, nnz)
    if mask == "third":
        sub = G.F16_SUB if dt == "f16" else G.F32_SUB
        kind = rng.integers(0, 9, nnz)                        # 0, 1, 2: masked; 3: a live positive subnormal
        val = np.where(kind == 0, 0.0, np.where(kind == 1, -0.0, np.where(kind == 2, -rng.uniform(0.1, 1.0, nnz), val)))
        val = np.where(kind == 3, sub, val)
    elif mask == "chunks":
        val = np.where((chunk_of % 2 == 0) | (row_of % 4 == 3), -0.25, val)
    elif mask in ("ascend", "descend"):
        # column c carries the neighbour score 4 (c % K) + u_c in column 0 of Wh (a2[0] = 8, a1[0] = 0); the rest is small
        Wh *= 0.05 / 0.6
        att *= 0.1 * np.sqrt(n_feat)
        cls = np.arange(N_COLS) % K_CLASSES
        Wh[:, 0] = (4.0 * cls + rng.random(N_COLS)) / 8.0
        att[0], att[n_feat] = 0.0, 8.0
        k = np.minimum(chunk_of, K_CLASSES - 1)
        want = k if mask == "ascend" else K_CLASSES - 1 - k
        per = N_COLS // K_CLASSES
        col = want + K_CLASSES * rng.integers(0, per, nnz)
    val = _round(val, dt)
    return dict(rowptr=rp, col=col.astype(np.int64), val=val, Wh=_round(Wh, dt), att=_round(att, dt), n_rows=n, n_cols=N_COLS,
                capacity=nnz + extra, names={})


def fill_row(n_feat):
    return np.random.default_rng(99).standard_normal(n_feat).astype(np.float32)


N_NODES = 5000                    # the partitioned rule's node count


def reference(g, dt, relu, rule):
    """_gat_ref.forward, one head; rule in ("zero", "mean", "fill")"""
    F_ = g["Wh"].shape[1]
    return G.forward(g, 1, alpha=ALPHA, relu=bool(relu), dead_rule=rule, fill_row=fill_row(F_) if rule == "fill" else None,
                     n_nodes=N_NODES if rule == "fill" else None, out=dt)


def rel_of(g, ref):
    """per row: (l_i in float64, the largest rel_e of the row's live entries) -- _gat_ref's weight bound, restated on forward()'s
    E and bE: rel_e = 2 max_row(delta) + (C + |x_e - m_i|) 4U + (deg_i + 2) U"""
    rp = g["rowptr"]
    x, delta, live, row = ref["E"], ref["bE"], ref["live"], ref["row"]
    deg = np.diff(rp)
    m = G._seg(np.maximum, np.where(live, x, -np.inf), rp, -np.inf)
    m0 = np.where(np.isfinite(m), m, 0.0)
    p = np.where(live, np.exp(np.where(live, x - m0[row], 0.0)), 0.0)
    l = G._seg(np.add, p, rp, 0.0)
    maxd = G._seg(np.maximum, np.where(live, delta, 0.0), rp, 0.0)
    rel = 2 * maxd[row] + (G.C + np.abs(x - m0[row])) * 4 * G.U + (deg[row] + 2) * G.U
    return l, G._seg(np.maximum, np.where(live, rel, 0.0), rp, 0.0)


# ---- the rule in fp32 ------------------------------------------------------------------------------------------------------

f32 = np.float32
STEP = 8                          # entries a step of the emulated walk scores together (a lane group's width)


def _piece_state(x, live, rows, m, l, acc):
    """a running state over the piece's entries, STEP at a time: the maximum folded, one rescale, the rows added"""
    for b in range(0, len(x), STEP):
        xs, lv = x[b:b + STEP], live[b:b + STEP]
        if not lv.any():
            continue
        m_new = max(m, f32(xs[lv].max()))
        scale = f32(0) if m == -np.inf else np.exp(f32(m - m_new))
        p = np.where(lv, np.exp((xs - m_new).astype(f32)), f32(0)).astype(f32)
        l = f32(l * scale)
        acc = (acc * scale).astype(f32)
        for t in range(len(xs)):
            l = f32(l + p[t])
            acc = (acc + p[t] * rows[b + t]).astype(f32)
        m = m_new
    return m, l, acc


def emulate(g, T, relu, rule, dt):
    """D [n_rows, F] as the rule gives it in fp32: per (chunk, row) piece a running state, a crossing row's states merged in
    chunk order, then the normalisation, the dead-row rule, the activation and the rounding to the output type."""
    rp, col, val = g["rowptr"], g["col"], g["val"]
    Wh, att = g["Wh"].astype(f32), g["att"].astype(f32)
    n, Fw = g["n_rows"], Wh.shape[1]
    s1 = (Wh[:, :].astype(np.float64) @ att[:Fw].astype(np.float64)).astype(f32)
    s2 = (Wh.astype(np.float64) @ att[Fw:].astype(np.float64)).astype(f32)
    sched = F.schedule(rp, T, g["capacity"])
    states = {}                                               # row -> [(m, l, acc)] in chunk order
    for c, r, e0, e1 in sorted(sched.reads):
        z = (s1[r] + s2[col[e0:e1]]).astype(f32)
        x = np.where(z > 0, z, (z * f32(ALPHA)).astype(f32)).astype(f32)
        st = _piece_state(x, val[e0:e1] > 0, Wh[col[e0:e1]], f32(-np.inf), f32(0), np.zeros(Fw, f32))
        states.setdefault(r, []).append(st)
    D = np.zeros((n, Fw), f32)
    dead = np.ones(n, bool)
    for r, sts in states.items():
        M = max(m for m, _, _ in sts)
        if M == -np.inf:
            continue
        l, acc = f32(0), np.zeros(Fw, f32)
        if len(sts) == 1:
            l, acc = sts[0][1], sts[0][2]
        else:
            for m, lk, ak in sts:
                w = f32(0) if m == -np.inf else np.exp(f32(m - M))
                l = f32(l + lk * w)
                acc = (acc + ak * w).astype(f32)
        D[r] = (acc / l).astype(f32)
        dead[r] = False
    if rule == "mean":
        D[dead] = Wh.astype(np.float64).mean(0).astype(f32)
    elif rule == "fill":
        D[dead] = fill_row(Fw)
    out = D.astype(np.float16 if dt == "f16" else np.float32)
    if relu:
        out = np.where(out > 0, out, 0).astype(out.dtype)
    return out.astype(np.float64), dead

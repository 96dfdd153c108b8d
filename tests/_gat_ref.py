"""The GAT edge-softmax aggregate restated in float64 on the edge list, with an element-wise error bound, and the
adversarial graphs the GAT path tests run it on.

The formula (include/sgx.h, sgx_gat_aggregate; SG.py:309-314, :634-661), per head h on its slice of f = F / heads columns
and its own attention vector a = attention[h] = [a1 ; a2]:

    x_e  = LeakyReLU_alpha(Wh_i . a1 + Wh_c . a2)          every stored entry e = (i, c)
    live = values[e] > 0                                   the stored value as stored (fp16 upcast without rounding)
    S_e  = exp(x_e - m_i) / sum over live entries of row i, m_i = max of the row's LIVE scores; 0 on a masked entry
    D_i  = act(sum_e S_e Wh_c)

A row without a live entry ("dead") gets, by the caller's rule: 0 (D = 0, S = 0); "mean" -- the reference's dense
emulation, a uniform softmax over all n_cols nodes: D = the mean row of Wh, S = 1 / n_cols on its stored entries; or
"fill" -- one rank of a partitioned graph: D = the caller's fill_row, S = 1 / n_nodes.

Next to every result the restatement returns a bound on the error of an fp32 evaluation, computed in float64 from the
same inputs (U = 2^-24, the fp32 unit roundoff):

    score    delta_e = (f + 4) U (|Wh_i|.|a1| + |Wh_c|.|a2|) + 2 U |x_e|         two dot products, the sum, LeakyReLU
    weight   rel_e   = 2 max_row(delta) + (C + |x_e - m_i|) 4U + (deg_i + 2) U
             |dS_e| <= S_e rel_e + 2^-126
    output   |dD_ij| <= sum_e S_e rel_e |Wh_cj| + (deg_i + 2) U sum_e S_e |Wh_cj| + rounding to the output type

A score error moves S_e by at most delta_e + max_row(delta) (numerator and denominator).  exp(x - m) of an fp32
difference -- and the hardware v_exp_f32 of the one-walk form, which exponentiates (x - m) log2(e) -- is off by
|x - m| U relative from the rounding of its argument; the restatement allows four times that.  (deg + 2) U is the
row sum of the exponentials in any order.  C = 8 covers the rest, a fixed number of roundings per weight: the
exponential's own result (<= 2 ulp), the reciprocal or division by the sum (<= 2), and the rescaling products of
online-softmax merges (a running state and one merge of partial states, <= 4).  2^-126 is fp32 underflow: a weight
below the smallest normal number may come out as 0.  There is no other absolute tolerance.

The backward edge pass (sgx_gat_backward_edges) is restated the same way on the forward's own E and S.
"""
import numpy as np

U = 2.0 ** -24
C = 8.0
TINY32 = 2.0 ** -126                 # fp32 underflow floor of a softmax weight
SUB = 2.0 ** -149                    # the spacing of fp32 subnormals
F16_SUB = 2.0 ** -24                 # the smallest positive fp16 subnormal
F32_SUB = float(np.float32(1e-40))   # a positive fp32 subnormal (0 once stored as fp16)
SCALE = 1024.0                       # the attention entries that carry the designed scores
OUT_U = {"f16": 2.0 ** -11, "f32": U}
OUT_SUB = {"f16": 2.0 ** -25, "f32": 2.0 ** -150}


def _seg(ufunc, a, rowptr, empty):
    """ufunc reduced over each row's entries [rowptr[i], rowptr[i+1]); rows without entries give `empty`."""
    pad = np.concatenate([a, np.full((1,) + a.shape[1:], empty, dtype=a.dtype)], 0)
    out = ufunc.reduceat(pad, rowptr[:-1], axis=0)
    out[np.diff(rowptr) == 0] = empty
    return out


def rows_of(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def forward(g, heads, alpha=0.2, relu=False, dead_rule="zero", fill_row=None, n_nodes=None, out="f16", live=None):
    """The stored-edge formula on graph g (dict: rowptr, col, val, Wh, att as float64 of the stored values).
    Returns a dict of D [n_rows, F], E / S [nnz, heads] and their bounds bD / bE / bS, plus dead [n_rows] and
    live [nnz].  `live` overrides the mask (the mutation checks use it)."""
    rowptr, col, val = g["rowptr"].astype(np.int64), g["col"].astype(np.int64), g["val"]
    Wh, att = g["Wh"], g["att"]
    n_rows, nnz, (n_cols, F) = len(rowptr) - 1, len(col), Wh.shape
    f = F // heads
    row, deg = rows_of(rowptr), np.diff(rowptr)
    a = att.reshape(heads, 2, f)
    Whh = Wh.reshape(n_cols, heads, f)
    s1 = np.einsum("nhk,hk->nh", Whh[:n_rows], a[:, 0])
    s2 = np.einsum("nhk,hk->nh", Whh, a[:, 1])
    A1 = np.einsum("nhk,hk->nh", np.abs(Whh[:n_rows]), np.abs(a[:, 0]))
    A2 = np.einsum("nhk,hk->nh", np.abs(Whh), np.abs(a[:, 1]))
    al = float(np.float32(alpha))                       # the kernels take alpha as fp32
    z = s1[row] + s2[col]
    x = np.where(z > 0, z, al * z)
    delta = (f + 4) * U * (A1[row] + A2[col]) + 2 * U * np.abs(x)
    live = (val > 0) if live is None else live
    lv = live[:, None]
    m = _seg(np.maximum, np.where(lv, x, -np.inf), rowptr, -np.inf)
    dead = ~np.isfinite(m[:, 0]) if nnz else np.ones(n_rows, bool)
    m0 = np.where(np.isfinite(m), m, 0.0)
    p = np.where(lv, np.exp(np.where(lv, x - m0[row], 0.0)), 0.0)
    l = _seg(np.add, p, rowptr, 0.0)
    w = np.where(lv, p / np.where(l > 0, l, 1.0)[row], 0.0)
    maxd = _seg(np.maximum, np.where(lv, delta, 0.0), rowptr, 0.0)
    rel = 2 * maxd[row] + (C + np.abs(x - m0[row])) * 4 * U + (deg[row, None] + 2) * U
    S, bS = w.copy(), np.where(lv, w * rel + TINY32, 0.0)
    Wc = Whh[col]                                                       # [nnz, heads, f]
    D = _seg(np.add, w[:, :, None] * Wc, rowptr, 0.0)
    absD = _seg(np.add, w[:, :, None] * np.abs(Wc), rowptr, 0.0)
    bD = _seg(np.add, (w * rel)[:, :, None] * np.abs(Wc), rowptr, 0.0) + (deg[:, None, None] + 2) * U * absD
    bD += deg[:, None, None] * TINY32 * np.abs(Wh).max()
    D, bD = D.reshape(n_rows, F), bD.reshape(n_rows, F)
    de = dead[row]
    if dead_rule == "mean":
        D[dead] = Wh.mean(0)
        bD[dead] = (n_cols + 2) * U * np.abs(Wh).mean(0)
        S[de], bS[de] = 1.0 / n_cols, U / n_cols
    elif dead_rule == "fill":
        D[dead], bD[dead] = np.asarray(fill_row, np.float64), 0.0
        S[de], bS[de] = 1.0 / n_nodes, U / n_nodes
    else:
        assert dead_rule == "zero"
        D[dead], bD[dead] = 0.0, 0.0
    if relu:
        D = np.maximum(D, 0.0)
    bD = bD + (np.abs(D) + bD) * OUT_U[out] + OUT_SUB[out]
    if heads == 1:
        x, delta, S, bS = x[:, 0], delta[:, 0], S[:, 0], bS[:, 0]
    return dict(D=D, bD=bD, E=x, bE=delta, S=S, bS=bS, dead=dead, live=live, row=row)


def backward_edges(g, E, S, G, Wh, alpha=0.2, dead=None):
    """sgx_gat_backward_edges (one head) in float64 on the forward's own E, S (fp32, as given) with bounds:
        d_e = G_i . Wh_c;  dx_e = S_e d_e;  rs_i = sum_row dx  (dead row: G_i . colsum(Wh) / n_cols)
        sg_e = (dx_e - S_e rs_i) (E_e > 0 ? 1 : alpha), 0 on a masked entry;  g1_i = sum_row sg.
    Returns (sg, g1, b_sg, b_g1)."""
    rowptr, col, val = g["rowptr"].astype(np.int64), g["col"].astype(np.int64), g["val"]
    E, S, G, Wh = (np.asarray(t, np.float64) for t in (E, S, G, Wh))
    n_cols, F = Wh.shape
    row, deg = rows_of(rowptr), np.diff(rowptr)
    d = np.einsum("ek,ek->e", G[row], Wh[col])
    bd = (F + 2) * U * np.einsum("ek,ek->e", np.abs(G[row]), np.abs(Wh[col]))
    # (SUB: one fp32 rounding in the subnormal range, where the product of a weight below 2^-126 lands)
    dx, bdx = S * d, S * bd + U * np.abs(S * d) + SUB
    rs = _seg(np.add, dx, rowptr, 0.0)
    brs = _seg(np.add, bdx, rowptr, 0.0) + (deg + 2) * U * _seg(np.add, np.abs(dx), rowptr, 0.0)
    if dead is not None:
        mean, amean = Wh.mean(0), np.abs(Wh).mean(0)
        rs = np.where(dead, G @ mean, rs)
        brs = np.where(dead, (F + 2) * U * (np.abs(G) @ amean) + np.abs(G) @ ((n_cols + 2) * U * amean), brs)
    al = float(np.float32(alpha))
    slope = np.where(E > 0, 1.0, al)
    live = val > 0
    sg = np.where(live, (dx - S * rs[row]) * slope, 0.0)
    bsg = np.where(live, bdx + S * brs[row] + 3 * U * (np.abs(dx) + np.abs(S * rs[row])) + 3 * SUB, 0.0)
    g1 = _seg(np.add, sg, rowptr, 0.0)
    bg1 = _seg(np.add, bsg, rowptr, 0.0) + (deg + 2) * (U * _seg(np.add, np.abs(sg), rowptr, 0.0) + SUB)
    return sg, g1, bsg, bg1


def check(what, got, want, bound, row_of, names):
    """Raises AssertionError naming the graph rows where |got - want| > bound or got is not finite."""
    got = np.asarray(got, np.float64).reshape(want.shape)
    bad = ~(np.abs(got - want) <= bound)
    if not bad.any():
        return
    idx = np.argwhere(bad)
    rows = sorted({int(row_of[i[0]]) for i in idx})
    shown = ", ".join(f"{names.get(r, 'row %d' % r)}" for r in rows[:8])
    i = tuple(idx[0])
    raise AssertionError(f"{what}: {int(bad.sum())} elements outside the bound in {len(rows)} rows ({shown}); first at "
                         f"{i}: got {got[i]!r}, want {want[i]!r}, bound {bound[i]!r}")


def check_forward(got, ref, names, parts=("D", "E", "S")):
    """The GPU test's comparison of (D, E, S) against forward()'s result and bounds."""
    n_rows = ref["D"].shape[0]
    for k in parts:
        if got.get(k) is None:
            continue
        row_of = np.arange(n_rows) if k == "D" else ref["row"]
        check(k, got[k], ref[k], ref["b" + k], row_of, names)


# ---- graphs -----------------------------------------------------------------------------------------------------------

def _round(a, dt):
    return np.asarray(a, np.float64).astype(np.float16 if dt == "f16" else np.float32).astype(np.float64)


def adversarial_graph(dt, heads, f_head, seed=0, n_filler=4600):
    """A graph whose named rows sit where softmax code breaks (scores tens to hundreds apart, masked entries with the
    highest scores, mask edge values, dead rows, rows around the kernels' size steps, long rows with masked or low
    tasks) followed by short filler rows (enough one-step rows for the degree order's tail form) and a dead last row.
    Scores are made large through the attention vector: per head, column 0 of the slice carries a row's score share
    (a1[0] = SCALE) and column 1 a neighbour's (a2[1] = SCALE); Wh stays within [-4, 4].  Nodes of the same
    (row share, neighbour share) have identical rows of Wh, so their scores tie exactly.  The columns n_rows.. are
    neighbour-only nodes.  Returns dict(rowptr, col, val, Wh, att, names, n_rows, n_cols) of float64 stored values."""
    assert f_head >= 2
    rng = np.random.default_rng(seed)
    F = heads * f_head
    # neighbour pool: one node per neighbour score T (x SCALE / 1024), two copies each (ties)
    T_set = [-400, -256, -64, -16, 0, 16, 32, 48, 64, 80, 96, 128, 160, 192, 200, 240]
    protos = {}

    def proto(u, t):
        if (u, t) not in protos:
            r = np.random.default_rng([seed, 7, u + 8192, t + 8192])
            v = r.standard_normal(F) * 0.5
            v = v.reshape(heads, f_head)
            v[:, 0], v[:, 1] = u / SCALE, t / SCALE
            protos[(u, t)] = _round(v.reshape(F), dt)
        return protos[(u, t)]

    rows, names = [], {}                  # rows: (name, U, [(T, value)]) ; value None = a random live value
    LIVE = None

    def add(name, U, ents):
        names[len(rows)] = name
        rows.append((U, ents))

    neg_tiny = -F16_SUB if dt == "f16" else -F32_SUB
    add("spread80", 0, [(t, LIVE) for t in (0, 80, 32, 80, 0, 64, 16, 48)])
    add("spread160_through_leaky", 0, [(-400, LIVE), (0, LIVE), (80, LIVE), (-400, LIVE)])
    add("all_live_le_-500", -3072, [(t, LIVE) for t in (0, 16, 32, 240, 128, 0)])
    add("all_live_ge_100", 512, [(t, LIVE) for t in (0, -256, 160, -16, 96)])
    add("masked_150_above_last", 0, [(0, LIVE), (32, LIVE), (16, LIVE), (192, -0.25)])
    add("masked_150_above_first", 0, [(192, -0.5), (32, LIVE), (0, LIVE)])
    add("ties", 0, [(80, LIVE), (80, LIVE), (80, -0.25), (0, LIVE), (80, LIVE), (80, 0.0)])
    add("tie_with_masked_max", 0, [(160, LIVE), (160, -0.25), (160, LIVE)])
    add("one_live_first", 0, [(0, LIVE)] + [(192, -0.25)] * 7)
    add("one_live_middle", 0, [(192, -0.25)] * 4 + [(0, LIVE)] + [(192, -0.25)] * 4)
    add("one_live_last", 0, [(192, -0.25)] * 9 + [(0, LIVE)])
    add("mask_plus_zero", 0, [(0, LIVE), (240, 0.0), (16, LIVE)])
    add("mask_minus_zero", 0, [(0, LIVE), (240, -0.0), (16, LIVE)])
    add("mask_tiny_negative", 0, [(0, LIVE), (240, neg_tiny), (200, -1e-4), (16, LIVE)])
    add("live_f16_subnormal", 0, [(0, LIVE), (160, F16_SUB), (16, LIVE)])
    add("live_f32_subnormal", 0, [(0, LIVE), (160, F32_SUB), (16, LIVE)])     # (stored as +0.0 in fp16: masked there)
    add("only_f16_subnormal_live", -3072, [(240, -0.25), (0, F16_SUB)])
    add("dead_empty", 0, [])
    add("dead_all_masked", 0, [(240, -0.25), (0, 0.0), (160, -0.0), (16, neg_tiny)])
    add("dead_empty_2", 0, [])

    def spread(n, last_max=False, masked=0.1):
        ts = rng.choice([0, 16, 32, 48, 64, 80, 96, 128, 160], n)
        if last_max:
            ts[-1] = 240
        return [(int(t), (-0.25 if rng.random() < masked and not (last_max and k == n - 1) else LIVE))
                for k, t in enumerate(ts)]

    for n in (8, 9, 32, 33, 64, 65, 256, 257):
        add(f"deg{n}", 0, spread(n))
        add(f"deg{n}_max_last", 0, spread(n, last_max=True))
    add("long_first_tasks_masked", 0, [(240, -0.25)] * 512 + spread(522, masked=0.0))
    add("long_all_but_last_task_masked", 0, [(240, -0.25)] * 768 + spread(40, masked=0.0))
    add("long_task_150_below", 0, [(0, LIVE)] * 256 + [(int(t), LIVE) for t in rng.choice([160, 192, 200], 700)])
    add("long_all_le_-500", -3072, spread(600))
    add("long_dead", 0, [(240, -0.25)] * 300)
    n_named = len(rows)
    for _ in range(n_filler):
        d = int(rng.integers(0, 9))
        U = int(rng.choice([0, 16, 64, -64]))
        add_rows = [(int(t), (-0.25 if rng.random() < 0.05 else LIVE)) for t in rng.choice(T_set, d)]
        rows.append((U, add_rows))
    names[len(rows)] = "dead_last_row"
    rows.append((0, [(192, -0.25), (0, 0.0)]))
    n_rows = len(rows)
    pool = {t: [n_rows + 2 * k, n_rows + 2 * k + 1] for k, t in enumerate(T_set)}
    n_cols = n_rows + 2 * len(T_set)
    node_key = [(U, 0) for U, _e in rows] + [(0, t) for t in T_set for _ in range(2)]
    keys = sorted(set(node_key))
    proto_id = np.array([keys.index(k) for k in node_key])
    P = np.stack([proto(*k) for k in keys])
    Wh = P[proto_id]
    rowptr = np.zeros(n_rows + 1, np.int64)
    rowptr[1:] = np.cumsum([len(e) for _U, e in rows])
    col = np.empty(rowptr[-1], np.int64)
    val = np.empty(rowptr[-1])
    k = 0
    for r, (U, ents) in enumerate(rows):
        for t, v in ents:
            col[k] = pool[t][int(rng.integers(0, 2))] if (r < n_named or rng.random() < 0.5) else int(rng.integers(0, n_cols))
            val[k] = rng.uniform(0.1, 1.0) if v is None else v
            k += 1
    # "ties": the same node twice, and a masked entry on the live maximum's node
    r = next(r for r, n in names.items() if n == "ties")
    col[rowptr[r]:rowptr[r + 1]] = [pool[80][0], pool[80][0], pool[80][0], pool[0][0], pool[80][1], pool[80][0]]
    val = _round(val, dt)
    if dt == "f16":
        val[np.signbit(val) & (val == 0)] = -0.0
    att = np.empty((heads, 2, f_head))
    att[:] = rng.standard_normal((heads, 2, f_head)) * (0.3 / np.sqrt(f_head))
    att[:, 0, 0], att[:, 0, 1], att[:, 1, 0], att[:, 1, 1] = SCALE, 0.0, 0.0, SCALE
    return dict(rowptr=rowptr, col=col, val=val, Wh=Wh, att=_round(att.reshape(-1), dt), names=names,
                n_rows=n_rows, n_cols=n_cols, protos=P, proto_id=proto_id)


def plain_graph(dt, heads, f_head, seed=0, n=600):
    """Inputs like the suite's other GAT tests: scores of order 1 (attention scaled to 1 / sqrt(f_head)), masked
    entries -0.25, short random rows."""
    rng = np.random.default_rng(seed)
    F = heads * f_head
    deg = rng.integers(0, 40, n)
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(deg)
    col = rng.integers(0, n, rowptr[-1])
    val = rng.uniform(0.05, 1.0, rowptr[-1])
    val[rng.random(rowptr[-1]) < 0.05] = -0.25
    Wh = _round(rng.standard_normal((n, F)) * 0.6, dt)
    att = _round(rng.standard_normal(2 * F) / np.sqrt(f_head), dt)
    return dict(rowptr=rowptr, col=col, val=_round(val, dt), Wh=Wh, att=att, names={}, n_rows=n, n_cols=n)


# ---- deliberately wrong forms, for the mutation checks ----------------------------------------------------------------

def mutant(g, heads, kind, dead_rule="zero", out="f16", relu=False, alpha=0.2):
    """D and S of a broken variant of the aggregate, rounded as a kernel's output would be:
    "max_stored"     the row maximum over the STORED entries, fp32 exponentials;
    "max_from_zero"  a running maximum started at 0 instead of -inf, fp32 exponentials;
    "merge_no_rescale"  rows taken in chunks of 8 entries whose states are merged, the accumulator not rescaled;
    "mask_ne0", "mask_ge0", "mask_ftz"  the mask as values != 0, >= 0, > 0 with fp32 subnormals flushed."""
    if kind.startswith("mask_"):
        v = g["val"]
        live = {"mask_ne0": v != 0, "mask_ge0": v >= 0, "mask_ftz": (v > 0) & (np.abs(v) >= 2.0 ** -126)}[kind]
        r = forward(g, heads, alpha=alpha, relu=relu, dead_rule=dead_rule, out=out, live=live)
        return dict(D=r["D"], S=r["S"])
    ref = forward(g, heads, alpha=alpha, relu=relu, dead_rule=dead_rule, out=out)
    rowptr, col = g["rowptr"].astype(np.int64), g["col"].astype(np.int64)
    n_rows, F = ref["D"].shape
    f = F // heads
    Whh = g["Wh"].reshape(-1, heads, f)
    x = ref["E"].reshape(len(col), heads)
    live = ref["live"][:, None]
    row = ref["row"]
    D, S = ref["D"].copy(), ref["S"].reshape(len(col), heads).copy()
    if kind in ("max_stored", "max_from_zero"):
        x32 = x.astype(np.float32)
        if kind == "max_stored":
            m = _seg(np.maximum, x32, rowptr, np.float32(-np.inf))
        else:
            m = np.maximum(_seg(np.maximum, np.where(live, x32, np.float32(-np.inf)), rowptr, np.float32(-np.inf)),
                           np.float32(0))
        with np.errstate(all="ignore"):
            p = np.where(live, np.exp((x32 - m[row]).astype(np.float32)), np.float32(0))
            l = _seg(np.add, p.astype(np.float32), rowptr, np.float32(0))
            w = (p / l[row]).astype(np.float64)
            Dm = _seg(np.add, w[:, :, None] * Whh[col], rowptr, 0.0).reshape(n_rows, F)
        keep = ~ref["dead"]
        D[keep] = np.maximum(Dm[keep], 0) if relu else Dm[keep]
        S[~ref["dead"][row]] = w[~ref["dead"][row]]
    else:
        assert kind == "merge_no_rescale"
        for i in np.nonzero((np.diff(rowptr) > 8) & ~ref["dead"])[0]:
            e0, e1 = rowptr[i], rowptr[i + 1]
            m = np.full(heads, -np.inf)
            l = np.zeros(heads)
            acc = np.zeros((heads, f))
            for c0 in range(e0, e1, 8):
                xs, lv = x[c0:min(c0 + 8, e1)], live[c0:min(c0 + 8, e1)]
                mk = np.where(lv, xs, -np.inf).max(0)
                mn = np.maximum(m, mk)
                mn0 = np.where(np.isfinite(mn), mn, 0.0)
                with np.errstate(invalid="ignore"):
                    l = np.where(np.isfinite(m), l * np.exp(m - mn0), 0.0)
                p = np.where(lv, np.exp(np.where(lv, xs - mn0, 0.0)), 0.0)
                l = l + p.sum(0)
                acc = acc + np.einsum("eh,ehk->hk", p, Whh[col[c0:min(c0 + 8, e1)]])     # (acc is not rescaled)
                m = mn
            d = (acc / l[:, None]).reshape(F)
            D[i] = np.maximum(d, 0) if relu else d
    return dict(D=D, S=S[:, 0] if heads == 1 else S)

"""sgx_quant_stack_forward on the GPU (include/sgx.h, "quantised layers in the small-graph stack"), stage by stage: layer
l + 1's reference input is the device's own D_l (want_layer_outputs), so no grid step flipped by a last-ulp difference
propagates and no tolerance is invented.

GCN layers, pooled and logits: the same BITS as the chain ops.layer_forward(quant=...) x n -> ops.readout_mean_linear, on
the fused and on the chained path.  Derivable: X_q . W_q on grid values is exact in fp32 while the sum of |code products|
stays below 2^24 (asserted on every layer's inputs, _quant_ref.stage1), and the aggregate is the same fma chain in CSR
order.  GAT layers: H from _quant_ref.stage1 on the device's D_{l-1} (exact), D inside _gat_ref's bound times deq_factor.
Parity of the quantised layer itself is unpinned: the reference records no quantised output.
"""
import os

import numpy as np
import pytest
import torch

import _gat_stack_ref as S
import _quant_ref as Q
import _quant_stack_ref as QS

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ALPHA = 0.2
I32 = dict(dtype=torch.int32, device=DEV)


def bits_of(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits_of(a), bits_of(b))


def f32(t):
    return t.float().cpu().numpy()


def no_workspace(monkeypatch):
    """The fused path: sgx_quant_stack_workspace_bytes is 0, so ops asks for no workspace."""
    from sgracex1_amd import ops

    def refuse(device, nbytes):
        raise AssertionError(f"a workspace of {nbytes} bytes was asked for: not the fused path")
    monkeypatch.setattr(ops, "_workspace", refuse)


def needs_workspace(monkeypatch):
    from sgracex1_amd import ops
    asked, real = [], ops._workspace

    def record(device, nbytes):
        asked.append(int(nbytes))
        return real(device, nbytes)
    monkeypatch.setattr(ops, "_workspace", record)
    return asked


def constants(nbits, n_layers):
    """Layer 1 on the constants of init_SGRACE, every later layer on second_layer()."""
    from sgracex1_amd import quant
    c = quant.constants(nbits)
    return [c] + [c.second_layer()] * (n_layers - 1)


def tie_values(c, rng, n):
    """n feature values x with fl(fl(1 / f_s) * x) + f_z == k + 0.5 exactly in fp32: grid ties of the quantiser."""
    inv = np.float32(1 / c.f_s)
    k = rng.integers(0, 2 ** c.w_qbits - 1, 4 * n + 64)
    x = ((k + 0.5) * c.f_s).astype(np.float32)
    t = (inv * x).astype(np.float32) + np.float32(c.f_z)
    x = x[t == (k + 0.5).astype(np.float32)]
    assert len(x) >= n, "no exact tie among the candidates"
    return x[:n]


def host_case(nbits, m_in, widths, gat, sparse, seed, budget=None, **batch):
    """_gat_stack_ref.build_batch's block structure (a 1-row graph, an empty one, one of exactly the row budget) with
    operands for the quantiser: adjacency values over the unsigned range and past it, a tenth below half a step (stored
    entries that quantise to 0, inside rows that keep live ones) and one row whose every entry does; features over
    [0, 1] and past it, negative, at exact grid ties, -0.0 and hot rows that drive H to its clip bounds with
    _quant_ref.weights' hot columns.  Returns the host arrays."""
    n = len(widths)
    qs = constants(nbits, n)
    c = qs[0]
    width = max(list(widths) + ([] if sparse else [m_in]))
    R_ = S.rows_budget("f32", width)
    b = S.build_batch("f32", R_ if budget is None else budget, m_in, seed=seed, **batch)
    rng = np.random.default_rng([seed, 11])
    rowptr, col, N = b["rowptr"], b["col"], b["n_rows"]
    nnz = len(col)
    val = (rng.uniform(0.6, 2 ** nbits + 0.4, nnz) * c.a_s).astype(np.float32)
    val[rng.random(nnz) < 0.1] = np.float32(0.3 * c.a_s)
    deg = np.diff(rowptr)
    # graph 0 of build_batch: rows 8 .. 15 hold a self loop and two more entries; row 9 loses every entry to the
    # quantiser, row 10 keeps live entries beside one that quantises to 0
    killed, mixed = 9, 10
    assert deg[killed] >= 2 and deg[mixed] >= 2
    val[rowptr[killed]:rowptr[killed + 1]] = np.float32(0.3 * c.a_s)
    val[rowptr[mixed]:rowptr[mixed + 1]] = np.float32(0.9)
    val[rowptr[mixed]] = np.float32(0.3 * c.a_s)
    x = Q.features(N, m_in, c, seed, dense=True)
    flat = x.reshape(-1)
    where = rng.choice(flat.size, 24, replace=False)
    flat[where[:8]] = tie_values(c, rng, 8)
    flat[where[8:16]] = -0.0
    flat[where[16:]] = -0.25
    stored = (x != 0) | np.signbit(x)                                    # a CSR X stores its -0.0 entries too
    Ws = []
    m = m_in
    for l, P in enumerate(widths):
        Ws.append(Q.weights(m, P, qs[l], seed + l))
        m = P
    atts = [Q.attention(P, qs[l], seed + l) if g else None for l, (P, g) in enumerate(zip(widths, gat))]
    fea_host = x
    if sparse:
        fr = np.concatenate([[0], np.cumsum(stored.sum(1))])
        fea_host = (fr.astype(np.int64), np.nonzero(stored)[1].astype(np.int64), x[stored])
    return dict(b=b, qs=qs, a_val=val, fea_host=fea_host, x=x, Ws=Ws, atts=atts, width=width, budget=R_, killed=killed,
                mixed=mixed, sparse=sparse, nbits=nbits, m_in=m_in, seed=seed, widths=widths)


def build_case(nbits, m_in, widths, gat, sparse, seed, budget=None, **batch):
    """host_case and its device copies."""
    from sgracex1_amd import ops
    c = host_case(nbits, m_in, widths, gat, sparse, seed, budget, **batch)
    b, val, x, fea_host = c["b"], c["a_val"], c["x"], c["fea_host"]
    rowptr, col, N = b["rowptr"], b["col"], b["n_rows"]
    adj = ops.Csr(torch.tensor(rowptr, **I32), torch.tensor(col, **I32), torch.tensor(val, device=DEV), N)
    if sparse:
        fea = ops.Csr(torch.tensor(fea_host[0], **I32), torch.tensor(fea_host[1], **I32), torch.tensor(fea_host[2], device=DEV), m_in)
    else:
        fea = torch.tensor(x, device=DEV)
    rng = np.random.default_rng(seed + 77)
    c.update(adj=adj, fea=fea, ptr=torch.tensor(b["graph_ptr"], **I32),
             wts=[torch.tensor(W.T.copy(), device=DEV) for W in c["Ws"]],
             atts_d=[None if a is None else torch.tensor(a, device=DEV) for a in c["atts"]],
             head_w=torch.tensor(rng.standard_normal((3, widths[-1])), device=DEV, dtype=torch.float32),
             head_b=torch.tensor(rng.standard_normal(3), device=DEV, dtype=torch.float32))
    return c


def run(c, relus, plan=None, adj=None, adj_quantised=False, quants="case"):
    from sgracex1_amd import ops
    plan = ops.BatchPlan.cached(c["adj"], c["ptr"], c["width"]) if plan is None else plan
    (logits, pooled), outs = ops.quant_stack_forward(
        c["adj"] if adj is None else adj, c["fea"], c["wts"], c["atts_d"], relus, c["ptr"], c["qs"] if quants == "case" else quants,
        c["head_w"], c["head_b"], alpha=ALPHA, plan=plan, adj_quantised=adj_quantised, want_layer_outputs=True, want_pooled=True)
    return dict(logits=logits, pooled=pooled, outs=outs, plan=plan)


def assert_input_edges(c):
    """The edges the case was built for are in its inputs (on the reference's own numbers)."""
    q0, x, b = c["qs"][0], c["x"], c["b"]
    t = (np.float32(1 / q0.f_s) * x).astype(np.float32) + np.float32(q0.f_z)
    assert (t - np.floor(t) == 0.5).sum() >= 4, "no feature at a grid tie"
    assert (t > 2 ** q0.w_qbits - 1).any() and (x < 0).any() and (np.signbit(x) & (x == 0)).any()
    aq = Q.quantise_adj(c["a_val"], q0)
    rp = b["rowptr"]
    k, m = c["killed"], c["mixed"]
    assert not (aq[rp[k]:rp[k + 1]] > 0).any() and (c["a_val"][rp[k]:rp[k + 1]] > 0).all()       # the row that loses every entry
    assert aq[rp[m]] == 0 and (aq[rp[m] + 1:rp[m + 1]] > 0).all()                               # a zero inside a live row
    if q0.w_qbits == 4:
        assert c["a_val"][rp[m]] < 1 / 30
    sizes = b["sizes"]
    assert 1 in sizes and 0 in sizes and max(sizes) == c["b"]["sizes"][7]                        # 1-row, empty, budget-sized


def check_stages(c, relus, got, gat):
    """Every layer on the device's own D_{l-1}: GCN layers and the readout bit-equal to the chained calls, GAT layers
    inside the bound on the exact H."""
    from sgracex1_amd import ops
    adj_host = (c["b"]["rowptr"], c["b"]["col"])
    X_dev, X_host = c["fea"], c["fea_host"]
    clipped = above = 0
    for l, (Wt, relu, q) in enumerate(zip(c["wts"], relus, c["qs"])):
        r = QS.layer_ref(adj_host, c["a_val"], X_host, c["Ws"][l], c["atts"][l], q, relu, alpha=ALPHA)
        assert r["magnitude"] < Q.EXACT_BELOW, f"layer {l}: the code sums reach 2^24"
        clipped += r["facts"]["clip_hi"] + r["facts"]["clip_lo"]
        D = got["outs"][l]
        if not gat[l]:
            want = ops.layer_forward(c["adj"], X_dev, Wt, relu=relu, quant=q)
            assert same_bits(D, want), f"GCN layer {l}"
            Q.check_D(f32(D), r["D"], r["bound"])                          # (and the chain is where the reference says)
        else:
            Q.check_D(f32(D), r["D"], r["bound"], c["b"]["names"])
            assert r["dead"][c["killed"]] and not r["dead"].all()
            assert not bits_of(D)[torch.tensor(r["dead"], device=DEV)].any(), f"dead rows of layer {l}"
        if l + 1 < len(relus):
            q2 = c["qs"][l + 1]
            above += int((f32(D) / q2.f_s + q2.f_z > 2 ** q2.w_qbits - 1).sum())
        X_dev, X_host = D, f32(D)
    logits, pooled = ops.readout_mean_linear(X_dev, c["ptr"], c["head_w"], c["head_b"], want_pooled=True)
    assert same_bits(got["pooled"], pooled) and same_bits(got["logits"], logits)
    return clipped, above


# ---- 1. GCN layers bit-equal to the chain, fused and chained ---------------------------------------------------------
GCN = [  # bits, K of layer 0, widths, sparse layer 0
    (8, 7, (64,), True),
    (8, 18, (7, 20), False),
    (8, 64, (65, 252, 1, 64), False),
    (4, 7, (20, 64), True),
    (4, 64, (64, 7, 65, 1), True),
    (4, 18, (252,), False),
    (2, 18, (64, 20), False),
    (2, 7, (7,), True),
    (1, 64, (20, 64, 7, 65), False),
    (1, 7, (1, 64), True),
]
RELUS = [True, False, True, False]


@pytest.mark.parametrize("path", ["fused", "chained"])
@pytest.mark.parametrize("case", range(len(GCN)))
def test_gcn_layers_bit_equal_to_the_chain(case, path, monkeypatch):
    nbits, m_in, widths, sparse = GCN[case]
    n = len(widths)
    width = max(widths + (() if sparse else (m_in,)))
    over = S.rows_budget("f32", width) + 1                               # chained: one graph over the budget
    c = build_case(nbits, m_in, widths, [0] * n, sparse, seed=case, budget=over if path == "chained" else None)
    assert_input_edges(c)
    if path == "fused":
        no_workspace(monkeypatch)
        got = run(c, RELUS[:n])
        assert got["plan"].fits and got["plan"].max_graph == c["budget"] and got["plan"].groups >= 3
    else:
        asked = needs_workspace(monkeypatch)
        got = run(c, RELUS[:n])
        assert not got["plan"].fits and got["plan"].groups == 0 and len(asked) == 1 and asked[0] > 0
    monkeypatch.undo()
    clipped, above = check_stages(c, RELUS[:n], got, [0] * n)
    if Q.can_clip(c["qs"][0], m_in) and widths[0] > 1:
        assert clipped > 0, "no H entry on a clip bound"
    if n > 1 and nbits >= 4:
        assert above > 0, "no layer output above the next layer's feature range"


# ---- 2. GAT layers --------------------------------------------------------------------------------------------------
GAT = [  # bits, K, widths, gat_mode per layer, sparse
    (8, 7, (64, 64), (1, 1), True),
    (8, 18, (20, 65, 7), (1, 0, 1), False),
    (4, 7, (64, 20), (0, 1), True),
    (4, 64, (7, 252), (1, 1), False),
]


@pytest.mark.parametrize("path", ["fused", "chained"])
@pytest.mark.parametrize("case", range(len(GAT)))
def test_gat_layers_inside_the_bound(case, path, monkeypatch):
    nbits, m_in, widths, gat, sparse = GAT[case]
    n = len(widths)
    width = max(widths + (() if sparse else (m_in,)))
    over = S.rows_budget("f32", width) + 1
    c = build_case(nbits, m_in, widths, gat, sparse, seed=20 + case, budget=over if path == "chained" else None)
    assert c["qs"][1] == c["qs"][0].second_layer()
    assert_input_edges(c)
    if path == "fused":
        no_workspace(monkeypatch)
        got = run(c, RELUS[:n])
        assert got["plan"].fits and got["plan"].groups >= 3
    else:
        asked = needs_workspace(monkeypatch)
        got = run(c, RELUS[:n])
        assert not got["plan"].fits and len(asked) == 1 and asked[0] > 0
    monkeypatch.undo()
    check_stages(c, RELUS[:n], got, gat)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_tiles_that_fill_64_kib_on_a_second_device_of_the_process(monkeypatch):
    """Width 252 (the last GAT case) on device 0 and then on device 1: the kernel's opt-in to more than 64 KiB of LDS is per
    device."""
    nbits, m_in, widths, gat, sparse = GAT[3]
    assert max(widths) == 252
    for k in (0, 1):
        with torch.cuda.device(k):
            c = build_case(nbits, m_in, widths, gat, sparse, seed=23)
            no_workspace(monkeypatch)
            got = run(c, RELUS[:2])
            assert got["plan"].fits
            monkeypatch.undo()
            check_stages(c, RELUS[:2], got, gat)


# ---- 3. adjacency quantised in flight against quantised beforehand ----------------------------------------------------
@pytest.mark.parametrize("nbits,gat", [(8, (1, 0)), (4, (0, 1))])
def test_adjacency_quantised_in_flight_and_beforehand(nbits, gat, monkeypatch):
    no_workspace(monkeypatch)
    c = build_case(nbits, 18, (20, 64), gat, False, seed=31)
    flight = run(c, [True, False])
    monkeypatch.undo()
    before = c["adj"].quantized(c["qs"][0])
    assert not torch.equal(before.val, c["adj"].val)
    no_workspace(monkeypatch)
    done = run(c, [True, False], adj=before, adj_quantised=True)
    for l in range(2):
        assert same_bits(flight["outs"][l], done["outs"][l]), l
    assert same_bits(flight["logits"], done["logits"]) and same_bits(flight["pooled"], done["pooled"])


# ---- 4. repeatability and grouping ------------------------------------------------------------------------------------
def test_same_bits_on_every_run_and_for_every_grouping(monkeypatch):
    from sgracex1_amd import _lib, ops
    no_workspace(monkeypatch)
    small = S.rows_budget("f32", 64, backward=True)
    assert 16 <= small < S.rows_budget("f32", 64)
    c = build_case(8, 7, (64, 64), (1, 0), True, seed=5, budget=small, n_graphs=20, filler=(20, 30))
    a = run(c, [True, False])
    again = run(c, [True, False])
    other = run(c, [True, False], plan=ops.BatchPlan(c["adj"], c["ptr"], 64, _lib.SGX_BATCH_BACKWARD))
    assert c["b"]["n_rows"] > 256 and a["plan"].fits and other["plan"].fits
    ga, go = a["plan"].export_groups().cpu().numpy(), other["plan"].export_groups().cpu().numpy()
    assert len(ga) != len(go) or (ga != go).any()
    for name, r in (("second run", again), ("backward plan", other)):
        for l in range(2):
            assert same_bits(a["outs"][l], r["outs"][l]), (name, l)
        assert same_bits(a["logits"], r["logits"]) and same_bits(a["pooled"], r["pooled"]), name


# ---- 5. the null quantiser ----------------------------------------------------------------------------------------------
def test_null_quantisers_give_gat_stack_forward(monkeypatch):
    from sgracex1_amd import ops
    no_workspace(monkeypatch)
    c = build_case(8, 7, (64, 20), (1, 0), True, seed=41)
    got = run(c, [True, False], quants=[None, None])
    logits, outs = ops.gat_stack_forward(c["adj"], c["fea"], c["wts"], c["atts_d"], [True, False], c["ptr"], c["head_w"],
                                         c["head_b"], alpha=ALPHA, want_layer_outputs=True, plan=got["plan"])
    for l in range(2):
        assert same_bits(got["outs"][l], outs[l]), l
    assert same_bits(got["logits"], logits)
    # one layer with, one without: the plain layer is layer_forward's
    mixed = run(c, [True, False], quants=[c["qs"][0], None])
    monkeypatch.undo()
    assert same_bits(mixed["outs"][1], ops.layer_forward(c["adj"], mixed["outs"][0], c["wts"][1], relu=False, use_plan=False))


# ---- 6. edge shapes and errors ------------------------------------------------------------------------------------------
def test_empty_batch_and_single_row_graph(monkeypatch):
    from sgracex1_amd import ops, quant
    no_workspace(monkeypatch)
    qs = constants(8, 2)
    wts = [torch.tensor(Q.weights(7, 8, qs[0], 0).T.copy(), device=DEV), torch.tensor(Q.weights(8, 4, qs[1], 1).T.copy(), device=DEV)]
    atts = [torch.tensor(Q.attention(8, qs[0], 0), device=DEV), None]
    head_w = torch.randn(2, 4, device=DEV)
    adj = ops.Csr(torch.zeros(1, **I32), torch.zeros(0, **I32), torch.zeros(0, device=DEV), 0)
    logits, outs = ops.quant_stack_forward(adj, torch.zeros((0, 7), device=DEV), wts, atts, [True, False], torch.zeros(1, **I32),
                                           qs, head_w, want_layer_outputs=True)
    assert logits.shape == (0, 2) and [tuple(o.shape) for o in outs] == [(0, 8), (0, 4)]
    # one graph of one row with a self loop: stage by stage the layer's bits
    adj = ops.Csr(torch.tensor([0, 1], **I32), torch.zeros(1, **I32), torch.full((1,), 0.5, device=DEV), 1)
    x = torch.tensor(np.random.default_rng(1).uniform(-0.1, 1.2, (1, 7)).astype(np.float32), device=DEV)
    ptr = torch.tensor([0, 1], **I32)
    pooled, outs = ops.quant_stack_forward(adj, x, wts, atts, [True, False], ptr, qs, want_layer_outputs=True)
    # ... and with the self loop below half a step the row is dead for the GAT layer: 0 from there on
    low = ops.Csr(torch.tensor([0, 1], **I32), torch.zeros(1, **I32), torch.full((1,), 0.3 * qs[0].a_s, device=DEV), 1)
    _pooled, dead_outs = ops.quant_stack_forward(low, x, wts, atts, [True, False], ptr, qs, want_layer_outputs=True)
    monkeypatch.undo()
    r = QS.layer_ref(([0, 1], [0]), [0.5], f32(x), f32(wts[0]).T, f32(atts[0]), qs[0], True, alpha=ALPHA)
    Q.check_D(f32(outs[0]), r["D"], r["bound"])
    assert same_bits(outs[1], ops.layer_forward(adj, outs[0], wts[1], relu=False, quant=qs[1]))
    assert torch.equal(pooled, outs[1])
    assert not bits_of(dead_outs[0]).any()


def test_errors_and_workspace(monkeypatch):
    from sgracex1_amd import _lib, ops, quant
    c = build_case(8, 7, (20,), (0,), True, seed=51)
    half = ops.Csr(c["adj"].rowptr, c["adj"].col, c["adj"].val.half(), c["adj"].n_cols)
    fea16 = ops.Csr(c["fea"].rowptr, c["fea"].col, c["fea"].val.half(), c["fea"].n_cols)
    with pytest.raises(_lib.SgxError) as e:
        ops.quant_stack_forward(half, fea16, [c["wts"][0].half()], [None], [True], c["ptr"], c["qs"])
    assert e.value.status == -3                                          # fp16 with a quantiser
    bad = quant.constants(8, f_z=1)
    with pytest.raises(_lib.SgxError) as e:
        ops.quant_stack_forward(c["adj"], c["fea"], c["wts"], [None], [True], c["ptr"], [bad])
    assert e.value.status == -3                                          # a zero point on a sparse layer 0
    # ... which a dense layer 0 takes, on both paths the layer's bits
    dense = torch.tensor(c["x"], device=DEV)
    no_workspace(monkeypatch)
    pooled, outs = ops.quant_stack_forward(c["adj"], dense, c["wts"], [None], [True], c["ptr"], [bad], want_layer_outputs=True)
    monkeypatch.undo()
    assert same_bits(outs[0], ops.layer_forward(c["adj"], dense, c["wts"][0], relu=True, quant=bad))


# ---- 7. capture ----------------------------------------------------------------------------------------------------------
def test_fused_call_replays_from_a_captured_graph():
    """One stream, no parallel branches: the captured graph is one kernel node."""
    from sgracex1_amd import ops
    c = build_case(8, 7, (64, 64), (1, 0), True, seed=2)
    plan = ops.BatchPlan.cached(c["adj"], c["ptr"], 64)
    assert plan.fits
    call = lambda: ops.quant_stack_forward(c["adj"], c["fea"], c["wts"], c["atts_d"], [True, False], c["ptr"], c["qs"],
                                           c["head_w"], c["head_b"], alpha=ALPHA, plan=plan)
    eager = call()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = call()
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(eager, captured)


# ---- 8. the model ----------------------------------------------------------------------------------------------------------
def _mutag_graphs(n=48):
    from sgracex1_amd import pyg_lite as G
    raw = np.load(os.path.join(GOLD, "mutag_raw.npz"))
    return G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])[:n]


def _mutag_batch(n=48, extra=None):
    from sgracex1_amd import pyg_lite as G
    graphs = _mutag_graphs(n)
    if extra is not None:
        graphs = graphs[:-1] + [extra]
    return G.collate(graphs).to(DEV)


def _bipartite(k=31):
    """K_{k,k}: every normalised entry is 1 / k -- below half a step of the 4-bit adjacency grid (1 / 30) for k = 31, so the
    quantiser kills every row of it, while unquantised every row is live."""
    from sgracex1_amd import pyg_lite as G
    a, b = np.meshgrid(np.arange(k), k + np.arange(k), indexing="ij")
    e = np.concatenate([np.stack([a.ravel(), b.ravel()]), np.stack([b.ravel(), a.ravel()])], axis=1)
    x = torch.zeros((2 * k, 7))
    x[:, 0] = 1.0
    return G.Graph(x, torch.as_tensor(e), torch.tensor([0]))


@pytest.fixture
def quant_model():
    from sgracex1_amd import config, sgrace
    saved = config.snapshot()

    def make(w_qbits=8, hidden=64, **flags):
        config.acc, config.float_type, config.fake_quantization, config.w_qbits = 1, np.float32, 1, w_qbits
        for k, v in flags.items():
            setattr(config, k, v)
        ip = sgrace.init_SGRACE()
        torch.manual_seed(7)
        return sgrace.GAT_POOL_PYNQ(7, hidden, 2).to(DEV).eval(), ip
    yield make, config, sgrace
    config.restore(saved)
    sgrace.init_SGRACE()


def _count_calls(monkeypatch):
    from sgracex1_amd import ops
    calls, real = [], ops.quant_stack_forward

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ops, "quant_stack_forward", counting)
    return calls


def _both(model, ip, b):
    with torch.no_grad():
        ip.register_map.layer_count = 1
        one = model(b.x, b.edge_index, b.batch)
        ip.register_map.layer_count = 2
        two = model(b.x, b.edge_index, b.batch)
    return one, two


def test_model_gcn_one_call_bit_equal(quant_model, monkeypatch):
    make, config, sgrace = quant_model
    model, ip = make(8, compute_attention=0)
    calls = _count_calls(monkeypatch)
    b = _mutag_batch()
    one, two = _both(model, ip, b)
    assert len(calls) == 1 and same_bits(one, two)
    assert sgrace.layern == 1                                            # as two layer calls leave it
    assert int(ip.register_map.scale_fea) == sgrace.quant_constants.second_layer().scale_fea


def test_model_gat_one_call_stage_by_stage(quant_model, monkeypatch):
    """The one call's logits are the stack's on the model's operands; the stack is checked stage by stage on them."""
    from sgracex1_amd import ops
    make, config, sgrace = quant_model
    model, ip = make(8, compute_attention=1)
    calls = _count_calls(monkeypatch)
    b = _mutag_batch()
    one, two = _both(model, ip, b)
    assert len(calls) == 1
    qc = sgrace.quant_constants
    ei, norm = sgrace.sym_norm2(b.edge_index, b.num_nodes)
    adj = sgrace._edge_csr(None, ei, norm, b.num_nodes, torch.float32)
    ptr = ops.graph_ptr_of(b.batch)
    fea = ops.Csr.from_dense(b.x, torch.float32)
    wts = [m.weight.detach().t().contiguous() for m in (model.att1, model.att2)]
    atts = [m.attention.detach().reshape(-1).contiguous() for m in (model.att1, model.att2)]
    qs = [qc, qc.second_layer()]
    monkeypatch.undo()
    logits, outs = ops.quant_stack_forward(adj.quantized(qc), fea, wts, atts, [True, False], ptr, qs, model.lin.weight,
                                           model.lin.bias, alpha=model.att1.alpha, adj_quantised=True, want_layer_outputs=True)
    assert same_bits(two, logits)
    adj_host = (adj.rowptr.cpu().numpy(), adj.col.cpu().numpy())
    aq = f32(adj.quantized(qc).val)[:adj.nnz]
    X = (fea.rowptr.cpu().numpy(), fea.col.cpu().numpy(), f32(fea.val))
    layer_outs = []
    with torch.no_grad():                                                # the layer-by-layer path's own stages
        ip.register_map.layer_count = 1
        d1 = model.reluh(model.att1(1, 0, 1, b.x, ei, norm, adj))
        d2 = model.att2(1, 1, 0, d1, ei, norm, adj)
        layer_outs = [d1, d2]
    for l in range(2):
        r = QS.layer_ref(adj_host, aq, X, f32(wts[l]).T, f32(atts[l]), qs[l], l == 0, adj_quantised=True, alpha=model.att1.alpha)
        assert r["magnitude"] < Q.EXACT_BELOW and not r["dead"].any()
        Q.check_D(f32(outs[l]), r["D"], r["bound"])
        if l == 0:
            Q.check_D(f32(layer_outs[0]), r["D"], r["bound"])           # both paths inside the same bound on the same input
        X = f32(outs[l])
    want = ops.readout_mean_linear(outs[1], ptr, model.lin.weight, model.lin.bias)
    assert same_bits(logits, want)
    assert torch.isfinite(one).all() and one.shape == two.shape


@pytest.mark.parametrize("why", ["killed_row", "float16", "int8_hidden_200"])
def test_model_declines_the_route(why, quant_model, monkeypatch):
    make, config, sgrace = quant_model
    calls = _count_calls(monkeypatch)
    if why == "killed_row":
        model, ip = make(4, compute_attention=1)
        b = _mutag_batch(extra=_bipartite())
        one, two = _both(model, ip, b)
        assert not calls and same_bits(one, two)
        # ... and it was the quantiser that killed the rows: unquantised the same batch takes the one call
        ei, norm = sgrace.sym_norm2(b.edge_index, b.num_nodes)
        adj = sgrace._edge_csr(None, ei, norm, b.num_nodes, torch.float32)
        assert adj.quantized(sgrace.quant_constants).has_dead_rows
        plain = adj.val[:adj.nnz] > 0
        deg = (adj.rowptr[1:] - adj.rowptr[:-1]).long()
        row = torch.repeat_interleave(torch.arange(adj.n_rows, device=DEV), deg)
        assert torch.zeros(adj.n_rows, device=DEV).index_add_(0, row, plain.float()).min() > 0
    elif why == "float16":
        model, ip = make(8, compute_attention=0, float_type=np.float16)
        b = _mutag_batch()
        for count in (1, 2):                                             # the layer's own refusal, on either setting
            ip.register_map.layer_count = count
            with torch.no_grad(), pytest.raises(TypeError, match="float32 buffers"):
                model(b.x, b.edge_index, b.batch)
        assert not calls
    else:
        model, ip = make(8, hidden=200, compute_attention=0, hardware_quantize=1)
        b = _mutag_batch()
        one, two = _both(model, ip, b)
        assert not calls and same_bits(one, two)
        # with 128 hidden columns the layer takes the fp32 form and the one call is made
        model, ip = make(8, hidden=128, compute_attention=0, hardware_quantize=1)
        one, two = _both(model, ip, b)
        assert len(calls) == 1 and same_bits(one, two)

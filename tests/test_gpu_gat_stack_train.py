"""sgx_gat_stack_backward on the GPU (include/sgx.h, "training the GAT stack"): all-GCN descriptors against
sgx_stack_backward (G bit for bit); GAT layers -- E, S, G, grad_W and grad_attention -- inside the derived bound of the
float64 restatement (tests/_gat_stack_grad_ref.py) on the device's own layer outputs, on tests/_gat_stack_ref.py's batch
of mask and softmax edge cases; the grid and its ordering; edge shapes; refusals; GAT_POOL_PYNQ(train_stack=True); a
captured step; twenty epochs on MUTAG."""
import os

import numpy as np
import pytest
import torch

import _gat_ref as R
import _gat_stack_ref as S
from _gat_stack_grad_ref import gat_stack_grad_f64, top_attention_grad_f64, top_layer_g, within
from _stack_grad_ref import stack_grad_bound, stack_grad_f64

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TORCH = {"f16": torch.float16, "f32": torch.float32}
UNIT = {"f16": 2.0 ** -11, "f32": 2.0 ** -24}
ALPHA = 0.2
BACKWARD = 1


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def f64(t):
    return t.detach().double().cpu().numpy()


def on_device(b, dt, sparse):
    from sgracex1_amd import ops
    td = TORCH[dt]
    adj = ops.Csr(torch.tensor(b["rowptr"], dtype=torch.int32, device=DEV), torch.tensor(b["col"], dtype=torch.int32, device=DEV),
                  torch.tensor(b["val"], device=DEV).to(td), b["n_rows"])
    x = torch.tensor(b["x"], device=DEV).to(td)
    return adj, (ops.Csr.from_dense(x, td) if sparse else x), torch.tensor(b["graph_ptr"], dtype=torch.int32, device=DEV)


def layers_for(dt, m_in, widths, gat, seed):
    """Per layer (W [M, P] float64 of dt values, attention [2 P] or None): the first GAT layer on the features carries the
    designed scores of _gat_stack_ref.build_batch, the others scores of order 1."""
    Ws, atts = [], []
    m = m_in
    for l, (P, g) in enumerate(zip(widths, gat)):
        W, att = S.first_layer(dt, m, P, seed) if (l == 0 and g) else S.plain_layer(dt, m, P, seed + l)
        Ws.append(W)
        atts.append(att if g else None)
        m = P
    return Ws, atts


def run(b, dt, Ws, atts, relus, sparse, width, seed=0, plan=None):
    """The forward (for the D_l the backward reads) and the backward on batch b; everything the checks need."""
    from sgracex1_amd import ops
    td = TORCH[dt]
    adj, x, ptr = on_device(b, dt, sparse)
    if plan is None:
        plan = ops.BatchPlan(adj, ptr, width, BACKWARD)
    assert plan.fits
    wts = [torch.tensor(W.T.copy(), device=DEV).to(td).contiguous() for W in Ws]
    atts_d = [None if a is None else torch.tensor(a, device=DEV).to(td) for a in atts]
    _, outs = ops.gat_stack_forward(adj, x, wts, atts_d, relus, ptr, alpha=ALPHA, want_layer_outputs=True, plan=plan)
    rng = np.random.default_rng(seed + 5)
    gp = torch.tensor(rng.standard_normal((len(b["graph_ptr"]) - 1, Ws[-1].shape[1])), device=DEV, dtype=torch.float32)
    w32 = [torch.tensor(W, device=DEV, dtype=torch.float32) for W in Ws]
    a32 = [None if a is None else torch.tensor(a, device=DEV, dtype=torch.float32) for a in atts]
    call = lambda: ops.gat_stack_backward(adj, x, w32, a32, relus, ptr, outs, gp, alpha=ALPHA, plan=plan, want_G=True,
                                          want_edge_outputs=True)
    dW, dA, G, ES = call()
    return dict(b=b, adj=adj, x=x, ptr=ptr, plan=plan, outs=outs, gp=gp, w32=w32, a32=a32, dW=dW, dA=dA, G=G, ES=ES, call=call)


def check(c, dt, Ws, atts, relus, figures=None):
    """E, S and G per layer, grad_W and grad_attention against the restatement on the device's own D_l; rows without a
    live entry exactly 0 in S and G."""
    b = c["b"]
    nnz = int(b["rowptr"][-1])
    E_dev = [None if es is None else f64(es[0]) for es in c["ES"]]
    ref = gat_stack_grad_f64((b["rowptr"], b["col"], b["val"]), b["x"], Ws, atts, relus, b["graph_ptr"], f64(c["gp"]),
                             [f64(D) for D in c["outs"]], alpha=ALPHA, E_dev=E_dev, unit=UNIT[dt], sub=R.OUT_SUB[dt])
    worst = {}
    for l in range(len(Ws)):
        if atts[l] is not None:
            E, Sd = f64(c["ES"][l][0])[:nnz], f64(c["ES"][l][1])[:nnz]
            row = R.rows_of(np.asarray(b["rowptr"], np.int64))
            R.check(f"E_{l}", E, ref["E"][l], ref["bE"][l], row, b["names"])
            R.check(f"S_{l}", Sd, ref["S"][l], ref["bS"][l], row, b["names"])
            live = np.asarray(b["val"])[:nnz] > 0
            assert not bits(c["ES"][l][1][:nnz])[torch.tensor(~live, device=DEV)].any(), f"S_{l} on masked entries"
            dead = torch.tensor(ref["dead"][l], device=DEV)
            if ref["dead"][l].any():
                assert not bits(c["G"][l])[dead].any(), f"G_{l} on rows without a live entry"
            ok, worst[f"dA_{l}"] = within(f64(c["dA"][l]), ref["dA"][l], ref["mA"][l], ref["tA"][l])
            print(f"grad_attention_{l}: worst {worst[f'dA_{l}']:.3f} of the bound")
            assert ok, (l, "grad_attention", worst[f"dA_{l}"])
        else:
            assert c["dA"][l] is None and c["ES"][l] is None
        for name, got, key in (("G", c["G"][l], "G"), ("dW", c["dW"][l], "W")):
            ok, worst[f"{name}_{l}"] = within(f64(got), ref["G" if key == "G" else "dW"][l], ref["m" + key][l], ref["t" + key][l])
            print(f"{name}_{l}: worst {worst[f'{name}_{l}']:.3f} of the bound")
            assert ok, (l, name, worst[f"{name}_{l}"])
    if figures is not None:
        figures.update(worst)
    return ref


# ---- 1. all layers gat_mode = 0 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("m_in,widths,sparse", [(7, (64, 64), True), (21, (100, 3, 64), False), (7, (16,), True)])
def test_all_gcn_descriptors_are_sgx_stack_backward(dt, m_in, widths, sparse):
    from sgracex1_amd import ops
    relus = [True, False, True][:len(widths)]
    width = max(list(widths) + ([] if sparse else [m_in]))
    b = S.build_batch(dt, S.rows_budget(dt, width, backward=True), m_in, seed=1)
    Ws, atts = layers_for(dt, m_in, widths, [0] * len(widths), 1)
    c = run(b, dt, Ws, atts, relus, sparse, width, seed=1)
    assert c["plan"].groups >= 3
    dW, G = ops.gcn_stack_backward(c["adj"], c["x"], c["w32"], relus, c["ptr"], c["outs"], c["gp"], plan=c["plan"], want_G=True)
    adj_np = (b["rowptr"], b["col"], b["val"])
    outs_np = [f64(D) for D in c["outs"]]
    ref, _ = stack_grad_f64(adj_np, b["x"], Ws, relus, b["graph_ptr"], f64(c["gp"]), outs=outs_np)
    bounds = stack_grad_bound(adj_np, b["x"], Ws, b["graph_ptr"], f64(c["gp"]), outs_np, UNIT[dt])
    for l in range(len(widths)):
        assert same_bits(c["G"][l], G[l]), f"G_{l}"
        assert c["dA"][l] is None
        err = np.abs(f64(c["dW"][l]) - ref[l])
        assert (err <= bounds[l]).all(), f"dW_{l}: {float((err / bounds[l]).max())}"


# ---- 2. GAT layers on the batch of mask and softmax edge cases ------------------------------------------------------------
CASES = [  # m_in, widths, gat_mode per layer, relu per layer, sparse layer 0
    (7, (64,), (1,), (1,), True),
    (20, (1,), (1,), (0,), False),
    (7, (64, 64), (1, 1), (1, 0), True),
    (7, (7, 20), (1, 0), (1, 1), False),
    (9, (65, 20, 7), (0, 1, 1), (1, 0, 1), True),
    (65, (20, 64), (1, 1), (0, 0), False),
    (7, (20, 64, 7, 1), (1, 0, 1, 1), (1, 1, 0, 0), False),
    (7, (252, 64), (1, 1), (1, 0), True),                    # the budget is 16 rows
]


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_gat_layers_against_the_restatement(dt, case):
    m_in, widths, gat, relus, sparse = CASES[case]
    relus = [bool(r) for r in relus]
    width = max(list(widths) + ([] if sparse else [m_in]))
    budget = S.rows_budget(dt, width, backward=True)
    if 252 in widths:
        assert budget == 16
    b = S.build_batch(dt, budget, m_in, seed=case)
    Ws, atts = layers_for(dt, m_in, widths, gat, case)
    c = run(b, dt, Ws, atts, relus, sparse, width, seed=case)
    assert c["plan"].rows == budget and c["plan"].max_graph == budget and c["plan"].groups >= 3
    ref = check(c, dt, Ws, atts, relus)
    first = next(l for l in range(len(gat)) if gat[l])
    if first == 0 and widths[0] >= 2:
        # the special graph's rows: none live on rows 0 and 1, weights that underflow on the spread rows
        assert ref["dead"][0][:2].all() and not ref["dead"][0][2]
        assert (ref["S"][0][np.asarray(b["val"])[:len(ref["S"][0])] > 0] < 1e-30).any()
    again = c["call"]()
    for a_, b_ in zip(again[0] + [g for g in again[1] if g is not None], c["dW"] + [g for g in c["dA"] if g is not None]):
        assert same_bits(a_, b_)


def test_a_batch_of_masked_rows_gives_no_gradient():
    """Every stored value masked (+0.0, -0.0, negative): S, G, sg and with them every gradient are exactly 0."""
    dt = "f32"
    rng = np.random.default_rng(3)
    sizes = [3, 1, 5, 2]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = []
    for a, e in zip(ptr[:-1], ptr[1:]):
        for i in range(a, e):
            rows.append([(int(c), float(rng.choice([0.0, -0.0, -0.5, -2.0]))) for c in range(a, e) if rng.random() < 0.7])
    b = dict(rowptr=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
             col=np.array([c for r in rows for c, _ in r], np.int64), val=np.array([v for r in rows for _, v in r], np.float64),
             x=R._round(rng.standard_normal((int(ptr[-1]), 7)), dt), graph_ptr=ptr, names={}, n_rows=int(ptr[-1]))
    Ws, atts = layers_for(dt, 7, (20, 7), (1, 1), 0)
    Ws[0], atts[0] = S.plain_layer(dt, 7, 20, 9)
    c = run(b, dt, Ws, atts, [False, False], False, 20)
    for l in range(2):
        for t in (c["dW"][l], c["dA"][l], c["G"][l], c["ES"][l][1]):
            assert not bits(t).any()


def well_conditioned_batch(dt, seed, m_in):
    """Ten graphs of 3 to 8 rows, up to four entries a row (the self loop among them), one neighbour value in five masked
    inside otherwise live rows; dense features of order 1."""
    rng = np.random.default_rng(seed)
    sizes = [int(s) for s in rng.integers(3, 9, 10)]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = []
    for a, n in zip(ptr[:-1], sizes):
        for i in range(n):
            cs = sorted(set(rng.choice(n, min(n, 3), replace=False).tolist()) | {i})
            rows.append([(int(a + c), -0.25 if (c != i and rng.random() < 0.2) else float(rng.uniform(0.1, 1.0))) for c in cs])
    x = rng.standard_normal((int(ptr[-1]), m_in))
    return dict(rowptr=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
                col=np.array([c for r in rows for c, _ in r], np.int64),
                val=R._round(np.array([v for r in rows for _, v in r], np.float64), dt), x=R._round(x, dt), graph_ptr=ptr,
                names={}, n_rows=int(ptr[-1]))


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("widths,relus", [((7,), (1,)), ((20, 7), (1, 1)), ((64, 20), (1, 1)), ((20, 64), (0, 1))])
def test_top_layer_grad_attention_where_the_bound_separates(dt, widths, relus):
    """The top layer's grad_attention against float64 on the device's own E and S and the exact g_{L-1}
    (_gat_stack_grad_ref.top_attention_grad_f64): the tolerance counts only the fp32 operations behind S.  On these small
    graphs with scores of order 1 and a ReLU mask that makes g vary within a graph, each half of the gradient is tens to
    hundreds of times the bound, and the same reference with another LeakyReLU slope, with its halves swapped or with its
    sign turned lies outside it -- as a kernel with one of those mistakes would.  Entries masked inside live rows take
    part: they carry S = 0 and must add nothing."""
    relus = [bool(r) for r in relus]
    b = well_conditioned_batch(dt, 1, 7)
    Ws, atts, m = [], [], 7
    for l, P in enumerate(widths):
        W, a = S.plain_layer(dt, m, P, 3 + l)
        Ws.append(W)
        atts.append(a)
        m = P
    c = run(b, dt, Ws, atts, relus, False, max(widths + (7,)), seed=0)
    check(c, dt, Ws, atts, relus)
    top, P = len(widths) - 1, widths[-1]
    nnz = int(b["rowptr"][-1])
    assert (np.asarray(b["val"])[:nnz] < 0).any()
    X = b["x"] if top == 0 else f64(c["outs"][top - 1])
    g = top_layer_g(f64(c["gp"]), b["graph_ptr"], b["n_rows"], f64(c["outs"][top]), relus[top], dt)
    assert (np.ptp(g[:int(b["graph_ptr"][1])], axis=0) > 0).any()             # g varies within graph 0
    adj = (b["rowptr"], b["col"], b["val"])
    E, Sd = f64(c["ES"][top][0]), f64(c["ES"][top][1])
    want, mag, tol = top_attention_grad_f64(adj, X, Ws[top], E, Sd, g, ALPHA)
    bound = tol * mag + 1e-30
    got = f64(c["dA"][top])
    ratio = float((np.abs(got - want) / bound).max())
    print(f"top grad_attention: worst {ratio:.3f} of the bound; |gradient| / bound per half "
          f"{float((np.abs(want[:P]) / bound[:P]).max()):.0f}, {float((np.abs(want[P:]) / bound[P:]).max()):.0f}")
    for half in (slice(0, P), slice(P, 2 * P)):
        assert (np.abs(want[half]) > 3 * bound[half]).any()
    other_slope, _, _ = top_attention_grad_f64(adj, X, Ws[top], E, Sd, g, 0.25)
    for name, wrong in (("alpha 0.25", other_slope), ("halves swapped", np.roll(want, P)), ("sign", -want)):
        assert (np.abs(wrong - want) > 3 * bound).any(), name
    assert ratio <= 1.0, ratio


# ---- 3. grid and ordering ------------------------------------------------------------------------------------------------
def small_graphs(dt, n_graphs, m_in, seed):
    """Graphs of 1 to 2 rows: self loops and, in a 2-row graph, the two edges; one value in six masked."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 3, n_graphs)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = []
    for a, n in zip(ptr[:-1], sizes):
        for i in range(n):
            rows.append([(int(a + c), -0.25 if rng.random() < 1 / 6 else float(rng.uniform(0.1, 1.0))) for c in range(n)])
    x = rng.standard_normal((int(ptr[-1]), m_in)) * 0.5
    x[rng.random(x.shape) < 0.5] = 0.0
    return dict(rowptr=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
                col=np.array([c for r in rows for c, _ in r], np.int64),
                val=R._round(np.array([v for r in rows for _, v in r], np.float64), dt), x=R._round(x, dt), graph_ptr=ptr,
                names={}, n_rows=int(ptr[-1]))


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_more_groups_than_the_grid(dt):
    """Width 252: groups of 16 rows, so 6 000 graphs of 1 to 2 rows make more groups than the 512 workgroups; every
    workgroup adds several groups into its slice.  Two runs give the same bits."""
    b = small_graphs(dt, 6000, 7, 11)
    Ws, atts = [S.plain_layer(dt, 7, 252, 4)[0]], [S.plain_layer(dt, 7, 252, 4)[1]]
    c = run(b, dt, Ws, atts, [True], True, 252, seed=2)
    assert c["plan"].rows == 16 and c["plan"].groups > 512
    check(c, dt, Ws, atts, [True])
    again = c["call"]()
    assert same_bits(again[0][0], c["dW"][0]) and same_bits(again[1][0], c["dA"][0]) and same_bits(again[2][0], c["G"][0])


# ---- 4. edge shapes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_one_row_graph_and_a_graph_of_the_budget(dt):
    budget = S.rows_budget(dt, 64, backward=True)
    rng = np.random.default_rng(8)
    for sizes in ([1], [budget]):
        n = sizes[0]
        dense = (rng.random((n, n)) < 0.2) | np.eye(n, dtype=bool)
        r, cidx = np.nonzero(dense)
        b = dict(rowptr=np.concatenate([[0], np.cumsum(np.bincount(r, minlength=n))]).astype(np.int64), col=cidx.astype(np.int64),
                 val=R._round(rng.uniform(0.1, 1.0, len(r)), dt), x=R._round(rng.standard_normal((n, 7)), dt),
                 graph_ptr=np.array([0, n], np.int64), names={}, n_rows=n)
        Ws, atts = layers_for(dt, 7, (64, 64), (1, 1), 3)
        Ws[0], atts[0] = S.plain_layer(dt, 7, 64, 5)
        c = run(b, dt, Ws, atts, [True, False], True, 64)
        assert c["plan"].max_graph == n
        check(c, dt, Ws, atts, [True, False])


def test_empty_batch_zeroes_every_gradient():
    from sgracex1_amd import ops
    adj = ops.Csr(torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
                  torch.zeros(0, dtype=torch.float16, device=DEV), 0)
    x = torch.zeros((0, 7), dtype=torch.float16, device=DEV)
    ptr = torch.zeros(1, dtype=torch.int32, device=DEV)
    plan = ops.BatchPlan(adj, ptr, 64, BACKWARD)
    w = [torch.randn(7, 64, device=DEV), torch.randn(64, 16, device=DEV)]
    a = [torch.randn(128, device=DEV), None]
    outs = [torch.zeros((0, 64), dtype=torch.float16, device=DEV), torch.zeros((0, 16), dtype=torch.float16, device=DEV)]
    dW, dA = ops.gat_stack_backward(adj, x, w, a, [True, False], ptr, outs, torch.zeros((0, 16), device=DEV), plan=plan)
    assert not dW[0].any() and not dW[1].any() and not dA[0].any() and dA[1] is None
    assert dW[0].shape == (7, 64) and dA[0].shape == (128,)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------
def _status(fn):
    from sgracex1_amd import _lib
    with pytest.raises(_lib.SgxError) as e:
        fn()
    return e.value.status


def test_unsupported_batches_are_refused_by_the_c_call():
    from sgracex1_amd import ops
    dt = "f16"
    budget = S.rows_budget(dt, 64, backward=True)
    assert S.rows_budget(dt, 64) > budget
    n = budget + 1                                           # within the forward's budget, over the backward's
    b = dict(rowptr=np.arange(n + 1, dtype=np.int64), col=np.arange(n, dtype=np.int64), val=np.full(n, 0.5),
             x=R._round(np.random.default_rng(0).standard_normal((n, 7)), dt), graph_ptr=np.array([0, n], np.int64), names={},
             n_rows=n)
    adj, x, ptr = on_device(b, dt, True)
    w = [torch.randn(7, 64, device=DEV), torch.randn(64, 64, device=DEV)]
    a = [torch.randn(128, device=DEV), torch.randn(128, device=DEV)]
    outs = [torch.zeros((n, 64), dtype=torch.float16, device=DEV)] * 2
    gp = torch.randn(1, 64, device=DEV)
    plan = ops.BatchPlan(adj, ptr, 64, BACKWARD)
    assert not plan.fits
    assert _status(lambda: ops.gat_stack_backward(adj, x, w, a, [True, False], ptr, outs, gp, plan=plan)) == -3
    fplan = ops.BatchPlan(adj, ptr, 64)                      # a forward-kind plan (which fits)
    assert fplan.fits
    assert _status(lambda: ops.gat_stack_backward(adj, x, w, a, [True, False], ptr, outs, gp, plan=fplan)) == -3


# ---- 6. the model ------------------------------------------------------------------------------------------------------------
def _mutag(n=None):
    from sgracex1_amd import pyg_lite as G
    raw = np.load(os.path.join(GOLD, "mutag_raw.npz"))
    graphs = G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])
    return G.collate(graphs[:n] if n else graphs).to(DEV)


@pytest.fixture
def sgrace_env():
    from sgracex1_amd import config, sgrace
    saved = config.snapshot()
    config.acc, config.float_type, config.compute_attention = 1, np.float32, 1
    ip = sgrace.init_SGRACE()
    ip.register_map.layer_count = 2
    yield ip, config, sgrace
    config.restore(saved)
    sgrace.init_SGRACE()


def _count(monkeypatch):
    from sgracex1_amd import ops
    calls = {"fwd": 0, "bwd": 0, "gp": []}
    real_f, real_b = ops.gat_stack_forward, ops.gat_stack_backward

    def f(*a, **k):
        calls["fwd"] += 1
        return real_f(*a, **k)

    def b(*a, **k):
        calls["bwd"] += 1
        calls["gp"].append(a[7].detach().clone())                    # grad_pooled
        return real_b(*a, **k)
    monkeypatch.setattr(ops, "gat_stack_forward", f)
    monkeypatch.setattr(ops, "gat_stack_backward", b)
    return calls


def _step(model, b, weight=None):
    model.zero_grad(set_to_none=True)
    out = model(b.x, b.edge_index, b.batch)
    loss = torch.nn.functional.cross_entropy(out, b.y) if weight is None else (out * weight).sum()
    loss.backward()
    return loss


def test_model_declines_the_route(sgrace_env, monkeypatch):
    ip, config, sgrace = sgrace_env
    from sgracex1_amd import ops
    b = _mutag(48)
    calls = _count(monkeypatch)
    torch.manual_seed(7)
    model = sgrace.GAT_POOL_PYNQ(7, 64, 2, train_stack=True).to(DEV).train()
    n_graphs = int(b.batch.max()) + 1
    # an unsorted batch
    _step(model, _Batch(b.x, b.edge_index, (n_graphs - 1) - b.batch, b.y))
    # layer_count = 1
    ip.register_map.layer_count = 1
    _step(model, b)
    ip.register_map.layer_count = 2
    # a dead row: the adjacency handed in as a Csr whose row 0 has no positive value
    ei, norm = sgrace.sym_norm2(b.edge_index, b.num_nodes)
    adj = sgrace._edge_csr(None, ei, norm, b.num_nodes, torch.float32)
    val = adj.val.clone()
    val[int(adj.rowptr[0]):int(adj.rowptr[1])] = -1.0
    dead = ops.Csr(adj.rowptr, adj.col, val, adj.n_cols)
    assert dead.has_dead_rows
    assert model._train_stack(b.x, dead, b.batch) is None
    assert model._train_stack(b.x, adj, b.batch) is not None and calls["fwd"] == 1
    calls["fwd"] = 0
    # a quantiser
    config.fake_quantization, config.w_qbits = 1, 8
    sgrace.init_SGRACE().register_map.layer_count = 2
    _step(model, b)
    config.fake_quantization = 0
    sgrace.init_SGRACE().register_map.layer_count = 2
    # train_stack off
    model.train_stack = False
    _step(model, b)
    assert (calls["fwd"], calls["bwd"]) == (0, 0)
    model.train_stack = True
    for k in range(1, 3):
        _step(model, b)
        assert (calls["fwd"], calls["bwd"]) == (k, k)
    config.compute_attention = 0                                     # two GCN layers in the same two calls
    _step(model, b)
    assert (calls["fwd"], calls["bwd"]) == (3, 3)
    assert model.att1.weight.grad is not None and model.att1.attention.grad is None


class _Batch:
    def __init__(self, x, edge_index, batch, y):
        self.x, self.edge_index, self.batch, self.y = x, edge_index, batch, y


def test_model_step_agrees_with_the_layer_by_layer_step(sgrace_env, monkeypatch):
    """One MUTAG step with a fixed gradient on the logits (eval mode: no dropout): the parameter gradients of the
    train_stack step and of the layer-by-layer step on the same weights both lie inside the restatement's bound around
    the float64 value.  (Equal bits are not expected: the fused backward forms E and S again in fp32.)"""
    ip, config, sgrace = sgrace_env
    from sgracex1_amd import ops
    b = _mutag()
    calls = _count(monkeypatch)
    torch.manual_seed(7)
    ref_model = sgrace.GAT_POOL_PYNQ(7, 64, 2).to(DEV).eval()
    fused = sgrace.GAT_POOL_PYNQ(7, 64, 2, train_stack=True).to(DEV).eval()
    fused.load_state_dict(ref_model.state_dict())
    n_graphs = int(b.batch.max()) + 1
    weight = torch.randn(n_graphs, 2, device=DEV)
    _step(ref_model, b, weight)
    assert (calls["fwd"], calls["bwd"]) == (0, 0)
    _step(fused, b, weight)
    assert (calls["fwd"], calls["bwd"]) == (1, 1)
    ei, norm = sgrace.sym_norm2(b.edge_index, b.num_nodes)
    adj = sgrace._edge_csr(None, ei, norm, b.num_nodes, torch.float32)
    ptr = ops.graph_ptr_of(b.batch)
    layers = (ref_model.att1, ref_model.att2)
    Ws = [f64(c.weight) for c in layers]
    atts = [f64(c.attention).reshape(-1) for c in layers]
    fea = ops.Csr.from_dense(b.x.float(), torch.float32)
    _, outs = ops.gat_stack_forward(adj, fea, [c.weight.detach().t().contiguous() for c in layers],
                                    [c.attention.detach().reshape(-1).contiguous() for c in layers], [True, False], ptr,
                                    alpha=ALPHA, want_layer_outputs=True)
    ref = gat_stack_grad_f64((adj.rowptr.cpu().numpy(), adj.col.cpu().numpy(), f64(adj.val)[:adj.nnz]), f64(b.x), Ws, atts,
                             [True, False], ptr.cpu().numpy(), f64(calls["gp"][0]), [f64(D) for D in outs], alpha=ALPHA)
    # What the bound says here.  For grad_W it separates: no gradient at all lies outside it on both layers, and so does
    # layer 0's gradient under a uniform softmax (the attention vectors zeroed; layer 1's does not depend on S, its g
    # being constant within a graph and S's rows summing to 1).  For grad_attention it is a worst-case bound on sums
    # that cancel (the softmax backward's row sums are 0 before the slope) over 3371 rows, and on this batch the
    # gradient itself is within it; tests/test_gat_stack_train_cpu.py shows it separate on a 12-graph batch.
    uniform = gat_stack_grad_f64((adj.rowptr.cpu().numpy(), adj.col.cpu().numpy(), f64(adj.val)[:adj.nnz]), f64(b.x), Ws,
                                 [np.zeros_like(a) for a in atts], [True, False], ptr.cpu().numpy(), f64(calls["gp"][0]),
                                 [f64(D) for D in outs], alpha=ALPHA)
    for l in range(2):
        assert (np.abs(ref["dW"][l]) > ref["tW"][l] * ref["mW"][l] + 1e-30).any(), l
    assert (np.abs(uniform["dW"][0] - ref["dW"][0]) > ref["tW"][0] * ref["mW"][0] + 1e-30).any()
    for name, model in (("layer by layer", ref_model), ("train_stack", fused)):
        for l, c in enumerate((model.att1, model.att2)):
            ok, ratio = within(f64(c.weight.grad), ref["dW"][l], ref["mW"][l], ref["tW"][l])
            print(f"{name} dW_{l}: worst {ratio:.3f} of the bound")
            assert ok, (name, l, "dW", ratio)
            assert c.attention.grad.shape == c.attention.shape
            ok, ratio = within(f64(c.attention.grad).reshape(-1), ref["dA"][l], ref["mA"][l], ref["tA"][l])
            print(f"{name} grad_attention_{l}: worst {ratio:.3f} of the bound")
            assert ok, (name, l, "grad_attention", ratio)
    assert same_bits(ref_model.lin.bias.grad, fused.lin.bias.grad)


def test_features_that_need_a_gradient_are_refused(sgrace_env):
    from sgracex1_amd import ops
    dt = "f32"
    b = S.build_batch(dt, S.rows_budget(dt, 64, backward=True), 7, seed=2)
    adj, x, ptr = on_device(b, dt, False)
    plan = ops.BatchPlan(adj, ptr, 64, BACKWARD)
    w, a = torch.randn(7, 64, device=DEV, requires_grad=True), torch.randn(128, 1, device=DEV, requires_grad=True)
    with pytest.raises(ValueError):
        ops.GatStack.apply(adj, x.clone().requires_grad_(True), ptr, plan, (False,), ALPHA, w, a)


def test_captured_step_replays_to_the_eager_bits():
    from sgracex1_amd import ops
    dt = "f16"
    b = S.build_batch(dt, S.rows_budget(dt, 64, backward=True), 7, seed=2)
    adj, x, ptr = on_device(b, dt, True)
    plan = ops.BatchPlan(adj, ptr, 64, BACKWARD)
    Ws, atts = layers_for(dt, 7, (64, 64), (1, 1), 2)
    params = [torch.tensor(W, device=DEV, dtype=torch.float32, requires_grad=True) for W in Ws] + \
        [torch.tensor(a, device=DEV, dtype=torch.float32).reshape(-1, 1).requires_grad_(True) for a in atts]
    gp = torch.randn(len(b["graph_ptr"]) - 1, 64, device=DEV)

    def step():
        for p in params:
            p.grad = None
        pooled = ops.GatStack.apply(adj, x, ptr, plan, (True, False), ALPHA, *params)
        pooled.backward(gp)
        return [pooled.detach()] + [p.grad for p in params]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            eager = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(s)
    for p in params:
        p.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert all(same_bits(a, e) for a, e in zip(out, eager))
    assert all(t.shape == p.shape for t, p in zip(eager[1:], params)) and eager[3].abs().max() > 0


def test_twenty_epochs_on_mutag(sgrace_env, monkeypatch):
    """examples/molecule_gcn_train.py --model gat --layer-count 2 --train-stack, inline, against the layer-by-layer run
    from the same seed: the training loss falls, the test accuracies lie within 0.03 of each other."""
    ip, config, sgrace = sgrace_env
    from sgracex1_amd import pyg_lite as G
    raw = np.load(os.path.join(GOLD, "mutag_raw.npz"))
    graphs = G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])
    torch.manual_seed(12345)
    graphs = [graphs[i] for i in torch.randperm(len(graphs)).tolist()]
    train, test = G.collate(graphs[:2000]).to(DEV), G.collate(graphs[50:100]).to(DEV)
    calls = _count(monkeypatch)

    def fit(train_stack):
        torch.manual_seed(12345)
        model = sgrace.GAT_POOL_PYNQ(7, 64, 2, train_stack=train_stack).to(DEV)
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
        losses = []
        for _ in range(20):
            model.train()
            opt.zero_grad()
            loss = torch.nn.functional.cross_entropy(model(train.x, train.edge_index, train.batch), train.y)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        model.eval()
        with torch.no_grad():
            pred = model(test.x, test.edge_index, test.batch).argmax(1)
        return losses, float((pred == test.y).float().mean())

    base_losses, base_acc = fit(False)
    assert calls["bwd"] == 0
    losses, acc = fit(True)
    assert calls["bwd"] == 20
    print(f"layer by layer: loss {base_losses[0]:.4f} -> {base_losses[-1]:.4f}, test accuracy {base_acc:.2f}; "
          f"train_stack: loss {losses[0]:.4f} -> {losses[-1]:.4f}, test accuracy {acc:.2f}")
    assert losses[-1] < losses[0]
    assert abs(acc - base_acc) <= 0.03, (acc, base_acc)

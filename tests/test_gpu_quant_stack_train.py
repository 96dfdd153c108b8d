"""sgx_quant_stack_backward on the GPU (include/sgx.h, "training the quantised stack"): descriptors without a quantiser
against sgx_gat_stack_backward and all-GCN quantised ones against sgx_stack_backward (bit for bit); quantised GAT layers
-- E, S, G, grad_W and grad_attention -- inside the derived bound of the float64 restatement
(tests/_quant_stack_grad_ref.py) on the device's own layer outputs, on test_gpu_quant_stack.py's batch of mask, grid and
clip edge cases with build_batch's masked rows put back; the adjacency quantised in flight or beforehand; the grid; edge
shapes; a captured step; refusals; GAT_POOL_PYNQ(train_stack=True) under fake quantisation; ten epochs on MUTAG."""
import numpy as np
import pytest
import torch

import _gat_ref as R
import _gat_stack_ref as S
import _quant_ref as Q
import _quant_stack_ref as QS
from _quant_stack_grad_ref import quant_stack_grad_f64, within
from _stack_grad_ref import stack_grad_bound, stack_grad_f64
from test_gpu_quant_stack import (_bipartite, _mutag_batch, bits_of, build_case, constants, f32,  # noqa: F401
                                  quant_model, same_bits)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
I32 = dict(dtype=torch.int32, device=DEV)
ALPHA = 0.2
BACKWARD = 1
U = 2.0 ** -24


def f64(t):
    return t.detach().double().cpu().numpy()


def grad_case(nbits, m_in, widths, gat, sparse, seed, quant_on=None, **batch):
    """test_gpu_quant_stack.build_case on the BACKWARD plan's row budget, with build_batch's masked values put back:
    graph 0 keeps its row without an entry (0), its row masked by +0.0, a negative subnormal, -0.0 and -0.25 (1) and its
    masked entries inside live rows; row 9 loses every entry to the quantiser, row 10 keeps live ones beside one that
    quantises to 0.  quant_on[l] = False takes layer l's quantiser away."""
    from sgracex1_amd import ops
    width = max(list(widths) + ([] if sparse else [m_in]))
    budget = S.rows_budget("f32", width, backward=True)
    c = build_case(nbits, m_in, widths, gat, sparse, seed, budget=budget, **batch)
    b = c["b"]
    nnz = len(b["col"])
    masked = np.asarray(b["val"])[:nnz] <= 0
    val = c["a_val"].copy()
    val[masked] = np.asarray(b["val"], np.float32)[:nnz][masked]
    rp = b["rowptr"]
    val[rp[c["killed"]]:rp[c["killed"] + 1]] = np.float32(0.3 * c["qs"][0].a_s)
    val[rp[c["mixed"]]:rp[c["mixed"] + 1]] = np.float32(0.9)
    val[rp[c["mixed"]]] = np.float32(0.3 * c["qs"][0].a_s)
    assert (val[rp[1]:rp[2]] <= 0).all() and rp[1] == rp[0] and np.signbit(val[rp[1]:rp[2]]).any() and (val[rp[1]:rp[2]] == 0).any()
    c["a_val"] = val
    c["adj"] = ops.Csr(torch.tensor(rp, **I32), torch.tensor(b["col"], **I32), torch.tensor(val, device=DEV), b["n_rows"])
    if quant_on is not None:
        c["qs"] = [q if on else None for q, on in zip(c["qs"], quant_on)]
    c["width"], c["budget"] = width, budget
    c["plan"] = ops.BatchPlan(c["adj"], c["ptr"], width, BACKWARD)
    assert c["plan"].fits and c["plan"].rows == budget
    c["w32"] = [torch.tensor(W, device=DEV, dtype=torch.float32) for W in c["Ws"]]
    c["a32"] = [None if a is None else torch.tensor(a, device=DEV, dtype=torch.float32) for a in c["atts"]]
    rng = np.random.default_rng(seed + 5)
    c["gp"] = torch.tensor(rng.standard_normal((len(b["graph_ptr"]) - 1, widths[-1])), device=DEV, dtype=torch.float32)
    return c


def run(c, relus, pre_quantised=True):
    """The quantised forward (for the D_l the backward reads) and the backward; pre_quantised: both mask / aggregate with
    adj.quantized(qc) as stored (SGX_QUANT_ADJ_DONE), else the adjacency is quantised as it is read."""
    from sgracex1_amd import ops
    q0 = next((q for q in c["qs"] if q is not None), None)
    adj_q = c["adj"].quantized(q0) if (pre_quantised and q0 is not None) else None
    _, outs = ops.quant_stack_forward(c["adj"] if adj_q is None else adj_q, c["fea"], c["wts"], c["atts_d"], relus, c["ptr"],
                                      c["qs"], alpha=ALPHA, plan=c["plan"], adj_quantised=adj_q is not None,
                                      want_layer_outputs=True)
    call = lambda: ops.quant_stack_backward(c["adj"], c["fea"], c["w32"], c["a32"], relus, c["ptr"], outs, c["gp"], c["qs"],
                                            alpha=ALPHA, plan=c["plan"], adj_q=adj_q, want_G=True, want_edge_outputs=True)
    dW, dA, G, ES = call()
    return dict(outs=outs, dW=dW, dA=dA, G=G, ES=ES, call=call, adj_q=adj_q)


def flat(r):
    return list(r["dW"]) + [g for g in r["dA"] if g is not None] + list(r["G"]) + [t for es in r["ES"] if es is not None for t in es]


def check(c, r, relus, figures=None):
    """Per layer E, S, G, grad_W and grad_attention against the restatement on the device's own D_l; H_q exact (asserted in
    the restatement); masked entries and rows without a live entry exactly 0."""
    from sgracex1_amd import ops
    b = c["b"]
    nnz = int(b["rowptr"][-1])
    rowptr = np.asarray(b["rowptr"], np.int64)
    E_dev = [None if es is None else f64(es[0]) for es in r["ES"]]
    ref = quant_stack_grad_f64((b["rowptr"], b["col"], c["a_val"]), c["x"], c["Ws"], c["atts"], relus, b["graph_ptr"],
                               f64(c["gp"]), [f64(D) for D in r["outs"]], c["qs"], alpha=ALPHA, E_dev=E_dev)
    row = R.rows_of(rowptr)
    worst = {}
    X_dev, X_host = c["fea"], c["fea_host"]
    for l in range(len(c["Ws"])):
        q = c["qs"][l]
        if c["atts"][l] is not None:
            E, Sd = f64(r["ES"][l][0])[:nnz], f64(r["ES"][l][1])[:nnz]
            R.check(f"E_{l}", E, ref["E"][l], ref["bE"][l], row, b["names"])
            R.check(f"S_{l}", Sd, ref["S"][l], ref["bS"][l], row, b["names"])
            aq = Q.quantise_adj(c["a_val"], q) if q is not None else c["a_val"]
            live = aq[:nnz] > 0
            assert not bits_of(r["ES"][l][1][:nnz])[torch.tensor(~live, device=DEV)].any(), f"S_{l} on masked entries"
            dead = ref["dead"][l]
            assert dead[0] and dead[1] and (q is None or dead[c["killed"]]) and not dead[c["mixed"]]
            assert not bits_of(r["G"][l])[torch.tensor(dead, device=DEV)].any(), f"G_{l} on rows without a live entry"
            if q is not None:
                # _quant_stack_ref.layer_ref's E and S on the same input, and sgx_layer_forward's own side outputs
                lr = QS.layer_ref((b["rowptr"], b["col"]), c["a_val"], X_host, c["Ws"][l], c["atts"][l], q, relus[l], alpha=ALPHA)
                assert lr["magnitude"] < Q.EXACT_BELOW
                att_q, _ = Q.quantise(np.asarray(c["atts"][l], np.float32), 1, q)
                _D, _bD, g = Q.stage2_gat((b["rowptr"], b["col"]), lr["aq"], lr["H"], att_q, q, relus[l], "zero", alpha=ALPHA)
                R.check(f"E_{l} (layer_ref)", E, g["E"], g["bE"], row, b["names"])
                R.check(f"S_{l} (layer_ref)", Sd, g["S"], g["bS"], row, b["names"])
                _, E_l, S_l = ops.layer_forward(c["adj"], X_dev, c["wts"][l], relu=relus[l], gat_attention=c["atts_d"][l], alpha=ALPHA,
                                                want_edge_outputs=True, quant=q)
                lv = live & ~dead[row]                                       # (the layer gives a dead row the mean of all rows)
                assert (np.abs(E - f64(E_l)[:nnz])[lv] <= 2 * g["bE"][lv] + 1e-30).all(), f"E_{l} against sgx_layer_forward"
                assert (np.abs(Sd - f64(S_l)[:nnz])[lv] <= 2 * g["bS"][lv] + 1e-30).all(), f"S_{l} against sgx_layer_forward"
            ok, worst[f"dA_{l}"] = within(f64(r["dA"][l]), ref["dA"][l], ref["mA"][l], ref["tA"][l])
            print(f"grad_attention_{l}: worst {worst[f'dA_{l}']:.3f} of the bound")
            assert ok, (l, "grad_attention", worst[f"dA_{l}"])
        else:
            assert r["dA"][l] is None and r["ES"][l] is None
        for name, got, key in (("G", r["G"][l], "G"), ("dW", r["dW"][l], "W")):
            ok, worst[f"{name}_{l}"] = within(f64(got), ref["G" if key == "G" else "dW"][l], ref["m" + key][l], ref["t" + key][l])
            print(f"{name}_{l}: worst {worst[f'{name}_{l}']:.3f} of the bound")
            assert ok, (l, name, worst[f"{name}_{l}"])
        X_dev, X_host = r["outs"][l], f32(r["outs"][l])
    if figures is not None:
        figures.update(worst)
    return ref


# ---- 1. no quantiser: sgx_gat_stack_backward bit for bit --------------------------------------------------------------------
@pytest.mark.parametrize("m_in,widths,gat,sparse", [(7, (64, 64), (1, 1), True), (18, (65, 7, 20), (0, 1, 1), False),
                                                    (7, (252,), (1,), True)])
def test_null_quantisers_are_sgx_gat_stack_backward(m_in, widths, gat, sparse):
    from sgracex1_amd import ops
    relus = [True, False, True][:len(widths)]
    c = grad_case(8, m_in, widths, gat, sparse, 1, quant_on=[False] * len(widths))
    r = run(c, relus)
    want = ops.gat_stack_backward(c["adj"], c["fea"], c["w32"], c["a32"], relus, c["ptr"], r["outs"], c["gp"], alpha=ALPHA,
                                  plan=c["plan"], want_G=True, want_edge_outputs=True)
    for a, b in zip(flat(r), flat(dict(dW=want[0], dA=want[1], G=want[2], ES=want[3]))):
        assert same_bits(a, b)
    assert any(g is not None and g.abs().max() > 0 for g in r["dA"])


# ---- 2. all-GCN quantised descriptors: sgx_stack_backward on the same D_l ----------------------------------------------------
@pytest.mark.parametrize("nbits,m_in,widths,sparse", [(8, 7, (64, 64), True), (4, 18, (65, 1, 64), False), (1, 64, (7,), False)])
def test_quantised_gcn_layers_are_sgx_stack_backward(nbits, m_in, widths, sparse):
    from sgracex1_amd import ops
    relus = [True, False, True][:len(widths)]
    c = grad_case(nbits, m_in, widths, [0] * len(widths), sparse, 2)
    r = run(c, relus)
    dW, G = ops.gcn_stack_backward(c["adj"], c["fea"], c["w32"], relus, c["ptr"], r["outs"], c["gp"], plan=c["plan"], want_G=True)
    b = c["b"]
    adj_np = (b["rowptr"], b["col"], c["a_val"].astype(np.float64))
    outs_np = [f64(D) for D in r["outs"]]
    ref, _ = stack_grad_f64(adj_np, c["x"].astype(np.float64), c["Ws"], relus, b["graph_ptr"], f64(c["gp"]), outs=outs_np)
    bounds = stack_grad_bound(adj_np, c["x"].astype(np.float64), c["Ws"], b["graph_ptr"], f64(c["gp"]), outs_np, U)
    for l in range(len(widths)):
        assert same_bits(r["G"][l], G[l]), f"G_{l}"
        assert r["dA"][l] is None
        err = np.abs(f64(r["dW"][l]) - ref[l])
        assert (err <= bounds[l]).all(), f"dW_{l}: {float((err / bounds[l]).max())}"


# ---- 3. quantised GAT layers against the restatement --------------------------------------------------------------------------
CASES = [  # bits, K of layer 0, widths, gat_mode per layer, quantiser per layer, relu per layer, sparse layer 0
    (8, 7, (64,), (1,), (1,), (1,), True),
    (8, 18, (1,), (1,), (1,), (0,), False),
    (8, 7, (64, 64), (1, 1), (1, 1), (1, 0), True),
    (4, 64, (7, 20), (1, 0), (1, 1), (1, 1), False),
    (4, 7, (65, 20, 7), (0, 1, 1), (1, 1, 0), (1, 0, 1), True),
    (2, 18, (20, 64), (1, 1), (0, 1), (0, 0), False),
    (2, 7, (20, 64, 7, 1), (1, 0, 1, 1), (1, 1, 1, 1), (1, 1, 0, 0), False),
    (1, 64, (64, 7), (1, 1), (1, 1), (1, 0), False),
    (1, 7, (65,), (1,), (1,), (1,), True),
    (8, 7, (252, 64), (1, 1), (1, 1), (1, 0), True),                  # the budget is 16 rows
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_quantised_gat_layers_against_the_restatement(case):
    nbits, m_in, widths, gat, qon, relus, sparse = CASES[case]
    relus = [bool(v) for v in relus]
    c = grad_case(nbits, m_in, widths, gat, sparse, case, quant_on=[bool(v) for v in qon])
    if 252 in widths:
        assert c["budget"] == 16
    assert c["plan"].max_graph == c["budget"] and c["plan"].groups >= 3
    sizes = c["b"]["sizes"]
    assert 1 in sizes and 0 in sizes and max(sizes) == c["budget"]            # a 1-row graph, an empty one, a budget-sized one
    r = run(c, relus)
    fig = {}
    check(c, r, relus, fig)
    print("worst error over the bound:", {k: round(v, 3) for k, v in fig.items()})
    again = r["call"]()
    for a, b in zip(flat(r), flat(dict(dW=again[0], dA=again[1], G=again[2], ES=again[3]))):
        assert same_bits(a, b)


@pytest.mark.parametrize("nbits", [8, 2])
def test_small_graphs_where_the_bound_separates_the_mutants(nbits):
    """test_quant_stack_train_cpu.py's batch -- ten graphs of 3 to 8 rows, scores of order 1, features on and above the
    grid, an entry that quantises to 0 in a live row -- on the device: the gradients lie inside the derived tolerance, and
    on the device's own D_l each of the restatement's three mutants (scores from the unquantised Wh, d_e from H_q, the mask
    on the unquantised adjacency) lies outside it, as a kernel with that mistake would."""
    from sgracex1_amd import ops, quant
    from test_quant_stack_train_cpu import separating_batch, separating_layers
    qc = quant.constants(nbits)
    b = separating_batch(qc, 1, 7)
    Ws, atts = separating_layers(qc, 7, (20, 7), 3)
    relus = [True, False]
    val = b["val"].astype(np.float32)
    x = b["x"].astype(np.float32)
    adj = ops.Csr(torch.tensor(b["rowptr"], **I32), torch.tensor(b["col"], **I32), torch.tensor(val, device=DEV), b["n_rows"])
    ptr = torch.tensor(b["graph_ptr"], **I32)
    c = dict(adj=adj, fea=torch.tensor(x, device=DEV), ptr=ptr, qs=[qc, qc], plan=ops.BatchPlan(adj, ptr, 20, BACKWARD),
             wts=[torch.tensor(W.T.copy(), device=DEV, dtype=torch.float32) for W in Ws],
             atts_d=[torch.tensor(a, device=DEV, dtype=torch.float32) for a in atts],
             w32=[torch.tensor(W, device=DEV, dtype=torch.float32) for W in Ws],
             a32=[torch.tensor(a, device=DEV, dtype=torch.float32) for a in atts],
             gp=torch.tensor(np.random.default_rng(5).standard_normal((len(b["graph_ptr"]) - 1, 7)), device=DEV, dtype=torch.float32))
    r = run(c, relus)
    args = ((b["rowptr"], b["col"], b["val"]), b["x"], Ws, atts, relus, b["graph_ptr"], f64(c["gp"]), [f64(D) for D in r["outs"]],
            [qc, qc])
    E_dev = [f64(es[0]) for es in r["ES"]]
    ref = quant_stack_grad_f64(*args, E_dev=E_dev)
    for l in range(2):
        for name, got, key, m, t in (("grad_attention", r["dA"][l], "dA", "mA", "tA"), ("dW", r["dW"][l], "dW", "mW", "tW"),
                                     ("G", r["G"][l], "G", "mG", "tG")):
            ok, ratio = within(f64(got), ref[key][l], ref[m][l], ref[t][l])
            print(f"{name}_{l}: worst {ratio:.3f} of the bound")
            assert ok, (l, name, ratio)
    for mutant in ("scores_unquantised_wh", "d_from_hq", "mask_unquantised"):
        bad = quant_stack_grad_f64(*args, E_dev=None if mutant == "scores_unquantised_wh" else E_dev, mutant=mutant)
        worst = max(float((np.abs(bad[key][l] - ref[key][l]) / (ref[t][l] * ref[m][l] + 1e-30)).max())
                    for l in range(2) for key, m, t in (("dA", "mA", "tA"), ("dW", "mW", "tW")))
        print(f"mutant {mutant}: {worst:.1f} times the bound")
        assert worst > 2.0, mutant                                           # (so the device, inside 1.0, is told from it)


@pytest.mark.parametrize("nbits", [8, 4, 2, 1])
def test_adjacency_quantised_in_flight_and_beforehand(nbits):
    c = grad_case(nbits, 7, (64, 20), (1, 1), True, 3)
    before, inflight = run(c, [True, False], True), run(c, [True, False], False)
    assert before["adj_q"] is not None and inflight["adj_q"] is None
    for a, b in zip(before["outs"] + flat(before), inflight["outs"] + flat(inflight)):
        assert same_bits(a, b)
    aq = Q.quantise_adj(c["a_val"], c["qs"][0])
    assert ((aq == 0) & (c["a_val"] > 0)).any() and np.array_equal(f32(before["adj_q"].val)[:len(aq)], aq)


# ---- 4. the grid -------------------------------------------------------------------------------------------------------------
def test_more_groups_than_the_grid():
    """Width 252: groups of 16 rows, so 6 000 graphs of 1 to 2 rows make more groups than the 512 workgroups."""
    from sgracex1_amd import ops, quant
    qc = quant.constants(8)
    rng = np.random.default_rng(11)
    sizes = rng.integers(1, 3, 6000)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = []
    for a, n in zip(ptr[:-1], sizes):
        for i in range(n):
            rows.append([(int(a + k), 0.3 * qc.a_s if (k != i and rng.random() < 1 / 6) else float(rng.uniform(0.1, 1.0)))
                         for k in range(n)])
    N = int(ptr[-1])
    b = dict(rowptr=np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
             col=np.array([k for r in rows for k, _ in r], np.int64), graph_ptr=ptr, names={}, n_rows=N, sizes=list(sizes))
    val = np.array([v for r in rows for _, v in r], np.float32)
    x = Q.features(N, 7, qc, 4, dense=True)
    W, att = Q.weights(7, 252, qc, 4), Q.attention(252, qc, 4)
    adj = ops.Csr(torch.tensor(b["rowptr"], **I32), torch.tensor(b["col"], **I32), torch.tensor(val, device=DEV), N)
    ptr_d = torch.tensor(ptr, **I32)
    plan = ops.BatchPlan(adj, ptr_d, 252, BACKWARD)
    assert plan.rows == 16 and plan.groups > 512 and plan.fits
    fea = ops.Csr.from_dense(torch.tensor(x, device=DEV), torch.float32)
    c = dict(b=b, a_val=val, x=x, Ws=[W], atts=[att], qs=[qc], adj=adj, fea=fea, ptr=ptr_d, plan=plan,
             wts=[torch.tensor(W.T.copy(), device=DEV)], atts_d=[torch.tensor(att, device=DEV)],
             w32=[torch.tensor(W, device=DEV)], a32=[torch.tensor(att, device=DEV)],
             gp=torch.tensor(rng.standard_normal((6000, 252)), device=DEV, dtype=torch.float32), killed=0, mixed=0)
    r = run(c, [True])
    nnz = len(val)
    ref = quant_stack_grad_f64((b["rowptr"], b["col"], val), x, [W], [att], [True], ptr, f64(c["gp"]), [f64(r["outs"][0])], [qc],
                               alpha=ALPHA, E_dev=[f64(r["ES"][0][0])])
    row = R.rows_of(b["rowptr"])
    R.check("S", f64(r["ES"][0][1])[:nnz], ref["S"][0], ref["bS"][0], row, {})
    for name, got, key in (("G", r["G"][0], "G"), ("dW", r["dW"][0], "W"), ("dA", r["dA"][0], "A")):
        ok, ratio = within(f64(got), ref[{"G": "G", "W": "dW", "A": "dA"}[key]][0], ref["m" + key][0], ref["t" + key][0])
        print(f"{name}: worst {ratio:.3f} of the bound")
        assert ok, (name, ratio)
    again = r["call"]()
    assert same_bits(again[0][0], r["dW"][0]) and same_bits(again[1][0], r["dA"][0]) and same_bits(again[2][0], r["G"][0])


# ---- 5. edge shapes ----------------------------------------------------------------------------------------------------------
def test_empty_batch_zeroes_every_gradient():
    from sgracex1_amd import ops, quant
    qc = quant.constants(8)
    adj = ops.Csr(torch.zeros(1, **I32), torch.zeros(0, **I32), torch.zeros(0, dtype=torch.float32, device=DEV), 0)
    x = torch.zeros((0, 7), dtype=torch.float32, device=DEV)
    ptr = torch.zeros(1, **I32)
    plan = ops.BatchPlan(adj, ptr, 64, BACKWARD)
    w = [torch.randn(7, 64, device=DEV), torch.randn(64, 16, device=DEV)]
    a = [torch.randn(128, device=DEV), None]
    outs = [torch.zeros((0, 64), device=DEV), torch.zeros((0, 16), device=DEV)]
    for adj_q in (None, adj):
        dW, dA = ops.quant_stack_backward(adj, x, w, a, [True, False], ptr, outs, torch.zeros((0, 16), device=DEV),
                                          [qc, qc.second_layer()], plan=plan, adj_q=adj_q)
        assert not dW[0].any() and not dW[1].any() and not dA[0].any() and dA[1] is None
        assert dW[0].shape == (7, 64) and dA[0].shape == (128,)


# ---- 6. a captured step --------------------------------------------------------------------------------------------------------
def test_captured_step_replays_to_the_eager_bits():
    from sgracex1_amd import ops
    c = grad_case(8, 7, (64, 64), (1, 1), True, 2)
    adj_q = c["adj"].quantized(c["qs"][0])
    params = [w.clone().requires_grad_(True) for w in c["w32"]] + [a.clone().reshape(-1, 1).requires_grad_(True) for a in c["a32"]]
    gp = c["gp"]

    def step():
        for p in params:
            p.grad = None
        pooled = ops.QuantStack.apply(c["adj"], adj_q, c["fea"], c["ptr"], c["plan"], (True, False), ALPHA, tuple(c["qs"]), *params)
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
    g.replay()
    torch.cuda.synchronize()
    assert all(same_bits(a, e) for a, e in zip(out, eager))
    assert all(t.shape == p.shape for t, p in zip(eager[1:], params)) and eager[3].abs().max() > 0
    with pytest.raises(ValueError):                                          # no gradient for the features
        ops.QuantStack.apply(c["adj"], adj_q, torch.tensor(c["x"], device=DEV).requires_grad_(True), c["ptr"], c["plan"],
                             (True, False), ALPHA, tuple(c["qs"]), *params)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def _status(fn):
    from sgracex1_amd import _lib
    with pytest.raises(_lib.SgxError) as e:
        fn()
    return e.value.status


def test_refusals_of_the_c_call():
    from sgracex1_amd import ops, quant
    qc = quant.constants(8)
    c = grad_case(8, 7, (64, 64), (1, 1), True, 4)
    r = run(c, [True, False])
    fplan = ops.BatchPlan(c["adj"], c["ptr"], 64)                            # a forward-kind plan (which fits)
    assert fplan.fits
    assert _status(lambda: ops.quant_stack_backward(c["adj"], c["fea"], c["w32"], c["a32"], [True, False], c["ptr"], r["outs"],
                                                    c["gp"], c["qs"], alpha=ALPHA, plan=fplan)) == -3
    # fp16 with a quantiser
    adj16 = ops.Csr(c["adj"].rowptr, c["adj"].col, c["adj"].val.half(), c["adj"].n_rows)
    x16 = torch.tensor(c["x"], device=DEV).half()
    plan16 = ops.BatchPlan(adj16, c["ptr"], 64, BACKWARD)
    outs16 = [D.half() for D in r["outs"]]
    call16 = lambda qs: ops.quant_stack_backward(adj16, x16, c["w32"], c["a32"], [True, False], c["ptr"], outs16, c["gp"], qs,
                                                 alpha=ALPHA, plan=plan16)
    assert _status(lambda: call16([qc, None])) == -3
    dW, dA = call16([None, None])                                            # (without one it is sgx_gat_stack_backward)
    assert torch.isfinite(dW[0]).all() and dA[0] is not None


# ---- 8. the model ----------------------------------------------------------------------------------------------------------------
def _count(monkeypatch):
    from sgracex1_amd import ops
    calls = {"fwd": 0, "bwd": 0, "gp": []}
    real_f, real_b = ops.quant_stack_forward, ops.quant_stack_backward

    def f(*a, **k):
        calls["fwd"] += 1
        return real_f(*a, **k)

    def b(*a, **k):
        calls["bwd"] += 1
        calls["gp"].append(a[7].detach().clone())                    # grad_pooled
        return real_b(*a, **k)
    monkeypatch.setattr(ops, "quant_stack_forward", f)
    monkeypatch.setattr(ops, "quant_stack_backward", b)
    return calls


def _step(model, b, weight):
    model.zero_grad(set_to_none=True)
    out = model(b.x, b.edge_index, b.batch)
    (out * weight).sum().backward()
    return out


def _registers(ip):
    rm = ip.register_map
    return tuple(int(getattr(rm, k)) for k in ("scale_fea", "deq_factor", "quantization_scale_fea", "quantization_scale_w",
                                               "quantization_scale_adj", "quantized_multiplier"))


def test_model_step_agrees_with_the_layer_by_layer_step(quant_model, monkeypatch):
    """One MUTAG step under fake quantisation at 8 bits with a fixed gradient on the logits (eval mode: no dropout): one
    forward and one backward stack call; the parameter gradients of the train_stack step and of the layer-by-layer step on
    the same weights both lie inside the restatement's bound around the float64 value; `layern` and the quantiser
    registers end as the two layer calls leave them."""
    from sgracex1_amd import ops
    make, config, sgrace = quant_model
    ref_model, ip = make(8, compute_attention=1)
    ip.register_map.layer_count = 2
    fused = sgrace.GAT_POOL_PYNQ(7, 64, 2, train_stack=True).to(DEV).eval()
    fused.load_state_dict(ref_model.state_dict())
    calls = _count(monkeypatch)
    b = _mutag_batch()
    n_graphs = int(b.batch.max()) + 1
    torch.manual_seed(1)
    weight = torch.randn(n_graphs, 2, device=DEV)
    assert sgrace.layern == 1
    _step(ref_model, b, weight)
    assert (calls["fwd"], calls["bwd"]) == (0, 0)
    after_layers = (sgrace.layern, _registers(ip))
    ip.register_map.scale_fea = 0                                            # (so that the stack step has to write it)
    _step(fused, b, weight)
    assert (calls["fwd"], calls["bwd"]) == (1, 1)
    assert (sgrace.layern, _registers(ip)) == after_layers
    qc = sgrace.quant_constants
    qs = [qc, qc.second_layer()]
    ei, norm = sgrace.sym_norm2(b.edge_index, b.num_nodes)
    adj = sgrace._edge_csr(None, ei, norm, b.num_nodes, torch.float32)
    ptr = ops.graph_ptr_of(b.batch)
    layers = (ref_model.att1, ref_model.att2)
    Ws = [f64(m.weight) for m in layers]
    atts = [f64(m.attention).reshape(-1) for m in layers]
    fea = ops.Csr.from_dense(b.x.float(), torch.float32)
    monkeypatch.undo()
    _, outs = ops.quant_stack_forward(adj.quantized(qc), fea, [m.weight.detach().t().contiguous() for m in layers],
                                      [m.attention.detach().reshape(-1).contiguous() for m in layers], [True, False], ptr, qs,
                                      alpha=ALPHA, adj_quantised=True, want_layer_outputs=True)
    ref = quant_stack_grad_f64((adj.rowptr.cpu().numpy(), adj.col.cpu().numpy(), f64(adj.val)[:adj.nnz]), f64(b.x), Ws, atts,
                               [True, False], ptr.cpu().numpy(), f64(calls["gp"][0]), [f64(D) for D in outs], qs,
                               adj_q=f32(adj.quantized(qc).val)[:adj.nnz], alpha=ALPHA)
    for l in range(2):
        assert (np.abs(ref["dW"][l]) > ref["tW"][l] * ref["mW"][l] + 1e-30).any(), l       # the bound separates from no gradient
    for name, model in (("layer by layer", ref_model), ("train_stack", fused)):
        for l, m in enumerate((model.att1, model.att2)):
            ok, ratio = within(f64(m.weight.grad), ref["dW"][l], ref["mW"][l], ref["tW"][l])
            print(f"{name} dW_{l}: worst {ratio:.3f} of the bound")
            assert ok, (name, l, "dW", ratio)
            assert m.attention.grad.shape == m.attention.shape
            ok, ratio = within(f64(m.attention.grad).reshape(-1), ref["dA"][l], ref["mA"][l], ref["tA"][l])
            print(f"{name} grad_attention_{l}: worst {ratio:.3f} of the bound")
            assert ok, (name, l, "grad_attention", ratio)
    assert same_bits(ref_model.lin.bias.grad, fused.lin.bias.grad)


@pytest.mark.parametrize("why", ["killed_row", "float16", "int8_hidden_200"])
def test_model_declines_the_route(why, quant_model, monkeypatch):
    """Where the quantised eval route is declined the training route is too, and the step is today's layer-by-layer step:
    the same bits in every parameter gradient as with train_stack off."""
    make, config, sgrace = quant_model
    calls = _count(monkeypatch)

    def grads(model, b, weight):
        _step(model, b, weight)
        return [p.grad.clone() for p in model.parameters() if p.grad is not None]

    def pair(bits, hidden, **flags):
        model, ip = make(bits, hidden=hidden, **flags)
        ip.register_map.layer_count = 2
        fused = sgrace.GAT_POOL_PYNQ(7, hidden, 2, train_stack=True).to(DEV).eval()
        fused.load_state_dict(model.state_dict())
        return model, fused, ip

    if why == "killed_row":
        model, fused, ip = pair(4, 64, compute_attention=1)
        b = _mutag_batch(extra=_bipartite())
        weight = torch.ones(int(b.batch.max()) + 1, 2, device=DEV)
        want, got = grads(model, b, weight), grads(fused, b, weight)
        assert (calls["fwd"], calls["bwd"]) == (0, 0) and len(want) == len(got) >= 4
        assert all(same_bits(a, g) for a, g in zip(want, got))
        ok = _mutag_batch()                                                  # ... and without the killed rows it is taken
        grads(fused, ok, torch.ones(int(ok.batch.max()) + 1, 2, device=DEV))
        assert (calls["fwd"], calls["bwd"]) == (1, 1)
    elif why == "float16":
        model, fused, ip = pair(8, 64, compute_attention=1, float_type=np.float16)
        b = _mutag_batch()
        with pytest.raises(TypeError, match="float32 buffers"):              # the layer's own refusal, as today
            fused(b.x, b.edge_index, b.batch)
        assert (calls["fwd"], calls["bwd"]) == (0, 0)
    else:
        model, fused, ip = pair(8, 200, compute_attention=0, hardware_quantize=1)
        b = _mutag_batch()
        weight = torch.ones(int(b.batch.max()) + 1, 2, device=DEV)
        want, got = grads(model, b, weight), grads(fused, b, weight)
        assert (calls["fwd"], calls["bwd"]) == (0, 0)
        assert all(same_bits(a, g) for a, g in zip(want, got))
        model, fused, ip = pair(8, 128, compute_attention=0, hardware_quantize=1)   # 128 columns: the fp32 form, the route is taken
        grads(fused, b, weight)
        assert (calls["fwd"], calls["bwd"]) == (1, 1)


def test_ten_epochs_on_mutag(quant_model, monkeypatch):
    """examples/molecule_gcn_train.py --model gat --layer-count 2 --train-stack --qbits 8, inline, against the
    layer-by-layer run from the same seed: the training loss falls, the test accuracies lie within 0.03 of each other
    (test_gpu_gat_stack_train.py's twenty-epoch criterion)."""
    import os
    from sgracex1_amd import pyg_lite as G
    make, config, sgrace = quant_model
    _, ip = make(8, compute_attention=1)
    ip.register_map.layer_count = 2
    raw = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mutag_raw.npz"))
    graphs = G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])
    torch.manual_seed(12345)
    graphs = [graphs[i] for i in torch.randperm(len(graphs)).tolist()]
    train, test = G.collate(graphs[:2000]).to(DEV), G.collate(graphs[50:100]).to(DEV)
    calls = _count(monkeypatch)

    def fit(train_stack):
        torch.manual_seed(12345)
        sgrace.layern = 1
        model = sgrace.GAT_POOL_PYNQ(7, 64, 2, train_stack=train_stack).to(DEV)
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
        losses = []
        for _ in range(10):
            model.train()
            opt.zero_grad()
            loss = torch.nn.functional.cross_entropy(model(train.x, train.edge_index, train.batch), train.y)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        model.eval()
        ip.register_map.layer_count = 1                                      # (both evaluated layer by layer)
        with torch.no_grad():
            pred = model(test.x, test.edge_index, test.batch).argmax(1)
        ip.register_map.layer_count = 2
        return losses, float((pred == test.y).float().mean())

    base_losses, base_acc = fit(False)
    assert calls["bwd"] == 0
    losses, acc = fit(True)
    assert calls["bwd"] == 10
    print(f"layer by layer: loss {base_losses[0]:.4f} -> {base_losses[-1]:.4f}, test accuracy {base_acc:.2f}; "
          f"train_stack: loss {losses[0]:.4f} -> {losses[-1]:.4f}, test accuracy {acc:.2f}")
    assert losses[-1] < losses[0]
    assert abs(acc - base_acc) <= 0.03, (acc, base_acc)

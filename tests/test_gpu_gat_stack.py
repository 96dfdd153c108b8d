"""sgx_gat_stack_forward on the GPU (include/sgx.h, "GAT layers in the small-graph stack"): GCN layers bit-equal to
sgx_stack_forward; GAT layers, stage by stage, inside the bound of the float64 edge softmax (tests/_gat_ref.py) on the
device's own H, on the fused and on the chained path; determinism; edge shapes; the model's one-call eval path.

Sensitivity, shown on tests/_gat_stack_ref.py's batch with the deliberately wrong forms of _gat_ref.mutant (float64
restatements rounded as a kernel's output; the mutant kernels themselves have not been run on a device), at every first-
layer width of test_gat_layers_fused, fp16 and fp32: the mask as `values != 0` leaves the bound on the rows
all_masked_plus0_minus0_negative, one_live_among_masked and masked_max, as `values >= 0` on
all_masked_plus0_minus0_negative; the row maximum over masked entries too on masked_max and one_live_among_masked (their
live weights underflow to 0).  Skipping the division by the sum scales every row with two comparable live entries.
"""
import os

import numpy as np
import pytest
import torch

import _gat_ref as R
import _gat_stack_ref as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
TORCH = {"f16": torch.float16, "f32": torch.float32}
ALPHA = 0.2


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def f64(t):
    return t.double().cpu().numpy()


def on_device(b, dt, sparse):
    """build_batch's arrays as (adj Csr, x Csr or dense, graph_ptr) in dt on the GPU."""
    from sgracex1_amd import ops
    td = TORCH[dt]
    adj = ops.Csr(torch.tensor(b["rowptr"], dtype=torch.int32, device=DEV), torch.tensor(b["col"], dtype=torch.int32, device=DEV),
                  torch.tensor(b["val"], device=DEV).to(td), b["n_rows"])
    x = torch.tensor(b["x"], device=DEV).to(td)
    return adj, (ops.Csr.from_dense(x, td) if sparse else x), torch.tensor(b["graph_ptr"], dtype=torch.int32, device=DEV)


def layers_for(dt, m_in, widths, gat, seed):
    """Per layer (W [M, P] float64 of dt values, attention [2 P] or None): the first GAT layer on the features carries the
    designed scores, the others scores of order 1."""
    Ws, atts = [], []
    m = m_in
    for l, (P, g) in enumerate(zip(widths, gat)):
        W, att = S.first_layer(dt, m, P, seed) if (l == 0 and g) else S.plain_layer(dt, m, P, seed + l)
        Ws.append(W)
        atts.append(att if g else None)
        m = P
    return Ws, atts


def dev_layers(dt, Ws, atts):
    td = TORCH[dt]
    return ([torch.tensor(W.T.copy(), device=DEV).to(td).contiguous() for W in Ws],
            [None if a is None else torch.tensor(a, device=DEV).to(td) for a in atts])


def no_workspace(monkeypatch):
    """The fused path: sgx_gat_stack_workspace_bytes is 0, so ops asks for no workspace, and the call runs without one."""
    from sgracex1_amd import ops

    def refuse(device, nbytes):
        raise AssertionError(f"sgx_gat_stack_workspace_bytes = {nbytes}: not the fused path")
    monkeypatch.setattr(ops, "_workspace", refuse)


def needs_workspace(monkeypatch):
    from sgracex1_amd import ops
    asked, real = [], ops._workspace

    def record(device, nbytes):
        asked.append(int(nbytes))
        return real(device, nbytes)
    monkeypatch.setattr(ops, "_workspace", record)
    return asked


def check_layers(b, dt, adj, x, ptr, wts, atts_d, atts, relus, outs, logits, pooled, head_w, head_b):
    """Layer by layer on the device's own D_{l-1}: H_l from the chained product (test_all_gcn_layers_bit_equal shows the
    stack's product is that one), D_l of a GAT layer inside _gat_ref's bound on that H (dead rows exactly 0), D_l of a GCN
    layer bit-equal to the chained aggregate; pooled and logits against float64 on the device's own last D."""
    from sgracex1_amd import ops
    X = x
    rows = np.arange(b["n_rows"])
    for l, (Wt, att, relu) in enumerate(zip(wts, atts, relus)):
        H = ops.xw_sparse(X, Wt.t().contiguous(), use_plan=False) if isinstance(X, ops.Csr) else ops.xw_dense(X, Wt)
        if att is None:
            want = ops.spmm(adj, H, relu=relu, use_plan=False)
            assert same_bits(outs[l], want), f"GCN layer {l}"
        else:
            g = dict(rowptr=b["rowptr"], col=b["col"], val=b["val"], Wh=f64(H)[:, :Wt.shape[0]], att=np.asarray(att, np.float64))
            r = R.forward(g, 1, alpha=ALPHA, relu=bool(relu), dead_rule="zero", out=dt)
            R.check(f"D_{l}", f64(outs[l]), r["D"], r["bD"], rows, b["names"])
            assert r["dead"].any() and not bits(outs[l])[torch.tensor(r["dead"], device=DEV)].any(), f"dead rows of layer {l}"
        X = outs[l]
    wp, wl, bP, bL = S.readout_f64(f64(X), b["graph_ptr"], None if head_w is None else f64(head_w),
                                   None if head_b is None else f64(head_b))
    R.check("pooled", f64(pooled), wp, bP, np.arange(len(wp)), {})
    if logits is not None:
        R.check("logits", f64(logits), wl, bL, np.arange(len(wl)), {})


def run_case(dt, m_in, widths, gat, relus, sparse, budget=None, plan_kind=None, seed=0, **batch):
    """Builds the batch for the case's plan and runs ops.gat_stack_forward with and without a head."""
    from sgracex1_amd import ops
    width = max(list(widths) + ([] if sparse else [m_in]))
    R_ = S.rows_budget(dt, width)
    b = S.build_batch(dt, R_ if budget is None else budget, m_in, seed=seed, **batch)
    adj, x, ptr = on_device(b, dt, sparse)
    Ws, atts = layers_for(dt, m_in, widths, gat, seed)
    wts, atts_d = dev_layers(dt, Ws, atts)
    rng = np.random.default_rng(seed + 77)
    head_w = torch.tensor(rng.standard_normal((3, widths[-1])), device=DEV, dtype=torch.float32)
    head_b = torch.tensor(rng.standard_normal(3), device=DEV, dtype=torch.float32)
    plan = ops.BatchPlan.cached(adj, ptr, width) if plan_kind is None else ops.BatchPlan(adj, ptr, width, plan_kind)
    logits, outs = ops.gat_stack_forward(adj, x, wts, atts_d, relus, ptr, head_w, head_b, alpha=ALPHA, want_layer_outputs=True,
                                         plan=plan)
    pooled = ops.gat_stack_forward(adj, x, wts, atts_d, relus, ptr, alpha=ALPHA, plan=plan)
    return dict(b=b, adj=adj, x=x, ptr=ptr, wts=wts, atts_d=atts_d, atts=atts, relus=relus, outs=outs, logits=logits,
                pooled=pooled, head_w=head_w, head_b=head_b, plan=plan, budget=R_, width=width)


def check_case(c, dt):
    check_layers(c["b"], dt, c["adj"], c["x"], c["ptr"], c["wts"], c["atts_d"], c["atts"], c["relus"], c["outs"], c["logits"],
                 c["pooled"], c["head_w"], c["head_b"])


# ---- 1. all layers gat_mode = 0 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("widths,sparse", [((64,), True), ((21,), False), ((64, 100, 7), True), ((100, 3, 64), False)])
def test_all_gcn_layers_bit_equal_to_gcn_stack_forward(dt, widths, sparse, monkeypatch):
    from sgracex1_amd import ops
    no_workspace(monkeypatch)
    m_in = 7
    relus = [True, False, True][:len(widths)]
    c = run_case(dt, m_in, widths, [0] * len(widths), relus, sparse)
    assert c["plan"].fits and c["plan"].max_graph == c["budget"] and c["plan"].groups >= 3
    (logits, pooled), outs = ops.gcn_stack_forward(c["adj"], c["x"], c["wts"], relus, c["ptr"], c["head_w"], c["head_b"],
                                                   want_layer_outputs=True, want_pooled=True, plan=c["plan"])
    for l, (a, w) in enumerate(zip(c["outs"], outs)):
        assert same_bits(a, w), f"D_{l}"
    assert same_bits(c["logits"], logits) and same_bits(c["pooled"], pooled)


# ---- 2. GAT layers on the fused path -------------------------------------------------------------------------------------
FUSED = [  # m_in, widths, gat_mode per layer, relu per layer, sparse layer 0
    (7, (64,), (1,), (1,), True),
    (7, (1,), (1,), (0,), False),
    (7, (3,), (1,), (1,), True),
    (64, (64, 64), (1, 1), (1, 0), False),
    (7, (256, 64), (1, 1), (0, 1), True),
    (64, (256,), (1,), (1,), False),
    (64, (64, 3, 64, 1), (1, 1, 1, 1), (0, 1, 1, 0), False),
    (7, (64, 3, 256, 64), (1, 0, 1, 0), (1, 1, 0, 1), True),        # mixed GCN and GAT
    (64, (3, 64), (0, 1), (0, 0), False),                            # a GCN layer first
    (300, (64, 64), (1, 1), (1, 0), True),                          # a sparse layer 0 wider than the plan's max_width
]


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("case", range(len(FUSED)))
def test_gat_layers_fused(dt, case, monkeypatch):
    no_workspace(monkeypatch)
    m_in, widths, gat, relus, sparse = FUSED[case]
    c = run_case(dt, m_in, widths, gat, [bool(r) for r in relus], sparse, seed=case)
    assert c["plan"].fits and c["plan"].max_graph == c["budget"] and c["plan"].groups >= 3
    assert c["width"] == max(widths + (() if sparse else (m_in,)))        # (300 is not in it)
    monkeypatch.undo()
    check_case(c, dt)


# ---- 3. the same descriptors on the chained path -------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("case", [0, 3, 7, 8])
def test_gat_layers_chained(dt, case, monkeypatch):
    asked = needs_workspace(monkeypatch)
    m_in, widths, gat, relus, sparse = FUSED[case]
    width = max(widths + (() if sparse else (m_in,)))
    over = S.rows_budget(dt, width) + 1                                  # one graph over the budget
    c = run_case(dt, m_in, widths, gat, [bool(r) for r in relus], sparse, budget=over, seed=case)
    assert not c["plan"].fits and c["plan"].max_graph == over and c["plan"].groups == 0
    assert len(asked) == 2 and min(asked) > 0                            # both calls took the workspace
    monkeypatch.undo()
    check_case(c, dt)


# ---- 4. determinism and grouping -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_same_bits_on_every_run_and_for_every_grouping(dt, monkeypatch):
    from sgracex1_amd import _lib
    no_workspace(monkeypatch)
    m_in, widths, gat, relus, sparse = 7, (64, 64), (1, 1), (True, False), True
    small = S.rows_budget(dt, 64, backward=True)                          # the batch fits the backward plan's budget too
    assert 16 <= small < S.rows_budget(dt, 64)
    # over 256 rows, so that the forward plan's groups take first rows in windows of two and the backward plan's of one
    big = dict(budget=small, seed=5, n_graphs=20, filler=(20, 30))
    a = run_case(dt, m_in, widths, gat, relus, sparse, **big)
    again = run_case(dt, m_in, widths, gat, relus, sparse, **big)
    other = run_case(dt, m_in, widths, gat, relus, sparse, plan_kind=_lib.SGX_BATCH_BACKWARD, **big)
    assert a["b"]["n_rows"] > 256 and a["plan"].fits and other["plan"].fits
    ga, go = a["plan"].export_groups().cpu().numpy(), other["plan"].export_groups().cpu().numpy()
    assert len(ga) != len(go) or (ga != go).any()                        # the two plans group differently
    for name, r in (("second run", again), ("backward plan", other)):
        for l in range(2):
            assert same_bits(a["outs"][l], r["outs"][l]), (name, l)
        assert same_bits(a["logits"], r["logits"]) and same_bits(a["pooled"], r["pooled"]), name


# ---- 5. edge shapes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_no_graphs_and_one_single_row_graph(dt, monkeypatch):
    from sgracex1_amd import ops
    no_workspace(monkeypatch)
    td = TORCH[dt]
    Ws, atts = layers_for(dt, 7, (8, 4), (1, 1), 0)
    wts, atts_d = dev_layers(dt, Ws, atts)
    head_w = torch.randn(2, 4, device=DEV)
    i32 = dict(dtype=torch.int32, device=DEV)
    # no graphs, no rows
    adj = ops.Csr(torch.zeros(1, **i32), torch.zeros(0, **i32), torch.zeros(0, dtype=td, device=DEV), 0)
    logits, outs = ops.gat_stack_forward(adj, torch.zeros((0, 7), dtype=td, device=DEV), wts, atts_d, [True, False],
                                         torch.zeros(1, **i32), head_w, want_layer_outputs=True)
    assert logits.shape == (0, 2) and [tuple(o.shape) for o in outs] == [(0, 8), (0, 4)]
    # one graph of one row with a self loop: the softmax weight is 1, so D = act(H) exactly
    adj = ops.Csr(torch.tensor([0, 1], **i32), torch.zeros(1, **i32), torch.full((1,), 0.5, dtype=td, device=DEV), 1)
    x = torch.tensor(np.random.default_rng(1).standard_normal((1, 7)), device=DEV).to(td)
    ptr = torch.tensor([0, 1], **i32)
    pooled, outs = ops.gat_stack_forward(adj, x, wts, atts_d, [True, False], ptr, want_layer_outputs=True)
    H0 = ops.xw_dense(x, wts[0])
    assert same_bits(outs[0], torch.relu(H0[:, :8]).contiguous())
    assert same_bits(outs[1], ops.xw_dense(outs[0], wts[1])[:, :4].contiguous())
    assert torch.equal(pooled, outs[1].float())
    # ... and without the self loop the row is dead: 0
    adj = ops.Csr(torch.tensor([0, 0], **i32), torch.zeros(0, **i32), torch.zeros(0, dtype=td, device=DEV), 1)
    pooled, outs = ops.gat_stack_forward(adj, x, wts, atts_d, [True, False], ptr, want_layer_outputs=True)
    assert not bits(outs[0]).any() and not bits(outs[1]).any() and not pooled.any()


def test_fp32_tiles_that_fill_64_kib(monkeypatch):
    """fp32 at width 252: 32 rows of two 1 KiB tile rows are 64 KiB exactly, the score arrays come on top of it."""
    no_workspace(monkeypatch)
    assert S.rows_budget("f32", 252) == 32
    c = run_case("f32", 64, (252, 64), (1, 1), [True, False], False, seed=9)
    assert c["plan"].fits and c["plan"].rows == 32 and c["plan"].max_graph == 32
    monkeypatch.undo()
    check_case(c, "f32")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_fp32_tiles_that_fill_64_kib_on_a_second_device_of_the_process(monkeypatch):
    """The same launch on device 0 and then on device 1: the kernel's opt-in to more than 64 KiB of LDS is per device."""
    for k in (0, 1):
        with torch.cuda.device(k):
            no_workspace(monkeypatch)
            c = run_case("f32", 64, (252, 64), (1, 1), [True, False], False, seed=9)
            assert c["plan"].fits and c["plan"].rows == 32 and c["outs"][0].device.index == k
            monkeypatch.undo()
            check_case(c, "f32")


# ---- 6. model and capture --------------------------------------------------------------------------------------------------
def _mutag_batch(n=48):
    from sgracex1_amd import pyg_lite as G
    raw = np.load(os.path.join(GOLD, "mutag_raw.npz"))
    graphs = G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])
    return G.collate(graphs[:n]).to(DEV)


@pytest.fixture
def sgrace_model():
    from sgracex1_amd import config, sgrace
    saved = config.snapshot()
    config.acc, config.float_type = 1, np.float32
    ip = sgrace.init_SGRACE()
    torch.manual_seed(7)
    model = sgrace.GAT_POOL_PYNQ(7, 64, 2).to(DEV).eval()
    yield model, ip, config, sgrace
    config.restore(saved)
    sgrace.init_SGRACE()


def _count_calls(monkeypatch):
    from sgracex1_amd import ops
    calls, real = [], ops.gat_stack_forward

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ops, "gat_stack_forward", counting)
    return calls


def test_gat_pool_pynq_layer_count_two(sgrace_model, monkeypatch):
    """GAT_POOL_PYNQ's eval forward with register layer_count 1 (layer by layer) and 2 (one call): each inside the bound
    of the float64 restatement (tests/_gat_stack_ref.py, chain_f64) of the model on the same rounded operands."""
    model, ip, config, sgrace = sgrace_model
    b = _mutag_batch()
    calls = _count_calls(monkeypatch)
    config.compute_attention = 1
    with torch.no_grad():
        ip.register_map.layer_count = 1
        one = model(b.x, b.edge_index, b.batch)
        assert not calls
        ip.register_map.layer_count = 2
        fused = model(b.x, b.edge_index, b.batch)
        assert len(calls) == 1
        model.train()
        model(b.x, b.edge_index, b.batch)                            # training: layer by layer
        model.eval()
    assert len(calls) == 1
    with torch.enable_grad():
        model(b.x, b.edge_index, b.batch)                            # gradients on: layer by layer
    assert len(calls) == 1
    ei, norm = sgrace.sym_norm2(b.edge_index, b.num_nodes)
    adj = sgrace._edge_csr(None, ei, norm, b.num_nodes, torch.float32)
    from sgracex1_amd import ops
    ptr = ops.graph_ptr_of(b.batch)
    val = lambda t: f64(t.detach())                                   # (fp32 layer buffers: the operands as stored)
    atts = [val(model.att1.attention).reshape(-1), val(model.att2.attention).reshape(-1)]
    chain = lambda a, **k: S.chain_f64((adj.rowptr.cpu().numpy(), adj.col.cpu().numpy(), f64(adj.val)[:adj.nnz]), val(b.x),
                                       [val(model.att1.weight), val(model.att2.weight)], a, [True, False],
                                       ptr.cpu().numpy(), val(model.lin.weight), val(model.lin.bias), alpha=model.att1.alpha, **k)
    ref = chain(atts, dt="f32")
    rows = np.arange(ref["logits"].shape[0])
    # the bound says something: the same model with the attention vectors zeroed (a uniform softmax over a row's live
    # entries) lies outside it, by more than twice the bound, on every graph
    uniform = chain([np.zeros_like(a) for a in atts])["logits"]
    assert (np.abs(uniform - ref["logits"]) > 2 * ref["b_logits"]).any(1).all()
    R.check("layer by layer", f64(one), ref["logits"], ref["b_logits"], rows, {})
    R.check("one call", f64(fused), ref["logits"], ref["b_logits"], rows, {})


def test_gat_pool_pynq_without_attention_is_the_gcn_path(sgrace_model, monkeypatch):
    model, ip, config, sgrace = sgrace_model
    b = _mutag_batch()
    calls = _count_calls(monkeypatch)
    config.compute_attention = 0
    with torch.no_grad():
        ip.register_map.layer_count = 1
        one = model(b.x, b.edge_index, b.batch)
        assert not calls
        ip.register_map.layer_count = 2
        fused = model(b.x, b.edge_index, b.batch)
    assert len(calls) == 1 and same_bits(one, fused)


def test_fused_call_replays_from_a_captured_graph():
    """One stream, no parallel branches: the captured graph is one kernel node."""
    from sgracex1_amd import ops
    dt = "f16"
    b = S.build_batch(dt, S.rows_budget(dt, 64), 7, seed=2)
    adj, x, ptr = on_device(b, dt, True)
    Ws, atts = layers_for(dt, 7, (64, 64), (1, 1), 2)
    wts, atts_d = dev_layers(dt, Ws, atts)
    head_w, head_b = torch.randn(2, 64, device=DEV), torch.randn(2, device=DEV)
    plan = ops.BatchPlan.cached(adj, ptr, 64)
    assert plan.fits
    call = lambda: ops.gat_stack_forward(adj, x, wts, atts_d, [True, False], ptr, head_w, head_b, alpha=ALPHA, plan=plan)
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

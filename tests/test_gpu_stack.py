"""sgx_stack_forward on the GPU (include/sgx.h, "a batch of small graphs"): every stage bit-equal to the chained
kernels, end to end within a magnitude bound of the float64 restatement (tests/_stack_ref.py), the fallbacks, and the
model's one-call eval path (register layer_count)."""
import os

import numpy as np
import pytest
import torch

from _stack_ref import stack_bound, stack_f64

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
UNIT = {torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def chain(adj, x, wts, relus, ptr, head_w=None, head_b=None):
    """The stack as separate launches: per layer X.W (sgx_xw_sparse without a plan / sgx_xw_dense) and the aggregation
    (sgx_spmm_csr without a plan), then sgx_readout_mean_linear."""
    from sgracex1_amd import ops
    X, outs = x, []
    for l, (Wt, relu) in enumerate(zip(wts, relus)):
        H = ops.xw_sparse(X, Wt.t().contiguous(), use_plan=False) if isinstance(X, ops.Csr) else ops.xw_dense(X, Wt)
        X = ops.spmm(adj, H, relu=relu, use_plan=False)
        outs.append(X)
    if ptr is None:
        return outs, None, None
    if head_w is None:
        return outs, ops.readout_mean_linear(X, ptr), None
    logits, pooled = ops.readout_mean_linear(X, ptr, head_w, head_b, want_pooled=True)
    return outs, pooled, logits


def check_stages(adj, x, wts, relus, ptr, outs, pooled=None, logits=None, head_w=None, head_b=None):
    """Each stage of the fused result against the chained kernels fed with the fused result's previous stage: the X.W
    contract and the aggregation order together (a D_l equal to spmm(A, xw(D_{l-1})) bit for bit)."""
    from sgracex1_amd import ops
    X = x
    for l, (Wt, relu) in enumerate(zip(wts, relus)):
        H = ops.xw_sparse(X, Wt.t().contiguous(), use_plan=False) if isinstance(X, ops.Csr) else ops.xw_dense(X, Wt)
        want = ops.spmm(adj, H, relu=relu, use_plan=False)
        assert same_bits(outs[l], want), f"layer {l}: {(outs[l].float() - want.float()).abs().max().item()}"
        X = outs[l]
    if logits is not None:
        wl, wp = ops.readout_mean_linear(X, ptr, head_w, head_b, want_pooled=True)
        assert same_bits(logits, wl)
        if pooled is not None:
            assert same_bits(pooled, wp)
    elif pooled is not None:
        assert same_bits(pooled, ops.readout_mean_linear(X, ptr))


# ---- MUTAG --------------------------------------------------------------------------------------------------------
def _mutag(device=DEV):
    from sgracex1_amd import pyg_lite as G
    raw = np.load(os.path.join(GOLD, "mutag_raw.npz"))
    graphs = G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])
    return G.collate(graphs).to(device), graphs


def _dense_np(csr):
    out = np.zeros((csr.n_rows, csr.n_cols))
    rp, c, v = csr.rowptr.cpu().numpy(), csr.col.cpu().numpy(), csr.val.double().cpu().numpy()
    row = np.repeat(np.arange(csr.n_rows), np.diff(rp))
    np.add.at(out, (row, c[:len(row)]), v[:len(row)])
    return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_mutag_stack_bit_equal_to_the_chain(dtype):
    from sgracex1_amd import molecule_gcn as M, ops
    b, _ = _mutag()
    adj = ops.csr_from_edge_index(b.edge_index, b.num_nodes, dtype=dtype)
    fea = M.as_csr(b.x, dtype)
    ptr = ops.graph_ptr_of(b.batch)
    torch.manual_seed(11)
    wts = [(torch.randn(64, 7, device=DEV) * 0.4).to(dtype), (torch.randn(64, 64, device=DEV) * 0.15).to(dtype)]
    head_w, head_b = torch.randn(2, 64, device=DEV) * 0.3, torch.randn(2, device=DEV) * 0.1
    (logits, pooled), outs = ops.gcn_stack_forward(adj, fea, wts, [True, False], ptr, head_w, head_b,
                                                   want_layer_outputs=True, want_pooled=True)
    plan = ops.BatchPlan.cached(adj, ptr, 64)
    assert plan.fits and plan.groups >= 188 and plan.max_graph == 28      # one launch: every graph fits, ~one per CU
    check_stages(adj, fea, wts, [True, False], ptr, outs, pooled, logits, head_w, head_b)
    # end to end against the float64 model on the same (rounded) operands
    args = ((adj.rowptr.cpu().numpy(), adj.col.cpu().numpy(), adj.val.double().cpu().numpy()), _dense_np(fea),
            [w.double().t().cpu().numpy() for w in wts], [True, False], ptr.cpu().numpy(), head_w.double().cpu().numpy(),
            head_b.double().cpu().numpy())
    _, _, ref = stack_f64(*args)
    bound = stack_bound(*args, UNIT[dtype])
    err = np.abs(logits.double().cpu().numpy() - ref)
    assert (err <= bound).all(), float((err / bound).max())
    # argmax: the chained path's wherever the top-two margin exceeds the bound; the float64 model's too
    _, _, chained = chain(adj, fea, wts, [True, False], ptr, head_w, head_b)
    lg = logits.double().cpu().numpy()
    margin = np.abs(lg[:, 0] - lg[:, 1])
    sure = margin > 2 * bound.max(1)
    assert sure.sum() >= 94                                             # at least half the graphs
    assert (lg.argmax(1)[sure] == chained.cpu().numpy().argmax(1)[sure]).all()
    assert (lg.argmax(1)[sure] == ref.argmax(1)[sure]).all()
    # determinism
    again = ops.gcn_stack_forward(adj, fea, wts, [True, False], ptr, head_w, head_b)
    assert same_bits(again, logits)


def _count_stack_calls(monkeypatch):
    from sgracex1_amd import ops
    calls = []
    real = ops.gcn_stack_forward

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ops, "gcn_stack_forward", counting)
    return calls


def test_gcn_pynq_layer_count_two_same_eval_accuracy(monkeypatch):
    """GCN_PYNQ trained a few epochs, then evaluated with register layer_count 1 (five launches) and 2 (one call):
    the same logits bit for bit, hence the same accuracy; training mode keeps the layer-by-layer path."""
    from sgracex1_amd import molecule_gcn as M, pynq_shim
    b, _ = _mutag()
    ip = pynq_shim.Overlay("gnn_all.bit").mmult_top_0
    model = M.GCN_PYNQ(64, 7, 2, ip).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    calls = _count_stack_calls(monkeypatch)
    ip.register_map.layer_count = 2
    for _ in range(15):
        model.train()
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(model(1, b.x, b.edge_index, b.batch), b.y)
        loss.backward()
        opt.step()
    assert not calls                                                 # training: layer by layer
    model.eval()
    with torch.no_grad():
        ip.register_map.layer_count = 1
        one = model(1, b.x, b.edge_index, b.batch)
        assert not calls
        ip.register_map.layer_count = 2
        fused = model(1, b.x, b.edge_index, b.batch)
        assert len(calls) == 1
    assert same_bits(fused, one)
    acc1 = float((one.argmax(1) == b.y).float().mean())
    acc2 = float((fused.argmax(1) == b.y).float().mean())
    assert acc1 == acc2 and acc2 > 0.6


def test_gcn_pynq_keeps_the_old_path_for_crossing_edges_and_unsorted_batches(monkeypatch):
    from sgracex1_amd import molecule_gcn as M, ops, pynq_shim
    b, _ = _mutag()
    ip = pynq_shim.Overlay("gnn_all.bit").mmult_top_0
    model = M.GCN_PYNQ(64, 7, 2, ip).to(DEV).eval()
    # an edge between graph 0 and graph 1: the plan refuses the batch (SGX_ERR_BLOCKS)
    ptr = ops.graph_ptr_of(b.batch)
    u, v = int(ptr[0]), int(ptr[1])
    ei = torch.cat([b.edge_index, torch.tensor([[u, v], [v, u]], device=DEV)], 1)
    adj = ops.csr_from_edge_index(ei, b.num_nodes, dtype=torch.float16)
    with pytest.raises(Exception) as e:
        ops.BatchPlan(adj, ptr, 64)
    assert getattr(e.value, "status", None) == -9
    calls = _count_stack_calls(monkeypatch)
    # a batch vector in descending order: its graphs are not row segments (graph_ptr_of gives None)
    unsorted = (b.num_graphs - 1) - b.batch
    for edges, batch in ((ei, b.batch), (b.edge_index, unsorted)):
        with torch.no_grad():
            ip.register_map.layer_count = 1
            one = model(1, b.x, edges, batch)
            ip.register_map.layer_count = 2
            two = model(1, b.x, edges, batch)
        assert same_bits(one, two)
    assert not calls


# ---- seeded random block-diagonal batches --------------------------------------------------------------------------
def _budget(dtype, width):
    from sgracex1_amd import ops
    one = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    adj = ops.Csr(torch.tensor([0, 0], dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
                  torch.zeros(0, dtype=dtype, device=DEV), 1)
    return ops.BatchPlan(adj, one, width).rows


def random_batch(seed, dtype, sizes, m_in, sparse, density=0.3):
    """Graphs of the given sizes, each with random directed edges inside it (graph 0 without any, some rows empty),
    random signed edge values and features, in dtype."""
    from sgracex1_amd import ops
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    off = 0
    for g, n in enumerate(sizes):
        if g > 0:
            m = rng.random((n, n)) < min(density, 6.0 / max(n, 1) + 0.05)
            m[rng.random(n) < 0.1] = False                          # empty rows
            r, c = np.nonzero(m)
            rows.append(r + off)
            cols.append(c + off)
        off += n
    N = off
    r = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    c = np.concatenate(cols) if cols else np.zeros(0, np.int64)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=N))]).astype(np.int32)
    val = rng.uniform(-1, 1, len(r))
    adj = ops.Csr(torch.tensor(rowptr, device=DEV), torch.tensor(c.astype(np.int32), device=DEV),
                  torch.tensor(val, device=DEV).to(dtype), N)
    X = rng.standard_normal((N, m_in))
    if sparse:
        X[rng.random((N, m_in)) < 0.8] = 0
    xt = torch.tensor(X, device=DEV).to(dtype)
    x = ops.Csr.from_dense(xt, dtype) if sparse else xt
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), device=DEV)
    return adj, x, ptr


CASES = [  # widths (m_in, P_1 .. P_n), relus, sparse layer 0, head width C (0 = pooled only), keep layer outputs
    ((7, 64, 64), (1, 0), True, 2, True),
    ((7, 21), (1,), False, 1, False),
    ((21, 100, 7), (0, 1), False, 10, True),
    ((100, 64, 100, 21, 64), (1, 1, 0, 1), True, 0, True),
    ((64, 256), (1,), False, 3, False),
    ((256, 7, 256, 64), (0, 1, 1), True, 5, True),
    ((300, 64, 64), (1, 0), True, 2, False),                    # a sparse layer 0 of any width
    ((7, 256, 256, 256, 256), (1, 1, 1, 0), False, 0, False),
]


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_random_batches_bit_equal_to_the_chain(dtype, case):
    from sgracex1_amd import ops
    widths, relus, sparse, C, keep = CASES[case]
    seed = 100 * case + (dtype == torch.float16)
    rng = np.random.default_rng(seed)
    width = max(widths[1:] + (() if sparse else widths[:1]))
    R = _budget(dtype, width)
    assert R >= 16
    sizes = [int(s) for s in rng.integers(1, R + 1, 40)] + [R, 1]
    sizes[0] = 5                                                     # graph 0: no edges
    adj, x, ptr = random_batch(seed, dtype, sizes, widths[0], sparse)
    wts = [(torch.tensor(rng.standard_normal((p, m)) / np.sqrt(m), device=DEV)).to(dtype)
           for m, p in zip(widths[:-1], widths[1:])]
    head_w = torch.tensor(rng.standard_normal((C, widths[-1])), device=DEV, dtype=torch.float32) if C else None
    head_b = torch.tensor(rng.standard_normal(C), device=DEV, dtype=torch.float32) if C and case % 2 else None
    plan = ops.BatchPlan.cached(adj, ptr, width)
    assert plan.fits and plan.max_graph == R
    res = ops.gcn_stack_forward(adj, x, wts, [bool(r) for r in relus], ptr, head_w, head_b, want_layer_outputs=keep,
                                want_pooled=bool(C) and case % 3 == 0)
    out, outs = res if keep else (res, None)
    logits, pooled = (out if isinstance(out, tuple) else (out, None)) if C else (None, out)
    want_outs, want_pooled, want_logits = chain(adj, x, wts, [bool(r) for r in relus], ptr, head_w, head_b)
    if keep:
        check_stages(adj, x, wts, [bool(r) for r in relus], ptr, outs, pooled, logits, head_w, head_b)
    if logits is not None:
        assert same_bits(logits, want_logits)
    if pooled is not None:
        assert same_bits(pooled, want_pooled)
    again = ops.gcn_stack_forward(adj, x, wts, [bool(r) for r in relus], ptr, head_w, head_b)     # determinism
    assert same_bits(again, want_logits if C else want_pooled)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_graph_over_the_budget_takes_the_chained_path(dtype):
    from sgracex1_amd import ops
    R = _budget(dtype, 64)
    sizes = [3, R + 1, 7, 1]
    adj, x, ptr = random_batch(7, dtype, sizes, 21, False, density=0.2)
    wts = [(torch.randn(64, 21, device=DEV) * 0.2).to(dtype), (torch.randn(64, 64, device=DEV) * 0.1).to(dtype)]
    head_w, head_b = torch.randn(3, 64, device=DEV), torch.randn(3, device=DEV)
    plan = ops.BatchPlan.cached(adj, ptr, 64)
    assert not plan.fits and plan.max_graph == R + 1 and plan.groups == 0
    (logits, pooled), outs = ops.gcn_stack_forward(adj, x, wts, [True, False], ptr, head_w, head_b, want_layer_outputs=True,
                                                   want_pooled=True)
    want_outs, want_pooled, want_logits = chain(adj, x, wts, [True, False], ptr, head_w, head_b)
    assert all(same_bits(a, b) for a, b in zip(outs, want_outs))
    assert same_bits(pooled, want_pooled) and same_bits(logits, want_logits)
    # one large graph (graph_ptr None): the last layer's output, through the chained path
    last = ops.gcn_stack_forward(adj, x, wts, [True, False], None)
    assert same_bits(last, want_outs[-1])

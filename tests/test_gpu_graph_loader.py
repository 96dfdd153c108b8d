"""GraphLoader and sgx_collate_graphs on the GPU: batch for batch the same tensors, CSRs, graph_ptr and plans as
pyg_lite.DataLoader's host collation followed by the host-side builders; the fused stack and the model's training
steps give the same bits through either loader; a graph over the budget falls back as before; no synchronisation per
batch; and a fixed batch's collation and plan can be captured and replayed."""
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def bits(t):
    t = t.contiguous()
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def _mutag_graphs():
    from sgracex1_amd import pyg_lite as G
    raw = np.load(os.path.join(GOLD, "mutag_raw.npz"))
    return G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])


def _random_graphs(seed, n_graphs, max_rows, n_feat=7):
    """Graphs of 1 to max_rows rows: isolated nodes, graphs without edges, self loops and repeated edges; a few
    non-one-hot features and zero rows."""
    from sgracex1_amd import pyg_lite as G
    rng = np.random.default_rng(seed)
    out = []
    for g in range(n_graphs):
        n = int(rng.integers(1, max_rows + 1)) if g % 5 else int(rng.choice([1, 2, max_rows]))
        E = int(rng.integers(0, 3 * n + 1)) if g % 7 else 0
        src, dst = rng.integers(0, n, E), rng.integers(0, n, E)
        if E > 2:
            src[0], dst[0] = src[1], dst[1]                   # a repeated edge
            dst[2] = src[2]                                    # a self loop
        x = np.zeros((n, n_feat), np.float32)
        x[np.arange(n), rng.integers(0, n_feat, n)] = 1.0
        x[rng.random(n) < 0.2] = 0.0                           # rows without features
        x[rng.random((n, n_feat)) < 0.05] = rng.standard_normal() * 3
        out.append(G.Graph(torch.as_tensor(x), torch.as_tensor(np.stack([src, dst]).astype(np.int64)),
                           torch.tensor([int(rng.integers(0, 2))])))
    return out


def _check_batch(db, hb, dtypes):
    """One loader batch `db` against the host collation `hb` (moved to the GPU) and the host-side builders."""
    from sgracex1_amd import _lib, ops
    hb = hb.to(DEV)
    n = hb.num_nodes
    assert db.num_graphs == hb.num_graphs
    for f in ("x", "edge_index", "y", "batch"):
        assert same(getattr(db, f), getattr(hb, f)), f
    gp = ops.recorded(db.batch, ("graph_ptr",))
    assert gp is not None and same(gp, ops.graph_ptr_of(hb.batch))
    for dt in dtypes:
        A = ops.recorded(db.edge_index, ("adj_csr", n, dt))
        R = ops.csr_from_edge_index(hb.edge_index, n, dtype=dt)
        assert A.nnz == R.nnz and same(A.rowptr, R.rowptr)
        assert same(A.col[:A.nnz], R.col[:R.nnz]) and same(A.val[:A.nnz], R.val[:R.nnz])
        X = ops.recorded(db.x, ("fea_csr", dt))
        XR = ops.Csr.from_dense(hb.x, dt)
        assert X.nnz == XR.nnz and X.n_cols == XR.n_cols and same(X.rowptr, XR.rowptr)
        assert same(X.col[:X.nnz], XR.col[:XR.nnz]) and same(X.val[:X.nnz], XR.val[:XR.nnz])
        for kind in (_lib.SGX_BATCH_FORWARD, _lib.SGX_BATCH_BACKWARD):
            p = ops.BatchPlan.cached(A, gp, 64, kind)
            assert p is not None and getattr(p, "_group_graph", "untrusted") != "untrusted"     # the trusted constructor
            q = ops.BatchPlan(R, ops.graph_ptr_of(hb.batch), 64, kind)
            assert (p.rows, p.groups, p.max_graph, p.fits) == (q.rows, q.groups, q.max_graph, q.fits)
            assert torch.equal(p.export_groups(), q.export_groups())


def _pair(graphs, batch_size, seed, dtypes=(torch.float16,)):
    from sgracex1_amd import pyg_lite as G
    dl = G.DataLoader(graphs, batch_size=batch_size, shuffle=True, generator=torch.Generator().manual_seed(seed))
    gl = G.GraphLoader(graphs, batch_size=batch_size, shuffle=True, generator=torch.Generator().manual_seed(seed),
                       device=DEV, dtypes=dtypes)
    assert len(dl) == len(gl)
    return dl, gl


@pytest.mark.parametrize("batch_size", [1, 7, 64, 256, "all"])
def test_mutag_batches_match_the_host_loader(batch_size):
    graphs = _mutag_graphs()
    bs = len(graphs) if batch_size == "all" else batch_size
    dl, gl = _pair(graphs, bs, 12345, (torch.float16, torch.float32))
    for epoch in range(2):
        count = 0
        for hb, db in zip(dl, gl):
            _check_batch(db, hb, (torch.float16, torch.float32))
            count += 1
        assert count == len(dl)


@pytest.mark.parametrize("batch_size", [1, 7, 64, 256, "all"])
def test_random_batches_match_the_host_loader(batch_size):
    # up to 140 rows: over the backward budget at width 64 (80 rows) and over the forward one (128)
    graphs = _random_graphs(batch_size if batch_size != "all" else 3, 90, 140)
    bs = len(graphs) if batch_size == "all" else batch_size
    dl, gl = _pair(graphs, bs, 99)
    for epoch in range(2):
        for hb, db in zip(dl, gl):
            _check_batch(db, hb, (torch.float16,))


def test_partial_last_batch_and_unshuffled_order():
    from sgracex1_amd import pyg_lite as G
    graphs = _random_graphs(5, 23, 12)
    dl = G.DataLoader(graphs, batch_size=10)
    gl = G.GraphLoader(graphs, batch_size=10, device=DEV)
    sizes = []
    for hb, db in zip(dl, gl):
        _check_batch(db, hb, (torch.float16,))
        sizes.append(db.num_graphs)
    assert sizes == [10, 10, 3]


def _weights(seed, dtype=torch.float16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    w1 = torch.randn(64, 7, device=DEV, generator=g) * 0.4
    w2 = torch.randn(64, 64, device=DEV, generator=g) * 0.15
    return w1, w2


def test_stack_forward_and_gradients_match_host_batches():
    from sgracex1_amd import _lib, molecule_gcn as M, ops
    graphs = _mutag_graphs()
    dl, gl = _pair(graphs, 64, 4)
    w1, w2 = _weights(1)
    hw, hb_ = torch.randn(2, 64, device=DEV), torch.randn(2, device=DEV)
    for hb, db in zip(dl, gl):
        hb = hb.to(DEV)
        outs = []
        for b, attached in ((hb, False), (db, True)):
            n = b.num_nodes
            if attached:
                adj = ops.recorded(b.edge_index, ("adj_csr", n, torch.float16))
                fea = ops.recorded(b.x, ("fea_csr", torch.float16))
                ptr = ops.recorded(b.batch, ("graph_ptr",))
            else:
                adj = ops.csr_from_edge_index(b.edge_index, n, dtype=torch.float16)
                fea = M.as_csr(b.x, torch.float16)
                ptr = ops.graph_ptr_of(b.batch)
            logits = ops.gcn_stack_forward(adj, fea, [w1.half(), w2.half()], [True, False], ptr, hw, hb_)
            W1, W2 = w1.t().contiguous().requires_grad_(), w2.t().contiguous().requires_grad_()
            plan = ops.BatchPlan.cached(adj, ptr, 64, _lib.SGX_BATCH_BACKWARD)
            assert plan.fits
            pooled = ops.GcnStack.apply(adj, fea, ptr, plan, (True, False), W1, W2)
            (pooled * torch.linspace(-1, 1, pooled.numel(), device=DEV).view_as(pooled)).sum().backward()
            outs.append((logits, pooled.detach(), W1.grad, W2.grad))
        for a, b in zip(*outs):
            assert same(a, b)


def _model(train_stack=True):
    from sgracex1_amd import molecule_gcn as M, pynq_shim
    ip = pynq_shim.Overlay("gnn_all.bit").mmult_top_0
    ip.register_map.layer_count = 2
    return M.GCN_PYNQ(64, 7, 2, ip, train_stack=train_stack).to(DEV)


def _train(loader, epochs, graphs_moved):
    """Per-step loss tensors of GCN_PYNQ(train_stack=True) trained through `loader`, Adam lr 0.01."""
    torch.manual_seed(777)
    model = _model()
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    crit = torch.nn.CrossEntropyLoss()
    losses = []
    for epoch in range(epochs):
        model.train()
        for b in loader:
            if graphs_moved:
                b = b.to(DEV)
            opt.zero_grad()
            loss = crit(model(1, b.x, b.edge_index, b.batch), b.y)
            loss.backward()
            opt.step()
            losses.append(loss.detach())
    return losses, model


def test_five_epochs_of_training_give_the_same_losses():
    graphs = _mutag_graphs()
    dl, gl = _pair(graphs, 64, 2024)
    host, mh = _train(dl, 5, True)
    dev, md = _train(gl, 5, False)
    assert len(host) == len(dev) == 5 * 3
    assert same(torch.stack(host), torch.stack(dev))
    for (na, pa), (nb, pb) in zip(mh.named_parameters(), md.named_parameters()):
        assert same(pa.detach(), pb.detach()), na
    # and the eval forward (layer_count 2: one sgx_stack_forward) on a loader batch matches the host batch's
    mh.eval()
    md.eval()
    for hb, db in zip(*_pair(graphs, 64, 5)):
        hb = hb.to(DEV)
        with torch.no_grad():
            assert same(mh(1, hb.x, hb.edge_index, hb.batch), md(1, db.x, db.edge_index, db.batch))


def test_a_graph_over_the_budget_falls_back_as_before():
    from sgracex1_amd import _lib, ops, pyg_lite as G
    graphs = _random_graphs(11, 12, 20)
    # a 100-row ring: over the backward budget at width 64 (80 rows), within the forward one (128)
    ring = torch.arange(100)
    big = G.Graph(torch.eye(7)[ring % 7], torch.stack([torch.cat([ring, (ring + 1) % 100]), torch.cat([(ring + 1) % 100, ring])]),
                  torch.tensor([1]))
    graphs.insert(3, big)
    dl = G.DataLoader(graphs, batch_size=len(graphs))
    gl = G.GraphLoader(graphs, batch_size=len(graphs), device=DEV)
    hb, db = next(iter(dl)).to(DEV), next(iter(gl))
    adj = ops.recorded(db.edge_index, ("adj_csr", db.num_nodes, torch.float16))
    plan = ops.BatchPlan.cached(adj, ops.recorded(db.batch, ("graph_ptr",)), 64, _lib.SGX_BATCH_BACKWARD)
    assert not plan.fits and plan.max_graph == 100 and plan.groups == 0
    results = []
    for b in (hb, db):
        torch.manual_seed(3)
        model = _model()
        model.train()
        loss = torch.nn.functional.cross_entropy(model(1, b.x, b.edge_index, b.batch), b.y)
        loss.backward()
        results.append([loss.detach()] + [p.grad for p in model.parameters() if p.grad is not None])   # (conv biases: unused)
    assert len(results[0]) == len(results[1]) == 5
    for a, b in zip(*results):
        assert same(a, b)


def test_an_epoch_does_not_synchronise():
    from sgracex1_amd import pyg_lite as G
    graphs = _mutag_graphs()
    gl = G.GraphLoader(graphs, batch_size=64, shuffle=True, generator=torch.Generator().manual_seed(8), device=DEV)
    torch.manual_seed(1)
    model = _model().train()
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    crit = torch.nn.CrossEntropyLoss()

    def epoch():
        for b in gl:
            opt.zero_grad()
            crit(model(1, b.x, b.edge_index, b.batch), b.y).backward()
            opt.step()

    epoch()                                               # warm-up: first launches, allocator growth
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        epoch()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


def test_collation_and_trusted_plan_capture_and_replay():
    from sgracex1_amd import _lib, ops, pyg_lite as G
    graphs = _random_graphs(21, 200, 30)
    gs = ops.GraphSet(graphs, DEV)
    idx = torch.randperm(len(graphs), generator=torch.Generator().manual_seed(3))[:77].numpy()
    index = gs.prepare(idx)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = ops.collate_graphs(gs, index)
        want = ops.collate_graphs(gs, index)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in [getattr(out, f) for f in ops.Collated.FIELDS] + list(out.adj_val.values()) + list(out.fea_val.values()):
        if t.numel():
            bits(t).fill_(-1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.collate_graphs(gs, index, out=out)
        plan = ops.BatchPlan.known(out.graph_ptr, index.n_rows, torch.float16, index.max_graph, 64, _lib.SGX_BATCH_BACKWARD)
    graph.replay()
    torch.cuda.synchronize()
    for f in ops.Collated.FIELDS:
        assert same(getattr(out, f), getattr(want, f)), f
    assert same(out.adj_val[torch.float16], want.adj_val[torch.float16])
    assert same(out.fea_val[torch.float16], want.fea_val[torch.float16])
    hb = G.collate([graphs[i] for i in idx]).to(DEV)
    ref = ops.BatchPlan(ops.csr_from_edge_index(hb.edge_index, hb.num_nodes), ops.graph_ptr_of(hb.batch), 64,
                        _lib.SGX_BATCH_BACKWARD)
    assert (plan.rows, plan.groups, plan.max_graph, plan.fits) == (ref.rows, ref.groups, ref.max_graph, ref.fits)
    assert torch.equal(plan.export_groups(), ref.export_groups())
    del graph

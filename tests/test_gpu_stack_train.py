"""sgx_stack_backward on the GPU (include/sgx.h, "training"): every G_l and handed-down gradient bit-equal to the
chained kernels the model's layer-by-layer backward runs, dW within the fp32 reordering bound of the chained weight
gradient and within a magnitude bound of the float64 restatement (tests/_stack_grad_ref.py), deterministic; the
fallbacks; the model's train_stack path; a captured step."""
import os

import numpy as np
import pytest
import torch

from _stack_grad_ref import stack_grad_bound, stack_grad_f64

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
UNIT = {torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -24}
U32 = 2.0 ** -24


def bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def _mutag(device=DEV):
    from sgracex1_amd import pyg_lite as G
    raw = np.load(os.path.join(GOLD, "mutag_raw.npz"))
    graphs = G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])
    return G.collate(graphs).to(device)


def _dense_np(x):
    from sgracex1_amd import ops
    if not isinstance(x, ops.Csr):
        return x.double().cpu().numpy()
    out = np.zeros((x.n_rows, x.n_cols))
    rp, c, v = x.rowptr.cpu().numpy(), x.col.cpu().numpy(), x.val.double().cpu().numpy()
    row = np.repeat(np.arange(x.n_rows), np.diff(rp))
    np.add.at(out, (row, c[:len(row)]), v[:len(row)])
    return out


def chain_grad(adj, x, weights, relus, ptr, outs, grad_pooled):
    """The backward as the model's layer-by-layer path runs it, with unplanned kernels: sgx_readout_mean_backward, then
    per layer from the top the ReLU mask, A . g (fp32 adjacency), X^T . G (sgx_xt_g, or the aggregation over X^T for
    CSR features) and G . W^T cast to dtype.  Returns (dW list, G list, handed-down g list)."""
    from sgracex1_amd import ops
    dtype = adj.val.dtype
    N = adj.n_rows
    A32 = adj.to(torch.float32)
    g = ops.readout_mean_backward(grad_pooled, ptr, N, dtype)
    L = len(weights)
    dWs, Gs, gs = [None] * L, [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        if relus[l]:
            ops.relu_mask_backward_(outs[l].contiguous(), g)
        gs[l] = g
        G = ops.spmm(A32, g.float().contiguous(), use_plan=False).contiguous()
        Gs[l] = G
        if l == 0 and isinstance(x, ops.Csr):
            dWs[l] = ops.spmm(ops.csr_transpose(x.to(torch.float32)), G, use_plan=False)
        else:
            X = x if l == 0 else outs[l - 1]
            dWs[l] = ops.xt_g(X.contiguous(), G)
        if l > 0:
            g = ops.xw_dense(G, weights[l].float().contiguous()).contiguous().to(dtype)
    return dWs, Gs, gs


def check_grads(adj, x, weights, relus, ptr, outs, grad_pooled, plan=None):
    """sgx_stack_backward against the chain (G bit for bit, dW within the reordering bound), against the float64
    restatement, and against itself (a second call)."""
    from sgracex1_amd import ops
    dtype = adj.val.dtype
    dW, G = ops.gcn_stack_backward(adj, x, weights, relus, ptr, outs, grad_pooled, plan=plan, want_G=True)
    cW, cG, _ = chain_grad(adj, x, weights, relus, ptr, outs, grad_pooled)
    N = adj.n_rows
    X_abs = [np.abs(_dense_np(x))] + [np.abs(D.double().cpu().numpy()) for D in outs[:-1]]
    for l in range(len(weights)):
        assert same_bits(G[l], cG[l]), f"G_{l}: {(G[l] - cG[l]).abs().max().item()}"
        assert torch.isfinite(dW[l]).all()
        mag = X_abs[l].T @ np.abs(cG[l].double().cpu().numpy())
        bound = 2 * max(N - 1, 1) * U32 * mag + 1e-30
        err = np.abs(dW[l].double().cpu().numpy() - cW[l].double().cpu().numpy())
        assert (err <= bound).all(), f"dW_{l}: {float((err / bound).max())}"
    # the float64 restatement, on the device's layer outputs (their zeros are the masks)
    adj_np = (adj.rowptr.cpu().numpy(), adj.col.cpu().numpy(), adj.val.double().cpu().numpy())
    outs_np = [D.double().cpu().numpy() if D is not None else np.zeros((N, w.shape[1])) for D, w in zip(outs, weights)]
    if not relus[-1]:
        outs_np[-1] = np.ones_like(outs_np[-1])                         # (unmasked; the value is never read)
    ws_np = [w.double().cpu().numpy() for w in weights]
    gp = grad_pooled.double().cpu().numpy()
    ref, _ = stack_grad_f64(adj_np, _dense_np(x), ws_np, relus, ptr.cpu().numpy(), gp, outs=outs_np)
    bounds = stack_grad_bound(adj_np, _dense_np(x), ws_np, ptr.cpu().numpy(), gp, outs_np, UNIT[dtype])
    for l in range(len(weights)):
        err = np.abs(dW[l].double().cpu().numpy() - ref[l])
        assert (err <= bounds[l]).all(), f"dW_{l} vs f64: {float((err / bounds[l]).max())}"
    again = ops.gcn_stack_backward(adj, x, weights, relus, ptr, outs, grad_pooled, plan=plan)
    assert all(same_bits(a, b) for a, b in zip(again, dW))
    return dW


def forward_outs(adj, x, weights, relus, ptr, plan=None):
    from sgracex1_amd import ops
    dtype = adj.val.dtype
    wts = [w.t().to(dtype).contiguous() for w in weights]
    pooled, outs = ops.gcn_stack_forward(adj, x, wts, relus, ptr, want_layer_outputs=True, plan=plan)
    return pooled, outs


# ---- MUTAG ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_mutag_backward_against_the_chain(dtype):
    from sgracex1_amd import _lib, molecule_gcn as M, ops
    b = _mutag()
    adj = ops.csr_from_edge_index(b.edge_index, b.num_nodes, dtype=dtype)
    fea = M.as_csr(b.x, dtype)
    ptr = ops.graph_ptr_of(b.batch)
    torch.manual_seed(11)
    weights = [torch.randn(7, 64, device=DEV) * 0.4, torch.randn(64, 64, device=DEV) * 0.15]
    plan = ops.BatchPlan.cached(adj, ptr, 64, _lib.SGX_BATCH_BACKWARD)
    assert plan.fits and plan.kind == _lib.SGX_BATCH_BACKWARD and plan.max_graph == 28
    pooled, outs = forward_outs(adj, fea, weights, [True, False], ptr, plan)
    gp = torch.randn(188, 64, device=DEV) * 0.1
    check_grads(adj, fea, weights, [True, False], ptr, outs, gp, plan)
    # the handed-down gradient: the chain's g_0 (after the mask) is what the fused G_0 aggregated
    _, cG, cg = chain_grad(adj, fea, weights, [True, False], ptr, outs, gp)
    assert cg[0].dtype == dtype


# ---- seeded random block-diagonal batches ---------------------------------------------------------------------------
def random_batch(seed, dtype, sizes, m_in, sparse, density=0.3):
    from sgracex1_amd import ops
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    off = 0
    for g, n in enumerate(sizes):
        if g > 0 and n > 0:
            m = rng.random((n, n)) < min(density, 6.0 / max(n, 1) + 0.05)
            m[rng.random(n) < 0.1] = False                          # isolated rows
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


CASES = [  # widths (m_in, P_1 .. P_n), relus, sparse layer 0
    ((7, 64, 64), (1, 0), True),
    ((7, 16), (1,), False),
    ((16, 100, 7), (0, 1), False),
    ((100, 64, 100, 16, 64), (1, 1, 0, 1), True),
    ((64, 256), (1,), False),
    ((256, 7, 256, 64), (0, 1, 1), True),
    ((1433, 16, 7), (1, 0), True),                  # a Cora-wide CSR layer 0 (the slow sparse path)
    ((7, 256, 256, 256, 256), (1, 1, 1, 0), False),
]


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_random_batches_against_the_chain(dtype, case):
    from sgracex1_amd import _lib, ops
    widths, relus, sparse = CASES[case]
    relus = [bool(r) for r in relus]
    seed = 200 * case + (dtype == torch.float16)
    rng = np.random.default_rng(seed)
    width = max(widths[1:] + (() if sparse else widths[:1]))
    R = _budget(dtype, width)
    assert R >= 16
    sizes = [int(s) for s in rng.integers(1, R + 1, 40)] + [R, 1, 0]
    sizes[0] = 5                                                     # graph 0: no edges
    sizes[3] = 0                                                     # an empty graph
    adj, x, ptr = random_batch(seed, dtype, sizes, widths[0], sparse)
    weights = [torch.tensor(rng.standard_normal((m, p)) / np.sqrt(m), device=DEV, dtype=torch.float32)
               for m, p in zip(widths[:-1], widths[1:])]
    plan = ops.BatchPlan.cached(adj, ptr, width, _lib.SGX_BATCH_BACKWARD)
    assert plan.fits and plan.max_graph == R
    _, outs = forward_outs(adj, x, weights, relus, ptr, plan)
    gp = torch.tensor(rng.standard_normal((len(sizes), widths[-1])), device=DEV, dtype=torch.float32)
    check_grads(adj, x, weights, relus, ptr, outs, gp, plan)


def _budget(dtype, width, kind=1):
    from sgracex1_amd import ops
    one = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    adj = ops.Csr(torch.tensor([0, 0], dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
                  torch.zeros(0, dtype=dtype, device=DEV), 1)
    return ops.BatchPlan(adj, one, width, kind).rows


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_more_groups_than_the_grid(dtype):
    """20 000 graphs: every workgroup of the persistent grid adds many groups into its slice."""
    from sgracex1_amd import _lib, ops
    rng = np.random.default_rng(77)
    sizes = [int(s) for s in rng.integers(0, 24, 20000)]
    adj, x, ptr = random_batch(78, dtype, sizes, 7, True)
    weights = [torch.tensor(rng.standard_normal((7, 64)) * 0.4, device=DEV, dtype=torch.float32),
               torch.tensor(rng.standard_normal((64, 32)) * 0.15, device=DEV, dtype=torch.float32)]
    plan = ops.BatchPlan.cached(adj, ptr, 64, _lib.SGX_BATCH_BACKWARD)
    assert plan.fits and plan.groups > 2 * 512
    _, outs = forward_outs(adj, x, weights, [True, True], ptr, plan)
    gp = torch.tensor(rng.standard_normal((len(sizes), 32)), device=DEV, dtype=torch.float32)
    check_grads(adj, x, weights, [True, True], ptr, outs, gp, plan)


# ---- forward on a backward plan -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_forward_on_a_backward_plan_gives_the_same_bits(dtype):
    from sgracex1_amd import _lib, ops
    rng = np.random.default_rng(9)
    R = _budget(dtype, 100)
    sizes = [int(s) for s in rng.integers(0, R + 1, 300)]
    adj, x, ptr = random_batch(10, dtype, sizes, 21, False)
    wts = [torch.tensor(rng.standard_normal((100, 21)) / 5, device=DEV).to(dtype),
           torch.tensor(rng.standard_normal((64, 100)) / 10, device=DEV).to(dtype)]
    hw, hb = torch.randn(3, 64, device=DEV), torch.randn(3, device=DEV)
    fwd = ops.BatchPlan(adj, ptr, 100)
    bwd = ops.BatchPlan(adj, ptr, 100, _lib.SGX_BATCH_BACKWARD)
    assert bwd.rows < fwd.rows and bwd.fits and fwd.fits and bwd.groups != fwd.groups
    (la, pa), oa = ops.gcn_stack_forward(adj, x, wts, [True, False], ptr, hw, hb, want_layer_outputs=True,
                                         want_pooled=True, plan=fwd)
    (lb, pb), ob = ops.gcn_stack_forward(adj, x, wts, [True, False], ptr, hw, hb, want_layer_outputs=True,
                                         want_pooled=True, plan=bwd)
    assert same_bits(la, lb) and same_bits(pa, pb) and all(same_bits(a, b) for a, b in zip(oa, ob))


# ---- fallbacks ------------------------------------------------------------------------------------------------------
def _status(fn):
    from sgracex1_amd import _lib
    with pytest.raises(_lib.SgxError) as e:
        fn()
    return e.value.status


def test_unsupported_batches_are_refused_by_the_c_call():
    from sgracex1_amd import _lib, ops
    dtype = torch.float16
    R = _budget(dtype, 64)
    # a graph over the backward budget (within the forward's)
    assert _budget(dtype, 64, 0) > R
    adj, x, ptr = random_batch(3, dtype, [4, R + 1, 6], 7, True)
    weights = [torch.randn(7, 64, device=DEV), torch.randn(64, 64, device=DEV)]
    plan = ops.BatchPlan(adj, ptr, 64, _lib.SGX_BATCH_BACKWARD)
    assert not plan.fits
    _, outs = forward_outs(adj, x, weights, [True, False], ptr)
    gp = torch.randn(3, 64, device=DEV)
    assert _status(lambda: ops.gcn_stack_backward(adj, x, weights, [True, False], ptr, outs, gp, plan=plan)) == -3
    # a forward plan
    adj, x, ptr = random_batch(4, dtype, [4, 9, 6], 7, True)
    _, outs = forward_outs(adj, x, weights, [True, False], ptr)
    fplan = ops.BatchPlan(adj, ptr, 64)
    assert _status(lambda: ops.gcn_stack_backward(adj, x, weights, [True, False], ptr, outs, gp, plan=fplan)) == -3
    # a width over 256
    wide = [torch.randn(7, 300, device=DEV), torch.randn(300, 8, device=DEV)]
    _, outs = forward_outs(adj, x, wide, [True, False], ptr)
    assert _status(lambda: ops.gcn_stack_backward(adj, x, wide, [True, False], ptr, outs, torch.randn(3, 8, device=DEV))) == -3


def _count(monkeypatch):
    from sgracex1_amd import ops
    calls = {"fwd": 0, "bwd": 0}
    real_f, real_b = ops.gcn_stack_forward, ops.gcn_stack_backward

    def f(*a, **k):
        calls["fwd"] += 1
        return real_f(*a, **k)

    def b(*a, **k):
        calls["bwd"] += 1
        return real_b(*a, **k)
    monkeypatch.setattr(ops, "gcn_stack_forward", f)
    monkeypatch.setattr(ops, "gcn_stack_backward", b)
    return calls


def _model(train_stack=True, layer_count=2):
    from sgracex1_amd import molecule_gcn as M, pynq_shim
    ip = pynq_shim.Overlay("gnn_all.bit").mmult_top_0
    ip.register_map.layer_count = layer_count
    return M.GCN_PYNQ(64, 7, 2, ip, train_stack=train_stack).to(DEV)


def _step(model, x, ei, batch, y):
    model.train()
    model.zero_grad(set_to_none=True)
    loss = torch.nn.functional.cross_entropy(model(1, x, ei, batch), y)
    loss.backward()
    return loss


def test_model_falls_back_layer_by_layer(monkeypatch):
    from sgracex1_amd import ops
    b = _mutag()
    calls = _count(monkeypatch)
    model = _model()
    ptr = ops.graph_ptr_of(b.batch)
    # a crossing edge
    u, v = int(ptr[0]), int(ptr[1])
    ei = torch.cat([b.edge_index, torch.tensor([[u, v], [v, u]], device=DEV)], 1)
    _step(model, b.x, ei, b.batch, b.y)
    # an unsorted batch
    _step(model, b.x, b.edge_index, (b.num_graphs - 1) - b.batch, b.y)
    # features that need a gradient
    _step(model, b.x.clone().requires_grad_(True), b.edge_index, b.batch, b.y)
    # a graph over the backward budget: MUTAG's graphs joined into chains of 4 (up to 4 x 28 rows > 80)
    joined = torch.div(b.batch, 4, rounding_mode="floor")
    ptr4 = ops.graph_ptr_of(joined)
    assert int((ptr4[1:] - ptr4[:-1]).max()) > _budget(torch.float16, 64)
    _step(model, b.x, b.edge_index, joined, b.y[: int(joined.max()) + 1])
    assert calls == {"fwd": 0, "bwd": 0}
    # train_stack off, layer_count 2: layer by layer as before
    model.train_stack = False
    _step(model, b.x, b.edge_index, b.batch, b.y)
    assert calls == {"fwd": 0, "bwd": 0}
    # and on: one fused forward and one fused backward per step
    model.train_stack = True
    for k in range(1, 3):
        _step(model, b.x, b.edge_index, b.batch, b.y)
        assert calls == {"fwd": k, "bwd": k}


def test_model_step_matches_the_layer_by_layer_step(monkeypatch):
    """Same weights, same RNG state: the same loss bits, the same head gradients, conv gradients within the item-4
    bound 2 (n - 1) u32 (|X_l|^T |G_l|) of the layer-by-layer step's."""
    from sgracex1_amd import molecule_gcn as M, ops
    b = _mutag()
    seen = []
    real = ops.gcn_stack_backward

    def recording(*a, **k):
        seen.append(a[6].detach().clone())                            # grad_pooled
        return real(*a, **k)
    monkeypatch.setattr(ops, "gcn_stack_backward", recording)
    ref, fused = _model(train_stack=False), _model(train_stack=True)
    fused.load_state_dict(ref.state_dict())
    torch.manual_seed(4)
    l_ref = _step(ref, b.x, b.edge_index, b.batch, b.y)
    torch.manual_seed(4)
    l_fused = _step(fused, b.x, b.edge_index, b.batch, b.y)
    assert len(seen) == 1
    assert same_bits(l_ref.detach(), l_fused.detach())
    assert same_bits(ref.lin.weight.grad, fused.lin.weight.grad) and same_bits(ref.lin.bias.grad, fused.lin.bias.grad)
    adj = ops.csr_from_edge_index(b.edge_index, b.num_nodes, dtype=M.ACC_DTYPE)
    ptr = ops.graph_ptr_of(b.batch)
    fea = M.as_csr(b.x, M.ACC_DTYPE)
    weights = [ref.conv1.weight.detach(), ref.conv2.weight.detach()]
    _, outs = forward_outs(adj, fea, weights, [True, False], ptr)
    _, cG, _ = chain_grad(adj, fea, weights, [True, False], ptr, outs, seen[0])
    X_abs = [np.abs(_dense_np(fea)), np.abs(outs[0].double().cpu().numpy())]
    N = b.num_nodes
    for l, (cr, cf) in enumerate(((ref.conv1, fused.conv1), (ref.conv2, fused.conv2))):
        assert cf.weight.grad is not None and cf.weight.grad.shape == cr.weight.grad.shape
        bound = 2 * (N - 1) * U32 * (X_abs[l].T @ np.abs(cG[l].double().cpu().numpy())) + 1e-30
        err = (cf.weight.grad - cr.weight.grad).abs().double().cpu().numpy()
        assert (err <= bound).all(), float((err / bound).max())
        assert (cf.bias.grad is None) == (cr.bias.grad is None)


def test_sixty_epochs_reach_the_notebook_accuracy(monkeypatch):
    """examples/molecule_gcn_train.py --layer-count 2 --train-stack, inline: best test accuracy >= 0.74."""
    from sgracex1_amd import pyg_lite as G
    raw = np.load(os.path.join(GOLD, "mutag_raw.npz"))
    graphs = G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])
    torch.manual_seed(12345)
    graphs = [graphs[i] for i in torch.randperm(len(graphs)).tolist()]
    train, test = G.collate(graphs[:2000]).to(DEV), G.collate(graphs[50:100]).to(DEV)
    calls = _count(monkeypatch)
    model = _model()
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    crit = torch.nn.CrossEntropyLoss()
    best = 0.0
    for epoch in range(60):
        model.train()
        opt.zero_grad()
        loss = crit(model(1, train.x, train.edge_index, train.batch), train.y)
        loss.backward()
        opt.step()
        model.eval()
        with torch.no_grad():
            pred = model(1, test.x, test.edge_index, test.batch).argmax(1)
        best = max(best, float((pred == test.y).float().mean()))
    assert calls["bwd"] == 60
    assert best >= 0.74, best


def test_captured_step_replays_to_the_eager_bits():
    from sgracex1_amd import _lib, molecule_gcn as M, ops
    b = _mutag()
    model = _model()
    model.eval()                                                     # no dropout: the replay must repeat the bits
    adj = ops.cached_on(b.edge_index, ("adj_csr", b.num_nodes, M.ACC_DTYPE),
                        lambda: ops.csr_from_edge_index(b.edge_index, b.num_nodes, dtype=M.ACC_DTYPE))
    ptr = ops.graph_ptr_of(b.batch)
    plan = ops.BatchPlan.cached(adj, ptr, 64, _lib.SGX_BATCH_BACKWARD)
    fea = M.feature_csr(b.x, M.ACC_DTYPE)
    w1, w2 = model.conv1.weight, model.conv2.weight
    gp = torch.randn(188, 64, device=DEV)

    def step():
        w1.grad = w2.grad = None
        pooled = ops.GcnStack.apply(adj, fea, ptr, plan, (True, False), w1, w2)
        pooled.backward(gp)
        return pooled.detach(), w1.grad, w2.grad

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            eager = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(s)
    w1.grad = w2.grad = None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert all(same_bits(a, e) for a, e in zip(out, eager))

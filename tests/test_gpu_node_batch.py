"""Layer-ready node batches on the GPU (sgx_node_batch_sample, ops.sample_node_batch, NeighborLoader(prepare=...)): bit
for bit against the restatement of the rule (tests/_node_batch_ref.py), against today's host path, through the demo
model, and a training epoch without a synchronisation."""
import importlib.util
import os
import time

import numpy as np
import pytest
import torch

import _node_batch_ref as NB
import _sampler_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")
REL = 2.0 ** -21          # tests/test_node_batch_cpu.py: the rounding count of the rule


def _host(A):
    return A.rowptr.cpu().numpy().astype(np.int64), A.col[:A.nnz].cpu().numpy().astype(np.int64)


def _np(t):
    return t.cpu().numpy()


def _features(n, f=24, seed=5):
    rng = np.random.default_rng(seed)
    x = ((rng.random((n, f)) < 0.15) * rng.random((n, f))).astype(np.float32)
    x[::17] = 0                                             # all-zero feature rows
    return x


def _prepared(A, seeds, fanouts, seed, step, fill, x=None, y=None, masks=(), fea=None, weight=None):
    from sgracex1_amd import ops
    return ops.sample_node_batch(A, torch.as_tensor(np.asarray(seeds, np.int64), device=DEV), fanouts, seed=seed, step=step,
                                 fill=fill, features=fea, y=y, masks=masks, edge_weight=weight)


def _check(A, seeds, fanouts, seed=0, step=0, fill=0, host=None, x=None, fea=None, weight=None, host_path=True):
    """One prepared batch against the restatement (exact, values bit for bit), against a second run (identical bits) and
    against today's host path (structure equal, values within 2 x 2^-21)."""
    from sgracex1_amd import ops, sgrace
    rowptr, col = host or _host(A)
    n = A.n_rows
    y = torch.arange(n, device=DEV, dtype=torch.int64) * 3 + 1
    masks = [(torch.arange(n, device=DEV) % 3 == 0), (torch.arange(n, device=DEV) % 5 == 1)]
    s = _prepared(A, seeds, fanouts, seed, step, fill, y=y, masks=masks, fea=fea, weight=weight)
    n_id, rp, oc, pos, hn, he = R.sample(rowptr, col, seeds, fanouts, seed=seed, step=step)
    assert s.hop_nodes == hn and s.hop_edges == he
    assert np.array_equal(_np(s.n_id), n_id) and np.array_equal(_np(s.adj.rowptr), rp)
    assert np.array_equal(_np(s.adj.col[:s.adj.nnz]), oc) and np.array_equal(_np(s.edge_pos), pos)
    w = None if weight is None else _np(weight)[pos]
    q_ptr, q_col, q_val, dead, has_dead, max_row = NB.sym_norm2_csr(rp, oc, w, fill)
    N = s.adj_norm
    assert N.n_rows == len(n_id) and N.nnz == len(q_col)
    assert np.array_equal(_np(N.rowptr), q_ptr) and np.array_equal(_np(N.col[:N.nnz]), q_col)
    assert np.array_equal(_np(N.val[:N.nnz]).view(np.int32), q_val.view(np.int32))           # the rule pins the rounding
    assert np.array_equal(_np(N._dead_row_mask), dead) and N._dead_rows == has_dead and N._max_row == max_row
    tgt = np.repeat(np.arange(len(n_id)), np.diff(rp))
    assert np.array_equal(_np(s.edge_index_agg), np.stack([tgt, oc])) and np.array_equal(_np(s.edge_index), np.stack([oc, tgt]))
    assert np.array_equal(_np(s.y), n_id * 3 + 1)
    assert np.array_equal(_np(s.masks[0]), n_id % 3 == 0) and np.array_equal(_np(s.masks[1]), n_id % 5 == 1)
    if fea is not None:
        f_ptr, f_col, f_val = NB.gather_csr(*NB.dense_to_csr(x), n_id)
        assert np.array_equal(_np(s.fea.rowptr), f_ptr) and np.array_equal(_np(s.fea.col[:s.fea.nnz]), f_col)
        assert np.array_equal(_np(s.fea.val[:s.fea.nnz]).view(np.int32), f_val.view(np.int32))
        if len(n_id):
            want = ops.Csr.from_dense(ops.pack_rows(torch.as_tensor(x, device=DEV), s.n_id))
            assert torch.equal(want.rowptr, s.fea.rowptr) and torch.equal(want.col[:want.nnz], s.fea.col[:s.fea.nnz])
            assert torch.equal(want.val[:want.nnz], s.fea.val[:s.fea.nnz])
    again = _prepared(A, seeds, fanouts, seed, step, fill, y=y, masks=masks, fea=fea, weight=weight)
    for a, b in ((again.adj_norm.rowptr, N.rowptr), (again.adj_norm.col, N.col), (again.adj_norm.val, N.val),
                 (again.adj_norm._dead_row_mask, N._dead_row_mask), (again.n_id, s.n_id)):
        assert torch.equal(a, b)
    if host_path and len(n_id):
        s0 = ops.sample_neighbors(A, torch.as_tensor(np.asarray(seeds, np.int64), device=DEV), fanouts, seed=seed, step=step)
        A0 = s0.adj
        target = torch.repeat_interleave(torch.arange(A0.n_rows, device=DEV), (A0.rowptr[1:] - A0.rowptr[:-1]).long())
        ei = torch.stack([target, A0.col[:A0.nnz].long()])
        wt = None if weight is None else weight[s0.edge_pos.long()]
        ei2, norm = sgrace.sym_norm2(ei, A0.n_rows, edge_weight=wt, fill=fill, dtype=torch.float32)
        H = sgrace._edge_csr(None, ei2, norm, A0.n_rows, torch.float32)
        assert torch.equal(H.rowptr, N.rowptr) and torch.equal(H.col[:H.nnz], N.col[:N.nnz])
        a, b = _np(H.val[:H.nnz]).astype(np.float64), q_val.astype(np.float64)
        assert (np.abs(a - b) <= 2 * REL * np.abs(b)).all(), float(np.abs(a - b).max())
        assert torch.equal(H.dead_rows, N._dead_row_mask) and H.has_dead_rows == N._dead_rows
    return s


def _seeds(n, b, seed):
    return np.random.default_rng(seed).permutation(n)[:b]


@pytest.mark.parametrize("fanouts", [[10], [15, 10, 5], [-1], [65]])
@pytest.mark.parametrize("kind", ["uniform", "rmat"])
def test_prepared_batch_equals_the_restatement_and_the_host_path(kind, fanouts):
    from sgracex1_amd import graphs, ops
    if kind == "uniform":
        A = graphs.uniform_graph(20000, 200000, seed=3, dtype=torch.float32, normalize=False)
    else:
        A = graphs.rmat_graph(14, 150000, seed=4, dtype=torch.float32, normalize=False)
    x = _features(A.n_rows)
    fea = ops.feature_csr(torch.as_tensor(x, device=DEV))
    b = 300 if fanouts != [-1] else 100
    for fill in (0, 1):
        _check(A, _seeds(A.n_rows, b, 1), fanouts, seed=5, step=2, fill=fill, x=x, fea=fea)


def _hub_graph():
    from sgracex1_amd import graphs
    rng = np.random.default_rng(0)
    n = 1000
    rows = [list(rng.integers(0, n, rng.integers(0, 30))) for _ in range(n)]
    rows[0] = list(rng.integers(0, n, 70000))                    # a hub: degree > 2^16
    rows[7] = []                                                 # isolated seeds
    rows[8] = []
    rows[9] = [9, 9, 9, 3, 3, 10]                                # self loops, repeated edges
    rows[10] = [9, 11, 0]
    rows[11] = [10, 10]
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.asarray([c for r in rows for c in r], np.int64)
    A = graphs.csr_from_numpy(rowptr, col, np.ones(len(col), np.float32), n, dtype=torch.float32)
    return A, rowptr, col


def test_hub_isolated_self_loops_and_repeats_with_weights():
    from sgracex1_amd import ops
    A, rowptr, col = _hub_graph()
    x = _features(A.n_rows)
    fea = ops.feature_csr(torch.as_tensor(x, device=DEV))
    weight = torch.as_tensor((np.random.default_rng(1).integers(1, 17, len(col)) / 8).astype(np.float32), device=DEV)
    seeds = [0, 7, 9, 10, 11, 8, 500]
    for fanouts in ([10], [15, 10, 5], [-1], [65]):
        for fill in (0, 3):
            _check(A, seeds, fanouts, seed=11, step=1, fill=fill, host=(rowptr, col), x=x, fea=fea)
    _check(A, seeds, [15, 10, 5], seed=11, step=2, fill=1, host=(rowptr, col), x=x, fea=fea, weight=weight, host_path=False)
    # the 70 000-entry hub row through the workgroup path: one call, timed alone (the host restatement is not)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s = _prepared(A, seeds, [-1], 11, 0, 0)
    torch.cuda.synchronize()
    took = time.perf_counter() - t0
    print(f"hub row under [-1]: {took * 1e3:.1f} ms, longest row {s.adj_norm._max_row}")
    assert s.adj_norm._max_row >= 70000 and took < 5.0


def test_empty_seed_list_and_a_batch_of_every_node():
    from sgracex1_amd import graphs, ops
    A = graphs.uniform_graph(5000, 40000, seed=6, dtype=torch.float32, normalize=False)
    x = _features(A.n_rows)
    fea = ops.feature_csr(torch.as_tensor(x, device=DEV))
    s = _check(A, [], [10, 5], x=x, fea=fea)
    assert s.n_id.numel() == 0 and s.adj_norm.nnz == 0 and s.adj_norm.rowptr.tolist() == [0] and s.fea.rowptr.tolist() == [0]
    _check(A, np.random.default_rng(2).permutation(5000), [5, 5], seed=1, fill=1, x=x, fea=fea)
    _check(A, np.arange(5000), [-1], seed=1, x=x, fea=fea)


def test_fp16_values_are_the_rounded_fp32_ones():
    from sgracex1_amd import graphs, ops
    A = graphs.uniform_graph(20000, 200000, seed=3, dtype=torch.float32, normalize=False)
    x = _features(A.n_rows)
    fea = ops.feature_csr(torch.as_tensor(x, device=DEV))
    seeds = torch.as_tensor(_seeds(A.n_rows, 300, 1), device=DEV)
    a = ops.sample_node_batch(A, seeds, [10, 10], seed=2, step=3, features=fea)
    b = ops.sample_node_batch(A, seeds, [10, 10], seed=2, step=3, features=fea, dtype=torch.float16)
    assert torch.equal(a.adj_norm.col, b.adj_norm.col) and torch.equal(a.adj_norm.val.half(), b.adj_norm.val)
    assert torch.equal(a.fea.val.half(), b.fea.val) and torch.equal(a.adj_norm._dead_row_mask, b.adj_norm._dead_row_mask)


def _planted(n=2000, seed=1):
    spec = importlib.util.spec_from_file_location("sgrace_nc", os.path.join(ROOT, "examples", "sgrace_node_classification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    x, ei, y = mod.planted_partition(n, 5, 200, 0.02, 0.002, seed, DEV)
    return mod, x, ei, y


def _train_mask(n):
    train = torch.zeros(n, dtype=torch.bool, device=DEV)
    train[torch.randperm(n, generator=torch.Generator().manual_seed(1))[: n // 5].to(DEV)] = True
    return train


def test_prepared_loader_batches_are_the_default_loaders():
    from sgracex1_amd import ops, pyg_lite
    _, x, ei, y = _planted()
    train = _train_mask(x.shape[0])
    data = pyg_lite.NodeData(x, ei, y, train_mask=train, test_mask=~train)
    kw = dict(batch_size=128, input_nodes=train, shuffle=True, seed=4)
    for a, b in zip(pyg_lite.NeighborLoader(data, [10, 10], **kw), pyg_lite.NeighborLoader(data, [10, 10], prepare="sym_norm2", **kw)):
        for name in ("x", "y", "train_mask", "test_mask", "n_id", "edge_index", "input_id"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        assert torch.equal(a.adj.rowptr, b.adj.rowptr) and torch.equal(a.adj.col, b.adj.col)
        assert (a.batch_size, a.num_sampled_nodes, a.num_sampled_edges) == (b.batch_size, b.num_sampled_nodes, b.num_sampled_edges)
        assert torch.equal(b.edge_index_agg, a.edge_index.flip(0))
        hit = ops.recorded(b.edge_index_agg, ("sym_norm2", b.num_nodes, 1, torch.float32))
        assert hit is not None and hit[2] is b.adj_norm
        assert ops.recorded(b.x, ("fea_csr", torch.float32)) is not None


def test_demo_model_on_prepared_batches_matches_the_default_loader():
    """GAT_PYNQ in eval() on every batch of one epoch, GCN and GAT: prepared loader against default loader, same weights,
    by the criterion of test_gpu_sampler.py::test_demo_model_on_loader_batches_matches_the_dense_twin."""
    from sgracex1_amd import config, pyg_lite, sgrace
    _, x, ei, y = _planted()
    train = _train_mask(x.shape[0])
    old = config.snapshot()
    try:
        for attention in (0, 1):
            config.acc, config.device, config.compute_attention = 1, "cuda", attention
            config.fake_quantization = config.hardware_quantize = 0
            config.w_qbits, config.float_type = 32, np.float32
            sgrace.init_SGRACE()
            torch.manual_seed(0)
            model = sgrace.GAT_PYNQ(x.shape[1], 16, 1, 5).to(DEV)
            model.eval()
            data = pyg_lite.NodeData(x, ei, y, train_mask=train)
            plain = pyg_lite.NeighborLoader(data, [10, 10], batch_size=128, input_nodes=train, seed=2)
            ready = pyg_lite.NeighborLoader(data, [10, 10], batch_size=128, input_nodes=train, seed=2, prepare="sym_norm2")
            with torch.no_grad():
                a = torch.cat([model(b.x, b.edge_index.flip(0)).cpu() for b in plain])
                b = torch.cat([model(b.x, b.edge_index_agg).cpu() for b in ready])
            assert a.shape[0] > 4 * 128
            assert torch.isclose(a, b, rtol=1e-3, atol=1e-3).float().mean() >= 0.999, float((a - b).abs().max())
            assert (a.argmax(1) == b.argmax(1)).float().mean() > 0.98
    finally:
        config.restore(old)
        sgrace.init_SGRACE()


@pytest.mark.parametrize("attention", [False, True])
def test_example_with_device_batches_learns(attention):
    """The settings and the floor of test_gpu_sampler.py::test_example_minibatch_mode_learns, with --device-batches."""
    from sgracex1_amd import config, sgrace
    mod, *_ = _planted(n=200)
    old = config.snapshot()
    try:
        res, _, _ = mod.run(attention, 32, epochs=20, acc=1, n=2000, verbose=False, batch_size=128, num_neighbors=[10, 10],
                            device_batches=True)
        print(res)
        assert res["batches_per_epoch"] == 4
        assert res["test_acc"] > 0.9, res
    finally:
        config.restore(old)
        sgrace.init_SGRACE()


def _epoch_under_sync_error(attention, lean, prepare):
    from sgracex1_amd import config, pyg_lite, sgrace
    _, x, ei, y = _planted()
    train = _train_mask(x.shape[0])
    config.acc, config.device, config.compute_attention = 1, "cuda", int(attention)
    config.gat_edge_outputs = 0 if lean else 1
    config.fake_quantization = config.hardware_quantize = 0
    config.w_qbits, config.float_type = 32, np.float32
    sgrace.init_SGRACE()
    torch.manual_seed(1)
    model = sgrace.GAT_PYNQ(x.shape[1], 16, 1, 5).to(DEV).train()
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    crit = torch.nn.CrossEntropyLoss()
    loader = pyg_lite.NeighborLoader(pyg_lite.NodeData(x, ei, y, train_mask=train), [10, 10], batch_size=128, input_nodes=train,
                                     shuffle=True, seed=3, prepare=prepare)

    def epoch():
        for b in loader:
            opt.zero_grad()
            if prepare:
                out = model(b.x, b.edge_index_agg)
            else:
                out = model(b.x, b.edge_index.flip(0))
            crit(out[:b.batch_size], b.y[:b.batch_size]).backward()
            opt.step()

    epoch()                                               # warm-up: first launches, allocator growth
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        epoch()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("attention,lean", [(False, False), (True, False), (True, True)])
def test_a_training_epoch_on_prepared_batches_does_not_synchronise(attention, lean):
    """The device of test_gpu_graph_loader.py::test_an_epoch_does_not_synchronise: loader, forward, loss, backward and Adam
    under torch.cuda.set_sync_debug_mode("error").  The same loop through the default loader raises."""
    from sgracex1_amd import config, sgrace
    old = config.snapshot()
    try:
        _epoch_under_sync_error(attention, lean, "sym_norm2")
        with pytest.raises(RuntimeError):
            _epoch_under_sync_error(attention, lean, None)
    finally:
        torch.cuda.set_sync_debug_mode(0)
        config.restore(old)
        sgrace.init_SGRACE()


def _tiny_graph(n=40, seed=3):
    """40 nodes, 150 edges i -> j, none into nodes 0..2 -> (n, edge_index [2, E] int64 on the host, the CSR on the targets
    as NeighborLoader builds it: rowptr, col)."""
    rng = np.random.default_rng(seed)
    m = rng.random((n, n)) < 0.1
    m[:, :3] = False
    src, dst = np.nonzero(m)
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(dst, minlength=n), out=rowptr[1:])
    return n, torch.as_tensor(np.stack([src, dst])), rowptr, src[np.argsort(dst * n + src, kind="stable")].astype(np.int64)


def _bits(t):
    return _np(t.contiguous().view(torch.uint8)).tobytes()


def _live_columns(T, n):
    """The CSR `T` without the entries of columns >= n (what filler rows add to a transposed matrix) -> rowptr, col, val."""
    rowptr, col, val = _np(T.rowptr).astype(np.int64), _np(T.col[:T.nnz]), T.val[:T.nnz]
    keep = col < n
    kept = np.concatenate([[0], np.cumsum(keep)])
    return kept[rowptr], col[keep], _bits(val[torch.as_tensor(keep, device=val.device)])


@pytest.mark.parametrize("fanouts", [[3, 2], [3, 0]])
@pytest.mark.parametrize("dtype,bits", [(torch.float32, None), (torch.float16, None), (torch.float32, 8)], ids=["f32", "f16", "f32-q8"])
def test_padded_loader_batch_carries_the_unpadded_batches_attachments(dtype, bits, fanouts):
    """One hand-over for both kinds of batch: NeighborLoader(prepare="sym_norm2", transposed=True) with pad=True attaches,
    for the same seeds and step, the same entries under the same keys as without -- ("fea_csr", dtype), ("fea_csr", float32),
    ("fea_csr_t", float32), ("sym_norm2", n, 1, dtype) with n each batch's own size, adj_norm._transpose_pattern and the
    keys of adj_norm._quantized -- and every one holds the unpadded batch's bits on its live part: the first rows and entries
    by loader.counts of a matrix over the batch's rows, the entries of the live columns of a transposed one.  Seed 1 has no
    in-edge (a row without a sampled neighbour); under [3, 0] the last hop samples no edge."""
    from sgracex1_amd import ops, pyg_lite, quant
    F32 = torch.float32
    n_nodes, ei, rowptr, col = _tiny_graph()
    seeds, step = [1, 17, 30, 8], 5
    n_id, rp, _, _, hop_nodes, hop_edges = R.sample(rowptr, col, seeds, fanouts, seed=7, step=step)
    assert np.diff(rp)[0] == 0 and (hop_edges[2] == hop_edges[1]) == (fanouts[1] == 0)      # the two cases, by the restatement
    x = torch.as_tensor(_features(n_nodes, f=8, seed=2), device=DEV)       # (rows 0, 17 and 34 all zero; 17 is a seed)
    data = pyg_lite.NodeData(x, ei.to(DEV), torch.arange(n_nodes, device=DEV) % 5, train_mask=torch.arange(n_nodes, device=DEV) % 2 == 0,
                             val_mask=torch.arange(n_nodes, device=DEV) % 3 == 0)
    kw = dict(batch_size=len(seeds), seed=7, prepare="sym_norm2", transposed=True, dtype=dtype, fill=1,
              quant=None if bits is None else quant.constants(bits))
    plain, padded = pyg_lite.NeighborLoader(data, fanouts, **kw), pyg_lite.NeighborLoader(data, fanouts, pad=True, **kw)
    seeds_dev = torch.as_tensor(seeds, device=DEV)
    u = plain._prepared(seeds_dev, None, step)
    assert padded.padded(seeds_dev)
    padded.load(seeds_dev, step)
    p = padded.padded_batch(None)
    padded.status()
    n, e, a, f = padded.counts[:4].tolist()
    N = padded.capacity.n_rows
    assert (n, e, a, f) == (u.num_real_nodes, sum(u.num_sampled_edges), u.adj_norm.nnz, ops.recorded(u.x, ("fea_csr", dtype)).nnz)
    assert np.array_equal(_np(u.n_id), n_id) and u.num_sampled_edges[-1] == hop_edges[2] - hop_edges[1] and p.num_nodes == N > n

    def same_prefix(P, U, rows, entries):
        assert U.n_rows == rows and U.nnz == entries
        assert _bits(P.rowptr[:rows + 1]) == _bits(U.rowptr) and _bits(P.col[:entries]) == _bits(U.col[:entries])
        assert P.val.dtype == U.val.dtype and _bits(P.val[:entries]) == _bits(U.val[:entries])

    def same_live_columns(P, U):
        assert P.n_rows == U.n_rows and P.val.dtype == U.val.dtype
        (p_ptr, p_col, p_val), (u_ptr, u_col, u_val) = _live_columns(P, n), _live_columns(U, n)
        assert np.array_equal(p_ptr, u_ptr) and u_ptr[-1] == U.nnz and np.array_equal(p_col, u_col) and p_val == u_val

    for key in [("fea_csr", dtype), ("fea_csr", F32)]:
        same_prefix(ops.recorded(p.x, key), ops.recorded(u.x, key), n, f)
        assert ops.recorded(p.x, key).n_cols == ops.recorded(u.x, key).n_cols == 8
    same_live_columns(ops.recorded(p.x, ("fea_csr_t", F32)), ops.recorded(u.x, ("fea_csr_t", F32)))
    hit_p, hit_u = ops.recorded(p.edge_index_agg, ("sym_norm2", N, 1, dtype)), ops.recorded(u.edge_index_agg, ("sym_norm2", n, 1, dtype))
    assert hit_p[0] is p.edge_index_agg and hit_u[0] is u.edge_index_agg and _bits(p.edge_index_agg[:, :e]) == _bits(u.edge_index_agg)
    assert hit_p[2] is p.adj_norm and hit_u[2] is u.adj_norm
    assert hit_p[1].dtype == hit_u[1].dtype == dtype and _bits(hit_p[1][:a]) == _bits(hit_u[1][:a])
    same_prefix(p.adj_norm, u.adj_norm, n, a)
    assert _bits(p.adj_norm.dead_rows[:n]) == _bits(u.adj_norm.dead_rows)
    (Pt, p_order), (Ut, u_order) = p.adj_norm._transpose_pattern, u.adj_norm._transpose_pattern
    same_prefix(Pt, Ut, n, a)                                       # (a filler row's entries all stand in its own column)
    assert _bits(p_order[:a]) == _bits(u_order[:a])
    assert list(p.adj_norm._quantized) == list(u.adj_norm._quantized) and bool(u.adj_norm._quantized) == (bits is not None)
    for key, Q in u.adj_norm._quantized.items():
        G = p.adj_norm._quantized[key]
        same_prefix(G, Q, n, a)
        same_prefix(G._lean_values, Q._lean_values, n, a)
        assert _bits(G.dead_rows[:n]) == _bits(Q.dead_rows)
    for name in ("x", "y", "train_mask", "val_mask", "n_id"):
        assert _bits(getattr(p, name)[:n]) == _bits(getattr(u, name)), name

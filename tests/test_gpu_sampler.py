"""The neighbour sampler on the GPU (sgx_sample_neighbors, ops.sample_neighbors) against the restatement of its rule in
tests/_sampler_ref.py, bit for bit; the NeighborLoader built on it; and the demo model trained on its batches."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import _sampler_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")


def _host(A):
    return A.rowptr.cpu().numpy().astype(np.int64), A.col[:A.nnz].cpu().numpy().astype(np.int64)


def _csr(rowptr, col):
    from sgracex1_amd import graphs
    return graphs.csr_from_numpy(rowptr, col, np.ones(len(col), np.float32), len(rowptr) - 1, dtype=torch.float32)


def _check(A, seeds, fanouts, seed=0, step=0, host=None):
    from sgracex1_amd import ops
    rowptr, col = host or _host(A)
    s = ops.sample_neighbors(A, torch.as_tensor(np.asarray(seeds, np.int64), device=DEV), fanouts, seed=seed, step=step)
    n_id, rp, oc, pos, hn, he = R.sample(rowptr, col, seeds, fanouts, seed=seed, step=step)
    assert s.hop_nodes == hn and s.hop_edges == he
    assert np.array_equal(s.n_id.cpu().numpy(), n_id)
    assert np.array_equal(s.adj.rowptr.cpu().numpy(), rp)
    assert np.array_equal(s.adj.col[:s.adj.nnz].cpu().numpy(), oc)
    assert np.array_equal(s.edge_pos.cpu().numpy(), pos)
    assert s.adj.n_rows == len(n_id) and s.adj.nnz == len(oc)
    return s


def _seeds(n, b, seed):
    return np.random.default_rng(seed).permutation(n)[:b]


@pytest.mark.parametrize("fanouts", [[10], [15, 10, 5], [-1], [100]])
@pytest.mark.parametrize("kind", ["uniform", "rmat"])
def test_sample_equals_the_restatement(kind, fanouts):
    from sgracex1_amd import graphs
    if kind == "uniform":
        A = graphs.uniform_graph(20000, 200000, seed=3, dtype=torch.float32, normalize=False)
    else:
        A = graphs.rmat_graph(14, 150000, seed=4, dtype=torch.float32, normalize=False)
    b = 300 if fanouts != [-1] else 100
    _check(A, _seeds(A.n_rows, b, 1), fanouts, seed=5, step=2)


def test_hub_isolated_and_neighbouring_seeds_self_loops_and_repeats():
    rng = np.random.default_rng(0)
    n = 1000
    rows = [list(rng.integers(0, n, rng.integers(0, 30))) for _ in range(n)]
    rows[0] = list(rng.integers(0, n, 70000))                    # a hub: degree > 2^16
    rows[7] = []                                                 # isolated seeds
    rows[8] = []
    rows[9] = [9, 9, 9, 3, 3, 10]                                # self loops, repeated edges
    rows[10] = [9, 11, 0]                                        # seeds 9, 10, 11 neighbours of each other
    rows[11] = [10, 10]
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.asarray([c for r in rows for c in r], np.int64)
    A = _csr(rowptr, col)
    seeds = [0, 7, 9, 10, 11, 8, 500]
    for fanouts in ([10], [15, 10, 5], [-1], [100], [2, 2], [64], [65]):
        for step in range(3):
            _check(A, seeds, fanouts, seed=11, step=step, host=(rowptr, col))


def test_empty_seed_list_and_a_batch_of_every_node():
    from sgracex1_amd import graphs
    A = graphs.uniform_graph(5000, 40000, seed=6, dtype=torch.float32, normalize=False)
    s = _check(A, [], [10, 5])
    assert s.n_id.numel() == 0 and s.adj.nnz == 0 and s.adj.rowptr.tolist() == [0]
    _check(A, np.random.default_rng(2).permutation(5000), [5, 5], seed=1)
    _check(A, np.arange(5000), [-1], seed=1)


def test_sample_properties_map_and_errors():
    from sgracex1_amd import graphs, ops
    from sgracex1_amd._lib import SgxError
    A = graphs.rmat_graph(13, 80000, seed=8, dtype=torch.float32, normalize=False)
    rowptr, col = _host(A)
    seeds = _seeds(A.n_rows, 400, 3)
    k = 10
    s = ops.sample_neighbors(A, torch.as_tensor(seeds, device=DEV), [k, 5], seed=9, step=4)
    n_id = s.n_id.cpu().numpy()
    rp, oc, pos = s.adj.rowptr.cpu().numpy(), s.adj.col[:s.adj.nnz].cpu().numpy(), s.edge_pos.cpu().numpy()
    assert np.array_equal(n_id[:len(seeds)], seeds) and len(set(n_id.tolist())) == len(n_id)
    assert np.array_equal(col[pos], n_id[oc])                    # every sampled edge exists in the graph
    for i, v in enumerate(seeds):
        deg = rowptr[v + 1] - rowptr[v]
        p = pos[rp[i]:rp[i + 1]]
        assert len(p) == min(deg, k) and len(set(p.tolist())) == len(p)
        assert ((p >= rowptr[v]) & (p < rowptr[v + 1])).all() and (np.diff(p) > 0).all()
    node_map = ops._node_maps[(DEV.index if DEV.index is not None else torch.cuda.current_device(),
                               torch.cuda.current_stream().cuda_stream)]
    assert bool((node_map == ops.SAMPLE_SENTINEL).all())         # back at the sentinel
    again = ops.sample_neighbors(A, torch.as_tensor(seeds, device=DEV), [k, 5], seed=9, step=4)
    assert torch.equal(again.n_id, s.n_id) and torch.equal(again.adj.col, s.adj.col) and torch.equal(again.edge_pos, s.edge_pos)
    other = ops.sample_neighbors(A, torch.as_tensor(seeds, device=DEV), [k, 5], seed=9, step=5)
    assert other.edge_pos.numel() != s.edge_pos.numel() or not torch.equal(other.edge_pos, s.edge_pos)
    for bad in ([3, 5, 3], [1, A.n_rows + 5], [-1, 2]):
        with pytest.raises(SgxError) as e:
            ops.sample_neighbors(A, torch.as_tensor(bad, device=DEV), [k])
        assert e.value.status == -8
        assert bool((node_map == ops.SAMPLE_SENTINEL).all())
    with pytest.raises(ValueError):
        ops.sample_neighbors(A, torch.as_tensor(seeds, device=DEV), [k, -2])


def test_products_shape_full_size():
    """The ogbn-products shape (2.45 M nodes, about 124 M edges, uniform), batch 1024, fan-outs [15, 10, 5]: equal to the
    restatement, which reads only the rows it samples from a host copy of the CSR."""
    from sgracex1_amd import graphs
    A = graphs.uniform_graph(2_450_000, 122_000_000, seed=12345, dtype=torch.float32, self_loops=True, normalize=False)
    assert A.nnz > 120_000_000
    host = _host(A)
    _check(A, _seeds(A.n_rows, 1024, 7), [15, 10, 5], seed=3, step=1, host=host)


def _planted(n=2000, seed=1):
    spec = importlib.util.spec_from_file_location("sgrace_nc", os.path.join(ROOT, "examples", "sgrace_node_classification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    x, ei, y = mod.planted_partition(n, 5, 200, 0.02, 0.002, seed, DEV)
    return mod, x, ei, y


def test_neighbor_loader_batches():
    from sgracex1_amd import pyg_lite
    _, x, ei, y = _planted()
    n = x.shape[0]
    g = torch.Generator().manual_seed(0)
    train = torch.rand(n, generator=g) < 0.3
    test = ~train
    data = pyg_lite.NodeData(x, ei, y, train_mask=train.to(DEV), test_mask=test.to(DEV))
    loader = pyg_lite.NeighborLoader(data, [10, 10], batch_size=128, input_nodes=data.train_mask, shuffle=True, seed=4)
    dense = torch.zeros((n, n), dtype=torch.int32)
    dense.index_put_((ei[1].cpu(), ei[0].cpu()), torch.ones(ei.shape[1], dtype=torch.int32), accumulate=True)
    for epoch in range(2):
        seen = []
        for batch in loader:
            B = batch.batch_size
            nid = batch.n_id
            seen.append(nid[:B])
            assert torch.equal(nid[:B], torch.nonzero(data.train_mask).reshape(-1)[batch.input_id])
            assert torch.equal(batch.x, x[nid]) and torch.equal(batch.y, y[nid])
            assert torch.equal(batch.train_mask, data.train_mask[nid]) and torch.equal(batch.test_mask, data.test_mask[nid])
            A = batch.adj
            # PyG orientation: row 0 = sampled neighbour, row 1 = the node it was sampled for; adj row = row 1
            deg = (A.rowptr[1:] - A.rowptr[:-1]).long()
            assert torch.equal(batch.edge_index[1], torch.repeat_interleave(torch.arange(A.n_rows, device=DEV), deg))
            assert torch.equal(batch.edge_index[0], A.col[:A.nnz].long())
            src, dst = nid[batch.edge_index[0]].cpu(), nid[batch.edge_index[1]].cpu()
            assert bool((dense[dst, src] > 0).all())              # every batch edge is an edge src -> dst of the graph
            # seeds: min(in-degree, 10) sampled neighbours each
            full = dense[nid[:B].cpu()].sum(1)
            assert torch.equal(deg[:B].cpu(), torch.clamp(full, max=10).long())
        seen = torch.cat(seen).sort().values
        assert torch.equal(seen, torch.nonzero(data.train_mask).reshape(-1))   # each input node exactly once
    assert len(loader) == (int(train.sum()) + 127) // 128


def test_demo_model_on_loader_batches_matches_the_dense_twin():
    """GAT_PYNQ in eval() mode (no dropout), one set of weights: the kernels (acc = 1) on every batch of one loader epoch
    against the reference's dense emulation (acc = 0) on the same batches, by the criterion of
    test_gpu_host.py::test_sgrace_demo_model_trains_on_the_kernels."""
    from sgracex1_amd import config, pyg_lite, sgrace
    _, x, ei, y = _planted()
    n = x.shape[0]
    train = torch.zeros(n, dtype=torch.bool, device=DEV)
    train[torch.randperm(n, generator=torch.Generator().manual_seed(1))[: n // 5].to(DEV)] = True
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
            loader = pyg_lite.NeighborLoader(pyg_lite.NodeData(x, ei, y, train_mask=train), [10, 10], batch_size=128,
                                             input_nodes=train, seed=2)
            batches = [(b.x, b.edge_index.flip(0)) for b in loader]
            assert len(batches) == 4
            with torch.no_grad():
                on_gpu = [model(bx, be).cpu() for bx, be in batches]
            config.acc, config.device = 0, "cpu"
            sgrace.init_SGRACE()
            twin = sgrace.GAT_PYNQ(x.shape[1], 16, 1, 5)
            twin.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
            twin.eval()
            with torch.no_grad():
                on_cpu = [twin(bx.cpu(), be.cpu()) for bx, be in batches]
            a, b = torch.cat(on_gpu), torch.cat(on_cpu)
            assert torch.isclose(a, b, rtol=1e-3, atol=1e-3).float().mean() >= 0.999, float((a - b).abs().max())
            assert (a.argmax(1) == b.argmax(1)).float().mean() > 0.98
    finally:
        config.restore(old)
        sgrace.init_SGRACE()


@pytest.mark.parametrize("attention", [False, True])
def test_example_minibatch_mode_learns(attention):
    """The example's mini-batch mode (batch 128, fan-out [10, 10]) on the planted-partition graph: full-graph test
    accuracy far above chance (0.2).  The first GPU run reached 0.996 (GCN) and 0.993 (GAT) after 20 epochs of 4 batches;
    the floor leaves margin below that (the full-batch test asserts > 0.93)."""
    from sgracex1_amd import config, sgrace
    mod, *_ = _planted(n=200)
    old = config.snapshot()
    try:
        res, _, _ = mod.run(attention, 32, epochs=20, acc=1, n=2000, verbose=False, batch_size=128, num_neighbors=[10, 10])
        print(res)
        assert res["batches_per_epoch"] == 4
        assert res["test_acc"] > 0.9, res
    finally:
        config.restore(old)
        sgrace.init_SGRACE()

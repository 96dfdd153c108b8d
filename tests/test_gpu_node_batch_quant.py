"""Node batches delivered ready for the quantised layers (sgx_node_batch_sample_quant, ops.sample_node_batch(quant=),
NeighborLoader(quant=)): the delivered arrays bit for bit against the existing quantiser kernel on the delivered fp32
values and against torch, the demo model on such batches bit for bit against the batches without them, a quantised
training epoch that synchronises nowhere, and the argument errors."""
import importlib.util
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import _node_batch_quant_ref as Q

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")


def _graph(name):
    from sgracex1_amd import graphs
    rowptr, col = Q.GRAPHS[name]()
    A = graphs.csr_from_numpy(rowptr, col, np.ones(len(col), np.float32), len(rowptr) - 1, dtype=torch.float32)
    w = Q.weights_of(name, len(col))
    return A, None if w is None else torch.as_tensor(w, device=DEV)


class _TwoScales:
    """Constants whose second layer reads the adjacency on another scale (the demo's layers share one): two sets."""

    def __init__(self, first, a_s2):
        self.first, self.second = first, replace(first.second_layer(), a_s=a_s2)
        self.w_qbits, self.a_s, self.a_z = first.w_qbits, first.a_s, first.a_z

    def second_layer(self):
        return self.second


def _check_delivered(s, sets, plain):
    """Every delivered array of one batch against the parent's path: the quantiser kernel over adj_norm.val, torch for the
    rest.  sets: the distinct constants delivered.  -> (dead rows, entries of live rows that rounded to 0), over the sets."""
    from sgracex1_amd import ops
    A = s.adj_norm
    for a, b in ((A.rowptr, plain.adj_norm.rowptr), (A.col, plain.adj_norm.col), (A.val, plain.adj_norm.val),
                 (A._dead_row_mask, plain.adj_norm._dead_row_mask), (s.n_id, plain.n_id)):
        assert torch.equal(a, b)                                   # the unquantised batch: the one sgx_node_batch_sample gives
    assert (A._dead_rows, A._max_row) == (plain.adj_norm._dead_rows, plain.adj_norm._max_row)
    assert len(A._quantized) == len(sets)
    lost = dead_count = 0
    val, row = A.val[:A.nnz], Q.rows_of(A.rowptr)
    for c in sets:
        D = A._quantized[(c.w_qbits, c.a_s, c.a_z)]
        assert A.quantized(c) is D                                 # what the layers look up
        assert D.rowptr is A.rowptr and D.n_rows == A.n_rows and D.n_cols == A.n_cols and D.nnz == A.nnz
        assert torch.equal(D.col[:D.nnz], A.col[:A.nnz])
        want = ops.fake_quantize(val.contiguous(), 0, c.w_qbits, c.a_s, c.a_z)
        assert torch.equal(D.val[:D.nnz].view(torch.int32), want.view(torch.int32))
        dead = Q.dead_rows(want, row, A.n_rows)
        assert torch.equal(D._dead_row_mask, dead)
        assert D._dead_rows is bool(dead.any()) and D._max_row == A._max_row
        lean = torch.where(dead[row], val, want)
        assert torch.equal(D._lean_values.val[:A.nnz].view(torch.int32), lean.view(torch.int32))
        assert D._lean_values.rowptr is A.rowptr and D._lean_values.nnz == A.nnz
        dead_count += int(dead.sum())
        lost += int(((want == 0) & (val > 0) & ~dead[row]).sum())
    return dead_count, lost


@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("f", [0, 1])
@pytest.mark.parametrize("name", ["seeded", "hub"])
def test_delivered_arrays_equal_the_quantiser_kernel_and_torch(name, f, fill):
    from sgracex1_amd import ops, quant
    A, w = _graph(name)
    seeds = torch.as_tensor(Q.SEEDS[name], device=DEV)
    kw = dict(seed=Q.SAMPLE_SEED, step=Q.SAMPLE_STEP, fill=fill, edge_weight=w)
    plain = ops.sample_node_batch(A, seeds, Q.FANOUTS[f], **kw)
    for bits in (8, 4, 2, 1):
        qc = quant.constants(bits)
        s = ops.sample_node_batch(A, seeds, Q.FANOUTS[f], quant=qc, **kw)
        dead, lost = _check_delivered(s, [qc], plain)              # the demo's two layers share the adjacency's constants
        print(f"{name} {Q.FANOUTS[f]} fill {fill} bits {bits}: rows {s.adj_norm.n_rows} nnz {s.adj_norm.nnz} dead {dead} lost {lost}")
        # not empty, as test_node_batch_quant_cpu.py shows from the restatement alone
        if fill == 0:
            assert 0 < dead < s.adj_norm.n_rows                    # the last hop's rows
        elif bits == 1:
            assert (lost > 0) == Q.LOSES[name, f]                  # a live row loses an entry to rounding
    # two constant sets in one call
    two = _TwoScales(quant.constants(4), 0.05)
    s = ops.sample_node_batch(A, seeds, Q.FANOUTS[f], quant=two, **kw)
    _check_delivered(s, [two.first, two.second], plain)
    a, b = (s.adj_norm.quantized(c).val for c in (two.first, two.second))
    assert not torch.equal(a, b)


def test_empty_seed_list_and_a_batch_of_every_node():
    from sgracex1_amd import ops, quant
    A, w = _graph("seeded")
    qc = quant.constants(2)
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    s = ops.sample_node_batch(A, none, [3, 2], quant=qc, edge_weight=w)
    D = s.adj_norm.quantized(qc)
    assert s.n_id.numel() == 0 and D.nnz == 0 and D._dead_rows is False and D._lean_values.nnz == 0
    assert D._dead_row_mask.numel() == 0
    every = torch.randperm(A.n_rows, generator=torch.Generator().manual_seed(2)).to(DEV)
    for fanouts, fill in (([3, 2], 1), ([-1], 0)):
        kw = dict(seed=1, fill=fill, edge_weight=w)
        s = ops.sample_node_batch(A, every, fanouts, quant=qc, **kw)
        assert s.adj_norm.n_rows == A.n_rows
        _check_delivered(s, [qc], ops.sample_node_batch(A, every, fanouts, **kw))


def _planted(n=1000, seed=1):
    spec = importlib.util.spec_from_file_location("sgrace_nc", os.path.join(ROOT, "examples", "sgrace_node_classification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.planted_partition(n, 5, 200, 0.02, 0.002, seed, DEV)


@pytest.fixture(scope="module")
def planted():
    x, ei, y = _planted()
    train = torch.zeros(x.shape[0], dtype=torch.bool, device=DEV)
    train[torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(1))[: x.shape[0] // 5].to(DEV)] = True
    return x, ei, y, train


def _configure(attention, lean, accb, bits):
    from sgracex1_amd import config, sgrace
    config.acc, config.device, config.compute_attention = 1, "cuda", int(attention)
    config.gat_edge_outputs, config.accb = (0 if lean else 1), int(accb)
    config.fake_quantization = config.hardware_quantize = 1         # as the example sets them for --qbits
    config.w_qbits, config.float_type = bits, np.float32
    sgrace.init_SGRACE()


def _outputs_and_gradients(planted, use_quant, batch_size, fanouts):
    """GAT_PYNQ on the first two batches of a loader: the eval() output of each, then the parameter gradients of one
    training step on each (dropout drawn from the same seed)."""
    from sgracex1_amd import pyg_lite, sgrace
    x, ei, y, train = planted
    torch.manual_seed(0)
    model = sgrace.GAT_PYNQ(x.shape[1], 16, 1, 5).to(DEV)
    loader = pyg_lite.NeighborLoader(pyg_lite.NodeData(x, ei, y, train_mask=train), fanouts, batch_size=batch_size,
                                     input_nodes=train, shuffle=True, seed=3, prepare="sym_norm2",
                                     quant=sgrace.quant_constants if use_quant else None)
    crit = torch.nn.CrossEntropyLoss()
    got = []
    for i, b in enumerate(loader):
        if i == 2:
            break
        assert bool(b.adj_norm._quantized) == use_quant
        model.eval()
        with torch.no_grad():
            got.append(model(b.x, b.edge_index_agg).clone())
        model.train()
        model.zero_grad()
        torch.manual_seed(5 + i)
        crit(model(b.x, b.edge_index_agg)[:b.batch_size], b.y[:b.batch_size]).backward()
        got += [p.grad.clone() for p in model.parameters() if p.grad is not None]
        dead = [D._dead_rows for D in b.adj_norm._quantized.values()]
    return got, dead


@pytest.mark.parametrize("accb", [0, 1])
@pytest.mark.parametrize("attention,lean", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("bits", [8, 1])
def test_model_on_quant_batches_equals_the_model_on_batches_without(planted, bits, attention, lean, accb):
    """Bit for bit: the delivered entries are what the layers would have built.  Batches of 16 x [3, 2] (fill 0: dead
    rows in every batch) and the example's 128 x [10, 10]."""
    from sgracex1_amd import config, sgrace
    old = config.snapshot()
    try:
        _configure(attention, lean, accb, bits)
        for batch_size, fanouts in ((16, [3, 2]), (128, [10, 10])):
            with_q, dead = _outputs_and_gradients(planted, True, batch_size, fanouts)
            without, _ = _outputs_and_gradients(planted, False, batch_size, fanouts)
            assert dead == [True]
            assert len(with_q) == len(without) >= 2 * (1 + 4)
            for k, (a, b) in enumerate(zip(with_q, without)):
                assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), (batch_size, k)
            assert all(bool(torch.isfinite(t).all()) for t in with_q) and any(bool((t != 0).any()) for t in with_q[1:])
    finally:
        config.restore(old)
        sgrace.init_SGRACE()


def _epoch_under_sync_error(planted, lean, use_quant):
    from sgracex1_amd import pyg_lite, sgrace
    x, ei, y, train = planted
    _configure(True, lean, 0, 8)
    torch.manual_seed(1)
    model = sgrace.GAT_PYNQ(x.shape[1], 16, 1, 5).to(DEV).train()
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    crit = torch.nn.CrossEntropyLoss()
    loader = pyg_lite.NeighborLoader(pyg_lite.NodeData(x, ei, y, train_mask=train), [10, 10], batch_size=64, input_nodes=train,
                                     shuffle=True, seed=3, prepare="sym_norm2",
                                     quant=sgrace.quant_constants if use_quant else None)

    def epoch():
        for b in loader:
            opt.zero_grad()
            crit(model(b.x, b.edge_index_agg)[:b.batch_size], b.y[:b.batch_size]).backward()
            opt.step()

    epoch()                                               # warm-up: first launches, allocator growth
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        epoch()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("lean", [False, True])
def test_a_quantised_training_epoch_on_quant_batches_does_not_synchronise(planted, lean):
    """Loader, quantised GAT forward, loss, backward and Adam under torch.cuda.set_sync_debug_mode("error"), the device of
    test_gpu_node_batch.py.  The same epoch through the prepared loader without quant= raises: the layers then read the
    quantised adjacency's dead-row flag back per batch."""
    from sgracex1_amd import config, sgrace
    old = config.snapshot()
    try:
        _epoch_under_sync_error(planted, lean, True)
        with pytest.raises(RuntimeError):
            _epoch_under_sync_error(planted, lean, False)
    finally:
        torch.cuda.set_sync_debug_mode(0)
        config.restore(old)
        sgrace.init_SGRACE()


def test_errors_leave_the_sampler_usable():
    from sgracex1_amd import _lib, ops, pyg_lite, quant
    A, w = _graph("seeded")
    seeds = torch.as_tensor(Q.SEEDS["seeded"], device=DEV)
    qc = quant.constants(8)
    before = ops.sample_node_batch(A, seeds, [3, 2], seed=4, edge_weight=w)
    with pytest.raises(ValueError, match="float32"):
        ops.sample_node_batch(A, seeds, [3, 2], seed=4, dtype=torch.float16, quant=qc)
    x = torch.rand(A.n_rows, 8, device=DEV)
    with pytest.raises(ValueError, match="float32"):
        pyg_lite.NeighborLoader(pyg_lite.NodeData(x, torch.zeros((2, 0), dtype=torch.int64, device=DEV)), [3],
                                prepare="sym_norm2", dtype=torch.float16, quant=qc)
    with pytest.raises(ValueError, match="prepare"):
        pyg_lite.NeighborLoader(pyg_lite.NodeData(x, torch.zeros((2, 0), dtype=torch.int64, device=DEV)), [3], quant=qc)
    with pytest.raises(_lib.SgxError) as e:
        ops.sample_node_batch(A, seeds, [3, 2], seed=4, edge_weight=w, quant=replace(qc, w_qbits=3))
    assert e.value.status == -2                                    # SGX_ERR_SHAPE
    # the node_map is as it was: an unquantised call on the same stream gives the same batch, and a quantised one works
    after = ops.sample_node_batch(A, seeds, [3, 2], seed=4, edge_weight=w)
    for a, b in ((after.n_id, before.n_id), (after.adj_norm.rowptr, before.adj_norm.rowptr),
                 (after.adj_norm.col, before.adj_norm.col), (after.adj_norm.val, before.adj_norm.val)):
        assert torch.equal(a, b)
    s = ops.sample_node_batch(A, seeds, [3, 2], seed=4, edge_weight=w, quant=qc)
    _check_delivered(s, [qc], before)

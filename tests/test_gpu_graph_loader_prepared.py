"""GraphLoader(prepare="sym_norm2", quant=) and sgx_collate_graphs_extras on the GPU, on the hand-made fixture of
tests/_graph_prep_ref.py (checked against torch on the CPU by tests/test_graph_loader_prepared_cpu.py): the delivered
normalised and quantised adjacencies, masks and flags bit for bit against the host path on the plain loader's batch;
every other tensor of the batch unchanged, K = 0 the old call's bytes; guard bands, a bad graph id and offsets over the
totals; a GAT_POOL_PYNQ(train_stack=True) step that synchronises nowhere (and does on a plain batch); the same training
through either loader; the fallbacks; the eval forward; the loader's argument errors."""
from unittest import mock

import numpy as np
import pytest
import torch

import _graph_prep_ref as P

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F16, F32 = torch.float16, torch.float32
SENTINEL = 0xA5
GUARD = 64


def bits(t):
    t = t.contiguous()
    return t.view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def _loaders(graphs=None, quant=None, dtypes=(F16, F32), **kw):
    """(plain, prepared) GraphLoaders over separate GraphSets of the same graphs."""
    from sgracex1_amd import pyg_lite as G
    graphs = P.torch_graphs() if graphs is None else graphs
    return (G.GraphLoader(graphs, device=DEV, dtypes=dtypes, **kw),
            G.GraphLoader(graphs, device=DEV, dtypes=dtypes, prepare="sym_norm2", quant=quant, **kw))


def _host_norm(b, dt):
    """What GAT_POOL_PYNQ.forward's normalise() builds for the batch."""
    from sgracex1_amd import sgrace
    ei, norm = sgrace.sym_norm2(b.edge_index, b.num_nodes)
    return sgrace._edge_csr(None, ei, norm, b.num_nodes, dt)


def _delivered(b, dt):
    from sgracex1_amd import ops
    hit = ops.recorded(b.edge_index, ("sym_norm2", b.num_nodes, 1, dt))
    assert hit is not None and hit[0] is b.edge_index and hit[1] is hit[2].val
    return hit[2]


def _same_csr(A, R, max_row):
    assert A.nnz == R.nnz and A.n_rows == R.n_rows and A.n_cols == R.n_cols
    assert same(A.rowptr, R.rowptr) and same(A.col[:A.nnz], R.col[:R.nnz]) and same(A.val[:A.nnz], R.val[:R.nnz])
    assert A._dead_rows is not None and A._dead_row_mask is not None            # facts, not computed on demand
    assert same(A.dead_rows, R.dead_rows) and A.has_dead_rows == R.has_dead_rows
    assert int((R.rowptr[1:] - R.rowptr[:-1]).max()) <= A._max_row == max_row


@pytest.mark.parametrize("nbits", [None, 8, 4, 2, 1])
def test_delivered_adjacencies_are_the_host_path_bit_for_bit(nbits):
    from sgracex1_amd import ops, quant
    qc = None if nbits is None else quant.constants(nbits)
    plain, prep = _loaders(quant=qc)
    fixture = P.fixture()
    dead_seen = killed_seen = False
    for ids in P.BATCHES:
        hb, pb = plain.collate(ids), prep.collate(ids)
        want = P.prepared_batch(fixture, ids)
        for dt in (F16, F32):
            A, R = _delivered(pb, dt), _host_norm(hb, dt)
            _same_csr(A, R, 23)                                         # the set's longest row: 21 repeats, a neighbour, a loop
            assert np.array_equal(A.rowptr.cpu().numpy(), want["rowptr"]) and np.array_equal(A.col.cpu().numpy(), want["col"])
            # (the pattern also against the CPU-checked restatement; the values only against the host path above: the
            # device's deg^-0.5 need not round as the CPU's)
            assert np.array_equal(A.dead_rows.cpu().numpy(), want["dead"])
            dead_seen |= A.has_dead_rows
        A, R = _delivered(pb, F32), _host_norm(hb, F32)
        assert _delivered(pb, F16).col is A.col                          # one pattern for both dtypes
        if qc is None:
            assert A._quantized == {}
            continue
        assert _delivered(pb, F16)._quantized == {}
        for c in (qc, qc.second_layer()):
            key = ops._adj_quant_key(c)
            assert key in A._quantized
            Q = A._quantized[key]
            assert Q.rowptr is A.rowptr and Q.col is A.col and A.quantized(c) is Q
            _same_csr(Q, R.quantized(c), 23)
            killed_seen |= bool((Q.dead_rows & ~A.dead_rows).any())
    assert dead_seen
    if nbits == 1:
        assert killed_seen


def _tensors(c):
    from sgracex1_amd import ops
    t = {f: getattr(c, f) for f in ops.Collated.FIELDS}
    for name in ("adj_val", "fea_val", "norm_val", "q_val", "q_dead"):
        for k, v in getattr(c, name).items():
            t[f"{name}/{k}"] = v
    if c.norm_rowptr is not None:
        t.update(norm_rowptr=c.norm_rowptr, norm_col=c.norm_col, norm_dead=c.norm_dead)
    return t


def _set_tensor(c, name, value):
    if "/" in name:
        field, key = name.split("/", 1)
        d = getattr(c, field)
        d[next(k for k in d if str(k) == key)] = value
    else:
        setattr(c, name, value)


def test_every_other_tensor_is_the_plain_loaders_and_k0_is_the_old_call():
    import ctypes
    from sgracex1_amd import _lib, ops, quant
    plain, prep = _loaders(quant=quant.constants(8))
    for ids in P.BATCHES:
        hb, pb = plain.collate(ids), prep.collate(ids)
        n = hb.num_nodes
        assert pb.num_graphs == hb.num_graphs == len(ids)
        for f in ("x", "edge_index", "batch", "y"):
            assert same(getattr(pb, f), getattr(hb, f)), f
        assert same(ops.recorded(pb.batch, ("graph_ptr",)), ops.recorded(hb.batch, ("graph_ptr",)))
        for dt in (F16, F32):
            for t, key in ((lambda b: b.edge_index, ("adj_csr", n, dt)), (lambda b: b.x, ("fea_csr", dt))):
                A, R = ops.recorded(t(pb), key), ops.recorded(t(hb), key)
                assert A.nnz == R.nnz and A.n_cols == R.n_cols and same(A.rowptr, R.rowptr)
                assert same(A.col[:A.nnz], R.col[:R.nnz]) and same(A.val[:A.nnz], R.val[:R.nnz])
        # both columns arrays are vouched for: trusted plans for the raw and for the normalised adjacency, both kinds
        gp = ops.recorded(pb.batch, ("graph_ptr",))
        for adj in (ops.recorded(pb.edge_index, ("adj_csr", n, F16)), _delivered(pb, F32)):
            for kind in (_lib.SGX_BATCH_FORWARD, _lib.SGX_BATCH_BACKWARD):
                p = ops.BatchPlan.cached(adj, gp, 64, kind)
                assert p is not None and getattr(p, "_group_graph", "untrusted") != "untrusted"
                q = ops.BatchPlan(adj, gp, 64, kind)
                assert (p.rows, p.groups, p.max_graph, p.fits) == (q.rows, q.groups, q.max_graph, q.fits)
                assert torch.equal(p.export_groups(), q.export_groups())
    # K = 0 through the new entry point: the old call's bytes
    gs = plain.graphs
    index = gs.prepare(P.PERMUTATION)
    old = ops.collate_graphs(gs, index, (F16, F32))
    new = ops.Collated(index, gs.n_feat, (F16, F32), DEV)
    for t in _tensors(new).values():
        bits(t).fill_(-1)
    b = ops._graph_batch(index, new, (F16, F32))
    assert _lib.lib.sgx_collate_graphs_extras(ctypes.byref(gs.desc), ctypes.byref(b), None, 0, ops._stream()) == 0
    torch.cuda.synchronize()
    for name, t in _tensors(old).items():
        assert same(t, _tensors(new)[name]), name


def _guarded(c):
    """Move every buffer of the Collated `c` into the middle of a sentinel-filled allocation with GUARD elements on each
    side; returns {name: the whole allocation as bytes}."""
    whole = {}
    for name, t in _tensors(c).items():
        es, nbytes = t.element_size(), t.numel() * t.element_size()
        big = torch.full((nbytes + 2 * GUARD * es,), SENTINEL, dtype=torch.uint8, device=DEV)
        _set_tensor(c, name, big[GUARD * es:GUARD * es + nbytes].view(t.dtype).view(t.shape))
        whole[name] = (big, GUARD * es)
    return whole


def _guards_intact(whole):
    for name, (big, g) in whole.items():
        assert bool((big[:g] == SENTINEL).all()) and bool((big[-g:] == SENTINEL).all()), name


def _owned(name, t, host, B, pos):
    """bool mask over t: the elements batch position `pos` writes (host: batch_offsets' array with five count arrays)."""
    off = lambda k: host[B + k * (B + 1):B + (k + 1) * (B + 1)]
    node, edge, adj, fea, norm = (off(k) for k in range(5))
    m = torch.zeros(t.shape, dtype=torch.bool, device=DEV)
    base = name.split("/")[0]
    if base in ("y", "graph_ptr"):
        m[pos] = True
    elif base == "edge_index":
        m[:, edge[pos]:edge[pos + 1]] = True
    elif base in ("adj_col", "adj_val"):
        m[adj[pos]:adj[pos + 1]] = True
    elif base in ("fea_col", "fea_val"):
        m[fea[pos]:fea[pos + 1]] = True
    elif base in ("norm_col", "norm_val", "q_val"):
        m[norm[pos]:norm[pos + 1]] = True
    else:                                       # x, batch, the row pointers (entry `row` belongs to the row's graph), masks
        assert base in ("x", "batch", "adj_rowptr", "fea_rowptr", "norm_rowptr", "norm_dead", "q_dead"), base
        m[node[pos]:node[pos + 1]] = True
    return m


@pytest.mark.parametrize("fault", [None, "graph_id", "negative_id", "norm_offset", "adj_offset"])
def test_guard_bands_and_skipped_graphs(fault):
    """Buffers between sentinel guards: nothing outside them is written; a graph whose id is outside the set, or one of whose
    ranges -- an extra's or the batch's own -- passes the totals, leaves its outputs unwritten and every other graph's as
    they are."""
    from sgracex1_amd import ops, quant
    qc = quant.constants(4)
    gs = ops.GraphSet(P.torch_graphs(), DEV)
    extras = gs.prepare_sym_norm2((F16, F32), qc)
    ids = np.array([3, 6, 4, 0, 2])
    pos = 1
    index = gs.prepare(ids)
    host, totals = ops.batch_offsets(gs.counts + (gs._sym_norm2.counts,), ids)
    B = len(ids)
    assert index.nnz_norm == totals[4] and len(extras.keys) >= 1
    good = ops.collate_graphs(gs, index, (F16, F32), extras=extras)
    bad = host.copy()
    if fault == "graph_id":
        bad[pos] = len(gs)
    elif fault == "negative_id":
        bad[pos] = -1
    elif fault == "norm_offset":
        bad[B + 4 * (B + 1) + pos] = totals[4]                               # its entries would end past nnz
    elif fault == "adj_offset":
        bad[B + 2 * (B + 1) + pos] = totals[2] + 1
    index = ops.BatchIndex(torch.from_numpy(bad).to(DEV), B, totals, index.max_graph, ids=ids)
    out = ops.Collated(index, gs.n_feat, (F16, F32), DEV, extras)
    whole = _guarded(out)
    assert ops.collate_graphs(gs, index, (F16, F32), out=out, extras=extras) is out
    torch.cuda.synchronize()
    _guards_intact(whole)
    want = _tensors(good)
    for name, t in _tensors(out).items():
        if fault is None:
            assert same(t, want[name]), name
            continue
        m = _owned(name, t, host, B, pos)
        assert bool(m.any()), name
        assert torch.equal(bits(t)[~m], bits(want[name])[~m]), name
        unwritten = torch.full((t.element_size(),), SENTINEL, dtype=torch.uint8, device=DEV).view(bits(t).dtype)
        assert bool((bits(t)[m] == unwritten).all()), name


def test_out_buffers_are_reused_and_refused_when_they_do_not_fit():
    from sgracex1_amd import ops, quant
    gs = ops.GraphSet(P.torch_graphs(), DEV)
    extras = gs.prepare_sym_norm2((F32,), quant.constants(8))
    first = ops.collate_graphs(gs, [1, 2, 3], (F32,), extras=extras)
    ptrs = {k: t.data_ptr() for k, t in _tensors(first).items()}
    again = ops.collate_graphs(gs, [3, 2, 1], (F32,), out=first, extras=extras)        # the same sizes, another order
    assert again is first and ptrs == {k: t.data_ptr() for k, t in _tensors(again).items()}
    fresh = ops.collate_graphs(gs, [3, 2, 1], (F32,), extras=extras)
    for k, t in _tensors(fresh).items():
        assert same(t, _tensors(again)[k]), k
    with pytest.raises(ValueError):
        ops.collate_graphs(gs, [1, 2, 4], (F32,), out=first, extras=extras)
    with pytest.raises(ValueError):                                                   # a Collated without extras
        ops.collate_graphs(gs, [3, 2, 1], (F32,), out=ops.collate_graphs(gs, [1, 2, 3], (F32,)), extras=extras)
    assert gs.prepare_sym_norm2((F32,), quant.constants(8)).prepared is extras.prepared   # built once per set


# ---- the model on prepared batches ------------------------------------------------------------------------------------
CASES = {"gcn": dict(compute_attention=0, fake_quantization=0), "gat": dict(compute_attention=1, fake_quantization=0),
         "gat8": dict(compute_attention=1, fake_quantization=1, w_qbits=8),
         "gat1": dict(compute_attention=1, fake_quantization=1, w_qbits=1)}


@pytest.fixture
def env():
    from sgracex1_amd import config, sgrace
    saved = config.snapshot()
    mode = torch.cuda.get_sync_debug_mode()

    def setup(case):
        config.acc, config.float_type = 1, np.float32
        for k, v in CASES[case].items():
            setattr(config, k, v)
        sgrace.init_SGRACE().register_map.layer_count = 2
        return sgrace.quant_constants
    yield setup
    torch.cuda.set_sync_debug_mode(mode)
    config.restore(saved)
    sgrace.init_SGRACE()


def _model(seed=11):
    from sgracex1_amd import sgrace
    torch.manual_seed(seed)
    return sgrace.GAT_POOL_PYNQ(P.N_FEAT, 64, 2, train_stack=True).to(DEV).train()


def _stack(case):
    from sgracex1_amd import ops
    return ops.QuantStack if CASES[case]["fake_quantization"] else ops.GatStack


def _connected():
    g = P.torch_graphs()
    return [g[i] for i in P.CONNECTED]


def _one_step(model, opt, b):
    opt.zero_grad()
    loss = torch.nn.functional.cross_entropy(model(b.x, b.edge_index, b.batch), b.y)
    loss.backward()
    opt.step()
    return loss.detach()


def _step_under_sync_error(case, setup, prepared):
    """A warm-up step on the epoch's first batch, then the second batch -- collation, forward, loss, backward, Adam --
    under set_sync_debug_mode("error"); returns how often the stack's apply ran inside it."""
    qc = setup(case)
    loaders = _loaders(_connected(), quant=qc, dtypes=(F32,), batch_size=3, shuffle=True,
                       generator=torch.Generator().manual_seed(1))
    it = iter(loaders[1 if prepared else 0])
    model = _model()
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    _one_step(model, opt, next(it))                                   # warm-up: first launches, allocator growth
    torch.cuda.synchronize()
    cls = _stack(case)
    with mock.patch.object(cls, "apply", wraps=cls.apply) as spy:
        torch.cuda.set_sync_debug_mode("error")
        try:
            _one_step(model, opt, next(it))
        finally:
            torch.cuda.set_sync_debug_mode(0)
        torch.cuda.synchronize()
        return spy.call_count


@pytest.mark.parametrize("case", ["gcn", "gat", "gat8"])
def test_a_train_stack_step_on_a_prepared_batch_does_not_synchronise(case, env):
    assert _step_under_sync_error(case, env, True) == 1
    if case != "gcn":
        # ... and the test measures something: the plain loader's batch reads the dead-row flag back
        with pytest.raises(RuntimeError):
            _step_under_sync_error(case, env, False)


def _train(case, setup, prepared, steps=3):
    qc = setup(case)
    loader = _loaders(_connected(), quant=qc, dtypes=(F32,), batch_size=3, shuffle=True,
                      generator=torch.Generator().manual_seed(5))[1 if prepared else 0]
    model = _model()
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    cls = _stack(case)
    losses = []
    with mock.patch.object(cls, "apply", wraps=cls.apply) as spy:
        while len(losses) < steps:
            for b in loader:
                if len(losses) < steps:
                    losses.append(_one_step(model, opt, b))
        assert spy.call_count == steps
    return torch.stack(losses), model


@pytest.mark.parametrize("case", ["gcn", "gat", "gat8"])
def test_three_steps_train_the_same_through_either_loader(case, env):
    la, ma = _train(case, env, False)
    lb, mb = _train(case, env, True)
    assert same(la, lb) and bool(torch.isfinite(la).all())
    compared = 0
    for (na, pa), (nb, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        if na in ("att1.bias", "att2.bias"):          # (GATConv_SGRACE's bias: allocated, never initialised, never added)
            continue
        assert na == nb and same(pa.detach(), pb.detach()), na
        compared += 1
    assert compared == 6                              # two weights, two attention vectors, the head's weight and bias


@pytest.mark.parametrize("why", ["dead_rows", "one_bit", "over_the_budget"])
def test_fallbacks_take_the_layers_and_give_the_plain_loaders_bits(why, env):
    case = "gat1" if why == "one_bit" else "gat"
    ids = {"dead_rows": [0, 1, 2, 6], "one_bit": P.CONNECTED, "over_the_budget": [7]}[why]
    results = []
    for prepared in (False, True):
        qc = env(case)
        b = _loaders(quant=qc, dtypes=(F32,))[int(prepared)].collate(ids)
        if prepared and why != "over_the_budget":
            A = _delivered(b, F32)
            assert (A if qc is None else A.quantized(qc)).has_dead_rows is True
        model = _model(3)
        cls = _stack(case)
        with mock.patch.object(cls, "apply", wraps=cls.apply) as spy:
            out = model(b.x, b.edge_index, b.batch)
            torch.nn.functional.cross_entropy(out, b.y).backward()
            assert spy.call_count == 0
        results.append([out.detach()] + [p.grad for p in model.parameters() if p.grad is not None])
    assert len(results[0]) == len(results[1]) >= 5
    for a, b in zip(*results):
        assert same(a, b)


@pytest.mark.parametrize("case", ["gcn", "gat", "gat8"])
def test_the_eval_forward_takes_the_stack_and_matches(case, env):
    from sgracex1_amd import ops
    name = "quant_stack_forward" if case == "gat8" else "gat_stack_forward"
    outs = []
    for prepared in (False, True):
        qc = env(case)
        b = _loaders(quant=qc, dtypes=(F32,))[int(prepared)].collate(P.CONNECTED)
        model = _model(4).eval()
        with mock.patch.object(ops, name, wraps=getattr(ops, name)) as spy, torch.no_grad():
            if prepared:
                torch.cuda.synchronize()
                torch.cuda.set_sync_debug_mode("error")
            try:
                outs.append(model(b.x, b.edge_index, b.batch))
            finally:
                torch.cuda.set_sync_debug_mode(0)
            assert spy.call_count == 1
    assert same(*outs) and bool(torch.isfinite(outs[0]).all())


def test_loader_argument_errors():
    from sgracex1_amd import pyg_lite as G, quant
    graphs, qc = _connected(), quant.constants(8)
    with pytest.raises(ValueError, match="quant needs prepare"):
        G.GraphLoader(graphs, device=DEV, quant=qc)
    with pytest.raises(ValueError, match="float32"):
        G.GraphLoader(graphs, device=DEV, prepare="sym_norm2", quant=qc, dtypes=(F16,))
    with pytest.raises(ValueError, match="prepare must be None or 'sym_norm2'"):
        G.GraphLoader(graphs, device=DEV, prepare="gcn_norm")
    assert len(G.GraphLoader(graphs, batch_size=3, device=DEV, prepare="sym_norm2", quant=qc, dtypes=(F16, F32))) == 2

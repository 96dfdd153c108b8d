"""Padded node batches on the device (include/sgx.h, "padded node batches"): sgx_node_batch_sample_padded against
sgx_node_batch_sample and the numpy restatement inside guard bands, its capture and replay on new seeds and a new step word,
the layers on a padded batch against the same batch unpadded, and train.NodeTrainer.capture_loader against eager steps."""
import copy

import numpy as np
import pytest
import torch

import _layer_grad_ref as LG
import _node_loss_ref as R
import _node_pad_ref as NP

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 37                                    # elements in front of and behind every output: odd, so no array is 16-byte aligned


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _graph(kind, seed=0):
    """-> (n_nodes, edge_index [2, E] int64 on the host, row 0 the source).  "complete": 6 nodes, every pair both ways, so
    fan-outs [5, 5] reach the whole graph from any seed; "isolated": nodes 0..7 have no in-edge; "repeated": every edge
    stored up to three times."""
    rng = np.random.default_rng(seed)
    if kind == "complete":
        n = 6
        src, dst = np.nonzero(~np.eye(n, dtype=bool))
    else:
        n = 230
        m = rng.random((n, n)) < 0.03
        np.fill_diagonal(m, rng.random(n) < 0.2)                     # some stored loops
        if kind == "isolated":
            m[:, :8] = False
        src, dst = np.nonzero(m)
        if kind == "repeated":
            rep = rng.integers(1, 4, len(src))
            src, dst = np.repeat(src, rep), np.repeat(dst, rep)
    return n, torch.as_tensor(np.stack([src, dst]))


def _csr(n, ei):
    from sgracex1_amd import ops
    dst, src = ei[1].to(DEV), ei[0].to(DEV)
    order = torch.argsort(dst * n + src, stable=True)
    return ops.Csr.from_coo(dst[order].to(torch.int32), src[order].to(torch.int32), torch.ones(order.numel(), device=DEV), n, n)


def _features(n, seed=1, width=24):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand((n, width), generator=g) < 0.3).float() * torch.rand((n, width), generator=g)
    x[min(3, n - 1)] = 0                                              # an empty feature row
    return x.to(DEV).contiguous()


def _guarded(buf):
    """Every output tensor of the NodePadBuffers `buf` moved into the middle of a sentinel-filled tensor -> the list of
    (name, whole tensor, copy of it) to compare after the calls."""
    bands = []
    names = ["n_id", "rowptr", "col", "pos", "n_rowptr", "n_col", "n_val", "dead", "ei", "ei_agg", "f_rowptr", "f_col", "f_val", "y",
             "status", "counts"]
    for name in names + [("masks", k) for k in range(len(buf.masks))]:
        t = buf.masks[name[1]] if isinstance(name, tuple) else getattr(buf, name)
        if t is None:
            continue
        whole = torch.empty(t.numel() + 2 * GUARD, dtype=t.dtype, device=DEV)
        whole.view(torch.uint8).fill_(0xA5)                          # (a NaN pattern in neither float type; a sentinel in all)
        view = whole[GUARD:GUARD + t.numel()]
        view.copy_(t)
        if isinstance(name, tuple):
            buf.masks[name[1]] = view
        else:
            setattr(buf, name, view)
        bands.append((name, whole, t.numel()))
    return bands


def _bands_intact(bands):
    for name, whole, k in bands:
        b = whole.view(torch.uint8).cpu().numpy()
        es = whole.element_size()
        assert (b[:GUARD * es] == 0xA5).all() and (b[(GUARD + k) * es:] == 0xA5).all(), name


def _np(t):
    return t.cpu().numpy()


def _expected(cap, u):
    """The numpy restatement's padded arrays of the unpadded NodeSample `u`."""
    c = dict(N=cap.n_rows, Ca=cap.nnz_norm, Cf=cap.nnz_fea, E=cap.n_edges)
    n, e = u.n_id.numel(), u.hop_edges[-1]
    A = u.adj_norm
    fea = (None, None, None) if u.fea is None else (_np(u.fea.rowptr), _np(u.fea.col[:u.fea.nnz]), _np(u.fea.val[:u.fea.nnz]))
    return NP.pad_batch(c, n, e, _np(u.n_id), _np(u.adj.rowptr), _np(u.adj.col[:e]), _np(u.edge_pos), _np(A.rowptr), _np(A.col[:A.nnz]),
                        _np(A.val[:A.nnz]), _np(A.dead_rows), _np(u.edge_index), _np(u.edge_index_agg), *fea,
                        None if u.y is None else _np(u.y), [_np(m) for m in u.masks])


def _assert_padded_equals(s, want, with_fea, with_y):
    got = dict(n_id=s.n_id, out_rowptr=s.out_rowptr, out_col=s.out_col, edge_pos=s.edge_pos, rowptr_norm=s.adj_norm.rowptr,
               col_norm=s.adj_norm.col, val_norm=s.adj_norm.val, dead=s.adj_norm.dead_rows, edge_index=s.edge_index,
               edge_index_agg=s.edge_index_agg)
    if with_fea:
        got.update(rowptr_fea=s.fea.rowptr, col_fea=s.fea.col, val_fea=s.fea.val)
    if with_y:
        got["y"] = s.y
    for name, t in got.items():
        g, w = _np(t), want[name]
        assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == w.tobytes(), name
    assert len(s.masks) == len(want["masks"])
    for g, w in zip(s.masks, want["masks"]):
        assert np.array_equal(_np(g), w)


CASES = [("complete", 2, [5, 5], torch.float32, True), ("complete", 2, [5, 5], torch.float16, False),
         ("isolated", 8, [3, 2], torch.float32, True), ("isolated", 8, [3, 2], torch.float16, True),
         ("repeated", 32, [5, 5], torch.float16, True), ("repeated", 13, [3, 2], torch.float32, False),
         ("repeated", 16, [63], torch.float32, True)]


@pytest.mark.parametrize("kind,batch,fan,dtype,extras", CASES)
def test_padded_call_against_the_unpadded_call_and_the_restatement(kind, batch, fan, dtype, extras):
    from sgracex1_amd import ops
    n, ei = _graph(kind, seed=batch)
    csr = _csr(n, ei)
    fea = ops.feature_csr(_features(n)) if extras else None
    y = torch.arange(n, device=DEV) % 5 + 1 if extras else None
    masks = [torch.arange(n, device=DEV) % 2 == 0, torch.arange(n, device=DEV) % 3 == 0] if extras else []
    seeds = torch.arange(batch, device=DEV) if kind == "isolated" else torch.randperm(n, generator=torch.Generator().manual_seed(4))[:batch].to(DEV)
    cap = ops.node_pad_capacity(csr, batch, fan, fea)
    want_cap = NP.capacity(n, csr.nnz, batch, fan, None if fea is None else _np(fea.rowptr[1:] - fea.rowptr[:-1]))
    assert (cap.n_rows, cap.nnz_norm, cap.nnz_fea, cap.n_edges) == tuple(want_cap[k] for k in ("N", "Ca", "Cf", "E"))
    buf = ops.NodePadBuffers(cap, n, dtype, DEV, None if fea is None else fea.n_cols, y is not None, len(masks))
    bands = _guarded(buf)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    for k in (5, 2 ** 40 + 3):                                       # two batches through the same buffers
        step.fill_(k)
        kw = dict(seed=11, fill=1 if k == 5 else 0, dtype=dtype, features=fea, y=y, masks=masks)
        s = ops.sample_node_batch(csr, seeds, fan, step=step, pad=cap, out=buf, **kw)
        u = ops.sample_node_batch(csr, seeds, fan, step=k, **kw)
        want = _expected(cap, u)
        _assert_padded_equals(s, want, fea is not None, y is not None)
        counts = _np(buf.counts).tolist()
        H = len(fan)
        assert counts[:4] == [u.n_id.numel(), u.hop_edges[-1], u.adj_norm.nnz, 0 if fea is None else u.fea.nnz]
        assert counts[4:5 + H] == list(u.hop_nodes) and counts[5 + H:] == list(u.hop_edges)
        assert int(buf.status) == 0
        # the consequences the header states
        lens = np.diff(want["rowptr_norm"])
        assert lens.max() <= max(max(fan) + 1, 64) == cap.max_row and want["rowptr_norm"][-1] == cap.nnz_norm == s.adj_norm.nnz
        assert s.adj_norm.has_dead_rows is True and not _np(s.adj_norm.dead_rows)[counts[0]:].any()
        if fea is not None:
            assert want["rowptr_fea"][-1] == cap.nnz_fea == s.fea.nnz and not s.fea.wants_plan
        assert not s.adj_norm.wants_plan
        if kind == "complete":
            assert counts[0] == n == cap.max_nodes                   # the batch reaches the whole graph: P = F
        if kind == "isolated":
            assert counts[:3] == [batch, 0, batch]                   # no edge: a = n
    assert (buf.node_map == ops.SAMPLE_SENTINEL).all()
    _bands_intact(bands)


def test_captured_call_replays_on_new_seeds_and_a_new_step_word():
    from sgracex1_amd import ops
    n, ei = _graph("repeated", seed=3)
    csr, fea = _csr(n, ei), ops.feature_csr(_features(n))
    y = torch.arange(n, device=DEV) % 7
    batch, fan = 16, [5, 5]
    cap = ops.node_pad_capacity(csr, batch, fan, fea)
    buf = ops.NodePadBuffers(cap, n, torch.float32, DEV, fea.n_cols, True, 0)
    bands = _guarded(buf)
    seeds = torch.arange(batch, device=DEV, dtype=torch.int32)
    step = torch.full((1,), 9, dtype=torch.int64, device=DEV)
    call = lambda: ops.sample_node_batch(csr, seeds, fan, seed=2, step=step, features=fea, y=y, pad=cap, out=buf)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                       # the side stream's workspace
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = call()
    first = {k: v.clone() for k, v in (("n_id", s.n_id), ("val", s.adj_norm.val))}
    for new_seeds, new_step in ((torch.arange(100, 100 + batch), 9), (torch.arange(batch), 10), (torch.arange(50, 50 + batch), 2 ** 33)):
        seeds.copy_(new_seeds)
        step.fill_(new_step)
        graph.replay()
        fresh = ops.sample_node_batch(csr, seeds.clone(), fan, seed=2, step=step.clone(), features=fea, y=y, pad=cap)
        for name in ("n_id", "out_rowptr", "out_col", "edge_pos", "edge_index", "edge_index_agg", "y"):
            assert same_bits(getattr(s, name), getattr(fresh, name)), name
        for a, b in ((s.adj_norm, fresh.adj_norm), (s.fea, fresh.fea)):
            assert same_bits(a.rowptr, b.rowptr) and same_bits(a.col, b.col) and same_bits(a.val, b.val)
        assert same_bits(s.adj_norm.dead_rows, fresh.adj_norm.dead_rows) and same_bits(buf.counts, fresh.counts)
        assert int(buf.status) == 0
    assert not same_bits(first["n_id"], s.n_id)                      # the replays did draw other batches
    # a repeated seed: the status word is set, the batch is one of filler rows only, nothing leaves the arrays
    seeds[3] = seeds[7]
    graph.replay()
    assert int(buf.status) == 1 and _np(buf.counts).tolist() == [0] * buf.counts.numel()
    assert (s.n_id == -1).all() and int(s.adj_norm.rowptr[-1]) == cap.nnz_norm and int(s.adj_norm.rowptr[0]) == 0
    assert (buf.node_map == ops.SAMPLE_SENTINEL).all()
    _bands_intact(bands)


@pytest.fixture(params=[(0, np.float32), (1, np.float32), (0, np.float16), (1, np.float16)], ids=["gcn-f32", "att-f32", "gcn-f16", "att-f16"])
def env(request):
    """accb = 0 on the kernels, unquantised; a 260-node planted-partition-like graph with labels and a training mask of 70
    nodes; a GAT_PYNQ in training mode and the loader arguments of the configuration (attention: transposed, fill = 1, so
    that no live row is dead -- a dead row's uniform softmax spans the padded width, the one documented difference)."""
    from sgracex1_amd import config, pyg_lite, sgrace
    gat, ft = request.param
    saved = config.snapshot()
    config.acc, config.accb, config.float_type, config.compute_attention = 1, 0, ft, gat
    config.fake_quantization = config.hardware_quantize = 0
    config.w_qbits, config.gat_edge_outputs, config.device = 32, 1, "cuda"
    sgrace.init_SGRACE()
    torch.manual_seed(5)
    n, ei = _graph("repeated", seed=8)
    x = _features(n, seed=9, width=40)
    y = (torch.arange(n) * 7 % 5).to(DEV)
    train_mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    train_mask[torch.randperm(n, generator=torch.Generator().manual_seed(2))[:70].to(DEV)] = True
    data = pyg_lite.NodeData(x, ei.to(DEV), y, train_mask=train_mask)
    model = sgrace.GAT_PYNQ(40, 16, 1, 5).to(DEV).train()
    kw = dict(batch_size=16, input_nodes=train_mask, shuffle=True, seed=3, prepare="sym_norm2", fill=1 if gat else 0,
              dtype=torch.float16 if ft == np.float16 else torch.float32, transposed=bool(gat))
    yield model, data, kw, gat
    config.restore(saved)
    sgrace.init_SGRACE()


def _reference_grads(model, b, H, gh64, e_gh, gat):
    """The layers' parameter gradients of the unpadded batch b in float64 (tests/_layer_grad_ref.py) for the head's gradient
    gh64 known to e_gh, with the bound the layer tests derive carried through both layers (tests/test_gpu_node_trainer.py)."""
    from sgracex1_amd import ops
    tol_of = dict(grad_input=1e-5, grad_weights=1e-5, grad_attention=1e-7)
    dt = b.adj_norm.val.dtype

    def layer(L, x_in, g64, e_g, gemm, relu):
        A = b.adj_norm
        W, att = L.weight.detach(), L.attention.detach()
        E = S = dead = None
        if gat:
            fea = ops.recorded(x_in, ("fea_csr", dt)) if gemm == 0 else x_in.detach().to(dt).contiguous()
            _, E, S = ops.layer_forward(A, fea, W.t().to(dt).contiguous(), relu=relu, alpha=L.alpha,
                                        gat_attention=att.reshape(-1).to(dt).contiguous(), want_edge_outputs=True)
            dead = LG.dead_rows_of(A.rowptr, A.val.float())
        run = lambda g: LG.dense(A.rowptr, A.col, A.val.float(), x_in.detach().float(), W, g, gat=bool(gat), E=E, S=S, dead=dead, alpha=L.alpha)
        grads, _ = run(g64)
        _, mag = run(g64.abs() + e_g)
        _, prop = run(e_g)
        return grads, {k: tol_of[k] * mag[k] + prop[k] for k in mag}

    X2 = model._x2.detach()
    ref2, tol2 = layer(model.conv22, X2, gh64, e_gh, 1, 0)
    live = (X2 != 0).double()
    ref1, tol1 = layer(model.att2, b.x, ref2["grad_input"] * live, tol2["grad_input"] * live, 0, 1)
    ref = {"conv22.weight": (ref2["grad_weights"], tol2["grad_weights"]), "att2.weight": (ref1["grad_weights"], tol1["grad_weights"])}
    if gat:
        ref.update({"conv22.attention": (ref2["grad_attention"], tol2["grad_attention"]),
                    "att2.attention": (ref1["grad_attention"], tol1["grad_attention"])})
    return ref


def test_layers_on_a_padded_batch_against_the_unpadded_batch(env):
    from sgracex1_amd import ops, pyg_lite
    model, data, kw, gat = env
    loader = pyg_lite.NeighborLoader(data, [5, 5], pad=True, **kw)
    seeds, input_id, step = next(iter(loader.epoch_batches()))
    assert loader.padded(seeds)
    hook = model.reluh.register_forward_hook(lambda m, i, o: setattr(model, "_x2", o))
    B = loader.batch_size
    names = [k for k, _ in model.named_parameters()]

    def run(b):
        for p in model.parameters():
            p.grad = None
        H = model.features(b.x, b.edge_index_agg).contiguous()
        loss = ops.NodeLoss.apply(H, model.lin.weight, model.lin.bias, b.y, None, B, 0.0, 0, 0, None)
        loss.backward()
        return H.detach().clone(), loss.detach().reshape(1).clone(), {k: None if p.grad is None else p.grad.clone() for k, p in model.named_parameters()}

    u = loader._prepared(seeds, input_id, step)
    u.adj_norm.with_facts(has_dead_rows=True)                         # the padded batch's constant fact: the same kernel path
    H_u, loss_u, g_u = run(u)
    n = u.num_real_nodes
    gh = ops.node_loss(H_u, model.lin.weight.detach(), model.lin.bias.detach(), u.y, n_prefix=B, p=0.0)[1]
    r = R.node_f64(H_u.cpu().numpy(), model.lin.weight.detach().cpu().numpy(), model.lin.bias.detach().cpu().numpy(), u.y.cpu().numpy(),
                   None, B)
    bound = R.node_bounds(r[6])
    d64 = lambda a: torch.as_tensor(a, dtype=torch.float64, device=DEV)
    assert (np.abs(gh.double().cpu().numpy() - r[2]) <= bound["grad_H"]).all()
    ref = _reference_grads(model, u, H_u, d64(r[2]), d64(bound["grad_H"]), gat)
    loader.load(seeds, step)
    p = loader.padded_batch(input_id)
    H_p, loss_p, g_p = run(p)
    hook.remove()
    assert p.num_real_nodes is None and int(loader.counts[0]) == n and p.x.shape[0] == loader.capacity.n_rows > n
    assert same_bits(p.x[:n], u.x) and not p.x[n:].any()
    assert same_bits(H_p[:n], H_u), "live rows"
    assert not H_p[n:].any(), "filler rows"
    assert same_bits(loss_p, loss_u)
    assert [k for k in names if g_p[k] is None] == [k for k in names if g_u[k] is None]
    for k in ("lin.weight", "lin.bias"):                              # the head sees the same prefix rows: the same bits
        assert same_bits(g_p[k], g_u[k]), k
    for k, (want, tol) in ref.items():
        # dense weight-gradient sums run over N rows instead of n and may associate differently: both sides inside the
        # float64 bound; equal bits where the implementation gives them
        equal = same_bits(g_p[k], g_u[k])
        ratios = [float(((g.double().reshape(want.shape) - want).abs() / tol.clamp_min(1e-300)).max()) for g in (g_p[k], g_u[k])]
        print(k, "bit-equal" if equal else "not bit-equal", "error / bound: padded", ratios[0], "unpadded", ratios[1])
        assert max(ratios) <= 1.0, (k, ratios)
        assert equal, k                                                # the implementation does give equal bits: the filler rows add exact zeros
        if not k.endswith("attention"):
            assert float(tol.max()) <= 0.01 * float(want.abs().max()), k           # a bound that a wrong gradient cannot pass
    if not gat:
        for k in ("conv22.attention", "att2.attention"):
            assert not g_p[k].any()


def test_capture_loader_replays_to_eager_steps_on_the_same_batches(env):
    from sgracex1_amd import pyg_lite
    from sgracex1_amd.train import NodeTrainer
    model, data, kw, gat = env
    twin = copy.deepcopy(model)
    a, b = NodeTrainer(model, lr=0.01, weight_decay=5e-4, seed=5), NodeTrainer(twin, lr=0.01, weight_decay=5e-4, seed=5)
    la, lb = pyg_lite.NeighborLoader(data, [5, 5], pad=True, **kw), pyg_lite.NeighborLoader(data, [5, 5], pad=True, **kw)
    assert len(la) == 5 and la.input_nodes.numel() == 70              # four full batches and a short one of 6 seeds
    with pytest.raises(ValueError, match="pad=True"):
        a.capture_loader(pyg_lite.NeighborLoader(data, [5, 5], **kw))
    epoch = a.capture_loader(la)
    assert int(a.t) == 0                                              # the warm-up ran on a copy of the state
    replayed = epoch()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                           # a replayed epoch reads nothing back through torch
    try:
        replayed += epoch()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    eager = []
    for _ in range(2):
        for bt in lb:
            assert (bt.num_real_nodes is None) == (bt.batch_size == 16)
            eager.append(b.step(bt.x, bt.edge_index_agg, bt.y, n_prefix=bt.batch_size))
    la.status(), lb.status()
    assert len(replayed) == len(eager) == 10
    for i, (r, e) in enumerate(zip(replayed, eager)):
        assert same_bits(r, e), i
    assert int(a.t) == int(b.t) == 10
    for x1, x2 in zip(a.state(), b.state()):
        assert same_bits(x1, x2)


def test_loader_refuses_what_would_want_a_plan_and_reports_a_failed_batch():
    from sgracex1_amd import _lib, pyg_lite
    n, ei = _graph("repeated", seed=1)
    wide = torch.rand((n, 80), device=DEV) + 0.5                      # feature rows of 80 entries
    with pytest.raises(ValueError, match="feature rows"):
        pyg_lite.NeighborLoader(pyg_lite.NodeData(wide, ei.to(DEV)), [3, 2], batch_size=8, prepare="sym_norm2", pad=True)
    big_n = 40000
    g = torch.Generator(device=DEV).manual_seed(0)
    big = torch.randint(0, big_n, (2, 1200000), device=DEV, generator=g)
    thin = torch.zeros((big_n, 4), device=DEV)
    with pytest.raises(ValueError, match="2\\^20"):
        pyg_lite.NeighborLoader(pyg_lite.NodeData(thin, big), [32, 32], batch_size=1024, prepare="sym_norm2", pad=True)
    x = _features(n)
    twice = torch.tensor([4, 9, 4, 30, 31, 32, 33, 34], device=DEV)   # a repeated input node: the eager call raises per batch
    loader = pyg_lite.NeighborLoader(pyg_lite.NodeData(x, ei.to(DEV)), [3, 2], batch_size=8, input_nodes=twice, prepare="sym_norm2", pad=True)
    (bt,) = list(loader)
    assert bt.num_real_nodes is None and (bt.n_id == -1).all() and not bt.x.any()
    with pytest.raises(_lib.SgxError) as err:
        loader.status()
    assert err.value.status == _lib.SGX_ERR_SEEDS
    loader.status()                                                   # cleared


def test_capture_loader_at_the_examples_shape_with_attention():
    """Batch 128 and [10, 10] on a 3000-node graph: the padded adjacency holds over 8192 entries, the size from which a CSR
    without known facts wants a plan -- and a plan's read-back cannot be recorded.  Every CSR of the step, the backward's
    attention matrix included, carries the loader's facts; two replayed epochs equal the eager steps bit for bit."""
    from sgracex1_amd import config, pyg_lite, sgrace
    from sgracex1_amd.train import NodeTrainer
    saved = config.snapshot()
    try:
        config.acc, config.accb, config.float_type, config.compute_attention = 1, 0, np.float32, 1
        config.fake_quantization = config.hardware_quantize = 0
        config.w_qbits, config.gat_edge_outputs, config.device = 32, 1, "cuda"
        sgrace.init_SGRACE()
        torch.manual_seed(1)
        g = torch.Generator().manual_seed(6)
        n = 3000
        ei = torch.randint(0, n, (2, 36000), generator=g).to(DEV)
        x = _features(n, seed=4, width=48)
        y = (torch.arange(n) % 5).to(DEV)
        train = torch.zeros(n, dtype=torch.bool, device=DEV)
        train[:300] = True                                            # two full batches and a short one
        data = pyg_lite.NodeData(x, ei, y, train_mask=train)
        kw = dict(batch_size=128, input_nodes=train, shuffle=True, seed=2, prepare="sym_norm2", fill=1, transposed=True, pad=True)
        model = sgrace.GAT_PYNQ(48, 16, 1, 5).to(DEV).train()
        twin = copy.deepcopy(model)
        a, b = NodeTrainer(model, lr=0.01, seed=3), NodeTrainer(twin, lr=0.01, seed=3)
        la, lb = pyg_lite.NeighborLoader(data, [10, 10], **kw), pyg_lite.NeighborLoader(data, [10, 10], **kw)
        assert la.capacity.nnz_norm >= 8192
        # two epochs: the short batch's eager step builds a plan (its transposed feature CSR wants one), with the plan's
        # allocations and read-back, between two replays; the replays behind it still start from cleared counters
        epoch = a.capture_loader(la)
        replayed = epoch() + epoch()
        eager = [b.step(bt.x, bt.edge_index_agg, bt.y, n_prefix=bt.batch_size) for _ in range(2) for bt in lb]
        la.status(), lb.status()
        assert len(replayed) == len(eager) == 6 and all(same_bits(r, e) for r, e in zip(replayed, eager))
        for x1, x2 in zip(a.state(), b.state()):
            assert same_bits(x1, x2)
    finally:
        config.restore(saved)
        sgrace.init_SGRACE()

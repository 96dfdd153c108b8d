"""Padded batches that carry the quantised adjacencies, on the device (include/sgx.h, sgx_collate_graphs_padded_quant):
every array of the call against the numpy restatement of tests/_padded_quant_ref.py inside guard bands, against the plain
padded call and against the unpadded collation; offsets that lie; the call captured and replayed; the fused quantised
forward and backward on a padded batch against the unpadded batch; and epochs and evaluation passes through
StackTrainer.capture_loader / capture_eval_loader against eager steps, bit for bit."""
import numpy as np
import pytest
import torch

import _graph_prep_ref as P
import _padded_quant_ref as RQ
import test_gpu_padded as T
from _padded_ref import N_SET, capacity, counts
from _quant_stack_grad_ref import quant_stack_grad_f64, within
from test_gpu_padded import B, BOTH, CASES, DEV, GUARD, HIDDEN, NO_DEAD, same_bits

pytestmark = pytest.mark.gpu
F32 = torch.float32
ALPHA = 0.2


def f64(t):
    return t.detach().cpu().double().numpy()


def _prepared(bits, graphs=None):
    """(set, extras carrying one quantised adjacency per entry of `bits`, extras of the same set without one, constants)."""
    from sgracex1_amd import ops, quant
    gs = ops.GraphSet(P.torch_graphs()[:N_SET] if graphs is None else graphs)
    qcs = [quant.constants(b) for b in bits]
    for qc in qcs:
        prepared = gs.prepare_sym_norm2(BOTH, qc).prepared
    return gs, ops.GraphExtras(prepared, BOTH, tuple(RQ.key(c) for c in qcs)), ops.GraphExtras(prepared, BOTH, ()), qcs


def _numpy(c):
    out = T._numpy(c)
    out["q_val"] = {k: v.cpu().numpy() for k, v in c.q_val.items()}
    out["q_dead"] = {k: v.cpu().numpy() for k, v in c.q_dead.items()}
    return out


def _guarded(gs, cap, extras):
    """T._guarded with the quantised arrays inside guard bands as well."""
    c, buffers = T._guarded(gs, cap, extras)
    for key in extras.keys:
        for group, fill in (("q_val", 90), ("q_dead", True)):
            t = getattr(c, group)[key]
            big = torch.full((t.numel() + 2 * GUARD,), fill, dtype=t.dtype, device=DEV)
            getattr(c, group)[key] = big[GUARD:GUARD + t.numel()]
            buffers[f"{group}.{key}"] = big
    return c, buffers


@pytest.mark.parametrize("bits", [(8,), (2,), (8, 2)], ids=["8 bits", "2 bits", "two keys"])
def test_call_against_the_restatement_the_plain_call_and_the_unpadded_collation(bits):
    from sgracex1_amd import ops
    gs, extras, plain, qcs = _prepared(bits)
    assert len(extras.keys) == len(bits)
    cap = ops.pad_capacity(gs, B)
    want_cap = capacity(counts(), B)
    assert cap.__dict__ == want_cap
    c, buffers = _guarded(gs, cap, extras)
    cp = ops.Collated.for_capacity(cap, gs.n_feat, BOTH, gs.device, plain)
    for where, ids in CASES.items():               # (one Collated for all: a batch leaves no trace in the next)
        live_c = ops.collate_graphs(gs, ids, BOTH, extras=extras)
        live = _numpy(live_c)
        assert ops.collate_graphs(gs, ids, BOTH, out=c, extras=extras, pad=cap, pad_quant=True) is c
        ops.collate_graphs(gs, ids, BOTH, out=cp, extras=plain, pad=cap)
        torch.cuda.synchronize()
        T._guards_untouched(buffers)
        T._assert_equal(_numpy(c), RQ.padded(live, want_cap, gs.n_feat, qcs), where)
        mine = T._tensors(c)
        for name, t in T._tensors(cp).items():     # every array the plain padded call writes: the same bits
            assert same_bits(t, mine[name]), (where, name)
        n, a = live_c.x.shape[0], live_c.norm_col.numel()
        for key in extras.keys:                    # the live prefix: the unpadded collation's bits
            assert same_bits(c.q_val[key][:a], live_c.q_val[key]) and same_bits(c.q_dead[key][:n], live_c.q_dead[key]), (where, key)
            assert bool((c.q_val[key][a:a + cap.n_rows - n] > 0).all()) and not c.q_val[key][a + cap.n_rows - n:].any()
    fresh = ops.collate_graphs(gs, CASES["P=0"], BOTH, extras=extras, pad=cap, pad_quant=True)
    again = ops.collate_graphs(gs, CASES["P=0"], BOTH, out=c, extras=extras, pad=cap, pad_quant=True)
    T._assert_equal(_numpy(fresh), _numpy(again), "fresh")
    with pytest.raises(ValueError, match="pad_quant"):
        ops.collate_graphs(gs, CASES["P=0"], BOTH, extras=extras, pad=cap)
    with pytest.raises(ValueError, match="another capacity"):      # a Collated without the quantised arrays does not fit
        ops.collate_graphs(gs, CASES["P=0"], BOTH, out=cp, extras=extras, pad=cap, pad_quant=True)


def test_wrong_offsets_write_nothing_outside_the_buffers():
    """The four corruptions of tests/test_gpu_padded.py: wrong contents, but every store inside [0, capacity)."""
    from sgracex1_amd import ops
    gs, extras, _, _ = _prepared((8, 2))
    cap = ops.pad_capacity(gs, B)
    c, buffers = _guarded(gs, cap, extras)
    ids = CASES["largest P, last filler partly filled"]
    for change in ("all + 1000", "last + 2^30", "last = -7", "all + 5"):
        index = gs.prepare(ids)
        off = index.dev[B:].view(-1, B + 1)        # the offset arrays, one row each
        if change == "all + 1000":
            off += 1000
        elif change == "last + 2^30":
            off[:, -1] += 2 ** 30
        elif change == "last = -7":
            off[:, -1] = -7
        else:
            off += 5
        ops.collate_graphs(gs, index, BOTH, out=c, extras=extras, pad=cap, pad_quant=True)
        torch.cuda.synchronize()
        T._guards_untouched(buffers)


def test_call_captured_once_and_replayed_over_every_case():
    from sgracex1_amd import ops
    gs, extras, _, _ = _prepared((8, 2))
    cap = ops.pad_capacity(gs, B)
    index = gs.prepare(CASES["P=0"])
    run = lambda: ops.collate_graphs(gs, index, BOTH, out=c, extras=extras, pad=cap, pad_quant=True)
    c = ops.collate_graphs(gs, index, BOTH, extras=extras, pad=cap, pad_quant=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for where, ids in list(CASES.items())[::-1]:
        index.refill(gs.prepare(ids).dev, ids)
        graph.replay()
        eager = ops.collate_graphs(gs, ids, BOTH, extras=extras, pad=cap, pad_quant=True)
        torch.cuda.synchronize()
        T._assert_equal(_numpy(c), _numpy(eager), where)


def _operands(c, key):
    from sgracex1_amd import ops
    n = c.x.shape[0]
    adj = ops.Csr(c.norm_rowptr, c.norm_col, c.norm_val[F32], n)
    adj_q = ops.Csr(c.norm_rowptr, c.norm_col, c.q_val[key], n)
    return adj, adj_q, ops.Csr(c.fea_rowptr, c.fea_col, c.fea_val[F32], c.n_feat)


def _parameters(gat, seed=3):
    g = torch.Generator().manual_seed(seed)
    Ws = [(torch.randn(7, HIDDEN, generator=g) * 0.3).to(DEV), (torch.randn(HIDDEN, HIDDEN, generator=g) * 0.3).to(DEV)]
    atts = [(torch.randn(2 * HIDDEN, generator=g) * 0.3).to(DEV) if gat else None for _ in Ws]
    return Ws, atts


@pytest.mark.parametrize("gat", [True, False], ids=["attention", "gcn"])
def test_forward_on_a_padded_batch_is_the_unpadded_forward(gat):
    """ops.quant_stack_forward: pooled[:B] bit-equal to the unpadded batch's, the filler graphs pool to 0.  At 8 bits: on
    the 2-bit grid these operands give an output that is 0 everywhere, on the unpadded batch as well, where equality
    would show nothing (the last assertion guards against that); the 2-bit padded arrays are held to the restatement
    above and run through the replayed 2-bit epochs below."""
    from sgracex1_amd import ops
    gs, extras, _, (qc,) = _prepared((8,))
    cap = ops.pad_capacity(gs, B)
    Ws, atts = _parameters(gat)
    wts = [w.t().contiguous() for w in Ws]
    for ids in ([1, 2, 5], [2, 4, 3]):
        pooled = []
        for pad in (None, cap):
            c = ops.collate_graphs(gs, ids, BOTH, extras=extras, pad=pad, pad_quant=pad is not None)
            assert not bool(c.q_dead[RQ.key(qc)].any())
            _, adj_q, fea = _operands(c, RQ.key(qc))
            pooled.append(ops.quant_stack_forward(adj_q, fea, wts, list(atts), [True, False], c.graph_ptr,
                                                  [qc, qc.second_layer()], alpha=ALPHA, adj_quantised=True))
        assert pooled[1].shape[0] == cap.n_graphs > B
        assert same_bits(pooled[1][:B], pooled[0]) and not pooled[1][B:].any()
        assert bool(pooled[0].abs().sum() > 0)


@pytest.mark.parametrize("gat", [True, False], ids=["attention", "gcn"])
def test_backward_on_a_padded_batch_within_the_unpadded_batchs_bound(gat):
    """ops.quant_stack_backward on the pair: every gradient inside the bound tests/_quant_stack_grad_ref.py derives for the
    UNPADDED batch (the padded batch's groups differ, so the per-workgroup partial sums may round differently); the filler
    rows' aggregated gradients are exactly 0."""
    from sgracex1_amd import ops
    gs, extras, _, (qc,) = _prepared((8,))
    cap = ops.pad_capacity(gs, B)
    quants, relus, ids = [qc, qc.second_layer()], [True, False], [1, 2, 5]
    Ws, atts = _parameters(gat)
    wts = [w.t().contiguous() for w in Ws]
    gp = torch.randn(B, HIDDEN, generator=torch.Generator().manual_seed(5)).to(DEV)
    runs = []
    for pad in (None, cap):
        c = ops.collate_graphs(gs, ids, BOTH, extras=extras, pad=pad, pad_quant=pad is not None)
        adj, adj_q, fea = _operands(c, RQ.key(qc))
        _, outs = ops.quant_stack_forward(adj_q, fea, wts, list(atts), relus, c.graph_ptr, quants, alpha=ALPHA,
                                          adj_quantised=True, want_layer_outputs=True)
        g = torch.cat([gp, torch.zeros(c.graph_ptr.numel() - 1 - B, HIDDEN, device=DEV)])
        dW, dA, Gs = ops.quant_stack_backward(adj, fea, Ws, list(atts), relus, c.graph_ptr, outs, g, quants, alpha=ALPHA,
                                              adj_q=adj_q, want_G=True)
        runs.append((c, outs, dW, dA, Gs))
    u = runs[0][0]
    n, a = u.x.shape[0], u.norm_col.numel()
    ref = quant_stack_grad_f64((u.norm_rowptr.cpu().numpy(), u.norm_col.cpu().numpy(), f64(u.norm_val[F32])), f64(u.x),
                               [f64(w) for w in Ws], [None if v is None else f64(v) for v in atts], relus,
                               u.graph_ptr.cpu().numpy(), f64(gp), [f64(D) for D in runs[0][1]], quants,
                               adj_q=u.q_val[RQ.key(qc)].cpu().numpy(), alpha=ALPHA)
    for l in range(2):
        assert (np.abs(ref["dW"][l]) > ref["tW"][l] * ref["mW"][l] + 1e-30).any(), l       # the bound separates from no gradient
    for name, (c, _, dW, dA, Gs) in zip(("unpadded", "padded"), runs):
        for l in range(2):
            figures = {"dW": within(f64(dW[l]), ref["dW"][l], ref["mW"][l], ref["tW"][l]),
                       "G": within(f64(Gs[l][:n]), ref["G"][l], ref["mG"][l], ref["tG"][l])}
            if gat:
                figures["dA"] = within(f64(dA[l]), ref["dA"][l], ref["mA"][l], ref["tA"][l])
            for what, (ok, ratio) in figures.items():
                print(f"{name} {what}_{l}: worst {ratio:.3f} of the bound")
                assert ok, (name, what, l, ratio)
            assert Gs[l].shape[0] == c.x.shape[0] and not Gs[l][n:].any(), (name, l)      # the filler rows: exactly 0
    assert runs[1][4][0].shape[0] == cap.n_rows > n


@pytest.fixture
def quantised():
    """make(bits, gat, hw) -> GAT_POOL_PYNQ(train_stack=True) under fake quantisation, the constants published."""
    from sgracex1_amd import config, sgrace
    saved = config.snapshot()

    def make(bits, gat, hw):
        config.acc, config.float_type, config.fake_quantization, config.w_qbits = 1, np.float32, 1, bits
        config.hardware_quantize, config.compute_attention = hw, gat
        ip = sgrace.init_SGRACE()
        ip.register_map.layer_count = 2
        torch.manual_seed(12345)
        return sgrace.GAT_POOL_PYNQ(7, HIDDEN, 2, train_stack=True).to(DEV).train()

    yield make, sgrace
    config.restore(saved)
    sgrace.init_SGRACE()


def _loader(sgrace, graphs, seed=None, **kw):
    from sgracex1_amd import ops, pyg_lite as G
    if seed is not None:
        kw.update(shuffle=True, generator=torch.Generator().manual_seed(seed))
    return G.GraphLoader(ops.GraphSet(graphs), batch_size=B, dtypes=(F32,), prepare="sym_norm2", quant=sgrace.quant_constants,
                         pad=True, pad_quant=True, **kw)


def _quantised_dead_graph():
    """Two nodes tied by an edge stored 61 times in each direction: every entry of both rows is 1 / 61, under half a step
    of the 2-bit adjacency grid (30 / 61 rounds to 0) -- live under sym_norm2, dead under the 2-bit quantised mask."""
    from sgracex1_amd import pyg_lite as G
    x = torch.zeros(2, 7)
    x[0, 1] = x[1, 4] = 1.0
    return G.Graph(x, torch.as_tensor(P._undirected([(0, 1)] * 61)), torch.tensor([1]))


def _epochs(trainer, loader, replayed, n_epochs=2, sync_error=True):
    losses = []
    if replayed:
        epoch = trainer.capture_loader(loader)
        assert int(trainer.t.item()) == 0 and epoch.collated.q_val
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error" if sync_error else mode)
        try:
            for _ in range(n_epochs):
                losses += [loss.clone() for loss in epoch()]
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    else:
        for _ in range(n_epochs):
            for b in loader:
                losses.append(trainer.step(b.x, b.edge_index, b.batch, b.y, b.num_real_graphs).clone())
    torch.cuda.synchronize()
    return losses


@pytest.mark.parametrize("bits,gat,hw,dead", [(8, 1, 1, False), (8, 1, 0, False), (8, 0, 1, False), (8, 0, 0, False), (2, 1, 1, True)],
                         ids=["attention hw", "attention", "gcn hw", "gcn", "2 bits, a quantised-dead graph"])
def test_two_epochs_replayed_against_eager_steps(quantised, bits, gat, hw, dead):
    """7 graphs at B = 3: two full batches and the short one per epoch.  dead: one graph is dead under the 2-bit mask alone,
    so its full batch arrives unpadded and runs eagerly in place, between the replays (layer by layer: that route may
    synchronise, so only the other cases' replayed epochs run under the sync-debug error mode)."""
    from sgracex1_amd import ops, train
    make, sgrace = quantised
    graphs = [P.torch_graphs()[i] for i in NO_DEAD]
    if dead:
        graphs[6] = _quantised_dead_graph()
    model = make(bits, gat, hw)
    start = {k: v.clone() for k, v in model.state_dict().items()}
    seed = 11
    probe = _loader(sgrace, graphs, seed)
    assert probe.quant is sgrace.quant_constants and probe.pad_quant
    kinds = [(len(ids), probe.padded(ids)) for _ in range(2) for ids in probe.batches()]
    assert [k for k, _ in kinds] == [3, 3, 1] * 2 and not any(p for k, p in kinds if k == 1)
    n_padded = sum(p for _, p in kinds)
    if dead:
        assert not probe.extras.prepared.has_dead.any() and list(np.nonzero(probe.has_dead())[0]) == [6]
        assert 1 <= n_padded < 4                                # a full batch holds graph 6 and arrives unpadded; another replays
        e = probe.collate([6, 0, 1])
        assert e.num_graphs == e.num_real_graphs == B
    else:
        assert n_padded == 4
        p = probe.collate([0, 1, 2])
        assert p.num_graphs == probe.capacity.n_graphs > B and p.num_real_graphs == B
        adj = ops.recorded(p.edge_index, ("sym_norm2", probe.capacity.n_rows, 1, F32))[2]
        Q = adj.quantized(sgrace.quant_constants)
        assert Q.has_dead_rows is False and Q._max_row == probe.extras.prepared.max_row and Q.val.numel() == probe.capacity.nnz_norm
    runs = []
    for replayed in (False, True):
        model.load_state_dict(start)
        trainer = train.StackTrainer(model, lr=0.01, p_drop=0.5, seed=99)
        losses = _epochs(trainer, _loader(sgrace, graphs, seed), replayed, sync_error=not dead)
        runs.append((losses, trainer.state(), trainer.fused_steps))
    (le, se, fe), (lr, sr, fr) = runs
    assert len(le) == len(lr) == 6 and int(sr[-1].item()) == 6
    assert all(same_bits(a, c) for a, c in zip(le, lr))
    assert all(same_bits(a, c) for a, c in zip(se, sr))
    assert not same_bits(lr[0], lr[1])
    if not dead:                                   # every step fused; the replays count nothing: the warm-up's two and the short batches
        assert fe == 6 and fr == 2 + 2


@pytest.mark.parametrize("gat", [1, 0], ids=["attention", "gcn"])
def test_replayed_evaluation_pass_is_the_eager_pass(quantised, gat):
    from sgracex1_amd import train
    make, sgrace = quantised
    graphs = [P.torch_graphs()[i] for i in NO_DEAD]
    model = make(8, gat, 1)
    trainer = train.StackTrainer(model, lr=0.01)
    before = trainer.state()
    sums = train.EvalSums(DEV)
    for b in _loader(sgrace, graphs, 4):
        trainer.evaluate(b.x, b.edge_index, b.batch, b.y, b.num_real_graphs, into=sums)
    eager = sums.buffer.clone()
    test = trainer.capture_eval_loader(_loader(sgrace, graphs, 4))
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        test()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert same_bits(test.sums.buffer, eager) and int(eager[0]) == 7
    assert all(same_bits(a, c) for a, c in zip(before, trainer.state())) and model.training


def test_a_workspace_replaced_inside_the_recording_is_refused(quantised, monkeypatch):
    """The host-side guard of the quantised recording: if a call inside the recording asks for more scratch than the warm-up
    did, ops._workspace replaces the stream's tensor; capture_loader then raises and returns no recording."""
    from sgracex1_amd import ops, train
    make, sgrace = quantised
    graphs = [P.torch_graphs()[i] for i in NO_DEAD]
    model = make(8, 1, 1)
    trainer = train.StackTrainer(model, lr=0.01)
    before = trainer.state()
    real, asked = ops._workspace, []

    def growing(device, nbytes):
        if torch.cuda.is_current_stream_capturing():
            asked.append(nbytes)
            nbytes = max(ws.numel() for ws in ops._workspaces.values()) + 4096
        return real(device, nbytes)

    monkeypatch.setattr(ops, "_workspace", growing)
    with pytest.raises(RuntimeError, match="workspace"):
        trainer.capture_loader(_loader(sgrace, graphs, 11))
    assert asked
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert all(same_bits(a, c) for a, c in zip(before, trainer.state())) and trainer.fused_steps == 2      # (the warm-up's)

"""Padded QUANTISED node batches on the device (include/sgx.h, sgx_node_batch_sample_padded_quant): the call against the
unpadded quantised call, the unquantised padded call and the numpy restatement (tests/_node_pad_quant_ref.py) inside guard
bands; its capture and replay; the quantised layers on a padded batch against the same batch unpadded; and
train.NodeTrainer.capture_loader / capture_eval_loader and the example on NeighborLoader(pad=True, quant=)."""
import copy
import importlib.util
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import _node_pad_quant_ref as PQ
import test_gpu_node_pad as TP
from test_gpu_node_pad import DEV, GUARD, _np, same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _TwoScales:
    """Constants whose second layer reads the adjacency on another scale (the demo's layers share one): two sets, as
    tests/test_gpu_node_batch_quant.py reaches them."""

    def __init__(self, first, a_s2):
        self.first, self.second = first, replace(first.second_layer(), a_s=a_s2)
        self.w_qbits, self.a_s, self.a_z = first.w_qbits, first.a_s, first.a_z

    def second_layer(self):
        return self.second


def _constants(bits, n_sets):
    from sgracex1_amd import quant
    qc = quant.constants(bits)
    if n_sets == 1:
        return qc, [qc]
    two = _TwoScales(qc, qc.a_s / 2)                                  # 1 / a_s doubles: 1 still clips to the top of the grid
    return two, [two.first, two.second]


def _key(c):
    return (c.w_qbits, c.a_s, c.a_z)


def _guard_quant(buf):
    """The quantised arrays of the NodePadBuffers `buf` moved into sentinel-filled tensors, as TP._guarded does the rest."""
    bands, moved = [], []
    for k, triple in enumerate(buf.quant):
        views = []
        for name, t in zip(("q_val", "q_dead", "q_lean"), triple):
            whole = torch.empty(t.numel() + 2 * GUARD, dtype=t.dtype, device=DEV)
            whole.view(torch.uint8).fill_(0xA5)
            view = whole[GUARD:GUARD + t.numel()]
            view.copy_(t)
            views.append(view)
            bands.append(((name, k), whole, t.numel()))
        moved.append(tuple(views))
    buf.quant = moved
    return bands


def _weights(nnz):
    """Edge weights 2^-k, k in 0 .. 8: every degree is exact in fp32, and a row whose only positive entries are light ones
    next to heavy degrees loses them all to the 1-bit grid (unit weights leave dead_row_q == dead_row on all four cases)."""
    return torch.as_tensor((2.0 ** -np.random.default_rng(1).integers(0, 9, nnz)).astype(np.float32), device=DEV)


# (kind, batch, fan-outs, with features / labels / masks): complete: P = F, no spare filler; isolated with fill = 0: no
# edge, every live row dead in both masks (values_lean takes the unquantised branch); 64-entry rows: a full wavefront stride
CASES = [("complete", 2, [5, 5], True), ("isolated", 8, [3, 2], True), ("repeated", 13, [3, 2], False), ("repeated", 16, [63], True)]
PLAIN = ["n_id", "rowptr", "col", "pos", "n_rowptr", "n_col", "n_val", "dead", "ei", "ei_agg", "f_rowptr", "f_col", "f_val", "y", "status",
         "counts"]


@pytest.mark.parametrize("n_sets", [1, 2])
@pytest.mark.parametrize("bits", [8, 1])
def test_padded_quantised_call_against_the_unpadded_call_and_the_restatement(bits, n_sets):
    from sgracex1_amd import ops
    qc, sets = _constants(bits, n_sets)
    masks_differ = 0
    for kind, batch, fan, extras in CASES:
        n, ei = TP._graph(kind, seed=batch)
        csr = TP._csr(n, ei)
        w = _weights(csr.nnz)
        fea = ops.feature_csr(TP._features(n)) if extras else None
        y = torch.arange(n, device=DEV) % 5 + 1 if extras else None
        masks = [torch.arange(n, device=DEV) % 2 == 0] if extras else []
        seeds = torch.arange(batch, device=DEV) if kind == "isolated" else torch.randperm(n, generator=torch.Generator().manual_seed(4))[:batch].to(DEV)
        cap = ops.node_pad_capacity(csr, batch, fan, fea)
        c = dict(N=cap.n_rows, Ca=cap.nnz_norm)
        n_feat = None if fea is None else fea.n_cols
        buf = ops.NodePadBuffers(cap, n, torch.float32, DEV, n_feat, y is not None, len(masks), n_sets)
        plain = ops.NodePadBuffers(cap, n, torch.float32, DEV, n_feat, y is not None, len(masks))
        assert len(buf.quant) == n_sets and plain.quant == []
        bands = TP._guarded(buf) + _guard_quant(buf)
        step = torch.zeros(1, dtype=torch.int64, device=DEV)
        for k in (5, 2 ** 40 + 3):                                       # two batches through the same buffers
            step.fill_(k)
            kw = dict(seed=11, fill=1 if k == 5 else 0, edge_weight=w, features=fea, y=y, masks=masks)
            s = ops.sample_node_batch(csr, seeds, fan, step=step, pad=cap, out=buf, quant=qc, **kw)
            ops.sample_node_batch(csr, seeds, fan, step=step, pad=cap, out=plain, **kw)
            u = ops.sample_node_batch(csr, seeds, fan, step=k, quant=qc, **kw)
            # every array of the unquantised padded call: the same bytes
            for name in PLAIN:
                a, b = getattr(buf, name), getattr(plain, name)
                assert (a is None) == (b is None), name
                if a is not None:
                    assert same_bits(a, b), (kind, name)
            assert all(same_bits(a, b) for a, b in zip(buf.masks, plain.masks))
            assert int(buf.status) == 0
            A, U = s.adj_norm, u.adj_norm
            live_n, a_live = U.n_rows, U.nnz
            assert _np(buf.counts)[:3].tolist() == [live_n, u.hop_edges[-1], a_live]
            assert set(A._quantized) == {_key(x) for x in sets} and len(A._quantized) == n_sets
            for x in sets:
                D, G = U._quantized[_key(x)], A._quantized[_key(x)]
                assert A.quantized(x) is G                               # what the layers look up
                assert G.rowptr is A.rowptr and G.col is A.col and G.nnz == cap.nnz_norm and G.n_rows == cap.n_rows
                assert G._dead_rows is True and G._max_row == cap.max_row and not G.wants_plan
                assert G._lean_values.rowptr is A.rowptr and G._lean_values.nnz == cap.nnz_norm
                inv, zero, q = PQ.constants_of(x)
                want = PQ.pad_quant(c, live_n, _np(U.rowptr), _np(U.val[:a_live]), _np(D.val[:a_live]), _np(D._dead_row_mask),
                                    _np(D._lean_values.val[:a_live]), inv, zero, q)
                # the unpadded call's arrays are the restatement's own, so the padded ones are the rule's from end to end
                rq, rdead, rlean = PQ.live_quant(live_n, _np(U.rowptr), _np(U.val[:a_live]), inv, zero, q)
                assert rq.tobytes() == want["values_q"][:a_live].tobytes() and rlean.tobytes() == want["values_lean"][:a_live].tobytes()
                assert np.array_equal(rdead, want["dead_row_q"][:live_n])
                got = dict(values_q=G.val, dead_row_q=G._dead_row_mask, values_lean=G._lean_values.val)
                for name, t in got.items():
                    g = _np(t)
                    assert g.shape == want[name].shape and g.dtype == want[name].dtype and g.tobytes() == want[name].tobytes(), (kind, k, name)
                # the whole capacity is fq of values_norm; no filler row is dead; its spare entries carry no weight
                assert PQ.fq(_np(A.val), inv, zero, q).tobytes() == _np(G.val).tobytes()
                assert not _np(G._dead_row_mask)[live_n:].any()
                first = _np(A.rowptr)[live_n:-1]
                filler = np.ones(cap.nnz_norm - a_live, bool)
                filler[first - a_live] = False
                assert (_np(G.val)[first] == PQ.fq([1.0], inv, zero, q)[0]).all() and not _np(G.val)[a_live:][filler].any()
                masks_differ += int(not torch.equal(G._dead_row_mask, A._dead_row_mask))
                if kind == "isolated" and k != 5:
                    assert _np(G._dead_row_mask)[:live_n].all() and _np(A._dead_row_mask)[:live_n].all()
                    assert same_bits(G._lean_values.val[:a_live], A.val[:a_live])            # the unquantised branch
            if kind == "complete":
                assert live_n == n == cap.max_nodes                      # the batch reaches the whole graph: P = F
            if kind == "isolated":
                assert _np(buf.counts)[:3].tolist() == [batch, 0, batch]
        assert (buf.node_map == ops.SAMPLE_SENTINEL).all()
        TP._bands_intact(bands)
        with pytest.raises(ValueError, match="out="):                   # buffers built for another number of constant sets
            ops.sample_node_batch(csr, seeds, fan, step=step, pad=cap, out=plain, quant=qc, **kw)
    if bits == 1:
        assert masks_differ > 0                                          # a row live in values_norm died on the 1-bit grid


def test_captured_quantised_call_replays_on_new_seeds_and_a_new_step_word():
    from sgracex1_amd import ops
    qc, sets = _constants(8, 2)
    n, ei = TP._graph("repeated", seed=3)
    csr, fea = TP._csr(n, ei), ops.feature_csr(TP._features(n))
    y = torch.arange(n, device=DEV) % 7
    batch, fan = 16, [5, 5]
    cap = ops.node_pad_capacity(csr, batch, fan, fea)
    buf = ops.NodePadBuffers(cap, n, torch.float32, DEV, fea.n_cols, True, 0, 2)
    bands = TP._guarded(buf) + _guard_quant(buf)
    seeds = torch.arange(batch, device=DEV, dtype=torch.int32)
    step = torch.full((1,), 9, dtype=torch.int64, device=DEV)
    call = lambda: ops.sample_node_batch(csr, seeds, fan, seed=2, step=step, features=fea, y=y, pad=cap, out=buf, quant=qc)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                           # the side stream's workspace
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s = call()
    first = s.adj_norm._quantized[_key(sets[0])].val.clone()
    for new_seeds, new_step in ((torch.arange(100, 100 + batch), 9), (torch.arange(batch), 10), (torch.arange(50, 50 + batch), 2 ** 33)):
        seeds.copy_(new_seeds)
        step.fill_(new_step)
        graph.replay()
        fresh = ops.sample_node_batch(csr, seeds.clone(), fan, seed=2, step=step.clone(), features=fea, y=y, pad=cap, quant=qc)
        assert same_bits(s.n_id, fresh.n_id) and same_bits(s.adj_norm.val, fresh.adj_norm.val) and same_bits(buf.counts, fresh.counts)
        for x in sets:
            a, b = s.adj_norm._quantized[_key(x)], fresh.adj_norm._quantized[_key(x)]
            assert same_bits(a.val, b.val) and same_bits(a._dead_row_mask, b._dead_row_mask)
            assert same_bits(a._lean_values.val, b._lean_values.val)
        assert int(buf.status) == 0
    assert not same_bits(first, s.adj_norm._quantized[_key(sets[0])].val)          # the replays did draw other batches
    # a repeated seed: the status word is set and every row is a filler row in the quantised arrays too
    seeds[3] = seeds[7]
    graph.replay()
    assert int(buf.status) == 1 and _np(buf.counts).tolist() == [0] * buf.counts.numel()
    rowptr = _np(s.adj_norm.rowptr)
    assert rowptr[0] == 0 and rowptr[-1] == cap.nnz_norm
    for x in sets:
        inv, zero, q = PQ.constants_of(x)
        none = np.zeros(0, np.float32)
        want = PQ.pad_quant(dict(N=cap.n_rows, Ca=cap.nnz_norm), 0, np.zeros(1, np.int32), none, none, np.zeros(0, bool), none, inv, zero, q)
        G = s.adj_norm._quantized[_key(x)]
        assert _np(G.val).tobytes() == want["values_q"].tobytes() and _np(G._lean_values.val).tobytes() == want["values_lean"].tobytes()
        assert not _np(G._dead_row_mask).any()
        one, nought = PQ.fq([1.0, 0.0], inv, zero, q)
        rest = np.ones(cap.nnz_norm, bool)
        rest[rowptr[:-1]] = False
        assert (_np(G.val)[rowptr[:-1]] == one).all() and (_np(G.val)[rest] == nought).all() and one > 0 and nought == 0
    assert (buf.node_map == ops.SAMPLE_SENTINEL).all()
    TP._bands_intact(bands)


CONFIGS = {"gcn-q8": (0, 0, 8), "att-q8": (1, 0, 8), "att-lean-q8": (1, 1, 8), "gcn-q1": (0, 0, 1)}


def _environment(gat, lean, bits, hwq):
    """The quantised model on the kernels (accb = 0) over the graph, features, labels and 70 training nodes of
    tests/test_gpu_node_pad.py's env -> (model, data, loader arguments).  attention: transposed, fill = 1."""
    from sgracex1_amd import config, pyg_lite, sgrace
    config.acc, config.accb, config.float_type, config.compute_attention = 1, 0, np.float32, gat
    config.fake_quantization, config.hardware_quantize = 1, hwq
    config.w_qbits, config.gat_edge_outputs, config.device = bits, 0 if lean else 1, "cuda"
    sgrace.init_SGRACE()
    torch.manual_seed(5)
    n, ei = TP._graph("repeated", seed=8)
    x = TP._features(n, seed=9, width=40)
    y = (torch.arange(n) * 7 % 5).to(DEV)
    train_mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    train_mask[torch.randperm(n, generator=torch.Generator().manual_seed(2))[:70].to(DEV)] = True
    data = pyg_lite.NodeData(x, ei.to(DEV), y, train_mask=train_mask)
    model = sgrace.GAT_PYNQ(40, 16, 1, 5).to(DEV).train()
    kw = dict(batch_size=16, input_nodes=train_mask, shuffle=True, seed=3, prepare="sym_norm2", fill=1 if gat else 0,
              transposed=bool(gat), quant=sgrace.quant_constants, pad=True)
    return model, data, kw


@pytest.fixture
def restore_config():
    from sgracex1_amd import config, sgrace
    saved = config.snapshot()
    yield
    config.restore(saved)
    sgrace.init_SGRACE()


@pytest.mark.parametrize("hwq", [0, 1], ids=["emulated", "hardware"])
@pytest.mark.parametrize("name", ["gcn-q8", "att-q8", "att-lean-q8"])
def test_quantised_layers_on_a_padded_batch_against_the_unpadded_batch(restore_config, name, hwq):
    """Against the route tests/test_gpu_node_batch_quant.py and tests/test_gpu_quant_paths.py hold to their references: the
    unpadded quantised batch.  fill = 1, [5, 5], batch 16 at 8 bits.  Live rows of H, the loss and the head gradients: the
    same bits; filler rows of H: zero; the layers' parameter gradients: the same bits (the filler rows add exact zeros)."""
    from sgracex1_amd import ops, pyg_lite, sgrace
    gat, lean, bits = CONFIGS[name]
    model, data, kw = _environment(gat, lean, bits, hwq)
    kw["fill"] = 1
    loader = pyg_lite.NeighborLoader(data, [5, 5], **kw)
    seeds, input_id, step = next(iter(loader.epoch_batches()))
    assert loader.padded(seeds)
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
    qc = sgrace.quant_constants
    assert set(u.adj_norm._quantized) == {_key(qc)} == {_key(qc.second_layer())}
    u.adj_norm.with_facts(has_dead_rows=True)                         # the padded batch's constant facts on both adjacencies:
    u.adj_norm.quantized(qc).with_facts(has_dead_rows=True)           # the same kernel path
    H_u, loss_u, g_u = run(u)
    n = u.num_real_nodes
    loader.load(seeds, step)
    p = loader.padded_batch(input_id)
    Q = p.adj_norm.quantized(qc)
    # unit weights and fan-outs [5, 5] with fill = 1: degrees within 6, entries at least 1 / 64, and 255 / 64 rounds to 4:
    # no live row of the drawn batch is dead under the quantised mask (asserted, not assumed)
    assert float(u.adj_norm.val[:u.adj_norm.nnz].min()) >= 1 / 64
    assert not Q.dead_rows[:n].any() and not Q.dead_rows[n:].any() and Q.has_dead_rows is True
    H_p, loss_p, g_p = run(p)
    assert p.num_real_nodes is None and int(loader.counts[0]) == n and p.x.shape[0] == loader.capacity.n_rows > n
    assert same_bits(p.x[:n], u.x) and not p.x[n:].any()
    assert same_bits(H_p[:n], H_u), "live rows"
    assert bool(H_u.any()) and bool(torch.isfinite(H_u).all())
    assert not H_p[n:].any(), "filler rows"
    assert same_bits(loss_p, loss_u)
    assert [k for k in names if g_p[k] is None] == [k for k in names if g_u[k] is None]
    for k in ("lin.weight", "lin.bias"):                              # the head sees the same prefix rows
        assert same_bits(g_p[k], g_u[k]), k
    layer_params = ["att2.weight", "conv22.weight"] + (["att2.attention", "conv22.attention"] if gat else [])
    for k in layer_params:
        assert bool(g_u[k].any()), k                                  # a gradient did arrive
        print(k, "bit-equal" if same_bits(g_p[k], g_u[k]) else "not bit-equal",
              "max |padded - unpadded|", float((g_p[k] - g_u[k]).abs().max()), "max |unpadded|", float(g_u[k].abs().max()))
        assert same_bits(g_p[k], g_u[k]), k
    if not gat:
        for k in ("conv22.attention", "att2.attention"):
            assert not g_p[k].any()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_capture_loader_replays_the_quantised_step_to_eager_steps(restore_config, name):
    from sgracex1_amd import pyg_lite
    from sgracex1_amd.train import NodeTrainer
    gat, lean, bits = CONFIGS[name]
    model, data, kw = _environment(gat, lean, bits, 1)
    twin = copy.deepcopy(model)
    a, b = NodeTrainer(model, lr=0.01, weight_decay=5e-4, seed=5), NodeTrainer(twin, lr=0.01, weight_decay=5e-4, seed=5)
    la, lb = pyg_lite.NeighborLoader(data, [5, 5], **kw), pyg_lite.NeighborLoader(data, [5, 5], **kw)
    assert len(la) == 5 and la.input_nodes.numel() == 70              # four full batches and a short one of 6 seeds
    assert len(la.buffers.quant) == 1
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
            assert len(bt.adj_norm._quantized) == 1                   # padded or short: the quantised adjacency is delivered
            eager.append(b.step(bt.x, bt.edge_index_agg, bt.y, n_prefix=bt.batch_size))
    la.status(), lb.status()
    assert len(replayed) == len(eager) == 10
    for i, (r, e) in enumerate(zip(replayed, eager)):
        assert same_bits(r, e), i
        assert bool(torch.isfinite(r).all())
    assert int(a.t) == int(b.t) == 10
    for x1, x2 in zip(a.state(), b.state()):
        assert same_bits(x1, x2)


@pytest.mark.parametrize("name", ["gcn-q8", "att-q8"])
def test_capture_eval_loader_replays_the_quantised_pass_to_the_eager_pass(restore_config, name):
    from sgracex1_amd import pyg_lite
    from sgracex1_amd.train import EvalSums, NodeTrainer
    gat, lean, bits = CONFIGS[name]
    model, data, kw = _environment(gat, lean, bits, 1)
    kw.update(transposed=False, shuffle=False)
    trainer = NodeTrainer(model, lr=0.01, weight_decay=5e-4, seed=5)
    la, lb = pyg_lite.NeighborLoader(data, [5, 5], **kw), pyg_lite.NeighborLoader(data, [5, 5], **kw)
    state = trainer.state()
    run_pass = trainer.capture_eval_loader(la)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        replayed = run_pass().buffer.clone()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    sums = EvalSums(DEV)
    for bt in lb:
        trainer.evaluate(bt.x, bt.edge_index_agg, bt.y, n_prefix=bt.batch_size, into=sums)
    la.status(), lb.status()
    assert same_bits(replayed, sums.buffer), (replayed.tolist(), sums.buffer.tolist())
    (rows, hits, loss), = EvalSums.read(sums)
    assert rows == 70 and 0 <= hits <= 70 and np.isfinite(loss) and loss > 0
    assert all(same_bits(x, y) for x, y in zip(state, trainer.state())) and model.training and int(trainer.t) == 0


def test_example_replays_the_quantised_mini_batch_step(restore_config):
    spec = importlib.util.spec_from_file_location("sgrace_nc", os.path.join(ROOT, "examples", "sgrace_node_classification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    kw = dict(epochs=3, acc=1, n=600, verbose=False, batch_size=32, num_neighbors=[5, 5], device_batches=True, trainer=True, replay=True)
    plain, _, _ = mod.run(qbits=32, **kw)
    res, _, _ = mod.run(qbits=8, **kw)
    assert set(res) == set(plain) and {"train_acc", "test_acc", "epoch_loss", "batches_per_epoch"} <= set(res)
    assert 0.0 <= res["train_acc"] <= 1.0 and 0.0 <= res["test_acc"] <= 1.0
    assert len(res["epoch_loss"]) == 3 and all(np.isfinite(v) for v in res["epoch_loss"])

"""Padded batches on the device (include/sgx.h, "padded batches"): every array of a padded collation against the numpy
restatement of tests/_padded_ref.py inside guard bands, the regrouped plan table against a fresh plan, the fused forward
and one training step on a padded batch against the unpadded batch, and two epochs through
StackTrainer.capture_loader against eager steps, bit for bit."""
import numpy as np
import pytest
import torch

import _graph_prep_ref as P
import _padded_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
B, HIDDEN, GUARD = 3, 16, 61                      # (61 elements: the guarded arrays start off the 16-byte grid)
BOTH = (torch.float16, torch.float32)
NAMES = {torch.float16: "f16", torch.float32: "f32"}
# rows of graphs 0 .. 6: 1 2 5 9 6 3 4 -> N = 20, R_f = 9, two fillers
CASES = {"P=0": [3, 4, 2], "largest P, last filler partly filled": [0, 1, 5], "one filler partly filled, one empty": [2, 6, 5],
         "one full filler, one empty, a graph twice": [2, 5, 5]}
NO_DEAD = [1, 2, 3, 4, 5, 1, 2]                   # a 7-graph set without a dead row under sym_norm2 (for GAT)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.fixture(scope="module")
def sets():
    from sgracex1_amd import ops
    graphs = P.torch_graphs()[:R.N_SET]
    plain, prepared = ops.GraphSet(graphs), ops.GraphSet(graphs)
    extras = prepared.prepare_sym_norm2(BOTH)
    return {False: (plain, None), True: (prepared, extras)}


def _tensors(c):
    """name -> tensor of every array of a Collated."""
    out = {f: getattr(c, f) for f in c.FIELDS}
    for group in ("adj_val", "fea_val", "norm_val"):
        out.update({f"{group}.{NAMES[dt]}": t for dt, t in getattr(c, group).items()})
    if c.norm_rowptr is not None:
        out.update(norm_rowptr=c.norm_rowptr, norm_col=c.norm_col, norm_dead=c.norm_dead)
    return out


def _numpy(c):
    out = {}
    for name, t in _tensors(c).items():
        group, _, key = name.partition(".")
        if key:
            out.setdefault(group, {})[key] = t.cpu().numpy()
        else:
            out[group] = t.cpu().numpy()
    return out


def _guarded(gs, cap, extras):
    """A capacity-sized Collated whose every array lies inside a larger buffer of sentinels -> (Collated, {name: buffer})."""
    from sgracex1_amd import ops
    c = ops.Collated.for_capacity(cap, gs.n_feat, BOTH, gs.device, extras)
    buffers = {}
    for name, t in _tensors(c).items():
        big = torch.full((t.numel() + 2 * GUARD,), True if t.dtype == torch.bool else 90, dtype=t.dtype, device=DEV)
        view = big[GUARD:GUARD + t.numel()].view(t.shape)
        group, _, key = name.partition(".")
        if key:
            getattr(c, group)[{v: k for k, v in NAMES.items()}[key]] = view
        else:
            setattr(c, group, view)
        buffers[name] = big
    return c, buffers


def _guards_untouched(buffers):
    for name, big in buffers.items():
        want = True if big.dtype == torch.bool else 90
        assert bool((big[:GUARD] == want).all()) and bool((big[-GUARD:] == want).all()), name


def _assert_equal(got, want, where):
    assert set(got) == set(want), where
    for name, w in want.items():
        if isinstance(w, dict):
            _assert_equal(got[name], w, f"{where} {name}")
        else:
            g = got[name]
            assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), f"{where} {name}"


@pytest.mark.parametrize("with_extras", [False, True])
def test_padded_collation_against_the_restatement(sets, with_extras):
    from sgracex1_amd import ops
    gs, extras = sets[with_extras]
    cap = ops.pad_capacity(gs, B)
    want_cap = R.capacity(R.counts(), B)
    if not with_extras:
        want_cap["nnz_norm"] = None
    assert cap.__dict__ == want_cap
    c, buffers = _guarded(gs, cap, extras)
    for where, ids in CASES.items():               # (one Collated for all: a batch leaves no trace in the next)
        live = _numpy(ops.collate_graphs(gs, ids, BOTH, extras=extras))
        out = ops.collate_graphs(gs, ids, BOTH, out=c, extras=extras, pad=cap)
        assert out is c
        torch.cuda.synchronize()
        _guards_untouched(buffers)
        _assert_equal(_numpy(c), R.padded(live, dict(want_cap, nnz_norm=cap.nnz_norm or 0), gs.n_feat), where)
        n = live["x"].shape[0]
        assert cap.n_rows - n == {"P=0": 0, "largest P, last filler partly filled": 14}.get(where, cap.n_rows - n)
    sizes = np.diff(c.graph_ptr.cpu().numpy())
    assert list(sizes[B:]) == [9, 0]               # the last case: a full filler, an empty one trailing at N
    # a fresh Collated (no `out`) gives the same
    fresh = ops.collate_graphs(gs, CASES["P=0"], BOTH, extras=extras, pad=cap)
    again = ops.collate_graphs(gs, CASES["P=0"], BOTH, out=c, extras=extras, pad=cap)
    _assert_equal(_numpy(fresh), _numpy(again), "fresh")


@pytest.mark.parametrize("with_extras", [False, True])
def test_wrong_offsets_write_nothing_outside_the_buffers(sets, with_extras):
    """Offsets too large, negative, or shifted: wrong contents, but every store inside [0, capacity)."""
    from sgracex1_amd import ops
    gs, extras = sets[with_extras]
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
        ops.collate_graphs(gs, index, BOTH, out=c, extras=extras, pad=cap)
        torch.cuda.synchronize()
        _guards_untouched(buffers)


def test_padded_collation_refusals(sets):
    from sgracex1_amd import ops, pyg_lite as G, sgrace
    gs, extras = sets[True]
    cap = ops.pad_capacity(gs, B)
    with pytest.raises(ValueError, match="does not fit"):
        ops.collate_graphs(gs, [1, 2], BOTH, pad=cap)
    small = ops.pad_capacity(gs, B, pad_rows=12)
    with pytest.raises(ValueError, match="does not fit"):
        ops.collate_graphs(gs, CASES["P=0"], BOTH, pad=small)
    with pytest.raises(ValueError, match="another capacity"):
        ops.collate_graphs(gs, CASES["P=0"], BOTH, out=ops.collate_graphs(gs, [0, 1, 5], BOTH, pad=small), pad=cap)
    with pytest.raises(ValueError, match="quant"):
        G.GraphLoader(gs, batch_size=B, prepare="sym_norm2", dtypes=(torch.float32,), quant=sgrace.quant.constants(8), pad=True)


def test_loader_batches_and_the_regrouped_plan(sets):
    from sgracex1_amd import ops, pyg_lite as G
    gs, _ = sets[False]
    plain = G.GraphLoader(gs, batch_size=B, shuffle=True, generator=torch.Generator().manual_seed(3), dtypes=BOTH)
    padded = G.GraphLoader(gs, batch_size=B, shuffle=True, generator=torch.Generator().manual_seed(3), dtypes=BOTH, pad=True)
    cap = padded.capacity
    for u, p in zip(plain, padded):
        n, real = u.num_nodes, u.num_graphs
        assert p.num_real_graphs == real and u.num_real_graphs == real
        assert same_bits(p.y[:real], u.y) and same_bits(p.x[:n], u.x) and same_bits(p.batch[:n], u.batch)
        if real == B:
            assert (p.num_graphs, p.num_nodes) == (cap.n_graphs, cap.n_rows)
        else:
            assert (p.num_graphs, p.num_nodes) == (real, n)         # the short last batch arrives unpadded
    # the plan cached for a padded Collated's buffers follows the next batch collated into them
    c = ops.collate_graphs(gs, CASES["P=0"], BOTH, pad=cap)
    b = G.attach_batch(c)
    adj = ops.recorded(b.edge_index, ("adj_csr", cap.n_rows, torch.float16))
    plan = ops.BatchPlan.cached(adj, c.graph_ptr, HIDDEN, ops._lib.SGX_BATCH_BACKWARD)
    assert plan.trusted and plan.fits and plan.max_graph == cap.filler_rows
    first = plan.export_groups().clone()
    ops.collate_graphs(gs, CASES["largest P, last filler partly filled"], BOTH, out=c, pad=cap)
    assert ops.BatchPlan.cached(adj, c.graph_ptr, HIDDEN, ops._lib.SGX_BATCH_BACKWARD) is plan
    fresh = ops.BatchPlan.known(c.graph_ptr, cap.n_rows, torch.float16, cap.filler_rows, HIDDEN, ops._lib.SGX_BATCH_BACKWARD)
    assert same_bits(plan.export_groups(), fresh.export_groups()) and not same_bits(first, fresh.export_groups())
    # by hand, and a plan that checked its batch on the device refuses
    ptr = c.graph_ptr.clone()
    mine = ops.BatchPlan.known(ptr, cap.n_rows, torch.float16, cap.filler_rows, HIDDEN)
    ptr.copy_(ops.collate_graphs(gs, CASES["P=0"], BOTH, pad=cap).graph_ptr)
    assert same_bits(mine.regroup(ptr).export_groups(),
                     ops.BatchPlan.known(ptr, cap.n_rows, torch.float16, cap.filler_rows, HIDDEN).export_groups())
    assert same_bits(mine.export_groups()[:-1].long(), torch.searchsorted(ptr.long(), torch.arange(plan.groups, device=DEV)))
    with pytest.raises(ops._lib.SgxError) as e:
        ops.BatchPlan(adj, c.graph_ptr, HIDDEN).regroup(c.graph_ptr)
    assert e.value.status == -3


@pytest.fixture
def sgrace_env():
    from sgracex1_amd import config, sgrace
    saved = config.snapshot()
    config.acc, config.float_type, config.compute_attention = 1, np.float32, 1
    ip = sgrace.init_SGRACE()
    ip.register_map.layer_count = 2
    yield sgrace
    config.restore(saved)
    sgrace.init_SGRACE()


def _model(kind, sgrace=None):
    if kind == "gat":
        torch.manual_seed(12345)
        return sgrace.GAT_POOL_PYNQ(7, HIDDEN, 2, train_stack=True).to(DEV).train()
    from sgracex1_amd import molecule_gcn as M, pynq_shim
    ip = pynq_shim.Overlay("gnn_all.bit").mmult_top_0
    ip.register_map.layer_count = 2
    return M.GCN_PYNQ(HIDDEN, 7, 2, ip, train_stack=True).to(DEV).train()


def _loaders(kind, graphs, **kw):
    """(plain, padding) GraphLoaders over the same new set, as the model of `kind` takes its batches."""
    from sgracex1_amd import ops, pyg_lite as G
    gs = ops.GraphSet(graphs)
    opts = dict(batch_size=B, dtypes=(torch.float32,), prepare="sym_norm2") if kind == "gat" else dict(batch_size=B)
    return G.GraphLoader(gs, **opts, **kw), G.GraphLoader(gs, pad=True, **opts, **kw)


def test_gcn_stack_fp32_forward_on_a_padded_batch(sets):
    """ops.GcnStack in float32 (GCN_PYNQ itself is a float16 model): pooled[:B] bit-equal, pooled[B:] == 0."""
    from sgracex1_amd import ops
    gs, _ = sets[False]
    cap = ops.pad_capacity(gs, B)
    torch.manual_seed(1)
    Ws = [torch.randn(7, HIDDEN, device=DEV) * 0.3, torch.randn(HIDDEN, HIDDEN, device=DEV) * 0.3]
    wts = [w.t().contiguous() for w in Ws]
    pooled = []
    for pad in (None, cap):
        c = ops.collate_graphs(gs, [0, 4, 6], BOTH, pad=pad)
        n = c.x.shape[0]
        adj = ops.Csr(c.adj_rowptr, c.adj_col, c.adj_val[torch.float32], n)
        fea = ops.Csr(c.fea_rowptr, c.fea_col, c.fea_val[torch.float32], 7)
        pooled.append(ops.gcn_stack_forward(adj, fea, wts, [True, False], c.graph_ptr))
    assert same_bits(pooled[1][:B], pooled[0]) and not pooled[1][B:].any() and pooled[1].shape[0] == cap.n_graphs
    assert bool(pooled[0].abs().sum() > 0)


@pytest.mark.parametrize("kind", ["gcn", "gat"])
def test_forward_and_one_step_on_a_padded_batch(kind, sgrace_env):
    """pooled[:B] of the padded batch bit-equal to the unpadded batch's, pooled[B:] == 0; the first step's loss and head
    gradients bit-equal; the stack's gradients inside the bounds derived for the UNPADDED batch (the padded batch's
    groups differ, so the partial sums may round differently)."""
    from sgracex1_amd import ops, train
    from test_gpu_trainer import _f64, _stack_reference
    graphs = P.torch_graphs()
    ids = [1, 2, 5] if kind == "gat" else [0, 4, 6]             # GCN: the graph without an edge, repeated edges, an isolated node
    plain, padding = _loaders(kind, graphs[:R.N_SET])
    u, p = plain.collate(ids), padding.collate(ids)
    assert p.num_graphs == padding.capacity.n_graphs > B and p.num_real_graphs == B
    model = _model(kind, sgrace_env)
    start = {k: v.clone() for k, v in model.state_dict().items()}
    of = _stack_reference(model, u, sgrace_env if kind == "gat" else None)
    pooled_u, pooled_p = (model.train_pooled(b.x, b.edge_index, b.batch) for b in (u, p))
    assert pooled_u is not None and pooled_p is not None
    assert same_bits(pooled_p.detach()[:B], pooled_u.detach()) and not pooled_p.detach()[B:].any()
    t0 = torch.zeros(1, dtype=torch.int64, device=DEV)
    _, gp, _, _ = ops.head_loss(pooled_u.detach(), model.lin.weight, model.lin.bias, u.y, p=0.5, seed=7, step_dev=t0)
    ref, bound, _ = of(_f64(gp))
    runs = []
    for b in (u, p):
        model.load_state_dict(start)
        trainer = train.StackTrainer(model, lr=0.01, p_drop=0.5, seed=7)
        loss = trainer.step(b.x, b.edge_index, b.batch, b.y, b.num_real_graphs)
        assert trainer.fused_steps == 1
        runs.append((loss.clone(), dict(zip([n for n, q in model.named_parameters() if q.requires_grad], trainer.last_grads))))
    (loss_u, g_u), (loss_p, g_p) = runs
    assert same_bits(loss_u, loss_p)
    for name in ("lin.weight", "lin.bias"):
        assert same_bits(g_u[name], g_p[name]), name
    assert ref
    for name in ref:
        for g in (g_u, g_p):
            err = np.abs(_f64(g[name]).reshape(ref[name].shape) - ref[name])
            print(kind, name, "padded" if g is g_p else "unpadded", "error / bound", float((err / bound[name]).max()))
            assert (err <= bound[name]).all(), name


@pytest.mark.parametrize("kind", ["gcn", "gat"])
def test_two_epochs_replayed_against_eager_steps(kind, sgrace_env):
    from sgracex1_amd import train
    graphs = P.torch_graphs()
    graphs = [graphs[i] for i in NO_DEAD] if kind == "gat" else graphs[:R.N_SET]
    runs, start = [], None
    for replayed in (False, True):
        _, loader = _loaders(kind, graphs, shuffle=True, generator=torch.Generator().manual_seed(11))
        model = _model(kind, sgrace_env)
        if start is None:
            start = {k: v.clone() for k, v in model.state_dict().items()}
        model.load_state_dict(start)
        trainer = train.StackTrainer(model, lr=0.01, p_drop=0.5, seed=99)
        losses = []
        if replayed:
            epoch = trainer.capture_loader(loader)
            assert int(trainer.t.item()) == 0
            mode = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")
            try:
                for _ in range(2):
                    losses += [loss.clone() for loss in epoch()]
            finally:
                torch.cuda.set_sync_debug_mode(mode)
        else:
            for _ in range(2):
                for b in loader:
                    losses.append(trainer.step(b.x, b.edge_index, b.batch, b.y, b.num_real_graphs).clone())
            assert trainer.fused_steps == len(losses)
        torch.cuda.synchronize()
        runs.append((losses, trainer.state(), trainer.fused_steps))
    (le, se, _), (lr, sr, fused) = runs
    assert len(le) == len(lr) == 6 and int(sr[-1].item()) == 6           # 7 graphs at B = 3: 3 + 3 + 1, twice
    assert all(same_bits(a, c) for a, c in zip(le, lr))
    assert all(same_bits(a, c) for a, c in zip(se, sr))
    assert not same_bits(lr[0], lr[1])
    assert fused == 2 + 2                         # the warm-up's two steps, and the short batch of each epoch run eagerly


def test_dead_row_batches_arrive_unpadded_and_replay_around_them(sgrace_env):
    """Graphs 0 and 6 of the set have a dead row under sym_norm2, so the fused attention route declines their batches.
    The padding loader hands such a batch over UNPADDED -- the very tensors of the plain loader's batch, so its step is
    the unpadded batch's step bit for bit -- and an epoch of capture_loader runs it eagerly between the replays: two
    epochs against eager steps over the same loader, bit for bit."""
    from sgracex1_amd import train
    graphs = P.torch_graphs()[:R.N_SET]
    plain, padding = _loaders("gat", graphs)
    dead_ids, live_ids = [0, 2, 3], [1, 2, 5]
    assert not padding.padded(dead_ids) and padding.padded(live_ids) and not padding.padded([6, 1, 2])
    u, p = plain.collate(dead_ids), padding.collate(dead_ids)
    assert p.num_graphs == p.num_real_graphs == B
    for name in ("x", "edge_index", "y", "batch"):
        assert same_bits(getattr(u, name), getattr(p, name)), name
    model = _model("gat", sgrace_env)
    start = {k: v.clone() for k, v in model.state_dict().items()}
    steps = []
    for b in (u, p):
        model.load_state_dict(start)
        trainer = train.StackTrainer(model, lr=0.01, p_drop=0.5, seed=3)
        loss = trainer.step(b.x, b.edge_index, b.batch, b.y, b.num_real_graphs)
        assert trainer.fused_steps == 0                                     # declined: the layers one by one
        steps.append([loss.clone()] + trainer.state())
    assert all(same_bits(a, c) for a, c in zip(*steps))
    runs = []
    # what the two epochs hold, by the loader's permutation rule: per batch whether a graph of it has a dead row
    g = torch.Generator().manual_seed(1)
    has_dead = [bool({0, 6} & set(order[i:i + B])) for order in (torch.randperm(R.N_SET, generator=g).tolist() for _ in range(2))
                for i in range(0, R.N_SET, B)]
    full_dead, full_live = sum(has_dead[0:2] + has_dead[3:5]), 4 - sum(has_dead[0:2] + has_dead[3:5])
    short_live = 2 - has_dead[2] - has_dead[5]
    assert full_dead >= 1 and full_live >= 1                                # both kinds of full batch occur
    for leg in ("eager", "replayed"):
        _, loader = _loaders("gat", graphs, shuffle=True, generator=torch.Generator().manual_seed(1))
        model.load_state_dict(start)
        trainer = train.StackTrainer(model, lr=0.01, p_drop=0.5, seed=99)
        losses = []
        if leg == "replayed":
            epoch = trainer.capture_loader(loader)
            for _ in range(2):
                losses += [loss.clone() for loss in epoch()]
            assert trainer.fused_steps == 2 + short_live                    # the warm-up; the replays count nothing
        else:
            for _ in range(2):
                for e in loader:
                    losses.append(trainer.step(e.x, e.edge_index, e.batch, e.y, e.num_real_graphs).clone())
            assert trainer.fused_steps == full_live + short_live
        torch.cuda.synchronize()
        runs.append((losses, trainer.state()))
    (le, se), (lr, sr) = runs
    assert len(lr) == 6 and int(sr[-1].item()) == 6
    assert all(same_bits(a, c) for a, c in zip(le, lr)) and all(same_bits(a, c) for a, c in zip(se, sr))


def test_step_refuses_a_padded_batch_the_fused_route_declines(sets, sgrace_env):
    """A padded batch never runs layer by layer: collated by hand with a dead-row graph, step() raises and changes nothing."""
    from sgracex1_amd import ops, pyg_lite as G, train
    gs = ops.GraphSet(P.torch_graphs()[:R.N_SET])
    extras = gs.prepare_sym_norm2((torch.float32,))
    b = G.attach_batch(ops.collate_graphs(gs, [0, 2, 3], (torch.float32,), extras=extras, pad=ops.pad_capacity(gs, B)))
    model = _model("gat", sgrace_env)
    trainer = train.StackTrainer(model, lr=0.01)
    before = trainer.state()
    with pytest.raises(RuntimeError, match="declined a padded batch"):
        trainer.step(b.x, b.edge_index, b.batch, b.y, b.num_real_graphs)
    assert all(same_bits(a, c) for a, c in zip(before, trainer.state())) and trainer.fused_steps == 0


def test_capture_loader_names_why_the_fused_route_declined():
    from sgracex1_amd import train
    _, loader = _loaders("gcn", P.torch_graphs()[:R.N_SET])
    model = _model("gcn")
    model.train_stack = False
    with pytest.raises(RuntimeError, match="train_stack"):
        train.StackTrainer(model).capture_loader(loader)
    plain, _ = _loaders("gcn", P.torch_graphs()[:R.N_SET])
    with pytest.raises(ValueError, match="pad=True"):
        train.StackTrainer(model).capture_loader(plain)

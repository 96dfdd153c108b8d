"""sgx_keep_best on the device (include/sgx.h, "model selection") against tests/_keep_best_ref.py: the copy at every
alignment of source and snapshot inside guard bands, bit for bit on NaN, -0.0, denormal and largest-finite patterns, the
state and the log after every call of the hand sequence; one recorded train.BestTracker.update replayed over that sequence
against eager calls; NodeTrainer and StackTrainer runs with the tracker under set_sync_debug_mode("error") against a twin
that does the loop on the host; restore() against a freshly built model; and the node example with --keep-best."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

import _graph_prep_ref as P
import _keep_best_ref as R
import _node_eval_ref as N

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 61                                        # elements of sentinel in front of and behind every array, at the least
SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 1027]
SENTINEL32, SENTINEL64 = 0x5A5A5A5A, -0x0123456789ABCDEF
SPECIAL = np.array([0x7FC00001, 0xFFFFFFFF, 0x7F800001, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000000],
                   dtype=np.uint32)              # quiet and signalling NaN, -0.0, denormals, the largest finite values, +0.0


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


class Banded:
    """n words (float32 seen as int32, or int64) inside a buffer of sentinels, the first of them `off` elements behind a
    16-byte boundary (float32) and at least GUARD elements from either end."""

    def __init__(self, n, off=0, dtype=torch.float32):
        self.n, self.wide = n, dtype == torch.int64
        raw = torch.int64 if self.wide else torch.int32
        self.start = GUARD + (off - GUARD) % 4
        self.whole = torch.full((self.start + n + GUARD + 3,), SENTINEL64 if self.wide else SENTINEL32, dtype=raw, device=DEV)
        assert self.whole.data_ptr() % 16 == 0
        self.raw = self.whole[self.start:self.start + n]
        self.view = self.raw if self.wide else self.raw.view(torch.float32)
        assert self.wide or n == 0 or (self.view.data_ptr() % 16) // 4 == off

    def set(self, words):
        self.raw.copy_(torch.from_numpy(np.asarray(words).astype(np.uint32).view(np.int32) if not self.wide
                                        else np.asarray(words, dtype=np.int64)).to(DEV))

    def get(self):
        host = self.raw.cpu().numpy()
        return host.copy() if self.wide else host.view(np.uint32).copy()

    def guards_untouched(self):
        want = SENTINEL64 if self.wide else SENTINEL32
        return bool((self.whole[:self.start] == want).all()) and bool((self.whole[self.start + self.n:] == want).all())


def _words(n, e, k):
    """The source of tensor k at call e: random bits with the special patterns spread over head, body and tail."""
    rng = np.random.default_rng(1000 * e + k)
    w = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if n:
        at = rng.permutation(n)[:min(n, len(SPECIAL))]
        w[at] = SPECIAL[:len(at)]
        w[0], w[-1] = SPECIAL[e % len(SPECIAL)], SPECIAL[(e + k) % len(SPECIAL)]
    return w


def _sums_of(e, n, hits, n_sums):
    """The EvalSums words of call e: the deciding counts, the bits of a loss sum, then passes that do not decide."""
    rows = [[n, hits, int(np.float64(0.1 * (e + 1)).view(np.int64))]]
    rows += [[7 + k, e + k, int(np.float64(-1.5 * e - k).view(np.int64))] for k in range(1, n_sums)]
    return np.array(rows, dtype=np.int64)


def _drive(sizes, offsets, n_sums, log_rows):
    """The hand sequence through ops.keep_best on banded arrays, checked against the restatement after every call."""
    from sgracex1_amd import ops
    src = [Banded(n, so) for n, (so, _) in zip(sizes, offsets)]
    dst = [Banded(n, do) for n, (_, do) in zip(sizes, offsets)]
    sums = [Banded(3, dtype=torch.int64) for _ in range(n_sums)]
    state, log = Banded(4, dtype=torch.int64), None if log_rows is None else Banded(log_rows * 3 * n_sums, dtype=torch.int64)
    state.set(R.fresh_state())
    want_dst = [_words(n, 99, k) for k, n in enumerate(sizes)]
    for d, w in zip(dst, want_dst):
        d.set(w)
    want_state = R.fresh_state()
    want_log = None if log_rows is None else np.full((log_rows, 3 * n_sums), SENTINEL64, dtype=np.int64)
    log_view = None if log is None else log.view.view(log_rows, 3 * n_sums)
    for e, (n, hits) in enumerate(R.SEQUENCE):
        words = [_words(m, e, k) for k, m in enumerate(sizes)]
        for s, w in zip(src, words):
            s.set(w)
        rows = _sums_of(e, n, hits, n_sums)
        for s, row in zip(sums, rows):
            s.set(row)
        ops.keep_best([s.view for s in src], [d.view for d in dst], [s.view for s in sums], state.view, log_view)
        won = R.keep_best(words, want_dst, list(rows), want_state, want_log)
        assert won == (e in (1, 3, 5))
        assert (state.get() == want_state).all(), (e, state.get(), want_state)
        for k, (d, w) in enumerate(zip(dst, want_dst)):
            assert np.array_equal(d.get(), w), (e, k, sizes[k], offsets[k])
        for k, (s, w) in enumerate(zip(src, words)):
            assert np.array_equal(s.get(), w), (e, k)                 # the sources are only read
        if log is not None:
            assert np.array_equal(log.get().reshape(want_log.shape), want_log), e
        for band in src + dst + sums + [state] + ([log] if log is not None else []):
            assert band.guards_untouched(), e
    assert tuple(want_state) == (2, 1, 5, len(R.SEQUENCE))


@pytest.mark.parametrize("src_off", range(4))
@pytest.mark.parametrize("dst_off", range(4))
def test_every_alignment_against_the_restatement(src_off, dst_off):
    """9 tensors of 0 .. 1027 floats, each at this pair of offsets from the 16-byte grid: head, body and tail of the vector
    copy are each empty for some tensor and non-empty for another; two sums, a log with a row for every call."""
    _drive(SIZES, [(src_off, dst_off)] * len(SIZES), 2, len(R.SEQUENCE))


@pytest.mark.parametrize("n_sums,log_rows", [(1, len(R.SEQUENCE)), (4, len(R.SEQUENCE)), (2, None), (2, 4), (4, 0)],
                         ids=["one-sum", "four-sums", "no-log", "short-log", "empty-log"])
def test_sums_and_logs(n_sums, log_rows):
    """A log shorter than the call count: the rows past it are not written and the state still advances."""
    offsets = [(k % 4, (k // 2) % 4) for k in range(len(SIZES))]
    _drive(SIZES, offsets, n_sums, log_rows)


def test_sixteen_tensors():
    _drive([5] * 16, [(k % 4, (k // 4) % 4) for k in range(16)], 1, 3)


def test_ops_checks_on_the_device():
    from sgracex1_amd import ops
    f = lambda n=4, dtype=torch.float32: torch.zeros(n, dtype=dtype, device=DEV)
    state, sums = torch.tensor([1, 0, -1, 0], device=DEV), [torch.zeros(3, dtype=torch.int64, device=DEV)]
    p = f()
    for params, snap, exc in (([p], [p], ValueError), ([f()], [f(5)], ValueError), ([f(4, torch.float16)], [f()], ValueError),
                              ([f(8)[::2]], [f()], ValueError), ([f()], [torch.zeros(4)], ValueError)):
        with pytest.raises(exc):
            ops.keep_best(params, snap, sums, state)
    for bad_state in (state.int(), state[:3]):
        with pytest.raises(TypeError):
            ops.keep_best([f()], [f()], sums, bad_state)
    with pytest.raises(TypeError):
        ops.keep_best([f()], [f()], [torch.zeros(2, dtype=torch.int64, device=DEV)], state)
    with pytest.raises(TypeError):
        ops.keep_best([f()], [f()], sums, state, log=torch.zeros((3, 4), dtype=torch.int64, device=DEV))
    assert state.tolist() == [1, 0, -1, 0]


# ---- capture ------------------------------------------------------------------------------------------------------------
class _Holder:
    """What train.BestTracker reads of a trainer."""

    def __init__(self, params):
        self.params, self.model = params, None


def test_a_recorded_update_replays_as_eager_calls():
    from sgracex1_amd.train import BestTracker, EvalSums
    sizes = [5, 64, 1027, 3]
    calls = len(R.SEQUENCE)
    sources = [[torch.from_numpy(_words(n, e, k).view(np.int32)).to(DEV).view(torch.float32) for k, n in enumerate(sizes)]
               for e in range(calls)]
    rows = torch.from_numpy(np.stack([_sums_of(e, n, hits, 1)[0] for e, (n, hits) in enumerate(R.SEQUENCE)])).to(DEV)
    runs = []
    for recorded in (False, True):
        params = [torch.zeros(n, device=DEV) for n in sizes]
        sums = EvalSums(DEV)
        tracker = BestTracker(_Holder(params), epochs=calls - 2)
        step = lambda: tracker.update(sums)
        if recorded:
            # (the eager leg ran first: the kernels are loaded; the recording itself computes nothing)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            step = graph.replay
            assert tracker.state.tolist() == list(R.FRESH)
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for e in range(calls):
                sums.buffer.copy_(rows[e])                            # device to device, between two replays
                for p, s in zip(params, sources[e]):
                    p.copy_(s)
                step()
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        runs.append(([s.clone() for s in tracker.snapshot], tracker.state.clone(), tracker.log.clone(), tracker.read()))
    (snap_e, state_e, log_e, read_e), (snap_r, state_r, log_r, read_r) = runs
    assert all(same_bits(a, b) for a, b in zip(snap_e, snap_r)) and same_bits(state_e, state_r) and same_bits(log_e, log_r)
    assert state_r.tolist() == [2, 1, 5, calls] and all(same_bits(s, src) for s, src in zip(snap_r, sources[5]))
    best_epoch, best_n, best_hits, done, log = read_r
    assert (best_epoch, best_n, best_hits, done) == (5, 2, 1, calls) and len(log) == calls - 2
    assert log == read_e[4] and log[3] == [(5, 2, 0.1 * 4)]


# ---- the trainers end to end ----------------------------------------------------------------------------------------------
EPOCHS = 6
# (trainer seed, lr) per configuration: chosen with the host twin alone so that the best epoch is neither the first nor the
# last -- the test asserts that, since it could not tell "best" from "last" otherwise
NODE_SEEDS = {0: (1, 0.05), 1: (5, 0.01)}
STACK_SEED = (99, 0.05)


@pytest.fixture(params=[0, 1], ids=["gcn", "att"])
def node_env(request):
    from sgracex1_amd import config, sgrace
    gat = request.param
    saved = config.snapshot()
    config.acc, config.accb, config.compute_attention = 1, 0, gat
    config.float_type = np.float32
    config.fake_quantization = config.hardware_quantize = 0
    config.w_qbits, config.gat_edge_outputs, config.device = 32, 1, "cuda"
    sgrace.init_SGRACE()
    yield sgrace, gat
    config.restore(saved)
    sgrace.init_SGRACE()


def _node_setup(sgrace, gat, seed, lr, start=None):
    """(trainer, the recorded epoch, [the pass that decides (test nodes), a second pass (training nodes)] -- each returns
    its EvalSums --, their loaders)"""
    from sgracex1_amd import pyg_lite
    from sgracex1_amd.train import NodeTrainer
    torch.manual_seed(5)
    data = N.node_data(DEV)
    model = sgrace.GAT_PYNQ(N.N_FEATURES, N.HIDDEN, 1, N.N_CLASSES).to(DEV).train()
    if start is not None:
        model.load_state_dict(start)
    trainer = NodeTrainer(model, lr=lr, weight_decay=5e-4, seed=seed)
    loader = lambda split, shuffle: pyg_lite.NeighborLoader(
        data, N.FANOUTS, input_nodes=data.test_mask if split == "test" else data.train_mask,
        **N.loader_kwargs(gat, False, split, shuffle))
    evs = [loader("test", False), loader("train", False)]
    epoch = trainer.capture_loader(loader("train", True))
    passes = [trainer.capture_eval_loader(ev) for ev in evs]
    return trainer, epoch, passes, evs


def _stack_setup(seed, lr, start=None):
    from sgracex1_amd import molecule_gcn as M, ops, pyg_lite as G, pynq_shim, train
    graphs = P.torch_graphs()[:7]
    ip = pynq_shim.Overlay("gnn_all.bit").mmult_top_0
    ip.register_map.layer_count = 2
    model = M.GCN_PYNQ(16, 7, 2, ip, train_stack=True).to(DEV).train()
    if start is not None:
        model.load_state_dict(start)
    trainer = train.StackTrainer(model, lr=lr, p_drop=0.5, seed=seed)
    gs = ops.GraphSet(graphs)
    epoch = trainer.capture_loader(G.GraphLoader(gs, batch_size=3, shuffle=True, generator=torch.Generator().manual_seed(11), pad=True))
    ev = G.GraphLoader(gs, batch_size=3, shuffle=False, pad=True)
    run_pass = trainer.capture_eval_loader(ev)

    def one():
        run_pass()
        return run_pass.sums

    return trainer, epoch, [one], [ev]


def _rewind(loaders, first, epoch):
    """The passes of `epoch` drew their samples from the loaders' epoch numbers first + epoch (graph loaders have none)."""
    for ev, f in zip(loaders, first):
        if f is not None:
            ev.epoch = f + epoch


def host_loop(setup):
    """The twin: EvalSums.read per epoch, the float comparison replaced by the same integer rule, a deep copy of the
    state dict on a win, load_state_dict behind the loop -> (best epoch, the saved state dict, the log, the final pass)."""
    from sgracex1_amd.train import EvalSums
    trainer, epoch, passes, loaders = setup
    first = [getattr(ev, "epoch", None) for ev in loaders]
    best, saved, log = (1, 0, -1), None, []
    for e in range(EPOCHS):
        epoch()
        rows = EvalSums.read(*[p() for p in passes])
        log.append(rows)
        if R.better(rows[0][0], rows[0][1], best[0], best[1]):
            best, saved = (rows[0][0], rows[0][1], e), copy.deepcopy(trainer.model.state_dict())
    if saved is not None:
        trainer.model.load_state_dict(saved)
    _rewind(loaders, first, max(best[2], 0))
    return best, saved, log, passes[0]().buffer.clone()


def device_loop(setup):
    trainer, epoch, passes, loaders = setup
    first = [getattr(ev, "epoch", None) for ev in loaders]
    tracker = trainer.track_best(EPOCHS)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                   # from the first epoch to the last
    try:
        for _ in range(EPOCHS):
            epoch()
            tracker.update(*[p() for p in passes])
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    last = [p.detach().clone() for p in trainer.params]
    best_epoch, best_n, best_hits, done, log = tracker.read()
    assert done == EPOCHS
    snapshot = tracker.state_dict()
    moments = [t.clone() for t in (*trainer.exp_avg, *trainer.exp_avg_sq, trainer.t)]
    tracker.restore()
    assert all(same_bits(a, b) for a, b in zip(moments, (*trainer.exp_avg, *trainer.exp_avg_sq, trainer.t)))
    assert all(same_bits(p.detach(), s) for p, s in zip(trainer.params, tracker.snapshot))
    assert not all(same_bits(p.detach(), q) for p, q in zip(trainer.params, last))        # best is not last
    _rewind(loaders, first, max(best_epoch, 0))
    return (best_n, best_hits, best_epoch), snapshot, log, passes[0]().buffer.clone()


def _compare(make):
    # both legs start from the same bits: the layers' never-used `bias` parameters are allocated and never initialised, so
    # two models built alike differ in them
    host = make(None)
    device = make(copy.deepcopy(host[0].model.state_dict()))
    (best_h, saved, log_h, final_h), (best_d, snapshot, log_d, final_d) = host_loop(host), device_loop(device)
    print("host twin: best", best_h, "deciding counts per epoch", [row[0][:2] for row in log_h])
    assert best_d == best_h
    assert 0 < best_h[2] < EPOCHS - 1, "the seeds must put the best epoch strictly inside the run"
    assert log_d == log_h
    assert set(snapshot) <= set(saved) and len(snapshot) > 0
    for name, s in snapshot.items():
        assert same_bits(s, saved[name]), name
    assert same_bits(final_d, final_h)
    assert tuple(final_d[:2].tolist()) == log_h[best_h[2]][0][:2]           # the restored model is the best epoch's model


def test_node_trainer_keeps_the_best_epoch(node_env):
    sgrace, gat = node_env
    seed, lr = NODE_SEEDS[gat]
    _compare(lambda start: _node_setup(sgrace, gat, seed, lr, start))


def test_stack_trainer_keeps_the_best_epoch():
    _compare(lambda start: _stack_setup(*STACK_SEED, start))


def test_restore_behind_a_fused_forward():
    """The model has run its fused eval forward on the weights of the moment, so whatever that route derives from them
    (the transposed fp16 copies) exists; after restore() the same forward equals a freshly built model's with the snapshot
    loaded, bit for bit."""
    from sgracex1_amd import pyg_lite as G
    from sgracex1_amd.train import EvalSums
    trainer, _, _, _ = _stack_setup(3, 0.05)
    model = trainer.model
    b = G.collate(P.torch_graphs()[:7]).to(DEV)

    def fused(m):
        m.eval()
        with torch.no_grad():
            out = m.eval_pooled(b.x, b.edge_index, b.batch)
        m.train()
        assert out is not None
        return out.clone()

    tracker = trainer.track_best()
    for _ in range(3):
        trainer.step(b.x, b.edge_index, b.batch, b.y)
    at_snapshot = fused(model)
    sums = EvalSums(DEV)
    sums.totals.copy_(torch.tensor([7, 4], device=DEV))
    tracker.update(sums)                                       # 4 / 7 beats 0 / 1: the weights of this moment are kept
    for _ in range(3):
        trainer.step(b.x, b.edge_index, b.batch, b.y)
    moved = fused(model)                                       # the route's derived copies are now those of the moved weights
    assert not same_bits(moved, at_snapshot)
    tracker.update(sums)                                       # a tie: not kept
    tracker.restore()
    restored = fused(model)
    fresh, _, _, _ = _stack_setup(3, 0.05)
    fresh.model.load_state_dict(tracker.state_dict())
    assert same_bits(restored, fused(fresh.model)) and same_bits(restored, at_snapshot)
    assert tracker.read()[:4] == (0, 7, 4, 2)


# ---- the example ----------------------------------------------------------------------------------------------------------
def _example(name):
    spec = importlib.util.spec_from_file_location(f"_example_{name}", os.path.join(ROOT, "examples", f"{name}.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_the_node_example_with_keep_best():
    from sgracex1_amd import config, sgrace
    example = _example("sgrace_node_classification")
    saved = config.snapshot()
    try:
        kw = dict(epochs=4, n=600, seed=1, verbose=False, batch_size=64, num_neighbors=[5, 5], device_batches=True, trainer=True,
                  replay=True)
        plain, _, _ = example.run(**kw)
        kept, _, _ = example.run(keep_best=True, **kw)
    finally:
        config.restore(saved)
        sgrace.init_SGRACE()
    assert kept["epoch_loss"] == plain["epoch_loss"] and kept["test_acc"] == plain["test_acc"]
    assert "restored_test_acc" not in plain and len(kept["epoch_acc"]) == 4
    assert 0 <= kept["best_epoch"] < 4
    assert kept["restored_test_acc"] == kept["epoch_acc"][kept["best_epoch"]][1] == kept["test_acc"]
    vals = [v for v, _ in kept["epoch_acc"]]
    assert kept["best_epoch"] == vals.index(max(vals))        # the first epoch that reaches the best validation accuracy


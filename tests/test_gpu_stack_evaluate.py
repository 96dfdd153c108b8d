"""train.StackTrainer.evaluate and capture_eval_loader on MUTAG (tests/golden/mutag_raw.npz), GCN_PYNQ in fp16 and
GAT_POOL_PYNQ in fp32 from a prepared loader: the hit count against the model's own eval forward, a pass over a padded
unshuffled loader (short last batch included) against the whole set, the replayed pass against the eager one bit for bit
under set_sync_debug_mode("error"), and the trainer's state and the model's mode left as they were."""
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
KINDS = ["gcn", "gat"]
BATCH = 64


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.fixture(scope="module")
def graphs():
    from sgracex1_amd import pyg_lite as G
    raw = np.load(os.path.join(GOLD, "mutag_raw.npz"))
    return G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])


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


def _model(kind, sgrace):
    """(model in training mode, its own forward)"""
    if kind == "gat":
        torch.manual_seed(12345)
        return sgrace.GAT_POOL_PYNQ(7, 64, 2, train_stack=True).to(DEV).train(), (lambda m, b: m(b.x, b.edge_index, b.batch))
    from sgracex1_amd import molecule_gcn as M, pynq_shim
    ip = pynq_shim.Overlay("gnn_all.bit").mmult_top_0
    ip.register_map.layer_count = 2
    return M.GCN_PYNQ(64, 7, 2, ip, train_stack=True).to(DEV).train(), (lambda m, b: m(1, b.x, b.edge_index, b.batch))


def _loader(kind, graphs, pad=True):
    from sgracex1_amd import ops, pyg_lite as G
    opts = dict(dtypes=(torch.float32,), prepare="sym_norm2") if kind == "gat" else {}
    return G.GraphLoader(ops.GraphSet(graphs), batch_size=BATCH, shuffle=False, pad=pad, **opts)


def _whole(graphs):
    from sgracex1_amd import pyg_lite as G
    return G.collate(graphs).to(DEV)


@pytest.mark.parametrize("kind", KINDS)
def test_evaluate_counts_what_the_models_forward_predicts(kind, graphs, sgrace_env):
    from sgracex1_amd import train
    model, forward = _model(kind, sgrace_env)
    trainer = train.StackTrainer(model, lr=0.01)
    b = _whole(graphs)
    for _ in range(30):                                                  # (a model that tells the classes apart; moments and t away from zero)
        trainer.step(b.x, b.edge_index, b.batch, b.y)
    before = trainer.state()
    for training in (True, False):
        model.train(training)
        totals, loss_sum = trainer.evaluate(b.x, b.edge_index, b.batch, b.y)
        assert model.training is training                                # the mode is put back
        assert totals.is_cuda and loss_sum.is_cuda and totals.dtype == torch.int64 and loss_sum.dtype == torch.float64
        model.eval()
        with torch.no_grad():
            logits = forward(model, b)
        hits = int((logits.argmax(1) == b.y).sum())
        print(kind, "totals", totals.tolist(), "the model's hits", hits, "loss_sum", float(loss_sum.cpu()[0]))
        assert totals.tolist() == [len(graphs), hits]
        assert 0 < hits < len(graphs)                                    # (the check can tell a right count from a trivial one)
        assert np.isfinite(float(loss_sum.cpu()[0])) and float(loss_sum.cpu()[0]) > 0
    model.train()
    assert all(same_bits(a, c) for a, c in zip(before, trainer.state()))  # parameters, moments, t: byte for byte


@pytest.mark.parametrize("kind", KINDS)
def test_a_pass_over_a_padded_loader_is_the_whole_set(kind, graphs, sgrace_env):
    from sgracex1_amd import train
    model, _ = _model(kind, sgrace_env)
    trainer = train.StackTrainer(model, lr=0.01)
    b = _whole(graphs)
    want, _ = trainer.evaluate(b.x, b.edge_index, b.batch, b.y)
    sums = train.EvalSums(DEV)
    sizes = []
    for e in _loader(kind, graphs):
        out = trainer.evaluate(e.x, e.edge_index, e.batch, e.y, e.num_real_graphs, into=sums)
        assert out[0] is sums.totals and out[1] is sums.loss_sum
        sizes.append((e.num_real_graphs, e.num_graphs))
    assert [n for n, _ in sizes] == [64, 64, 60] and sizes[0][1] > 64 and sizes[2] == (60, 60)    # two padded batches, a short last one
    assert sums.totals.tolist() == want.tolist()
    assert train.EvalSums.read(sums)[0][:2] == tuple(want.tolist())


@pytest.mark.parametrize("kind", KINDS)
def test_the_replayed_pass_is_the_eager_pass(kind, graphs, sgrace_env):
    from sgracex1_amd import train
    model, _ = _model(kind, sgrace_env)
    trainer = train.StackTrainer(model, lr=0.01)
    b = _whole(graphs)
    for _ in range(30):
        trainer.step(b.x, b.edge_index, b.batch, b.y)
    loader = _loader(kind, graphs)
    eager = train.EvalSums(DEV)
    for e in loader:
        trainer.evaluate(e.x, e.edge_index, e.batch, e.y, e.num_real_graphs, into=eager)
    before = trainer.state()
    run_pass = trainer.capture_eval_loader(loader)
    assert model.training
    got = []
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            totals, loss_sum = run_pass()
            got.append((totals.clone(), loss_sum.clone()))
        for _ in range(150):                                             # back to back, nothing read in between: a hand-off
            totals, loss_sum = run_pass()                                # inside the launch once lost whole batches this way
        got.append((totals.clone(), loss_sum.clone()))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    for totals, loss_sum in got:
        assert same_bits(totals, eager.totals) and same_bits(loss_sum, eager.loss_sum)
    assert eager.totals.tolist()[0] == len(graphs)                       # every graph exactly once
    assert model.training
    assert all(same_bits(a, c) for a, c in zip(before, trainer.state()))


def test_a_loader_that_does_not_pad_is_refused(graphs):
    from sgracex1_amd import train
    model, _ = _model("gcn", None)
    with pytest.raises(ValueError):
        train.StackTrainer(model).capture_eval_loader(_loader("gcn", graphs, pad=False))

"""train.StackTrainer on the device: one step against the autograd route and torch.optim.Adam inside the derived bounds
of tests/_train_tail_ref.py, a batch the fused route declines, the captured step replayed against eager steps bit for
bit under set_sync_debug_mode("error"), and 60 epochs of MUTAG to the accuracy the torch-tailed loop is held to."""
import os

import numpy as np
import pytest
import torch

import _gat_ref as R_GAT
import _train_tail_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _graphs():
    from sgracex1_amd import pyg_lite as G
    raw = np.load(os.path.join(GOLD, "mutag_raw.npz"))
    return G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])


def _mutag(n=None):
    from sgracex1_amd import pyg_lite as G
    graphs = _graphs()
    return G.collate(graphs[:n] if n else graphs).to(DEV)


@pytest.fixture
def sgrace_env():
    from sgracex1_amd import config, sgrace
    saved = config.snapshot()
    config.acc, config.float_type, config.compute_attention = 1, np.float32, 1
    ip = sgrace.init_SGRACE()
    ip.register_map.layer_count = 2
    yield ip, config, sgrace
    config.restore(saved)
    sgrace.init_SGRACE()


def _gcn():
    from sgracex1_amd import molecule_gcn as M, pynq_shim
    ip = pynq_shim.Overlay("gnn_all.bit").mmult_top_0
    ip.register_map.layer_count = 2
    return M.GCN_PYNQ(64, 7, 2, ip, train_stack=True).to(DEV).train(), (lambda m, b: m(1, b.x, b.edge_index, b.batch))


def _gat(sgrace):
    torch.manual_seed(12345)
    return sgrace.GAT_POOL_PYNQ(7, 64, 2, train_stack=True).to(DEV).train(), (lambda m, b: m(b.x, b.edge_index, b.batch))


def _f64(t):
    return t.detach().double().cpu().numpy()


def _stack_reference(model, b, sgrace=None):
    """What tests/_stack_grad_ref.py / tests/_gat_stack_grad_ref.py need of the model's fused route on batch b, and a
    function gp -> ({parameter name: float64 gradient}, {name: the kernel's bound against it}, {name: the magnitude the
    linear map gives |gp|}), all element-wise."""
    from sgracex1_amd import molecule_gcn as M, ops
    ptr = ops.graph_ptr_of(b.batch)
    if sgrace is None:
        from _gat_stack_grad_ref import gat_stack_grad_f64
        adj = ops.cached_on(b.edge_index, ("adj_csr", b.num_nodes, M.ACC_DTYPE),
                            lambda: ops.csr_from_edge_index(b.edge_index, b.num_nodes, dtype=M.ACC_DTYPE))
        layers = (model.conv1, model.conv2)
        wts = [c.weight.detach().t().to(M.ACC_DTYPE).contiguous() for c in layers]
        _, outs = ops.gcn_stack_forward(adj, M.feature_csr(b.x, M.ACC_DTYPE), wts, [True, False], ptr, want_layer_outputs=True)
        adj_np = (adj.rowptr.cpu().numpy(), adj.col.cpu().numpy(), _f64(adj.val)[:adj.nnz])
        x, Ws, outs_np = _f64(b.x), [_f64(c.weight) for c in layers], [_f64(D) for D in outs]

        def of(gp, sub=R_GAT.OUT_SUB["f16"]):
            # the GCN layers of the GAT restatement (atts None): tests/_stack_grad_ref.py's chain with the fp16 subnormal
            # term in its bound, which these pooled gradients (1e-3 over a graph's size) need
            r = gat_stack_grad_f64(adj_np, x, Ws, [None, None], [True, False], ptr.cpu().numpy(), gp, outs_np, unit=2.0 ** -11, sub=sub)
            names = ("conv1.weight", "conv2.weight")
            return (dict(zip(names, r["dW"])), {n: r["tW"][l] * r["mW"][l] + 1e-30 for l, n in enumerate(names)},
                    dict(zip(names, r["mW"])))
        return of
    from _gat_stack_grad_ref import gat_stack_grad_f64
    ei, norm = sgrace.sym_norm2(b.edge_index, b.num_nodes)
    adj = sgrace._edge_csr(None, ei, norm, b.num_nodes, torch.float32)
    layers = (model.att1, model.att2)
    fea = ops.Csr.from_dense(b.x.float(), torch.float32)
    _, outs = ops.gat_stack_forward(adj, fea, [c.weight.detach().t().contiguous() for c in layers],
                                    [c.attention.detach().reshape(-1).contiguous() for c in layers], [True, False], ptr,
                                    alpha=model.att1.alpha, want_layer_outputs=True)
    adj_np = (adj.rowptr.cpu().numpy(), adj.col.cpu().numpy(), _f64(adj.val)[:adj.nnz])
    x, Ws, atts = _f64(b.x), [_f64(c.weight) for c in layers], [_f64(c.attention).reshape(-1) for c in layers]
    outs_np = [_f64(D) for D in outs]

    def of(gp, sub=0.0):
        r = gat_stack_grad_f64(adj_np, x, Ws, atts, [True, False], ptr.cpu().numpy(), gp, outs_np, alpha=model.att1.alpha)
        ref, bd, mag = {}, {}, {}
        for l, name in enumerate(("att1", "att2")):
            ref[name + ".weight"], mag[name + ".weight"] = r["dW"][l], r["mW"][l]
            bd[name + ".weight"] = r["tW"][l] * r["mW"][l] + 1e-30
            ref[name + ".attention"], mag[name + ".attention"] = r["dA"][l], r["mA"][l]
            bd[name + ".attention"] = r["tA"][l] * r["mA"][l] + 1e-30
        return ref, bd, mag
    return of


def _one_step_checks(model, forward, b, sgrace=None):
    """trainer.step at p_drop = 0 against the model's own autograd route (dropout off: eval mode, gradients on) and
    torch.optim.Adam."""
    from sgracex1_amd import ops, train
    # the autograd route: the same fused stack, torch's Linear and cross entropy behind it
    model.eval()
    model.zero_grad(set_to_none=True)
    route, seen = model._train_stack, []

    def spy(*a):                                   # the gradient autograd hands the fused stack on that route
        pooled = route(*a)
        pooled.register_hook(lambda g: seen.append(g.detach().clone()))
        return pooled
    model._train_stack = spy
    try:
        torch.nn.functional.cross_entropy(forward(model, b), b.y).backward()
    finally:
        del model._train_stack
    (gp_auto,) = seen
    auto = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    model.train()
    model.zero_grad(set_to_none=True)
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    of = _stack_reference(model, b, sgrace)       # (reads the parameters now: the ones the step starts from)
    trainer = train.StackTrainer(model, lr=0.01, p_drop=0.0)
    # what the head is given, and what the stack's backward makes of the head's grad_pooled, from the same calls on the
    # same (still unchanged) parameters: the route is deterministic, so the step below works on these very bits
    params = dict(model.named_parameters())
    stack_names = [n for n in names if n in auto and not n.startswith("lin.")]
    with torch.enable_grad():
        pooled = model.train_pooled(b.x, b.edge_index, b.batch)
    assert pooled is not None
    _, gp, _, _ = ops.head_loss(pooled.detach(), params["lin.weight"], params["lin.bias"], b.y)
    again = dict(zip(stack_names, torch.autograd.grad(pooled, [params[n] for n in stack_names], gp)))
    pooled_np = pooled.detach().cpu().numpy()
    loss = trainer.step(b.x, b.edge_index, b.batch, b.y)
    torch.cuda.synchronize()
    assert trainer.fused_steps == 1 and int(trainer.t.item()) == 1
    grads = dict(zip(names, trainer.last_grads))
    assert {n for n, g in grads.items() if g is not None} == set(auto)
    # the head: both routes are fp32 evaluations of the same float64 function, each inside the derived bound of it
    W, bias = before["lin.weight"].cpu().numpy(), before["lin.bias"].cpu().numpy()
    r_loss, _, r_gp, r_gw, r_gb, aux = R.head_f64(pooled_np, W, bias, b.y.cpu().numpy())
    bound = R.head_bounds(aux)
    for name, ref, bd in (("lin.weight", r_gw, bound["grad_W"]), ("lin.bias", r_gb, bound["grad_bias"])):
        ours, torchs = grads[name].double().cpu().numpy(), auto[name].double().cpu().numpy()
        print(name, "trainer / bound", float((np.abs(ours - ref) / bd).max()), "autograd / bound", float((np.abs(torchs - ref) / bd).max()))
        assert (np.abs(ours - ref) <= bd).all() and (np.abs(ours - torchs) <= 2 * bd).all()
    assert abs(float(loss.item()) - r_loss) <= bound["loss"]
    # the stack: grad_pooled inside its bound, and the stack's gradients the stack's backward of exactly that grad_pooled
    assert (np.abs(gp.double().cpu().numpy() - r_gp) <= bound["grad_pooled"]).all()
    for n in stack_names:
        assert same_bits(grads[n], again[n]), n
    # ... and against the autograd route's .grad: the two routes hand the stack grad_pooleds that are both inside e_gp of
    # the float64 head, so they differ by at most 2 e_gp; the stack's backward is linear in grad_pooled, so its float64
    # results differ by at most its magnitude chain on 2 e_gp, and each device result is inside the kernel's own bound
    # of its float64 result (tests/_stack_grad_ref.py, tests/_gat_stack_grad_ref.py)
    e_gp = bound["grad_pooled"]
    assert (np.abs(_f64(gp) - _f64(gp_auto)) <= 2 * e_gp).all()
    ref_o, bd_o, _ = of(_f64(gp))
    _, bd_a, _ = of(_f64(gp_auto))
    _, _, mag = of(2 * e_gp, sub=0.0)             # the linear map alone: no rounding of its own in this term
    assert set(stack_names) == set(ref_o)
    for n in stack_names:
        ours, torchs = _f64(grads[n]).reshape(ref_o[n].shape), _f64(auto[n]).reshape(ref_o[n].shape)
        tol = mag[n] + bd_o[n] + bd_a[n]
        print(n, "trainer vs autograd / bound", float((np.abs(ours - torchs) / tol).max()), "trainer vs float64 / bound",
              float((np.abs(ours - ref_o[n]) / bd_o[n]).max()), "bound / |gradient|", float(np.median(tol) / np.median(np.abs(ref_o[n]))))
        assert (np.abs(ours - ref_o[n]) <= bd_o[n]).all(), n
        assert (np.abs(ours - torchs) <= tol).all(), n
    # Adam: the parameters against torch.optim.Adam on the gradients that reached the call
    twins = [before[n].clone().requires_grad_() for n in names]
    for tw, n in zip(twins, names):
        tw.grad = None if grads[n] is None else grads[n].clone()
    torch.optim.Adam(twins, lr=0.01).step()
    for tw, n in zip(twins, names):
        got = dict(model.named_parameters())[n].detach()
        if grads[n] is None:
            assert same_bits(got, before[n])
            continue
        z = np.zeros(before[n].numel())
        e_p, _, _ = R.adam_bound_step(before[n].double().cpu().numpy().ravel(), grads[n].double().cpu().numpy().ravel(), z, z, 1, lr=0.01)
        ref_p, _, _ = R.adam_f64(before[n].double().cpu().numpy().ravel(), grads[n].double().cpu().numpy().ravel(), z, z, 1, lr=0.01)
        ours, torchs = got.double().cpu().numpy().ravel(), tw.detach().double().cpu().numpy().ravel()
        assert not same_bits(got, before[n])
        assert (np.abs(ours - ref_p) <= e_p).all(), n
        assert (np.abs(ours - torchs) <= 2 * e_p).all(), n


def test_one_step_gcn():
    model, forward = _gcn()
    _one_step_checks(model, forward, _mutag())


def test_one_step_gat(sgrace_env):
    model, forward = _gat(sgrace_env[2])
    _one_step_checks(model, forward, _mutag(), sgrace_env[2])


def _with_one_node_graph():
    from sgracex1_amd import pyg_lite as G
    graphs = _graphs()[:16]
    graphs.insert(5, G.Graph(torch.eye(7)[:1].clone(), torch.zeros((2, 0), dtype=torch.int64), torch.tensor([1])))
    return G.collate(graphs).to(DEV)


def test_declined_batch_still_updates_everything(sgrace_env):
    """A 1-node graph has a dead row under sym_norm2's fill = 0: GAT's fused route declines the batch; the step runs the
    layers one by one with ops.HeadLoss behind them and the same optimiser."""
    from sgracex1_amd import train
    b = _with_one_node_graph()
    model, _ = _gat(sgrace_env[2])
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    trainer = train.StackTrainer(model, lr=0.01)
    loss = trainer.step(b.x, b.edge_index, b.batch, b.y)
    assert trainer.fused_steps == 0 and int(trainer.t.item()) == 1 and bool(torch.isfinite(loss).all())
    used = [n for n, g in zip(before, trainer.last_grads) if g is not None]
    assert {"att1.weight", "att2.weight", "att1.attention", "att2.attention", "lin.weight", "lin.bias"} <= set(used)
    for n, p in model.named_parameters():
        assert same_bits(p.detach(), before[n]) == (n not in used), n
    good = _mutag(16)                                                   # and the next batch takes the fused route on that state
    trainer.step(good.x, good.edge_index, good.batch, good.y)
    assert trainer.fused_steps == 1 and int(trainer.t.item()) == 2


def test_declined_batch_runs_the_trainers_tail(sgrace_env, monkeypatch):
    """On a declined (sorted) batch the tail is ops.HeadLoss with the trainer's p_drop and seed, not the model's
    F.dropout(0.5) from torch's generator: at p_drop = 0 the loss and the head's gradients are inside the derived bound of
    the float64 head on the route's pooled means and agree with the model's own forward without dropout (eval mode,
    gradients on); at p_drop = 0.5 two trainers give the same bits whatever torch's generator holds; the fused stack is
    not tried a second time."""
    import copy
    from sgracex1_amd import ops, train
    b = _with_one_node_graph()
    model, forward = _gat(sgrace_env[2])
    start = copy.deepcopy(model.state_dict())
    tries = []
    real = type(model)._train_stack
    monkeypatch.setattr(type(model), "_train_stack", lambda self, *a: tries.append(1) or real(self, *a))
    # the model's own route without dropout
    model.eval()
    model.zero_grad(set_to_none=True)
    loss_auto = torch.nn.functional.cross_entropy(forward(model, b), b.y)
    loss_auto.backward()
    auto = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    model.train()
    model.zero_grad(set_to_none=True)
    pooled = model.layers_pooled(b.x, b.edge_index, b.batch)
    assert pooled is not None and model.train_pooled(b.x, b.edge_index, b.batch) is None
    W, bias = _f64(model.lin.weight), _f64(model.lin.bias)
    r_loss, _, _, r_gw, r_gb, aux = R.head_f64(pooled.detach().cpu().numpy(), W, bias, b.y.cpu().numpy())
    bound = R.head_bounds(aux)
    tries.clear()
    trainer = train.StackTrainer(model, lr=0.01, p_drop=0.0)
    torch.manual_seed(1)
    loss = trainer.step(b.x, b.edge_index, b.batch, b.y)
    assert tries == [1] and trainer.fused_steps == 0
    grads = dict(zip([n for n, _ in model.named_parameters()], trainer.last_grads))
    assert abs(float(loss.item()) - r_loss) <= bound["loss"] and abs(float(loss.item()) - float(loss_auto.item())) <= 2 * bound["loss"]
    for name, ref, bd in (("lin.weight", r_gw, bound["grad_W"]), ("lin.bias", r_gb, bound["grad_bias"])):
        assert (np.abs(_f64(grads[name]) - ref) <= bd).all() and (np.abs(_f64(grads[name]) - _f64(auto[name])) <= 2 * bd).all(), name
    assert {n for n, g in grads.items() if g is not None} == set(auto)
    # the trainer's own dropout stream
    states = []
    for torch_seed in (1, 2):
        model.load_state_dict(start)
        trainer = train.StackTrainer(model, lr=0.01, p_drop=0.5, seed=7)
        torch.manual_seed(torch_seed)
        losses = [trainer.step(b.x, b.edge_index, b.batch, b.y).clone() for _ in range(2)]
        states.append(losses + trainer.state())
    assert all(same_bits(x, y) for x, y in zip(*states))
    assert not same_bits(states[0][0], states[0][1])


@pytest.mark.parametrize("kind", ["gcn", "gat"])
def test_captured_step_replays_to_eager_steps(kind, sgrace_env):
    from sgracex1_amd import train
    b = _mutag()
    n = 4
    runs = []
    start = None
    for captured in (False, True):
        model, _ = _gcn() if kind == "gcn" else _gat(sgrace_env[2])
        if start is None:
            start = {k: v.clone() for k, v in model.state_dict().items()}
        model.load_state_dict(start)              # the same bits in the parameters no layer reads (never initialised) too
        trainer = train.StackTrainer(model, lr=0.01, p_drop=0.5, seed=99)
        losses = []
        if captured:
            replay = trainer.capture(b.x, b.edge_index, b.batch, b.y)
            assert int(trainer.t.item()) == 0
            for _ in range(n):
                losses.append(replay().clone())
        else:
            trainer.step(b.x, b.edge_index, b.batch, b.y)               # the first step builds what the batch caches (it may read back)
            losses.append(None)
            mode = torch.cuda.get_sync_debug_mode()
            torch.cuda.set_sync_debug_mode("error")
            try:
                for _ in range(n - 1):
                    losses.append(trainer.step(b.x, b.edge_index, b.batch, b.y).clone())
            finally:
                torch.cuda.set_sync_debug_mode(mode)
            assert trainer.fused_steps == n
        torch.cuda.synchronize()
        runs.append((losses, trainer.state()))
    (le, se), (lc, sc) = runs
    assert int(sc[-1].item()) == n
    assert all(same_bits(a, c) for a, c in zip(le[1:], lc[1:]))
    assert not same_bits(lc[1], lc[2])                                  # dropout on: the steps differ
    assert all(same_bits(a, c) for a, c in zip(se, sc))


def test_mutag_through_the_trainer_reaches_reference_accuracy():
    """tests/test_gpu_host.py::test_mutag_training_reaches_reference_accuracy's thresholds: >= 0.74 and >= the acc = 0
    twin - 0.02 (one graph of the 50).  The trainer's dropout stream is its own, so only the accuracy is compared."""
    from sgracex1_amd import molecule_gcn as M, pyg_lite as G, pynq_shim, train
    graphs = _graphs()
    torch.manual_seed(12345)
    graphs = [graphs[i] for i in torch.randperm(len(graphs)).tolist()]
    tr, te = G.collate(graphs[:2000]).to(DEV), G.collate(graphs[50:100]).to(DEV)
    ip = pynq_shim.Overlay("gnn_all.bit").mmult_top_0
    ip.register_map.layer_count = 2

    def accuracy(model, acc):
        model.eval()
        with torch.no_grad():
            pred = model(acc, te.x, te.edge_index, te.batch).argmax(dim=1)
        model.train()
        return float((pred == te.y).float().mean())

    model = M.GCN_PYNQ(64, 7, 2, ip, train_stack=True).to(DEV).train()
    trainer = train.StackTrainer(model, lr=0.01)
    best1 = 0.0
    for _ in range(60):
        trainer.step(tr.x, tr.edge_index, tr.batch, tr.y)
        best1 = max(best1, accuracy(model, 1))
    assert trainer.fused_steps == 60
    twin = M.GCN_PYNQ(64, 7, 2, ip).to(DEV).train()
    opt = torch.optim.Adam(twin.parameters(), lr=0.01)
    torch.manual_seed(777)
    best0 = 0.0
    for _ in range(60):
        opt.zero_grad()
        torch.nn.functional.cross_entropy(twin(0, tr.x, tr.edge_index, tr.batch), tr.y).backward()
        opt.step()
        best0 = max(best0, accuracy(twin, 0))
    print(f"trainer best {best1:.2f}, acc = 0 twin best {best0:.2f}")
    assert best1 >= 0.74, best1
    assert best1 >= best0 - 0.02, (best1, best0)

"""config.accb = 1 on the entry-split route: the setup of test_gpu_node_pad_flat.py (fan-outs [80, 4], adjacency rows of 81
entries, feature rows of 72) with every layer's backward as ONE call, sgx_layer_backward on its entry-split schedules.  One
step's gradients against config.accb = 0 on the same batch inside test_gpu_layer_flat.py's tolerances; two replayed epochs of
NodeTrainer.capture_loader equal the eager steps bit for bit; no ops.Plan is constructed during a step, which runs under
sync-debug "error"; and FPYNQ_GAT trains on a flat-marked full-graph adjacency with accb = 1 -- what raised a ValueError before."""
import copy

import numpy as np
import pytest
import torch

import _layer_grad_ref as LG

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, HUB, WIDTH, BATCH, FAN = 400, 7, 72, 16, [80, 4]
# test_gpu_layer_flat.py's GRAD_TOL: error over the per-element magnitude bound sum |term| of _layer_grad_ref
GRAD_TOL = dict(grad_input=1e-5, grad_weights=1e-5, grad_attention=1e-7)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _data():
    from sgracex1_amd import pyg_lite
    rng = np.random.default_rng(3)
    m = rng.random((N, N)) < 0.02
    near = rng.choice(N, 330, replace=False)
    m[near, HUB] = True                                               # 330 edges j -> HUB and HUB -> j
    m[HUB, near] = True
    np.fill_diagonal(m, False)
    src, dst = np.nonzero(m)
    g = torch.Generator().manual_seed(1)
    x = (torch.rand((N, WIDTH), generator=g) < 0.25).float() * torch.rand((N, WIDTH), generator=g)
    x[::50] = torch.rand((len(range(0, N, 50)), WIDTH), generator=g) + 0.1    # feature rows of 72 entries
    x[3] = 0
    y = (torch.arange(N) * 7 % 5).to(DEV)
    train = torch.zeros(N, dtype=torch.bool, device=DEV)
    train[torch.randperm(N, generator=torch.Generator().manual_seed(2))[:39].to(DEV)] = True
    train[HUB] = True                                                 # 40 seeds: two full batches and a short one of 8
    return pyg_lite.NodeData(x.to(DEV).contiguous(), torch.as_tensor(np.stack([src, dst])).to(DEV), y, train_mask=train)


def _loader(data, gat):
    from sgracex1_amd import pyg_lite
    return pyg_lite.NeighborLoader(data, FAN, input_nodes=data.train_mask, schedule="flat", batch_size=BATCH, shuffle=True, seed=3,
                                   prepare="sym_norm2", fill=1 if gat else 0, dtype=torch.float32, transposed=True, pad=True)


@pytest.fixture(params=[0, 1], ids=["gcn", "att"])
def env(request):
    from sgracex1_amd import config, sgrace
    gat = request.param
    saved = config.snapshot()
    config.acc, config.accb, config.float_type, config.compute_attention = 1, 1, np.float32, gat
    config.fake_quantization = config.hardware_quantize = 0
    config.w_qbits, config.gat_edge_outputs, config.device = 32, 1, "cuda"
    sgrace.init_SGRACE()
    torch.manual_seed(5)
    data = _data()
    model = sgrace.GAT_PYNQ(WIDTH, 16, 1, 5).to(DEV).train()
    yield model, data, gat
    config.restore(saved)
    sgrace.init_SGRACE()


def _count_plans(monkeypatch):
    from sgracex1_amd import ops
    built = []
    init = ops.Plan.__init__

    def counting(self, *a, **k):
        built.append(1)
        return init(self, *a, **k)
    monkeypatch.setattr(ops.Plan, "__init__", counting)
    return built


def _restated(layer, A, seen, gat):
    """The float64 restatement (_layer_grad_ref.edges: gradients and the magnitude bounds sum |term|) of one layer's backward
    on what the layer saw: its input, its grad_output, and E / S formed from the statistics of the very forward it ran."""
    from sgracex1_amd import ops
    x, g, gemm, relu = seen["x"].detach(), seen["g"], seen["gemm"], seen["relu"]
    W, att = layer.weight.detach().float(), layer.attention.detach().float()
    kw = {}
    if gat:
        fea = ops.recorded(seen["x"], ("fea_csr", torch.float32)) if gemm == 0 else x.float().contiguous()
        if fea is None:
            fea = ops.Csr.from_dense(x.float(), torch.float32)
        out, stats = ops.layer_forward(A, fea, W.t().contiguous(), relu=relu, gat_attention=att.reshape(-1).contiguous(),
                                       alpha=layer.alpha, want_row_stats=True)
        assert torch.equal(out.float(), seen["out"])                  # the same forward the module ran
        dead = LG.dead_rows_of(A.rowptr, A.val.float())
        E, S = ops.gat_edge_outputs(A, stats, layer.alpha, dead_weight=1.0 / A.n_cols if bool(dead.any()) else 0.0)
        kw = dict(E=E, S=S, dead=dead)
    return LG.edges(A.rowptr, A.col, A.val, x.float(), W, g, gat=bool(gat), alpha=layer.alpha, **kw)


def _watch(layers):
    seen, handles = {}, []

    def hook(mod, args, out):
        seen[mod] = dict(x=args[3], relu=args[2], gemm=args[1], adj=args[6], out=out.detach())
        out.register_hook(lambda g: seen[mod].__setitem__("g", g.clone()))

    for layer in layers:
        handles.append(layer.register_forward_hook(hook))
    return seen, handles


def _layer_grads(layer, x_leaf, gat):
    got = dict(grad_weights=layer.weight.grad.clone())
    if gat:
        got["grad_attention"] = layer.attention.grad.clone()
    if x_leaf is not None and x_leaf.grad is not None:
        got["grad_input"] = x_leaf.grad.clone()
    return got


def _compare(one, staged, ref_one, ref_staged, what):
    """each path inside GRAD_TOL of the float64 restatement of its own backward, and accb = 1 against accb = 0 inside GRAD_TOL
    of the same per-element magnitude bounds"""
    f1 = LG.check(one, ref_one[0], ref_one[1], GRAD_TOL, what + ("accb 1",))
    f0 = LG.check(staged, ref_staged[0], ref_staged[1], GRAD_TOL, what + ("accb 0",))
    pair = {k: LG.worst(one[k], staged[k].double(), ref_one[1][k]) for k in one}
    print("accb 1 vs 0", what, {k: f"{v:.2e}" for k, v in pair.items()}, "vs float64", {k: f"{v:.2e}" for k, v in f1.items()},
          {k: f"{v:.2e}" for k, v in f0.items()})
    bad = {k: v for k, v in pair.items() if not v <= GRAD_TOL[k]}
    assert not bad, (what, bad)


def _model_step(model, batch, accb, gat):
    """forward + loss + backward of the two-layer model on the batch; -> per layer (gradients, restatement)"""
    from sgracex1_amd import config
    config.accb = accb
    layers = (model.att2, model.conv22)
    seen, handles = _watch(layers)
    try:
        model.zero_grad(set_to_none=True)
        x = batch.x.requires_grad_(True)                              # (the tensor the loader attached its CSRs to)
        x.grad = None
        out = model(x, batch.edge_index_agg)
        loss = torch.nn.functional.cross_entropy(out[:batch.batch_size], batch.y[:batch.batch_size])
        loss.backward()
    finally:
        for h in handles:
            h.remove()
    result = []
    for k, layer in enumerate(layers):
        result.append((_layer_grads(layer, x if k == 0 else None, gat), seen[layer]))
    return result


def test_one_step_against_accb_0_without_a_plan_or_a_sync(env, monkeypatch):
    from sgracex1_amd import config
    model, data, gat = env
    model.eval()                                                      # (no dropout: the two backwards see one forward)
    loader = _loader(data, gat)
    seeds, input_id, step = next(iter(loader.epoch_batches()))
    assert loader.padded(seeds)
    loader.load(seeds, step)
    batch = loader.padded_batch(input_id)
    _model_step(model, batch, 1, gat)                                 # warm: workspaces sized, nothing left to allocate lazily
    built = _count_plans(monkeypatch)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        one = _model_step(model, batch, 1, gat)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert not built, "a plan was constructed on the entry-split route"
    staged = _model_step(model, batch, 0, gat)
    config.accb = 1
    for k, layer in enumerate((model.att2, model.conv22)):
        (g1, s1), (g0, s0) = one[k], staged[k]
        assert g1.keys() == g0.keys() and ("grad_input" in g1) == (k == 0) and ("grad_attention" in g1) == bool(gat)
        A = s1["adj"]
        assert A._flat and A._plan is None
        _compare(g1, g0, _restated(layer, A, s1, gat), _restated(layer, A, s0, gat), ("batch", gat, k))
    loader.status()


def test_replayed_epochs_equal_eager_steps(env):
    from sgracex1_amd.train import NodeTrainer
    model, data, gat = env
    twin = copy.deepcopy(model)
    a, b = NodeTrainer(model, lr=0.01, weight_decay=5e-4, seed=5), NodeTrainer(twin, lr=0.01, weight_decay=5e-4, seed=5)
    la, lb = _loader(data, gat), _loader(data, gat)
    epoch = a.capture_loader(la)                                      # its sync probe is the arbiter: a plan anywhere raises here
    replayed = epoch()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        replayed += epoch()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    eager = [b.step(bt.x, bt.edge_index_agg, bt.y, n_prefix=bt.batch_size) for _ in range(2) for bt in lb]
    la.status(), lb.status()
    assert len(replayed) == len(eager) == 6
    for i, (r, e) in enumerate(zip(replayed, eager)):
        assert same_bits(r, e), i
    assert int(a.t) == int(b.t) == 6
    for x1, x2 in zip(a.state(), b.state()):
        assert same_bits(x1, x2)


def test_captured_eval_pass_takes_the_loader_unchanged(env):
    from sgracex1_amd.train import EvalSums, NodeTrainer
    model, data, gat = env
    trainer = NodeTrainer(model, lr=0.01, weight_decay=5e-4, seed=5)
    la, lb = _loader(data, gat), _loader(data, gat)
    run_pass = trainer.capture_eval_loader(la)
    replayed = run_pass().buffer.clone()
    sums = EvalSums(DEV)
    sums.zero_()
    for bt in lb:
        trainer.evaluate(bt.x, bt.edge_index_agg, bt.y, n_prefix=bt.batch_size, into=sums)
    assert same_bits(replayed, sums.buffer) and int(replayed[0]) == 40


@pytest.mark.parametrize("gat", [0, 1], ids=["gcn", "att"])
@pytest.mark.parametrize("gemm", [0, 1], ids=["csr", "dense"])
def test_full_graph_flat_marked_adjacency_trains_with_accb_1(gat, gemm):
    """FPYNQ_GAT on a flat-marked adjacency with a hub row: accb = 1 raised a ValueError before; now its gradients lie with
    accb = 0's, and no plan is built for the adjacency"""
    from sgracex1_amd import config, ops, sgrace
    rowptr, col, val, _ = LG.masked_graph(600, 4, density=0.02)
    saved = config.snapshot()
    try:
        config.acc, config.float_type, config.compute_attention, config.device = 1, np.float32, gat, "cuda"
        config.fake_quantization = config.hardware_quantize = 0
        config.w_qbits, config.gat_edge_outputs = 32, 1
        sgrace.init_SGRACE()
        torch.manual_seed(2)
        X = (torch.rand((600, 24)) * (torch.rand((600, 24)) < 0.3)).to(DEV)
        G = torch.randn((600, 16), device=DEV)
        runs = {}
        for accb in (1, 0):
            config.accb = accb
            A = ops.Csr(rowptr.to(torch.int32).to(DEV), col.to(torch.int32).to(DEV), val.to(DEV), 600).with_facts(flat=True)
            torch.manual_seed(3)
            layer = sgrace.GATConv_SGRACE(24, 16).to(DEV)
            seen, handles = _watch([layer])
            x = X.clone().requires_grad_(True)
            out = layer(gat, gemm, 1, x, None, A.val, A)
            out.backward(G)
            handles[0].remove()
            if accb == 1:
                assert A._plan is None                    # (X and X^T are not flat-marked here: theirs is their own business)
            runs[accb] = (_layer_grads(layer, x, gat), _restated(layer, A, seen[layer], gat))
        _compare(runs[1][0], runs[0][0], runs[1][1], runs[0][1], ("full graph", gat, gemm))
    finally:
        config.restore(saved)
        sgrace.init_SGRACE()

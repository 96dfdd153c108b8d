"""train.NodeTrainer and ops.NodeLoss on the device: the autograd function, one step against torch's tail and
torch.optim.Adam, the captured step against eager steps, the two mini-batch forms, evaluation, and the example's accuracy."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _layer_grad_ref as LG
import _node_loss_ref as R
import _train_tail_ref as RT

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _example():
    spec = importlib.util.spec_from_file_location("sgrace_nc", os.path.join(ROOT, "examples", "sgrace_node_classification.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(params=[0, 1], ids=["gcn", "attention"])
def env(request):
    """fp32, unquantised, accb = 0 on the kernels, with the GCN and with the attention aggregate; a 300-node
    planted-partition graph, a fifth of it the training rows; the model in training mode."""
    from sgracex1_amd import config, sgrace
    saved = config.snapshot()
    config.acc, config.accb, config.float_type, config.compute_attention = 1, 0, np.float32, request.param
    config.fake_quantization = config.hardware_quantize = 0
    config.w_qbits, config.gat_edge_outputs, config.device = 32, 1, "cuda"
    sgrace.init_SGRACE()
    torch.manual_seed(7)
    x, ei, y = _example().planted_partition(300, 5, 200, 0.05, 0.005, 3, torch.device(DEV))
    perm = torch.randperm(300, generator=torch.Generator().manual_seed(3)).to(DEV)
    train = perm[:60]
    mask = torch.zeros(300, dtype=torch.bool, device=DEV)
    mask[train] = True
    model = sgrace.GAT_PYNQ(200, 16, 1, 5).to(DEV).train()
    yield model, x, ei, y, train, mask
    config.restore(saved)
    sgrace.init_SGRACE()


def test_node_loss_autograd_function():
    from sgracex1_amd import ops
    c = R.make_case(3 * R.ROWS + 5, 64, 7, select="mask", p=0.5, seed=31)
    th, tw, tb = (torch.as_tensor(c[k], device=DEV).requires_grad_() for k in ("H", "W", "bias"))
    t, m = torch.as_tensor(c["target"], device=DEV), torch.as_tensor(c["mask"], device=DEV)
    loss = ops.NodeLoss.apply(th, tw, tb, t, m, None, 0.5, c["seed"], c["step"], None)
    (loss * 2.0).backward()
    r_loss, _, r_gh, r_gw, r_gb, _, aux = R.node_f64(c["H"], c["W"], c["bias"], c["target"], c["mask"], None, 0.5, c["seed"], c["step"], 2.0)
    bound = R.node_bounds(aux)
    assert abs(float(loss.detach()) - r_loss) <= bound["loss"]
    for got, ref, name in ((th.grad, r_gh, "grad_H"), (tw.grad, r_gw, "grad_W"), (tb.grad, r_gb, "grad_bias")):
        # the function forms the gradients at scale 1 and multiplies by grad_output: one more rounding
        assert (np.abs(got.double().cpu().numpy() - ref) <= bound[name] + RT.U * np.abs(ref)).all(), name
    raw = ops.node_loss(th, tw, tb, t, mask=m, p=0.5, seed=c["seed"], step=c["step"])
    assert same_bits(loss.detach().reshape(1), raw[0])
    for got, want in ((th.grad, raw[1]), (tw.grad, raw[2]), (tb.grad, raw[3])):
        assert same_bits(got, want * 2.0)


LAYER_TOL = dict(grad_input=1e-5, grad_weights=1e-5, grad_attention=1e-7)      # tests/test_gpu_layer_grad.py's TOL


def _layer_reference(layer, x_in, g64, e_g, gat, gemm, relu):
    """One layer's backward in float64 (tests/_layer_grad_ref.py) for the incoming gradient g64, known to e_g:
    -> (gradients, tolerance) with tolerance = the layer tests' bound (LAYER_TOL x the magnitude bound, here of
    |g64| + e_g: what an fp32 backward of any gradient inside e_g of g64 may be off by) + the same magnitude map applied to
    e_g (the backward is linear in the incoming gradient: what the gradient's own error becomes)."""
    from sgracex1_amd import ops
    A = layer._csr
    W, att = layer.weight.detach(), layer.attention.detach()
    E = S = dead = None
    if gat:
        fea = ops.cached_on(x_in, ("fea_csr", torch.float32), lambda: None) if gemm == 0 else x_in.detach().contiguous()
        _, E, S = ops.layer_forward(A, fea, W.t().contiguous(), relu=relu, alpha=layer.alpha,
                                    gat_attention=att.reshape(-1).contiguous(), want_edge_outputs=True)
        dead = LG.dead_rows_of(A.rowptr, A.val.float())
    run = lambda g: LG.dense(A.rowptr, A.col, A.val, x_in.detach(), W, g, gat=bool(gat), E=E, S=S, dead=dead, alpha=layer.alpha)
    grads, _ = run(g64)
    _, mag = run(g64.abs() + e_g)
    _, prop = run(e_g)
    return grads, {k: LAYER_TOL[k] * mag[k] + prop[k] for k in mag}


def test_one_step_against_torchs_tail_and_adam(env):
    """One NodeTrainer.step at p_drop = 0 against model.features -> lin -> F.cross_entropy(out[train], y[train]) ->
    torch.optim.Adam(weight_decay=5e-4): both routes' gradients inside the bounds of ONE float64 reference (the head's
    from _node_loss_ref, the layers' from _layer_grad_ref with grad_H's bound carried through both layers), and both
    routes' parameters after the step inside Adam's bound."""
    from sgracex1_amd import config, ops
    from sgracex1_amd.train import NodeTrainer
    model, x, ei, y, train, mask = env
    gat = int(config.compute_attention)
    names = [n for n, _ in model.named_parameters()]
    params = dict(model.named_parameters())
    before = {n: p.detach().clone() for n, p in params.items()}
    seen = {}
    hook = model.reluh.register_forward_hook(lambda m, i, o: seen.__setitem__("x2", o))
    # torch's route
    H_t = model.features(x, ei)
    hook.remove()
    X2 = seen["x2"].detach()
    loss_t = F.cross_entropy(model.lin(H_t)[train], y[train])
    g_all = torch.autograd.grad(loss_t, [H_t] + list(model.parameters()), allow_unused=True)
    gh_t, grads_t = g_all[0], dict(zip(names, g_all[1:]))
    # the float64 reference: the head, then layer 2 (dense input X2, no relu), RPYNQ's mask, layer 1 (sparse input x, relu)
    f = lambda t: t.detach().double().cpu().numpy()
    H = H_t.detach()
    r_loss, _, r_gh, r_gw, r_gb, counts, aux = R.node_f64(H.cpu().numpy(), before["lin.weight"].cpu().numpy(),
                                                         before["lin.bias"].cpu().numpy(), y.cpu().numpy(), mask.cpu().numpy())
    bound = R.node_bounds(aux)
    assert counts[0] == 60
    dev64 = lambda a: torch.as_tensor(a, dtype=torch.float64, device=DEV)
    ref2, tol2 = _layer_reference(model.conv22, X2, dev64(r_gh), dev64(bound["grad_H"]), gat, 1, 0)
    live = (X2 != 0).double()                               # RPYNQ: no gradient where the layer's output is exactly 0
    ref1, tol1 = _layer_reference(model.att2, x, ref2["grad_input"] * live, tol2["grad_input"] * live, gat, 0, 1)
    ref = {"lin.weight": dev64(r_gw), "lin.bias": dev64(r_gb), "conv22.weight": ref2["grad_weights"], "att2.weight": ref1["grad_weights"]}
    tol = {"lin.weight": dev64(bound["grad_W"]), "lin.bias": dev64(bound["grad_bias"]), "conv22.weight": tol2["grad_weights"],
           "att2.weight": tol1["grad_weights"]}
    if gat:
        ref.update({"conv22.attention": ref2["grad_attention"], "att2.attention": ref1["grad_attention"]})
        tol.update({"conv22.attention": tol2["grad_attention"], "att2.attention": tol1["grad_attention"]})
    # the trainer's route
    trainer = NodeTrainer(model, lr=0.01, weight_decay=5e-4, p_drop=0.0)
    loss = trainer.step(x, ei, y, mask=mask)
    torch.cuda.synchronize()
    after = {n: p.detach().clone() for n, p in params.items()}
    ours = dict(zip(names, trainer.last_grads))
    assert [n for n in names if ours[n] is None] == [n for n in names if grads_t[n] is None]        # the unused layer biases
    assert sorted(n for n in names if ours[n] is not None) == sorted(["lin.weight", "lin.bias", "conv22.weight", "att2.weight",
                                                                      "conv22.attention", "att2.attention"])
    print("loss", float(loss), r_loss, float(loss_t), "bound", float(bound["loss"]))
    assert abs(float(loss) - r_loss) <= bound["loss"] and abs(float(loss_t) - r_loss) <= bound["loss"]
    _, gh, _, _ = ops.node_loss(H, before["lin.weight"], before["lin.bias"], y, mask=mask, p=0.0)
    for route, g in (("trainer", gh), ("torch", gh_t)):
        assert (np.abs(f(g) - r_gh) <= bound["grad_H"]).all(), route
    assert not gh[~mask].any()
    for n in names:
        if ours[n] is None:
            continue
        if n not in ref:                                   # the GCN aggregate leaves the attention vectors without a gradient
            assert not ours[n].any() and not grads_t[n].any(), n
            continue
        for route, g in (("trainer", ours[n]), ("torch", grads_t[n])):
            ratio = float(((g.double().reshape(ref[n].shape) - ref[n]).abs() / tol[n].clamp_min(1e-300)).max())
            print(n, route, "error / bound", ratio, "bound / largest gradient", float(tol[n].max() / ref[n].abs().max()))
            assert ratio <= 1.0, (n, route, ratio)
        if not n.endswith("attention"):                    # (the attention vectors' sums cancel: their figure is printed)
            assert float(tol[n].max()) <= 0.01 * float(ref[n].abs().max()), n      # a bound that a wrong gradient cannot pass
    # Adam: the trainer's parameters after its step, and torch.optim.Adam's after a real step on torch's route's
    # gradients, each inside Adam's bound of the float64 step of its own gradients
    twin = [before[n].clone().requires_grad_() for n in names]
    opt = torch.optim.Adam(twin, lr=0.01, weight_decay=5e-4)
    for p, n in zip(twin, names):
        p.grad = None if grads_t[n] is None else grads_t[n].clone()
    opt.step()
    for p, n in zip(twin, names):
        if ours[n] is None:
            assert same_bits(after[n], before[n]) and same_bits(p.detach(), before[n])
            continue
        p0 = f(before[n]).ravel()
        z = np.zeros_like(p0)
        for route, got, g, rounded in (("trainer", after[n], f(ours[n]).ravel(), True), ("torch", p.detach(), f(grads_t[n]).ravel(), False)):
            want, _, _ = RT.adam_f64(p0, g, z, z, 1, lr=0.01, weight_decay=5e-4, rounded_constants=rounded)
            e_p, _, _ = RT.adam_bound_step(p0, g, z, z, 1, lr=0.01, weight_decay=5e-4)
            ratio = float((np.abs(f(got).ravel() - want) / e_p).max())
            print(n, route, "Adam error / bound", ratio)
            assert ratio <= 1.0, (n, route, ratio)
        # and the two updates themselves: apart by no more than both bounds and what the float64 steps of the two
        # gradients differ by
        w_o, _, _ = RT.adam_f64(p0, f(ours[n]).ravel(), z, z, 1, lr=0.01, weight_decay=5e-4)
        w_t, _, _ = RT.adam_f64(p0, f(grads_t[n]).ravel(), z, z, 1, lr=0.01, weight_decay=5e-4, rounded_constants=False)
        assert (np.abs(f(after[n]).ravel() - f(p).ravel()) <= 2 * e_p + np.abs(w_o - w_t)).all(), n
    assert int(trainer.t) == 1


def test_captured_step_replays_to_eager_steps(env):
    from sgracex1_amd.train import NodeTrainer
    model, x, ei, y, train, mask = env
    start = {n: p.detach().clone() for n, p in model.named_parameters()}
    a = NodeTrainer(model, lr=0.01, weight_decay=5e-4, p_drop=0.5, seed=5)
    eager_losses = []
    torch.cuda.set_sync_debug_mode("default")
    a.step(x, ei, y, mask=mask)                                 # builds what a step caches
    a.load_state([*start.values(), *[torch.zeros_like(m) for m in a.exp_avg], *[torch.zeros_like(m) for m in a.exp_avg_sq],
                  torch.zeros_like(a.t)])
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            eager_losses.append(a.step(x, ei, y, mask=mask).clone())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    eager_state = a.state()
    a.load_state([*start.values(), *[torch.zeros_like(m) for m in a.exp_avg], *[torch.zeros_like(m) for m in a.exp_avg_sq],
                  torch.zeros_like(a.t)])
    replay = a.capture(x, ei, y, mask)
    assert int(a.t) == 0 and all(same_bits(p.detach(), start[n]) for n, p in model.named_parameters())
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = [replay().clone() for _ in range(3)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(same_bits(u, v) for u, v in zip(losses, eager_losses))
    assert all(same_bits(u, v) for u, v in zip(a.state(), eager_state))
    assert not same_bits(losses[0], losses[1])


@pytest.mark.parametrize("prepared", [False, True], ids=["plain", "prepared"])
def test_mini_batches_mask_and_prefix_forms(env, prepared):
    from sgracex1_amd import ops, pyg_lite
    model, x, ei, y, train, mask = env
    data = pyg_lite.NodeData(x, ei, y, train_mask=mask)
    kw = {"prepare": "sym_norm2", "transposed": True} if prepared else {}
    loader = pyg_lite.NeighborLoader(data, [5, 5], batch_size=32, input_nodes=mask, shuffle=True, seed=3, **kw)
    seen = 0
    for b in loader:
        e = b.edge_index_agg if prepared else b.edge_index.flip(0)
        with torch.no_grad():
            H = model.features(b.x, e).contiguous()
            out = model.lin(H)
        w, bias = model.lin.weight.detach(), model.lin.bias.detach()
        f32 = lambda t: t.detach().cpu().numpy()
        bs = int(b.batch_size)
        forms = [("prefix", dict(n_prefix=bs), out[:bs], b.y[:bs], dict(n_prefix=bs))]
        tm = b.train_mask.bool()
        forms.append(("mask", dict(mask=tm), out[tm], b.y[tm], dict(mask=f32(tm))))
        for name, args, o_sel, y_sel, ref_args in forms:
            ours = ops.node_loss(H, w, bias, b.y, p=0.0, grads=False, **args)[0]
            torchs = F.cross_entropy(o_sel, y_sel)
            r = R.node_f64(f32(H), f32(w), f32(bias), f32(b.y), **ref_args)
            bound = R.node_bounds(r[6])["loss"]
            print(name, float(ours), float(torchs), r[0], bound)
            assert abs(float(ours) - r[0]) <= bound and abs(float(torchs) - r[0]) <= bound, name
        seen += 1
    assert seen == 2


def test_evaluate_counts_are_the_models_argmax(env):
    from sgracex1_amd.train import NodeTrainer
    model, x, ei, y, train, mask = env
    trainer = NodeTrainer(model)
    counts, loss = trainer.evaluate(x, ei, y, ~mask)
    assert model.training
    model.eval()
    with torch.no_grad():
        out = model(x, ei)
    model.train()
    assert counts.tolist() == [240, int((out.argmax(1) == y)[~mask].sum())]
    with torch.no_grad():
        H = model.eval().features(x, ei)
    model.train()
    f32 = lambda t: t.detach().cpu().numpy()
    r = R.node_f64(f32(H), f32(model.lin.weight), f32(model.lin.bias), f32(y), mask=f32(~mask))
    assert abs(float(loss) - r[0]) <= R.node_bounds(r[6])["loss"] and r[5] == tuple(counts.tolist())


@pytest.mark.parametrize("prepared", [False, True], ids=["plain", "prepared"])
def test_trainer_epoch_through_the_loaders_synchronises_nothing(env, prepared):
    """One NodeTrainer epoch of mini-batches: through the prepared loader the whole epoch, sampling included, under
    set_sync_debug_mode("error") with the prefix form; through the plain loader every step with batch.train_mask as the
    mask under it, once the batch's graph has been normalised (the layer path's sym_norm2 of a new edge list reads a count
    back, as it does under torch's tail; the boolean index of the loss and its read-back are what is gone).
    The first step's loss is the indexed torch form's inside the bound; every parameter with a gradient moves."""
    from sgracex1_amd import pyg_lite
    from sgracex1_amd.train import NodeTrainer
    model, x, ei, y, train, mask = env
    data = pyg_lite.NodeData(x, ei, y, train_mask=mask)
    kw = {"prepare": "sym_norm2", "transposed": True} if prepared else {}
    loader = pyg_lite.NeighborLoader(data, [5, 5], batch_size=32, input_nodes=mask, shuffle=True, seed=3, **kw)
    trainer = NodeTrainer(model, lr=0.01, weight_decay=5e-4, p_drop=0.0)

    def step(b, e=None):
        if prepared:
            return trainer.step(b.x, b.edge_index_agg, b.y, n_prefix=b.batch_size)
        return trainer.step(b.x, b.edge_index.flip(0) if e is None else e, b.y, mask=b.train_mask)

    for b in loader:                                            # an epoch that builds what steps cache
        step(b)
    trainer.load_state([*[p.detach().clone() for p in trainer.params], *[torch.zeros_like(m) for m in trainer.exp_avg],
                        *[torch.zeros_like(m) for m in trainer.exp_avg_sq], torch.zeros_like(trainer.t)])
    before = [p.detach().clone() for p in trainer.params]
    losses, first = [], None
    torch.cuda.synchronize()
    if prepared:
        torch.cuda.set_sync_debug_mode("error")
    try:
        for b in loader:
            e = b.edge_index_agg if prepared else b.edge_index.flip(0)
            if first is None or not prepared:
                with torch.no_grad():                           # (plain: this also normalises the batch's graph, kept on e)
                    H = model.features(b.x, e).contiguous()
            if first is None:
                first = (b, H, [p.detach().clone() for p in (model.lin.weight, model.lin.bias)])
            if not prepared:
                torch.cuda.set_sync_debug_mode("error")
            losses.append(step(b, e))
            if not prepared:
                torch.cuda.set_sync_debug_mode("default")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert len(losses) == 2 == int(trainer.t) and all(bool(torch.isfinite(v).all()) for v in losses)
    b, H, (w, bias) = first
    sel = torch.arange(H.shape[0], device=DEV) < int(b.batch_size) if prepared else b.train_mask.bool()
    torchs = F.cross_entropy(F.linear(H, w, bias)[sel], b.y[sel])
    f32 = lambda t: t.detach().cpu().numpy()
    r = R.node_f64(f32(H), f32(w), f32(bias), f32(b.y), mask=f32(sel))
    bound = R.node_bounds(r[6])["loss"]
    assert abs(float(losses[0]) - r[0]) <= bound and abs(float(torchs) - r[0]) <= bound
    for p, p0, g in zip(trainer.params, before, trainer.last_grads):
        assert (g is None) == same_bits(p.detach(), p0) or (g is not None and not g.any())


@pytest.mark.parametrize("device_batches", [False, True], ids=["plain", "prepared"])
def test_example_mini_batches_with_the_trainer(device_batches):
    from sgracex1_amd import config, sgrace
    old = config.snapshot()
    try:
        res, _, _ = _example().run(False, 32, epochs=20, acc=1, n=2000, verbose=False, trainer=True, batch_size=128,
                                   num_neighbors=[10, 10], device_batches=device_batches)
        print(res["epoch_loss"], res["test_acc"])
        assert res["batches_per_epoch"] == 4 and np.isfinite(res["epoch_loss"]).all()
        assert res["epoch_loss"][-1] < res["epoch_loss"][0]                   # it learns: 80 steps lower the loss
        assert 0.5 < res["test_acc"] <= 1.0                                   # far above the 0.2 of five balanced classes
    finally:
        config.restore(old)
        sgrace.init_SGRACE()


@pytest.mark.parametrize("attention,replay", [(False, False), (True, False), (False, True), (True, True)])
def test_example_with_the_trainer_reaches_the_torch_loops_floor(attention, replay):
    from sgracex1_amd import config, sgrace
    old = config.snapshot()
    try:
        res, _, _ = _example().run(attention, 32, epochs=60, acc=1, n=2000, verbose=False, trainer=True, replay=replay)
        print(res["train_acc"], res["test_acc"], res["ms_per_epoch"])
        assert res["test_acc"] > 0.93, res
    finally:
        config.restore(old)
        sgrace.init_SGRACE()

"""sgx_node_eval on the device (include/sgx.h, "the node evaluation head") against tests/_node_eval_ref.py: exact totals, the
summed loss within the bound the reference derives, logits and counts bit-equal to sgx_node_loss's at p = 0, accumulation
across calls, NaN in rows and blocks that are not selected, the same bits on every run, guard bands around everything the
call writes, the argument errors; and train.NodeTrainer.evaluate(into=) / capture_eval_loader against today's evaluate()
and against eager passes, bit for bit."""
import copy

import numpy as np
import pytest
import torch

import _node_eval_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _dev(case, poison=None):
    """The case's operands on the device -> (H, W, bias, target, mask); the rows of `poison` (a bool array) hold NaN."""
    H = case["H"].copy()
    if poison is not None:
        H[poison] = np.nan
    t = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    return t(H), t(case["W"]), t(case["bias"]), t(case["target"]), t(case["mask"])


def _zeros():
    return torch.zeros(2, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.float64, device=DEV)


def _eval(ops, operands, n_prefix=None, want_logits=False, into=None):
    H, W, b, t, mask = operands
    totals, loss_sum = _zeros() if into is None else into
    return ops.node_eval(H, W, b, t, totals, loss_sum, mask=mask, n_prefix=n_prefix, want_logits=want_logits)


SPECS = R.gpu_case_specs()


@pytest.mark.parametrize("spec", [s for _, s in SPECS], ids=[i for i, _ in SPECS])
def test_totals_loss_and_logits_against_the_restatement(spec):
    from sgracex1_amd import ops
    case = R.make_case(**spec)
    n = spec["n"]
    clean = _dev(case)
    for n_prefix in R.prefixes(n):
        (M, hits), loss, bound, z32, _ = R.eval_ref(case["H"], case["W"], case["bias"], case["target"], case["mask"], n_prefix)
        sel = R.selection(n, case["mask"], n_prefix)
        totals, loss_sum = _eval(ops, _dev(case, poison=~sel), n_prefix)           # unselected rows hold NaN
        got = float(loss_sum.cpu()[0])
        print(f"{spec} n_prefix={n_prefix}: totals {totals.tolist()} want {[M, hits]}; loss_sum {got!r} want {loss!r} "
              f"error {abs(got - loss):.3e} bound {bound:.3e}")
        assert totals.tolist() == [M, hits]
        assert np.isfinite(got) and abs(got - loss) <= bound
        if M == 0:
            assert got == 0.0
        # with the logits output every row is read and written: the rule's bits, and the same sums
        totals2, loss2, logits = _eval(ops, clean, n_prefix, want_logits=True)
        assert logits.shape == z32.shape and np.array_equal(logits.cpu().numpy().view(np.int32), z32.view(np.int32))
        assert torch.equal(totals2, totals) and same_bits(loss2, loss_sum)


def test_ties_go_to_the_first_maximum():
    from sgracex1_amd import ops
    case = R.make_tie_case()
    n = case["H"].shape[0]
    totals, loss_sum, logits = _eval(ops, _dev(case), want_logits=True)
    z = logits.cpu().numpy()
    assert np.array_equal(z[:, 2], z[:, 5]) and np.array_equal(z, R.logits_f32(case["H"], case["W"], case["bias"]))
    assert totals.tolist() == [n, (n + 1) // 2]
    _, loss, bound, _, _ = R.eval_ref(case["H"], case["W"], case["bias"], case["target"])
    assert abs(float(loss_sum.cpu()[0]) - loss) <= bound


@pytest.mark.parametrize("n,P,C,mask", [(1, 7, 5, "none"), (17, 1, 1, "sparse"), (33, 65, 7, "sparse"), (33, 64, 64, "none"),
                                       (8200, 7, 2, "sparse"), (33, 7, 5, "zero")])
def test_logits_and_counts_are_node_loss_bits(n, P, C, mask):
    """The existing path: sgx_node_loss with p = 0 and no gradients on the same operands."""
    from sgracex1_amd import ops
    case = R.make_case(n, P, C, mask=mask, seed=5)
    H, W, b, t, m = _dev(case)
    for n_prefix in R.prefixes(n):
        _, _, _, _, counts, want = ops.node_loss(H, W, b, t, mask=m, n_prefix=n_prefix, p=0.0, want_logits=True, want_counts=True,
                                                 grads=False)
        totals, _, logits = _eval(ops, (H, W, b, t, m), n_prefix, want_logits=True)
        assert same_bits(logits, want)
        assert torch.equal(totals, counts), (n_prefix, totals.tolist(), counts.tolist())


def test_calls_accumulate():
    """Two calls of unequal size into accumulators that start non-zero; a call that selects nothing leaves them alone."""
    from sgracex1_amd import ops
    a, b = R.make_case(33, 65, 7, mask="sparse", seed=1), R.make_case(8200, 65, 7, mask="none", seed=2)
    b["W"], b["bias"] = a["W"], a["bias"]
    A, B = _dev(a), _dev(b)
    ta, la = _eval(ops, A, 20)
    tb, lb = _eval(ops, B, 8199)
    totals = torch.tensor([5, 3], dtype=torch.int64, device=DEV)
    loss_sum = torch.tensor([1.25], dtype=torch.float64, device=DEV)
    out = _eval(ops, A, 20, into=(totals, loss_sum))
    assert out[0] is totals and out[1] is loss_sum
    _eval(ops, B, 8199, into=(totals, loss_sum))
    assert totals.tolist() == [5 + int(ta[0]) + int(tb[0]), 3 + int(ta[1]) + int(tb[1])]
    assert float(loss_sum.cpu()[0]) == (1.25 + float(la.cpu()[0])) + float(lb.cpu()[0])       # one double addition a call
    (Ma, ha), _, _, _, _ = R.eval_ref(a["H"], a["W"], a["bias"], a["target"], a["mask"], 20)
    (Mb, hb), _, _, _, _ = R.eval_ref(b["H"], b["W"], b["bias"], b["target"], b["mask"], 8199)
    assert totals.tolist() == [5 + Ma + Mb, 3 + ha + hb]
    # M == 0, by the prefix, by the mask and with the logits wanted: not a bit changes, the sign of a zero included
    zero = R.make_case(33, 65, 7, mask="zero", seed=1)
    for start in (0.0, -0.0, 2.5):
        totals = torch.tensor([7, 2], dtype=torch.int64, device=DEV)
        loss_sum = torch.tensor([start], dtype=torch.float64, device=DEV)
        before = loss_sum.clone()
        _eval(ops, A, 0, into=(totals, loss_sum))
        _eval(ops, _dev(zero, poison=np.ones(33, bool)), into=(totals, loss_sum))
        logits = _eval(ops, _dev(zero), 0, want_logits=True, into=(totals, loss_sum))[2]
        assert totals.tolist() == [7, 2] and same_bits(loss_sum, before)
        assert np.array_equal(logits.cpu().numpy(), R.logits_f32(zero["H"], zero["W"], zero["bias"]))


def test_unselected_rows_and_blocks_are_not_read():
    """NaN in every unselected row -- single rows inside selected blocks, whole blocks between selected ones, everything
    behind the prefix -- reaches no sum when the logits are not asked for."""
    from sgracex1_amd import ops
    n = 5 * R.ROWS + 3
    case = R.make_case(n, 64, 7, seed=9)
    mask = np.ones(n, bool)
    mask[R.ROWS:2 * R.ROWS] = False                          # a whole block
    mask[2 * R.ROWS + 1::3] = False                          # rows inside the blocks behind it
    case["mask"] = mask
    n_prefix = 4 * R.ROWS + 2                                # the last block lies behind the prefix
    sel = R.selection(n, mask, n_prefix)
    (M, hits), loss, bound, _, _ = R.eval_ref(case["H"], case["W"], case["bias"], case["target"], mask, n_prefix)
    totals, loss_sum = _eval(ops, _dev(case, poison=~sel), n_prefix)
    clean = _eval(ops, _dev(case), n_prefix)
    assert totals.tolist() == [M, hits] == clean[0].tolist() and M == int(sel.sum())
    assert same_bits(loss_sum, clean[1]) and abs(float(loss_sum.cpu()[0]) - loss) <= bound


def test_two_runs_give_the_same_bits():
    from sgracex1_amd import ops
    case = R.make_case(8200, 65, 7, mask="sparse", seed=3)
    operands = _dev(case)
    first = _eval(ops, operands, 8190, want_logits=True)
    torch.cuda.synchronize()
    junk = torch.full((1 << 22,), 0xFF, dtype=torch.uint8, device=DEV)  # the workspace is reused: its old contents must not matter
    del junk
    second = _eval(ops, operands, 8190, want_logits=True)
    for x, y in zip(first, second):
        assert same_bits(x, y)


GUARD = 37                                                   # elements in front of and behind every output: odd on purpose


def _banded(n, dtype, fill):
    """A tensor of n elements in the middle of a sentinel-filled one -> (whole, the view)."""
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return whole, whole[GUARD:GUARD + n]


@pytest.mark.parametrize("want_logits", [False, True])
def test_targets_outside_the_range_inside_guard_bands(want_logits):
    """Rows whose target lies outside [0, C), far outside included, count, give no hit and no loss, and nothing outside
    totals, loss_sum, logits and the workspace is written."""
    from sgracex1_amd import _lib, ops
    n, P, C = 3 * R.ROWS + 5, 7, 5
    case = R.make_case(n, P, C, seed=11)
    t = case["target"]
    outside = [C, -1, 2 ** 40, -2 ** 40, C + 1, 2 ** 31, -2 ** 31 - 1, 2 ** 32 + 1]   # the last is in range as a 32-bit word
    for k, i in enumerate(range(0, n, 4)):
        t[i] = outside[k % len(outside)]
    H, W, b, tgt, _ = _dev(case)
    whole_t, totals = _banded(2, torch.int64, -77)
    whole_l, loss_sum = _banded(1, torch.float64, -77.0)
    whole_z, logits = _banded(n * C, torch.float32, -77.0)
    totals.zero_(), loss_sum.zero_()
    need = _lib.lib.sgx_node_eval_workspace_bytes(n, n, P, C)
    whole_w = torch.full((need + 1024,), 0xA5, dtype=torch.uint8, device=DEV)
    off = (-whole_w.data_ptr()) % 256 + 256                  # a 256-byte aligned workspace with at least 256 bytes in front
    ws = whole_w[off:off + need]
    st = _lib.lib.sgx_node_eval(n, n, P, C, H.data_ptr(), W.data_ptr(), b.data_ptr(), tgt.data_ptr(), None, totals.data_ptr(),
                                loss_sum.data_ptr(), logits.data_ptr() if want_logits else None, ws.data_ptr(), need, ops._stream())
    assert st == 0
    torch.cuda.synchronize()
    (M, hits), loss, bound, z32, _ = R.eval_ref(case["H"], case["W"], case["bias"], t)
    live = (t >= 0) & (t < C)
    assert M == n and hits <= int(live.sum()) < n
    assert totals.tolist() == [M, hits] and abs(float(loss_sum.cpu()[0]) - loss) <= bound
    # the rows with a target in range alone give the same sums: the others added an exact 0 and no hit
    only = _eval(ops, (H, W, b, tgt, torch.from_numpy(live).to(DEV)))
    assert only[0].tolist() == [int(live.sum()), hits] and same_bits(only[1], loss_sum.clone())
    for whole, k in ((whole_t, 2), (whole_l, 1), (whole_z, n * C)):
        assert bool((whole[:GUARD] == -77).all()) and bool((whole[GUARD + k:] == -77).all())
    if want_logits:
        assert np.array_equal(logits.cpu().numpy().reshape(n, C).view(np.int32), z32.view(np.int32))
    else:
        assert bool((whole_z == -77).all())
    assert bool((whole_w[:off] == 0xA5).all()) and bool((whole_w[off + need:] == 0xA5).all())


def test_argument_errors_and_limits():
    """Argument checks made before anything is launched, through the C ABI and through ops."""
    from sgracex1_amd import _lib, ops
    R.check_argument_errors(_lib.lib)
    case = R.make_case(4, 8, 2)
    H, W, b, t, _ = _dev(case)
    totals, loss_sum = _zeros()
    with pytest.raises(ValueError):
        ops.node_eval(H, W, b, t, totals, loss_sum, n_prefix=-1)
    with pytest.raises(TypeError):
        ops.node_eval(H, W, b, t, totals.int(), loss_sum)
    with pytest.raises(TypeError):
        ops.node_eval(H, W, b, t, totals, loss_sum.float())
    with pytest.raises(TypeError):
        ops.node_eval(H, W, b, t.int(), totals, loss_sum)
    with pytest.raises(TypeError):
        ops.node_eval(H, W, b, t, totals, loss_sum, mask=torch.ones(4, dtype=torch.int32, device=DEV))
    wide = torch.zeros((4, 1025), device=DEV)
    with pytest.raises(_lib.SgxError) as err:
        ops.node_eval(wide, torch.zeros((2, 1025), device=DEV), None, t, totals, loss_sum)
    assert err.value.status == R.UNSUPPORTED
    assert totals.tolist() == [0, 0] and float(loss_sum.cpu()[0]) == 0.0


# ---- the trainer on the small graph ---------------------------------------------------------------------------------------
@pytest.fixture(params=[(0, False), (1, False), (0, True)], ids=["gcn-f32", "att-f32", "gcn-f16"])
def env(request):
    """accb = 0 on the kernels, unquantised; the small graph of the reference module; a GAT_PYNQ in training mode."""
    from sgracex1_amd import config, sgrace
    gat, half = request.param
    saved = config.snapshot()
    config.acc, config.accb, config.compute_attention = 1, 0, gat
    config.float_type = np.float16 if half else np.float32
    config.fake_quantization = config.hardware_quantize = 0
    config.w_qbits, config.gat_edge_outputs, config.device = 32, 1, "cuda"
    sgrace.init_SGRACE()
    torch.manual_seed(5)
    data = R.node_data(DEV)
    model = sgrace.GAT_PYNQ(R.N_FEATURES, R.HIDDEN, 1, R.N_CLASSES).to(DEV).train()
    yield model, data, gat, half
    config.restore(saved)
    sgrace.init_SGRACE()


def _loader(data, gat, half, split="test", shuffle=False):
    from sgracex1_amd import pyg_lite
    nodes = data.test_mask if split == "test" else data.train_mask
    return pyg_lite.NeighborLoader(data, R.FANOUTS, input_nodes=nodes, **R.loader_kwargs(gat, half, split, shuffle))


def test_evaluate_into_adds_what_evaluate_counts(env):
    from sgracex1_amd.train import EvalSums, NodeTrainer
    model, data, gat, half = env
    trainer = NodeTrainer(model, lr=0.01, weight_decay=5e-4, seed=5)
    loader = _loader(data, gat, half)
    assert len(loader) == 3 and loader.input_nodes.numel() == R.N_TEST
    state = trainer.state()
    sums = EvalSums(DEV)
    counts, want_loss, want, bound = torch.zeros(2, dtype=torch.int64, device=DEV), 0.0, 0.0, 0.0
    W, bias = model.lin.weight.detach().cpu().numpy(), model.lin.bias.detach().cpu().numpy()
    sizes = []
    for b in loader:
        B = b.batch_size
        sizes.append(B)
        c, mean = trainer.evaluate(b.x, b.edge_index_agg, b.y, n_prefix=B)          # today's call: fresh counts, the batch's mean
        assert trainer.evaluate(b.x, b.edge_index_agg, b.y, n_prefix=B, into=sums) is sums
        counts += c
        want_loss += float(mean.cpu()[0]) * int(c[0])
        # float64 on the batch's fp32 logits bounds both sides
        with torch.no_grad():
            H = model.features(b.x, b.edge_index_agg).contiguous().cpu().numpy()
        (M, _), loss64, e_eval, _, aux = R.eval_ref(H, W, bias, b.y.cpu().numpy(), None, B)
        assert M == B == int(c[0])
        want += loss64
        bound += e_eval + R.mean_loss_bound(H.shape[0], aux)
    loader.status()
    assert sizes == [R.BATCH, R.BATCH, R.N_TEST - 2 * R.BATCH]
    (rows, hits, loss), = EvalSums.read(sums)
    print(f"rows {rows} hits {hits} loss_sum {loss!r}; sum of mean * M {want_loss!r}; float64 {want!r}; bound {bound:.3e}")
    assert [rows, hits] == counts.tolist() and rows == R.N_TEST
    assert abs(loss - want_loss) <= bound and bound <= 1e-4 * want
    assert all(same_bits(x, y) for x, y in zip(state, trainer.state())) and model.training


def test_a_captured_pass_equals_the_eager_pass(env):
    from sgracex1_amd.train import EvalSums, NodeTrainer
    model, data, gat, half = env
    trainer = NodeTrainer(model, lr=0.01, weight_decay=5e-4, seed=5)
    la, lb = _loader(data, gat, half, shuffle=True), _loader(data, gat, half, shuffle=True)
    state = trainer.state()
    run_pass = trainer.capture_eval_loader(la)
    assert all(same_bits(x, y) for x, y in zip(state, trainer.state())) and model.training
    replayed = []
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                           # a pass reads nothing back through torch
    try:
        for _ in range(2):
            sums = run_pass()
            assert sums is run_pass.sums and isinstance(sums, EvalSums)
            replayed.append(sums.buffer.clone())
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    eager, sums = [], EvalSums(DEV)
    for _ in range(2):
        sums.zero_()
        for b in lb:
            assert (b.num_real_nodes is None) == (b.batch_size == R.BATCH)
            trainer.evaluate(b.x, b.edge_index_agg, b.y, n_prefix=b.batch_size, into=sums)
        eager.append(sums.buffer.clone())
    la.status(), lb.status()
    for i, (r, e) in enumerate(zip(replayed, eager)):
        assert same_bits(r, e), (i, r.tolist(), e.tolist())
        assert int(r[0]) == R.N_TEST and 0 <= int(r[1]) <= R.N_TEST
    assert not same_bits(replayed[0][2:], replayed[1][2:])           # the second pass drew new samples
    assert all(same_bits(x, y) for x, y in zip(state, trainer.state())) and model.training


def test_training_epochs_and_eval_passes_interleave_as_eager_ones(env):
    from sgracex1_amd.train import EvalSums, NodeTrainer
    model, data, gat, half = env
    twin = copy.deepcopy(model)
    a, b = NodeTrainer(model, lr=0.01, weight_decay=5e-4, seed=5), NodeTrainer(twin, lr=0.01, weight_decay=5e-4, seed=5)
    ta, tb = _loader(data, gat, half, "train", True), _loader(data, gat, half, "train", True)
    ea, eb = _loader(data, gat, half), _loader(data, gat, half)
    epoch, run_pass = a.capture_loader(ta), a.capture_eval_loader(ea)
    assert int(a.t) == 0
    got_losses, got_sums, want_losses, want_sums = [], [], [], []
    sums = EvalSums(DEV)
    for _ in range(2):
        got_losses += epoch()
        got_sums.append(run_pass().buffer.clone())
        want_losses += [b.step(bt.x, bt.edge_index_agg, bt.y, n_prefix=bt.batch_size) for bt in tb]
        sums.zero_()
        for bt in eb:
            b.evaluate(bt.x, bt.edge_index_agg, bt.y, n_prefix=bt.batch_size, into=sums)
        want_sums.append(sums.buffer.clone())
    for loader in (ta, tb, ea, eb):
        loader.status()
    assert len(got_losses) == len(want_losses) == 6 and all(same_bits(r, e) for r, e in zip(got_losses, want_losses))
    assert all(same_bits(r, e) for r, e in zip(got_sums, want_sums))
    assert not same_bits(got_sums[0], got_sums[1])                    # the parameters moved between the two passes
    assert int(a.t) == int(b.t) == 6 and model.training and twin.training
    for x1, x2 in zip(a.state(), b.state()):
        assert same_bits(x1, x2)

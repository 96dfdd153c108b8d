"""sgx_head_loss and sgx_adam_step on the device against the float64 restatement of their rules
(tests/_train_tail_ref.py), inside the bounds derived there from the operation counts."""
import numpy as np
import pytest
import torch

import _train_tail_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _head_case(G, P, C, seed, bias=True, big=False):
    rng = np.random.default_rng(seed)
    pooled = rng.standard_normal((G, P)).astype(np.float32)
    W = rng.standard_normal((C, P)).astype(np.float32)
    if big:                                    # logits of magnitude 80: sum exp(z) without the max overflows fp32
        W *= np.float32(80.0 / max(1.0, np.sqrt(P)))
    b = rng.standard_normal(C).astype(np.float32) if bias else None
    t = rng.integers(0, C, G)
    t[0], t[-1] = 0, C - 1                     # both ends of the class range
    return pooled, W, b, t


def _run_head(pooled, W, b, t, **kw):
    from sgracex1_amd import ops
    d = lambda a: None if a is None else torch.as_tensor(a, device=DEV)
    out = ops.head_loss(d(pooled), d(W), d(b), d(np.asarray(t, np.int64)), want_logits=True, **kw)
    torch.cuda.synchronize()
    return out


def _check_head(pooled, W, b, t, p, seed=77, step=5, grad_scale=1.0):
    loss, gp, gw, gb, logits = _run_head(pooled, W, b, t, p=p, seed=seed, step=step, grad_scale=grad_scale)
    r_loss, r_z, r_gp, r_gw, r_gb, aux = R.head_f64(pooled, W, b, t, p=p, seed=seed, step=step, grad_scale=grad_scale)
    bound = R.head_bounds(aux)
    worst = {}
    for name, got, ref in (("logits", logits, r_z), ("loss", loss, np.array([r_loss])), ("grad_pooled", gp, r_gp),
                           ("grad_W", gw, r_gw), ("grad_bias", gb, r_gb)):
        if ref is None:
            assert got is None
            continue
        err = np.abs(got.double().cpu().numpy() - ref)
        worst[name] = float((err / bound[name]).max())
    print("head error / bound:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst
    return (loss, gp, gw, gb, logits), aux, (r_loss, r_z, r_gp, r_gw, r_gb)


HEAD_SHAPES = [(1, 1, 1), (3, 7, 2), (64, 64, 7), (188, 64, 2), (257, 65, 64), (513, 7, 2), (3, 256, 64), (188, 65, 1)]


@pytest.mark.parametrize("G,P,C", HEAD_SHAPES)
@pytest.mark.parametrize("p", [0.0, 0.5, 0.9])
def test_head_loss_inside_the_bound(G, P, C, p):
    pooled, W, b, t = _head_case(G, P, C, seed=G * 1000 + P + C)
    _check_head(pooled, W, b, t, p)


@pytest.mark.parametrize("G,P", [(1, 1), (3, 7), (188, 64), (257, 64), (513, 33)])
@pytest.mark.parametrize("p", [0.5, 0.9])
def test_head_loss_mask_is_the_references(G, P, p):
    """The kernel's mask, element for element and exactly: with the identity as the head (C = P <= 64) and no bias,
    logit (g, j) is x[g][j] itself -- every other term of its sum is an exact zero -- so the logits are the reference's x
    bit for bit, 0 exactly where an element is dropped and pooled * scale (not 0) where it is kept."""
    rng = np.random.default_rng(G + P)
    pooled = (rng.standard_normal((G, P)) + np.where(rng.random((G, P)) < 0.5, 3.0, -3.0)).astype(np.float32)   # never 0
    t = rng.integers(0, P, G)
    logits = _run_head(pooled, np.eye(P, dtype=np.float32), None, t, p=p, seed=2024, step=9)[4].cpu().numpy()
    x, keep, _ = R.dropped(pooled, p, 2024, 9)
    assert np.array_equal(keep, R.keep_mask(G, P, p, 2024, 9)) and (x[keep] != 0).all()
    assert np.array_equal(logits != 0, keep)
    assert logits.tobytes() == x.tobytes()


@pytest.mark.parametrize("G,P,C", [(188, 65, 2), (257, 256, 7), (3, 1024, 64)])
@pytest.mark.parametrize("p", [0.5, 0.9])
def test_head_logits_with_dropout_are_readout_mean_linears_bits_on_the_references_x(G, P, C, p):
    """Wider than the identity head reaches: the logits at p > 0 are sgx_readout_mean_linear's bits on the reference's
    x (one-row graphs) -- the mask, the scale and the summation order at once."""
    from sgracex1_amd import ops
    pooled, W, b, t = _head_case(G, P, C, seed=12)
    logits = _run_head(pooled, W, b, t, p=p, seed=5, step=1)[4]
    x, _, _ = R.dropped(pooled, p, 5, 1)
    want = ops.readout_mean_linear(torch.as_tensor(x, device=DEV), torch.arange(G + 1, dtype=torch.int32, device=DEV),
                                   torch.as_tensor(W, device=DEV), torch.as_tensor(b, device=DEV))
    assert same_bits(logits, want)


@pytest.mark.parametrize("G,P,C", [(1, 1, 1), (3, 7, 2), (188, 64, 2), (257, 65, 7), (64, 256, 64)])
def test_head_logits_without_dropout_are_readout_mean_linears_bits(G, P, C):
    from sgracex1_amd import ops
    pooled, W, b, t = _head_case(G, P, C, seed=4)
    for bias in (b, None):
        logits = _run_head(pooled, W, bias, t, p=0.0)[4]
        want = ops.readout_mean_linear(torch.as_tensor(pooled, device=DEV), torch.arange(G + 1, dtype=torch.int32, device=DEV),
                                       torch.as_tensor(W, device=DEV), None if bias is None else torch.as_tensor(bias, device=DEV))
        assert same_bits(logits, want)


def test_head_loss_edges():
    """No bias; one target out of range (no loss, no gradient, the divisor stays G); logits of magnitude 80; a gradient
    scale."""
    pooled, W, b, t = _head_case(64, 65, 7, seed=5)
    _check_head(pooled, W, None, t, 0.5)
    t2 = t.copy()
    t2[3], t2[9] = 7, -1
    got, aux, ref = _check_head(pooled, W, b, t2, 0.5)
    assert not got[1][3].any() and not got[1][9].any()
    big = _head_case(188, 64, 7, seed=6, big=True)
    got, aux, ref = _check_head(*big, 0.0)
    assert np.abs(aux["z"]).max() > 80 and np.isfinite(got[0].cpu().numpy()).all()
    _check_head(pooled, W, b, t, 0.5, grad_scale=0.37)


def test_head_loss_repeats_its_bits_and_reads_the_device_step():
    pooled, W, b, t = _head_case(513, 65, 7, seed=8)
    a = _run_head(pooled, W, b, t, p=0.5, seed=1, step=40)
    c = _run_head(pooled, W, b, t, p=0.5, seed=1, step=40)
    assert all(same_bits(x, y) for x, y in zip(a, c))
    s = torch.tensor([33], dtype=torch.int64, device=DEV)
    e = _run_head(pooled, W, b, t, p=0.5, seed=1, step=7, step_dev=s)
    assert all(same_bits(x, y) for x, y in zip(a, e))
    f = _run_head(pooled, W, b, t, p=0.5, seed=1, step=41)
    assert not same_bits(a[1], f[1])


def test_head_loss_autograd_function():
    from sgracex1_amd import ops
    pooled, W, b, t = _head_case(64, 64, 2, seed=10)
    tp, tw, tb = (torch.as_tensor(a, device=DEV).requires_grad_() for a in (pooled, W, b))
    loss = ops.HeadLoss.apply(tp, tw, tb, torch.as_tensor(t, device=DEV), 0.5, 3, 4, None)
    (loss * 2.0).backward()
    raw = _run_head(pooled, W, b, t, p=0.5, seed=3, step=4)
    assert same_bits(loss.detach().reshape(1), raw[0])
    for got, want in ((tp.grad, raw[1]), (tw.grad, raw[2]), (tb.grad, raw[3])):
        assert same_bits(got, want * 2.0)


# ---- Adam --------------------------------------------------------------------------------------------------------------
HYPER = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8)


def _adam_run(sizes, steps, t0, wd, zero_grad_at=None, seed=0, none_at=None):
    """`steps` calls of ops.adam_step on tensors of `sizes` against the float64 rule; returns the worst error / bound."""
    from sgracex1_amd import ops
    rng = np.random.default_rng(seed)
    P = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    M = [(rng.standard_normal(n) * 0.1).astype(np.float32) if t0 else np.zeros(n, np.float32) for n in sizes]
    V = [(rng.random(n) * 0.01).astype(np.float32) if t0 else np.zeros(n, np.float32) for n in sizes]
    tp, tm, tv = ([torch.as_tensor(a, device=DEV) for a in arrs] for arrs in (P, M, V))
    counter = torch.tensor([t0], dtype=torch.int64, device=DEV)
    ref = [(p.astype(np.float64), m.astype(np.float64), v.astype(np.float64)) for p, m, v in zip(P, M, V)]
    err = [(0.0, 0.0, 0.0)] * len(sizes)
    worst = 0.0
    for k in range(steps):
        t = t0 + k + 1
        grads = [(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 2)).astype(np.float32) for n in sizes]
        if zero_grad_at == k:
            grads = [np.zeros_like(g) for g in grads]
        tg = [torch.as_tensor(g, device=DEV) for g in grads]
        if none_at is not None:
            tg[none_at] = None
        ops.adam_step(tp, tg, tm, tv, counter, lr=HYPER["lr"], betas=(HYPER["beta1"], HYPER["beta2"]), eps=HYPER["eps"], weight_decay=wd)
        for i, n in enumerate(sizes):
            if n == 0 or i == none_at:
                continue
            err[i] = R.adam_bound_step(*ref[i][:1], grads[i], *ref[i][1:], t, *err[i], weight_decay=wd, **HYPER)
            ref[i] = R.adam_f64(ref[i][0], grads[i], ref[i][1], ref[i][2], t, weight_decay=wd, **HYPER)
            for got, want, e in zip((tp[i], tm[i], tv[i]), ref[i], err[i]):
                worst = max(worst, float((np.abs(got.double().cpu().numpy() - want) / e).max()))
        if k == 0 or k == steps - 1:
            assert worst <= 1.0, (k, worst)
    assert int(counter.item()) == t0 + steps
    if none_at is not None:                                       # a skipped tensor is untouched
        assert np.array_equal(tp[none_at].cpu().numpy(), P[none_at]) and np.array_equal(tm[none_at].cpu().numpy(), M[none_at])
    print("adam error / bound:", round(worst, 4))
    return worst


@pytest.mark.parametrize("t0", [0, 999])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_sizes_inside_the_bound(t0, wd):
    _adam_run([1, 63, 64, 65, 7 * 64, 64 * 64, 256 * 256 + 1], 5, t0, wd, seed=t0 + 1)


@pytest.mark.parametrize("sizes,none_at", [([65], None), ([7 * 64, 0, 63], None), ([33 + 7 * k for k in range(16)], 5)])
def test_adam_tensor_counts_empty_and_missing_gradients(sizes, none_at):
    _adam_run(sizes, 5, 0, 0.01, zero_grad_at=2, seed=len(sizes), none_at=none_at)


def test_adam_all_zero_gradient_first_step():
    _adam_run([65, 1024], 1, 0, 0.0, zero_grad_at=0)


@pytest.mark.parametrize("rows,cols", [(7, 64), (64, 2)])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_adam_transposed_output_is_torchs_bits(rows, cols, dtype):
    from sgracex1_amd import ops
    g = torch.Generator(device=DEV).manual_seed(rows)
    p = torch.randn(rows, cols, device=DEV, generator=g)
    grad = torch.randn(rows, cols, device=DEV, generator=g)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    out = torch.full((cols, rows), float("nan"), dtype=dtype, device=DEV)
    before = p.clone()
    ops.adam_step([p], [grad], [m], [v], torch.zeros(1, dtype=torch.int64, device=DEV), lr=0.01, transposed_out=[out])
    assert not same_bits(p, before)
    assert same_bits(out, torch.transpose(p, 0, 1).to(dtype).contiguous())


def test_adam_captured_call_replays_to_the_eager_bits():
    from sgracex1_amd import ops
    sizes = [65, 7 * 64, 64 * 64]
    g = torch.Generator(device=DEV).manual_seed(1)
    new = lambda: [torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(n)) for n in sizes]
    grads = [torch.randn(n, device=DEV, generator=g) for n in sizes]
    states = []
    for _ in range(2):
        states.append((new(), [torch.zeros(n, device=DEV) for n in sizes], [torch.zeros(n, device=DEV) for n in sizes],
                       torch.zeros(1, dtype=torch.int64, device=DEV)))
    call = lambda s: ops.adam_step(s[0], grads, s[1], s[2], s[3], lr=0.01, weight_decay=0.01)
    for _ in range(3):
        call(states[0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(states[1])
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(states[1][3].item()) == 3
    for k in range(3):
        assert all(same_bits(a, b) for a, b in zip(states[0][k], states[1][k]))


def test_adam_refuses_more_tensors_than_one_launch_takes():
    from sgracex1_amd import ops
    ts = lambda: [torch.zeros(3, device=DEV) for _ in range(17)]
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="at most 16"):
        ops.adam_step(ts(), ts(), ts(), ts(), counter)
    assert int(counter.item()) == 0

"""sgx_node_loss on the device against the float64 restatement of its rule (tests/_node_loss_ref.py), inside the bounds
derived there from the operation counts, on the inputs tests/test_node_loss_cpu.py holds to the bounds' conditions."""
import ctypes

import numpy as np
import pytest
import torch

import _node_loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPECS = R.gpu_case_specs()


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def d(a):
    return None if a is None else torch.as_tensor(a, device=DEV)


def _run(c, p=None, **kw):
    from sgracex1_amd import ops
    out = ops.node_loss(d(c["H"]), d(c["W"]), d(c["bias"]), d(c["target"]), mask=d(c["mask"]), n_prefix=c["n_prefix"],
                        p=c["p"] if p is None else p, seed=c["seed"], step=c["step"], grad_scale=c["grad_scale"], want_logits=True,
                        want_counts=True, **kw)
    torch.cuda.synchronize()
    return out


def _ref(c, p=None):
    return R.node_f64(c["H"], c["W"], c["bias"], c["target"], c["mask"], c["n_prefix"], c["p"] if p is None else p, c["seed"], c["step"],
                      c["grad_scale"])


def _check(c):
    loss, gh, gw, gb, counts, logits = _run(c)
    r_loss, r_z, r_gh, r_gw, r_gb, r_counts, aux = _ref(c)
    bound = R.node_bounds(aux)
    worst = {}
    for name, got, ref in (("logits", logits, r_z), ("loss", loss, np.array([r_loss])), ("grad_H", gh, r_gh), ("grad_W", gw, r_gw),
                           ("grad_bias", gb, r_gb)):
        if ref is None:
            assert got is None
            continue
        err = np.abs(got.double().cpu().numpy() - ref)
        worst[name] = float((err / bound[name]).max())
    print("node loss error / bound:", {k: round(v, 4) for k, v in worst.items()}, "counts", counts.tolist(), r_counts)
    assert all(v <= 1.0 for v in worst.values()), worst
    assert tuple(counts.tolist()) == r_counts
    g = gh.cpu().numpy()
    sel, keep = aux["sel"], aux["keep"]
    assert not g[~sel].any() and g[~sel].tobytes() == bytes(g[~sel].nbytes)         # exact +0 in unselected rows
    # the mask element for element: a dropped element is an exact zero; a kept one of a selected row whose float64 value
    # exceeds its bound cannot be zero (W > 0, so such elements are nearly all of them: the CPU test's inputs)
    assert not g[sel][~keep[sel]].any()
    must = sel[:, None] & keep & (np.abs(r_gh) > bound["grad_H"])
    assert (g[must] != 0).all()
    if aux["M"] and c["W"].shape[0] > 1:
        assert must.sum() >= 0.9 * (sel[:, None] & keep).sum()
    # p = 0: the logits of every row
    z0 = _run(c, p=0.0)[5]
    r0 = _ref(c, p=0.0)
    assert (np.abs(z0.double().cpu().numpy() - r0[1]) <= R.node_bounds(r0[6])["logits"]).all()
    return (loss, gh, gw, gb, counts, logits), aux


@pytest.mark.parametrize("name,kw", SPECS, ids=[s[0] for s in SPECS])
def test_node_loss_inside_the_bound(name, kw):
    _check(R.make_case(**kw))


def test_node_loss_target_out_of_range():
    c = R.make_case(3 * R.ROWS + 5, 65, 7, select="all", p=0.5, seed=21)
    c["target"][3], c["target"][R.ROWS + 2] = 7, -1
    got, aux = _check(c)
    assert not got[1][3].any() and not got[1][R.ROWS + 2].any() and int(got[4][0]) == len(c["H"])


def test_evaluation_mode_writes_no_gradient_and_agrees_with_training_mode():
    from sgracex1_amd import _lib, ops
    c = R.make_case(3 * R.ROWS + 5, 65, 7, select="hole", p=0.0, seed=22)
    full = _run(c)
    ev = _run(c, grads=False)
    assert ev[1] is None and ev[2] is None and ev[3] is None
    assert same_bits(ev[0], full[0]) and same_bits(ev[4], full[4]) and same_bits(ev[5], full[5])
    ev2 = ops.node_loss(d(c["H"]), d(c["W"]), d(c["bias"]), d(c["target"]), mask=d(c["mask"]), p=0.0, grads=False)
    assert same_bits(ev2[0], full[0])                                    # without logits or counts: selected rows only
    # straight through the C ABI: evaluation mode IS the three gradient pointers being NULL, so there is no buffer it
    # could write; what a sentinel can show is that training mode fills exactly its buffers and nothing around them
    n, P, C = len(c["H"]), 65, 7
    H, W, b, t, m = d(c["H"]), d(c["W"]), d(c["bias"]), d(c["target"]), d(c["mask"]).view(torch.uint8)
    loss = torch.full((1,), 12345.0, device=DEV)
    nbytes = _lib.lib.sgx_node_loss_workspace_bytes(n, P, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())
    st = _lib.lib.sgx_node_loss(n, n, P, C, ptr(H), ptr(W), ptr(b), ptr(t), ptr(m), 0.0, 0, 0, None, 1.0, ptr(loss), None, None,
                                None, None, None, ptr(ws), nbytes, None)
    torch.cuda.synchronize()
    assert st == 0 and same_bits(loss, full[0])
    # and training mode fills exactly its buffers: sentinels around them survive
    buf = torch.full((n * P + C * P + C + 3 * 64,), 12345.0, device=DEV)
    gh, gw, gb = buf[64:64 + n * P], buf[128 + n * P:128 + n * P + C * P], buf[192 + n * P + C * P:192 + n * P + C * P + C]
    st = _lib.lib.sgx_node_loss(n, n, P, C, ptr(H), ptr(W), ptr(b), ptr(t), ptr(m), 0.0, 0, 0, None, 1.0, ptr(loss), None, None,
                                ptr(gh), ptr(gw), ptr(gb), ptr(ws), nbytes, None)
    torch.cuda.synchronize()
    assert st == 0 and same_bits(gh.reshape(n, P), full[1]) and same_bits(gw.reshape(C, P), full[2]) and same_bits(gb, full[3])
    pads = torch.cat([buf[:64], buf[64 + n * P:128 + n * P], buf[128 + n * P + C * P:192 + n * P + C * P]])
    assert bool((pads == 12345.0).all())


def test_node_loss_repeats_its_bits_and_reads_the_device_step():
    c = R.make_case(R.GRID * R.ROWS + R.ROWS + 1, 9, 5, select="mask", p=0.5, seed=23)
    a, b = _run(c), _run(c)
    assert all(same_bits(x, y) for x, y in zip(a, b))
    from sgracex1_amd import ops
    args = (d(c["H"]), d(c["W"]), d(c["bias"]), d(c["target"]))
    kw = dict(mask=d(c["mask"]), p=0.5, seed=c["seed"], want_logits=True, want_counts=True)
    s = torch.tensor([c["step"] - 2], dtype=torch.int64, device=DEV)
    e = ops.node_loss(*args, step=2, step_dev=s, **kw)
    assert all(same_bits(x, y) for x, y in zip(a, e))
    f = ops.node_loss(*args, step=c["step"] + 1, **kw)
    assert not same_bits(a[1], f[1])


def test_node_loss_captured_once_and_replayed_equals_eager_calls():
    from sgracex1_amd import ops
    c = R.make_case(3 * R.ROWS + 5, 65, 7, select="mask", p=0.5, seed=24)
    args = (d(c["H"]), d(c["W"]), d(c["bias"]), d(c["target"]))
    kw = dict(mask=d(c["mask"]), p=0.5, seed=9, want_counts=True)
    eager = []
    for k in range(3):
        eager.append([t.clone() for t in ops.node_loss(*args, step_dev=torch.tensor([k], dtype=torch.int64, device=DEV), **kw)])
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.node_loss(*args, step_dev=counter, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.node_loss(*args, step_dev=counter, **kw)
    for k in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert all(same_bits(x, y) for x, y in zip(out, eager[k])), k
        counter += 1
    assert not same_bits(eager[0][1], eager[1][1])


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_more_than_64_kib_of_lds_on_a_second_device_of_the_process():
    """The opt-in to more dynamic LDS belongs to a kernel on a device: at n = 17, P = 1024, C = 16 both node kernels ask
    for more than 64 KiB, on device 0 and then on device 1 of the one process, each against its own device's reference."""
    import _node_eval_ref as E
    from sgracex1_amd import ops
    n, P, C = R.ROWS + 1, 1024, 16
    c, e = R.make_case(n, P, C, select="mask", seed=31), E.make_case(n, P, C, mask="sparse", seed=31)
    (M, hits), loss, bound, z32, _ = E.eval_ref(e["H"], e["W"], e["bias"], e["target"], e["mask"], n)
    for k in (0, 1):
        with torch.cuda.device(k):
            _check(c)
            operands = [None if a is None else torch.from_numpy(a).to(f"cuda:{k}") for a in (e["H"], e["W"], e["bias"], e["target"], e["mask"])]
            totals = torch.zeros(2, dtype=torch.int64, device=f"cuda:{k}")
            loss_sum = torch.zeros(1, dtype=torch.float64, device=f"cuda:{k}")
            _, _, logits = ops.node_eval(*operands[:4], totals, loss_sum, mask=operands[4], n_prefix=n, want_logits=True)
            torch.cuda.synchronize()
            assert logits.device.index == k and totals.tolist() == [M, hits]
            assert abs(float(loss_sum.cpu()[0]) - loss) <= bound
            assert np.array_equal(logits.cpu().numpy().view(np.int32), z32.view(np.int32))


def test_node_loss_refuses_what_the_header_refuses():
    from sgracex1_amd import _lib, ops
    c = R.make_case(R.ROWS + 1, 257, 64, select="mask")
    assert _lib.lib.sgx_node_loss_workspace_bytes(R.ROWS + 1, 257, 64) == 0
    with pytest.raises(_lib.SgxError) as e:
        ops.node_loss(d(c["H"]), d(c["W"]), d(c["bias"]), d(c["target"]), mask=d(c["mask"]))
    assert e.value.status == -3
    ok = R.make_case(R.ROWS + 1, 8, 2, select="mask")
    with pytest.raises(_lib.SgxError) as e:
        ops.node_loss(d(ok["H"]), d(ok["W"]), d(ok["bias"]), d(ok["target"]), p=1.0)
    assert e.value.status == -3
    with pytest.raises(_lib.SgxError) as e:
        ops.node_loss(d(ok["H"]), d(ok["W"]), d(ok["bias"]), d(ok["target"]), n_prefix=-1)
    assert e.value.status == -2
    n, P, C = R.ROWS + 1, 8, 2
    H, W, b, t = d(ok["H"]), d(ok["W"]), d(ok["bias"]), d(ok["target"])
    out = torch.empty(n * P + C * P + C + 1, device=DEV)
    nbytes = _lib.lib.sgx_node_loss_workspace_bytes(n, P, C)
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
    ptr = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off)
    call = lambda **k: _lib.lib.sgx_node_loss(n, n, P, C, k.get("H", ptr(H)), ptr(W), ptr(b), ptr(t), None, 0.5, 0, 0, None, 1.0,
                                              k.get("loss", ptr(out)), None, None, k.get("gh", ptr(out, 4)), ptr(out, 4 + 4 * n * P),
                                              k.get("gb", ptr(out, 4 + 4 * n * P + 4 * C * P)), k.get("ws", ptr(ws)),
                                              k.get("wsb", nbytes), None)
    assert call() == 0
    assert call(H=None) == -1 and call(loss=None) == -1 and call(gh=None) == -1 and call(gb=None) == -1
    assert call(ws=None) == -4 and call(wsb=nbytes - 1) == -4 and call(ws=ptr(ws, 8)) == -7
    torch.cuda.synchronize()

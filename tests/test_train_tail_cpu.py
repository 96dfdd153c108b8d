"""CPU checks of the training tail's references (tests/_train_tail_ref.py) against torch in float64, of the dropout mask as
a fixed function, and of the argument errors of sgx_head_loss / sgx_adam_step, which answer before anything reaches a
device."""
import ctypes

import numpy as np
import pytest
import torch

import _train_tail_ref as R


def _case(G, P, C, seed=0, bias=True, scale=1.0):
    rng = np.random.default_rng(seed)
    pooled = rng.standard_normal((G, P)).astype(np.float32)
    W = (rng.standard_normal((C, P)) * scale).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32) if bias else None
    t = rng.integers(0, C, G)
    return pooled, W, b, t


@pytest.mark.parametrize("G,P,C,p,bias", [(5, 7, 3, 0.0, True), (64, 65, 7, 0.5, True), (33, 16, 2, 0.9, False), (3, 1, 1, 0.5, True)])
def test_head_reference_matches_torch_float64_autograd(G, P, C, p, bias):
    pooled, W, b, t = _case(G, P, C, seed=G, bias=bias)
    loss, z, gp, gw, gb, aux = R.head_f64(pooled, W, b, t, p=p, seed=11, step=3, grad_scale=1.0)
    x, keep, scale = R.dropped(pooled, p, 11, 3)
    # torch: F.linear on the masked and scaled input x (the fp32 values of the rule); dropout's own backward is the same
    # mask and scale on x's gradient
    tW = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    tb = None if b is None else torch.tensor(b, dtype=torch.float64, requires_grad=True)
    tx = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tl = torch.nn.functional.cross_entropy(torch.nn.functional.linear(tx, tW, tb), torch.tensor(t), reduction="mean")
    tl.backward()
    eps = np.finfo(np.float64).eps
    tol = lambda ref: 64 * eps * (P + C + G) * max(1.0, float(np.abs(ref).max()))       # float64 rounding of sums this long
    assert abs(loss - float(tl.detach())) <= tol(np.array([loss]))
    assert np.abs(gp - tx.grad.numpy() * np.where(keep, float(scale), 0.0)).max() <= tol(gp)
    assert np.abs(gw - tW.grad.numpy()).max() <= tol(gw)
    if b is not None:
        assert np.abs(gb - tb.grad.numpy()).max() <= tol(gb)
    else:
        assert gb is None


def test_head_reference_skips_targets_out_of_range():
    pooled, W, b, t = _case(6, 5, 3, seed=2)
    t2 = t.copy()
    t2[1], t2[4] = -1, 3
    loss, z, gp, gw, gb, aux = R.head_f64(pooled, W, b, t2)
    keep = np.array([0, 2, 3, 5])
    loss_k, _, gp_k, gw_k, gb_k, _ = R.head_f64(pooled[keep], W, b, t2[keep])
    assert np.isclose(loss * 6, loss_k * 4, rtol=1e-14)                      # the divisor stays G
    assert not gp[[1, 4]].any()
    assert np.allclose(gw * 6, gw_k * 4, rtol=1e-13, atol=1e-15) and np.allclose(gb * 6, gb_k * 4, rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_adam_reference_matches_torch_float64_over_five_steps(wd):
    rng = np.random.default_rng(5)
    p0 = rng.standard_normal(97)
    grads = [rng.standard_normal(97) * 10.0 ** rng.integers(-3, 2) for _ in range(5)]
    tp = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([tp], lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    p, m, v = p0.copy(), np.zeros(97), np.zeros(97)
    for t, g in enumerate(grads, 1):
        tp.grad = torch.tensor(g)
        opt.step()
        p, m, v = R.adam_f64(p, g, m, v, t, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=wd, rounded_constants=False)
        # float64 rounding: a dozen operations per step, the division by sqrt(v) + eps well conditioned
        assert np.abs(p - tp.detach().numpy()).max() <= 64 * t * np.finfo(np.float64).eps * max(1.0, np.abs(p).max())
    st = opt.state[tp]
    assert np.allclose(m, st["exp_avg"].numpy(), rtol=1e-13, atol=0) and np.allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-13, atol=0)


def test_adam_bound_covers_a_float32_run_of_the_rule():
    """The derived bound against the rule evaluated in numpy float32 operation by operation (what the kernel does)."""
    rng = np.random.default_rng(9)
    f = np.float32
    p32 = rng.standard_normal(500).astype(f)
    m32, v32 = np.zeros(500, f), np.zeros(500, f)
    p, m, v = p32.astype(np.float64), m32.astype(np.float64), v32.astype(np.float64)
    e = (0.0, 0.0, 0.0)
    for t in range(1, 6):
        g32 = (rng.standard_normal(500) * 10.0 ** rng.integers(-3, 2)).astype(f)
        if t == 3:
            g32[:] = 0
        c = {k: f(val) for k, val in R.adam_constants(0.01, 0.9, 0.999, 1e-8, 0.01, t).items()}
        e = R.adam_bound_step(p, g32, m, v, t, *e, lr=0.01, weight_decay=0.01)
        p, m, v = R.adam_f64(p, g32, m, v, t, lr=0.01, weight_decay=0.01)
        g = g32 + c["wd"] * p32
        m32 = c["b1"] * m32 + c["ob1"] * g
        v32 = c["b2"] * v32 + c["ob2"] * (g * g)
        p32 = p32 - (c["lr"] / c["bc1"]) * (m32 / (np.sqrt(v32) / c["sbc2"] + c["eps"]))
        assert p32.dtype == f
        assert (np.abs(p32 - p) <= e[0]).all() and (np.abs(m32 - m) <= e[1]).all() and (np.abs(v32 - v) <= e[2]).all()
        assert e[0].max() < 1e-4                                     # and the bound says something


def test_mask_is_a_fixed_function():
    a = R.keep_mask(16, 64, 0.5, 12345, 7)
    assert np.array_equal(a, R.keep_mask(16, 64, 0.5, 12345, 7))
    assert np.array_equal(a[:4, :], R.keep_mask_scalar(4, 64, 0.5, 12345, 7))       # numpy's wrap-around == Python integers
    assert not np.array_equal(a, R.keep_mask(16, 64, 0.5, 12345, 8))
    assert not np.array_equal(a, R.keep_mask(16, 64, 0.5, 12346, 7))
    assert R.keep_mask(16, 64, 0.0, 12345, 7).all()
    n, p = 1 << 16, 0.5
    share = R.keep_mask(256, 256, p, 12345, 0).mean()
    assert abs(share - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n)
    x, keep, scale = R.dropped(np.ones((4, 8), np.float32), 0.0, 1, 2)
    assert scale == 1 and x.tobytes() == np.ones((4, 8), np.float32).tobytes()


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def test_head_loss_argument_errors_need_no_gpu(L):
    one = ctypes.c_void_p(256)                     # never dereferenced: every error is returned before a launch
    call = lambda G=4, P=8, C=2, pooled=one, W=one, bias=one, target=one, p=0.5, loss=one, gp=one, gw=one, gb=one, ws=one, wsb=1 << 20: \
        L.lib.sgx_head_loss(G, P, C, pooled, W, bias, target, p, 1, 0, None, 1.0, loss, None, gp, gw, gb, ws, wsb, None)
    assert call(G=0) == -2 and call(P=0) == -2 and call(C=0) == -2
    for name in ("pooled", "W", "target", "loss", "gp", "gw", "gb"):
        assert call(**{name: None}) == -1, name
    assert call(p=1.0) == -3 and call(p=-0.1) == -3 and call(p=float("nan")) == -3
    assert call(P=1025) == -3 and call(C=65) == -3
    need = L.lib.sgx_head_loss_workspace_bytes(4, 8, 2)
    assert need >= 4 * (2 * 8 + 2 + 1) * 4 and need % 256 == 0
    assert L.lib.sgx_head_loss_workspace_bytes(1000, 1024, 64) == 256 * (64 * 1024 + 64 + 1) * 4
    assert L.lib.sgx_head_loss_workspace_bytes(4, 1025, 2) == 0 and L.lib.sgx_head_loss_workspace_bytes(0, 8, 2) == 0
    assert call(ws=None) == -4 and call(wsb=need - 1) == -4
    assert call(ws=ctypes.c_void_p(264)) == -7


def test_adam_step_argument_errors_need_no_gpu(L):
    d = L.AdamDesc()
    assert L.lib.sgx_adam_step(None, None) == -1
    assert L.lib.sgx_adam_step(ctypes.byref(d), None) == -1            # no counter
    d.step = 256
    d.lr, d.beta1, d.beta2, d.eps = 0.01, 0.9, 0.999, 1e-8
    d.n_tensors = 17
    assert L.lib.sgx_adam_step(ctypes.byref(d), None) == -2
    d.n_tensors = 1
    T = d.tensor[0]
    T.n, T.grad = 8, 256
    assert L.lib.sgx_adam_step(ctypes.byref(d), None) == -1            # param, m, v missing on a tensor with a gradient
    T.param = T.m = T.v = 256
    T.n = -1
    assert L.lib.sgx_adam_step(ctypes.byref(d), None) == -2
    T.n = 8
    T.param_t_out, T.rows, T.cols, T.dtype_t = 256, 3, 3, 0
    assert L.lib.sgx_adam_step(ctypes.byref(d), None) == -2
    T.rows, T.cols, T.dtype_t = 2, 4, 5
    assert L.lib.sgx_adam_step(ctypes.byref(d), None) == -3
    T.dtype_t = 0
    for field, bad in (("lr", -1.0), ("beta1", 1.0), ("beta2", -0.5), ("eps", float("nan")), ("weight_decay", -1e-3)):
        keep = getattr(d, field)
        setattr(d, field, bad)
        assert L.lib.sgx_adam_step(ctypes.byref(d), None) == -3, field
        setattr(d, field, keep)
    assert ctypes.sizeof(L.AdamDesc) == 8 + 5 * 8 + 8 + 16 * 64

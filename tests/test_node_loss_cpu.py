"""The float64 restatement of the node loss head (tests/_node_loss_ref.py) against torch's float64 autograd, the M == 0
rule, the conditions its bounds must meet on every input the GPU test uses, and the argument errors of sgx_node_loss, which
answer before anything reaches a device."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _node_loss_ref as R


def _torch_f64(c):
    """loss and gradients of F.cross_entropy(F.linear(x_dropped, W, b)[sel], y[sel]) * grad_scale in float64."""
    x32, keep, scale = R.dropped(c["H"], c["p"], c["seed"], c["step"])
    H = torch.tensor(c["H"], dtype=torch.float64, requires_grad=True)
    W = torch.tensor(c["W"], dtype=torch.float64, requires_grad=True)
    b = None if c["bias"] is None else torch.tensor(c["bias"], dtype=torch.float64, requires_grad=True)
    x = H * torch.tensor(np.where(keep, np.float64(scale), 0.0))
    sel = torch.tensor(R.selection(len(c["H"]), c["mask"], c["n_prefix"]))
    z = F.linear(x, W, b)
    t = torch.tensor(c["target"])
    C = W.shape[0]
    t_ign = torch.where((t >= 0) & (t < C), t, torch.tensor(-100))
    # the rule keeps an out-of-range row in the divisor: sum over the live rows, divided by the count of selected rows
    loss = F.cross_entropy(z[sel], t_ign[sel], ignore_index=-100, reduction="sum") / int(sel.sum())
    (loss * float(np.float32(c["grad_scale"]))).backward()
    return loss.item(), z.detach().numpy(), H.grad.numpy(), W.grad.numpy(), None if b is None else b.grad.numpy()


@pytest.mark.parametrize("name,kw", [
    ("mask", dict(select="mask")), ("prefix", dict(select="prefixR1")), ("both", dict(select="prefix+mask")),
    ("scale", dict(select="mask", grad_scale=0.37)), ("bad-target", dict(select="mask")), ("no-bias", dict(select="hole", bias=False))])
def test_reference_is_torchs_float64_autograd(name, kw):
    c = R.make_case(3 * R.ROWS + 5, 9, 5, p=0.5, seed=11, **kw)
    if name == "bad-target":
        sel = np.nonzero(R.selection(len(c["H"]), c["mask"], c["n_prefix"]))[0]
        c["target"][sel[0]], c["target"][sel[1]] = 5, -1
    loss, z, gh, gw, gb, (M, hits), aux = R.node_f64(c["H"], c["W"], c["bias"], c["target"], c["mask"], c["n_prefix"], c["p"], c["seed"],
                                                   c["step"], c["grad_scale"])
    t_loss, t_z, t_gh, t_gw, t_gb = _torch_f64(c)
    assert abs(loss - t_loss) <= 1e-12
    for got, want in ((z, t_z), (gh, t_gh), (gw, t_gw), (gb, t_gb)):
        assert (got is None) == (want is None)
        if got is not None:
            assert np.abs(got - want).max() <= 1e-12
    sel = R.selection(len(c["H"]), c["mask"], c["n_prefix"])
    assert M == sel.sum() and not gh[~sel].any()
    t = c["target"]
    assert hits == sum(1 for i in np.nonzero(sel)[0] if 0 <= t[i] < 5 and int(np.argmax(z[i])) == t[i])


def test_no_selected_row_gives_zeros_not_nans():
    for select in ("empty", "prefix0"):
        c = R.make_case(R.ROWS + 1, 9, 5, select=select)
        loss, z, gh, gw, gb, counts, aux = R.node_f64(c["H"], c["W"], c["bias"], c["target"], c["mask"], c["n_prefix"], c["p"], c["seed"],
                                                      c["step"])
        assert loss == 0.0 and counts == (0, 0) and not gh.any() and not gw.any() and not gb.any() and np.isfinite(z).all()
        bound = R.node_bounds(aux)
        assert all(np.max(bound[k]) <= R.TINY for k in ("loss", "grad_H", "grad_W", "grad_bias"))


@pytest.mark.parametrize("name,kw", R.gpu_case_specs(), ids=[s[0] for s in R.gpu_case_specs()])
def test_bounds_can_fail_a_wrong_kernel_on_every_gpu_input(name, kw):
    """Each bound is below 1 % of its output's largest magnitude (an output that is identically zero in float64 -- no
    selected row, one class -- is held to fp32's smallest normal number, that is to exact zeros), |H|, |W| <= 1, and the
    arg-max of every selected row outside the constructed ties is decided by more than twice the logits bound."""
    c = R.make_case(**kw)
    assert np.abs(c["H"]).max() <= 1 and np.abs(c["W"]).max() <= 1 and (c["W"] > 0).all()
    loss, z, gh, gw, gb, counts, aux = R.node_f64(c["H"], c["W"], c["bias"], c["target"], c["mask"], c["n_prefix"], c["p"], c["seed"],
                                                  c["step"], c["grad_scale"])
    bound = R.node_bounds(aux)
    for key, ref in (("logits", z), ("loss", np.array([loss])), ("grad_H", gh), ("grad_W", gw), ("grad_bias", gb)):
        if ref is None:
            continue
        assert np.max(bound[key]) <= max(0.01 * np.abs(ref).max(), R.TINY), (key, np.max(bound[key]), np.abs(ref).max())
    # the p == 0 logits too: what the GPU test compares its logits output against
    z0, aux0 = (lambda o: (o[1], o[6]))(R.node_f64(c["H"], c["W"], c["bias"], c["target"], c["mask"], c["n_prefix"], 0.0))
    b0 = R.node_bounds(aux0)["logits"]
    assert b0.max() <= 0.01 * np.abs(z0).max()
    for zz, bb, sel in ((z, bound["logits"], aux["sel"]), (z0, b0, aux0["sel"])):
        rows = np.setdiff1d(np.nonzero(sel)[0], c["tie_rows"])
        assert (R.top_two_gap(zz)[rows] > 2 * bb.max(1)[rows]).all()
    for r in c["tie_rows"]:
        assert z[r].tobytes() == c["bias"].astype(np.float64).tobytes() and np.sum(z[r] == z[r].max()) == 2


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def test_node_loss_argument_errors_need_no_gpu(L):
    one = ctypes.c_void_p(256)                     # never dereferenced: every error is returned before a launch

    def call(n=40, prefix=40, P=8, C=2, H=one, W=one, bias=one, target=one, mask=one, p=0.5, loss=one, counts=one, logits=one,
             gh=one, gw=one, gb=one, ws=one, wsb=1 << 26):
        return L.lib.sgx_node_loss(n, prefix, P, C, H, W, bias, target, mask, p, 1, 0, None, 1.0, loss, counts, logits, gh, gw, gb,
                                   ws, wsb, None)

    assert call(n=0) == -2 and call(P=0) == -2 and call(C=0) == -2 and call(prefix=-1) == -2
    for name in ("H", "W", "target", "loss"):
        assert call(**{name: None}) == -1, name
    for part in ({"gh": None}, {"gw": None}, {"gb": None}, {"gh": None, "gw": None}, {"gw": None, "gb": None}, {"gh": None, "gb": None}):
        assert call(**part) == -1, part
    assert call(bias=None, gh=None, gw=None) == -1                       # a bias gradient alone
    assert call(p=1.0) == -3 and call(p=-0.1) == -3 and call(p=float("nan")) == -3
    assert call(P=1025, C=1) == -3 and call(C=65, P=1) == -3 and call(P=257, C=64) == -3
    assert L.lib.sgx_node_loss_workspace_bytes(40, 257, 64) == 0 and L.lib.sgx_node_loss_workspace_bytes(0, 8, 2) == 0
    assert L.lib.sgx_node_loss_workspace_bytes(40, 1025, 1) == 0 and L.lib.sgx_node_loss_workspace_bytes(40, 1, 65) == 0
    need = L.lib.sgx_node_loss_workspace_bytes(40, 8, 2)
    assert need >= 2048 + 3 * (2 * 8 + 2 + 2) * 4 and need % 256 == 0
    big = L.lib.sgx_node_loss_workspace_bytes(10 ** 6, 256, 64)
    assert big == 2048 + L.SGX_NODE_LOSS_GRID * (16384 + 64 + 2) * 4
    assert L.lib.sgx_node_loss_workspace_bytes(L.SGX_NODE_LOSS_ROWS * 3 + 1, 8, 2) == 2048 + -(-4 * (16 + 2 + 2) * 4 // 256) * 256
    assert call(ws=None) == -4 and call(wsb=need - 1) == -4
    assert call(ws=ctypes.c_void_p(264)) == -7
    import re
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sgx.h")).read()
    assert int(re.search(r"#define\s+SGX_NODE_LOSS_ROWS\s+(\d+)", header).group(1)) == L.SGX_NODE_LOSS_ROWS == R.ROWS
    assert int(re.search(r"#define\s+SGX_NODE_LOSS_GRID\s+(\d+)", header).group(1)) == L.SGX_NODE_LOSS_GRID == R.GRID

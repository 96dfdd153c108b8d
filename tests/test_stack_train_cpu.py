"""sgx_stack_backward without a GPU: symbols, struct layout, the plan kinds, argument errors, and the float64
restatement the GPU tests compare against (tests/_stack_grad_ref.py) checked against torch.autograd on the model it
restates."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

NEW = ["sgx_batch_plan_create_ex", "sgx_stack_backward_workspace_bytes", "sgx_stack_backward"]


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def test_new_symbols_are_exported_and_the_version_stays(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    for name in NEW:
        assert name in L.SYMBOLS
        assert f" T {name}\n" in out, name
    assert L.lib.sgx_version() == 110
    assert (L.SGX_BATCH_FORWARD, L.SGX_BATCH_BACKWARD) == (0, 1)


def test_grad_structs_match_the_header(L, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "sgx.h"\nint main(void){\n'
        ' printf("sizeof_layer %zu\\n", sizeof(sgx_stack_grad_layer));\n'
        ' printf("sizeof_desc %zu\\n", sizeof(sgx_stack_grad_desc));\n'
        + "".join(f' printf("l.{n} %zu\\n", offsetof(sgx_stack_grad_layer, {n}));\n' for n, _ in L.StackGradLayer._fields_)
        + "".join(f' printf("d.{n} %zu\\n", offsetof(sgx_stack_grad_desc, {n}));\n' for n, _ in L.StackGradDesc._fields_)
        + " return (SGX_BATCH_FORWARD == 0 && SGX_BATCH_BACKWARD == 1) ? 0 : 1;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = 0
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if not ln:
            continue
        name, val = ln.split()
        seen += 1
        if name == "sizeof_layer":
            assert ctypes.sizeof(L.StackGradLayer) == int(val)
        elif name == "sizeof_desc":
            assert ctypes.sizeof(L.StackGradDesc) == int(val)
        elif name.startswith("l."):
            assert getattr(L.StackGradLayer, name[2:]).offset == int(val), name
        else:
            assert getattr(L.StackGradDesc, name[2:]).offset == int(val), name
    assert seen == 2 + len(L.StackGradLayer._fields_) + len(L.StackGradDesc._fields_)


def _empty_plan(L, kind, width=64, dtype=0):
    h = ctypes.c_void_p()
    assert L.lib.sgx_batch_plan_create_ex(dtype, 0, 0, None, None, None, width, kind, ctypes.byref(h), None) == 0 and h.value
    return h


def test_plan_kinds_need_no_gpu(L):
    lib = L.lib
    h = ctypes.c_void_p()
    assert lib.sgx_batch_plan_create_ex(0, 0, 0, None, None, None, 64, 2, ctypes.byref(h), None) == -3     # no such kind
    assert lib.sgx_batch_plan_create_ex(0, 0, 0, None, None, None, 64, 0, None, None) == -1
    assert lib.sgx_batch_plan_create_ex(0, 4, 1, None, None, None, 64, 1, ctypes.byref(h), None) == -1   # graph_ptr NULL
    f, b = _empty_plan(L, 0), _empty_plan(L, 1)
    f2 = ctypes.c_void_p()
    assert lib.sgx_batch_plan_create(0, 0, 0, None, None, None, 64, ctypes.byref(f2), None) == 0
    try:
        assert lib.sgx_batch_plan_rows(f) == lib.sgx_batch_plan_rows(f2) == 128        # the old entry point is kind 0
        # three tiles a row (dtype + two fp32) against two of dtype: fp16, 64 wide -> 65536 // (144 + 544) = 95 -> 80
        assert lib.sgx_batch_plan_rows(b) == 80
        assert lib.sgx_batch_plan_fits(b) == 1
    finally:
        for p in (f, b, f2):
            assert lib.sgx_batch_plan_destroy(p) == 0
    for width, want in ((256, 16), (128, 48), (7, 128)):
        p = _empty_plan(L, 1, width)
        try:
            assert lib.sgx_batch_plan_rows(p) == want, width
        finally:
            lib.sgx_batch_plan_destroy(p)
    p = _empty_plan(L, 1, 64, dtype=1)
    try:
        assert lib.sgx_batch_plan_rows(p) == 80                 # fp32, 64 wide: 65536 // (3 * 272) = 80
    finally:
        lib.sgx_batch_plan_destroy(p)


def _gdesc(L, n_layers=2):
    d = L.StackGradDesc()
    d.dtype, d.n_layers = 0, n_layers
    for l in range(4):
        d.layer[l].gemm_mode, d.layer[l].M_fea, d.layer[l].P_w = 1, 8, 8
        d.layer[l].W, d.layer[l].grad_W = 256, 512
    return d


def test_backward_argument_errors_need_no_gpu(L):
    lib = L.lib
    bwd = lambda d: lib.sgx_stack_backward(ctypes.byref(d), None)
    ws = lambda d: lib.sgx_stack_backward_workspace_bytes(ctypes.byref(d))
    assert lib.sgx_stack_backward(None, None) == -1                          # SGX_ERR_NULL
    assert lib.sgx_stack_backward_workspace_bytes(None) == 0
    for n in (0, 5):
        assert bwd(_gdesc(L, n)) == -2                                        # SGX_ERR_SHAPE
    d = _gdesc(L)
    assert bwd(d) == -1                                                      # no plan
    d.dtype = 7
    assert bwd(d) == -3
    b, f = _empty_plan(L, 1), _empty_plan(L, 0)
    try:
        d = _gdesc(L)
        d.plan = b
        assert ws(d) > 0 and ws(d) % 256 == 0
        assert bwd(d) == -4                                                  # no workspace
        d.workspace, d.workspace_bytes = 1 << 20, ws(d) - 4                  # too small
        assert bwd(d) == -4
        d.workspace, d.workspace_bytes = (1 << 20) + 16, ws(d)               # not 256-byte aligned
        assert bwd(d) == -7
        d.workspace = 1 << 20
        d.layer[0].W = None
        assert bwd(d) == -1 and ws(d) == 0                                   # W missing
        d.layer[0].W = 256
        d.layer[1].grad_W = None
        assert bwd(d) == -1                                                  # grad_W missing
        d.layer[1].grad_W = 512
        d.layer[1].M_fea = 9                                                 # widths do not chain
        assert bwd(d) == -2
        d.layer[1].M_fea, d.layer[1].gemm_mode = 8, 0                        # CSR input past layer 0
        assert bwd(d) == -3
        d.layer[1].gemm_mode, d.layer[1].ldd = 1, 4                          # ldd < P_w
        assert bwd(d) == -2
        d.layer[1].ldd = 0
        d.n_graphs = 1                                                       # graph count not the plan's
        assert bwd(d) == -2
        d.n_graphs = 0
        d.plan = f                                                           # a forward plan
        assert bwd(d) == -3 and ws(d) == 0
        d.plan = b
        d.layer[1].P_w, d.layer[2].M_fea = 65, 65                            # wider than the plan
        assert bwd(d) == -3 and ws(d) == 0
        d.layer[1].P_w = 8
        d.dtype = 1                                                          # the plan's dtype is fp16
        assert bwd(d) == -3
    finally:
        for p in (b, f):
            assert lib.sgx_batch_plan_destroy(p) == 0


# ---- the float64 restatement against torch.autograd -----------------------------------------------------------------
def _mutag_cpu():
    from sgracex1_amd import pyg_lite as G
    raw = np.load(os.path.join(GOLD, "mutag_raw.npz"))
    graphs = G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])
    return G.collate(graphs)


def _autograd(adj_dense, x, weights, relus, ptr, grad_pooled):
    """The dense float64 model: D_l = act(A X_l W_l), pooled = per-graph means; dW by torch.autograd of
    sum(pooled * grad_pooled).  A is symmetric here, so autograd's A^T g is the model's A g."""
    A = torch.tensor(adj_dense)
    X = torch.tensor(x)
    Ws = [torch.tensor(np.asarray(W, np.float64), requires_grad=True) for W in weights]
    for W, relu in zip(Ws, relus):
        X = A @ (X @ W)
        if relu:
            X = torch.relu(X)
    pooled = torch.stack([X[a:b].mean(0) if b > a else torch.zeros(X.shape[1], dtype=X.dtype)
                          for a, b in zip(ptr[:-1], ptr[1:])])
    (pooled * torch.tensor(grad_pooled)).sum().backward()
    return [W.grad.numpy() for W in Ws]


def _csr_of(dense):
    sp = torch.tensor(dense).to_sparse_csr()
    return sp.crow_indices().numpy(), sp.col_indices().numpy(), sp.values().numpy()


def test_f64_restatement_is_autograd_on_mutag():
    from _stack_grad_ref import stack_grad_f64
    from sgracex1_amd.pyg_lite import to_dense_adj
    b = _mutag_cpu()
    A = to_dense_adj(b.edge_index, b.num_nodes)[0].double().numpy()
    assert (A == A.T).all()
    ptr = np.concatenate([[0], np.cumsum(np.bincount(b.batch.numpy()))])
    rng = np.random.default_rng(5)
    ws = [rng.standard_normal((7, 64)) * 0.4, rng.standard_normal((64, 64)) * 0.15]
    gp = rng.standard_normal((188, 64))
    for relus in ((True, False), (True, True)):
        want = _autograd(A, b.x.double().numpy(), ws, relus, ptr, gp)
        got, _ = stack_grad_f64(_csr_of(A), b.x.double().numpy(), ws, relus, ptr, gp)
        for g, w in zip(got, want):
            np.testing.assert_allclose(g, w, rtol=1e-11, atol=1e-11)


def _sym_batch(rng, sizes):
    N = int(sum(sizes))
    A = np.zeros((N, N))
    off = 0
    for g, n in enumerate(sizes):
        if n and g % 3:
            m = np.triu(rng.random((n, n)) < 0.35)
            v = rng.uniform(-1, 1, (n, n)) * m
            A[off:off + n, off:off + n] = v + np.triu(v, 1).T
        off += n
    return A, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@pytest.mark.parametrize("seed", range(4))
def test_f64_restatement_is_autograd_on_random_batches(seed):
    """Symmetric blocks (the model multiplies by A where autograd takes A^T), empty graphs, isolated rows, 1 to 4
    layers, ReLU on the last layer too."""
    from _stack_grad_ref import stack_grad_f64
    rng = np.random.default_rng(seed)
    sizes = [int(s) for s in rng.integers(0, 12, 15)] + [0, 3]
    A, ptr = _sym_batch(rng, sizes)
    widths = [[5, 9], [7, 16, 3], [4, 6, 6, 8], [3, 5, 7, 2, 4]][seed]
    relus = [bool(r) for r in rng.integers(0, 2, len(widths) - 1)]
    relus[-1] = seed % 2 == 0
    x = rng.standard_normal((A.shape[0], widths[0]))
    ws = [rng.standard_normal((m, p)) for m, p in zip(widths[:-1], widths[1:])]
    gp = rng.standard_normal((len(sizes), widths[-1]))
    want = _autograd(A, x, ws, relus, ptr, gp)
    got, Gs = stack_grad_f64(_csr_of(A), x, ws, relus, ptr, gp)
    assert len(Gs) == len(ws)
    for g, w in zip(got, want):
        np.testing.assert_allclose(g, w, rtol=1e-10, atol=1e-10)

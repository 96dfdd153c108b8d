"""sgx_gat_stack_backward without a GPU: symbols, struct layouts, argument errors, the launch's LDS size, and the float64
restatement the GPU tests compare against (tests/_gat_stack_grad_ref.py) checked against torch.autograd through the
model's dense emulation (config.acc = 0, FPYNQ_GAT's own backward included) and against _stack_grad_ref."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

NEW = ["sgx_gat_stack_backward_workspace_bytes", "sgx_gat_stack_backward_lds_bytes", "sgx_gat_stack_backward"]


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


def test_gat_grad_structs_match_the_header(L, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "sgx.h"\nint main(void){\n'
        ' printf("sizeof_layer %zu\\n", sizeof(sgx_gat_stack_grad_layer));\n'
        ' printf("sizeof_desc %zu\\n", sizeof(sgx_gat_stack_grad_desc));\n'
        + "".join(f' printf("l.{n} %zu\\n", offsetof(sgx_gat_stack_grad_layer, {n}));\n' for n, _ in L.GatStackGradLayer._fields_)
        + "".join(f' printf("d.{n} %zu\\n", offsetof(sgx_gat_stack_grad_desc, {n}));\n' for n, _ in L.GatStackGradDesc._fields_)
        + " return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = 0
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if not ln:
            continue
        name, val = ln.split()
        seen += 1
        if name == "sizeof_layer":
            assert ctypes.sizeof(L.GatStackGradLayer) == int(val)
        elif name == "sizeof_desc":
            assert ctypes.sizeof(L.GatStackGradDesc) == int(val)
        elif name.startswith("l."):
            assert getattr(L.GatStackGradLayer, name[2:]).offset == int(val), name
        else:
            assert getattr(L.GatStackGradDesc, name[2:]).offset == int(val), name
    assert seen == 2 + len(L.GatStackGradLayer._fields_) + len(L.GatStackGradDesc._fields_)
    # the fields of sgx_stack_grad_layer / _desc come first, in their order
    assert [n for n, _ in L.GatStackGradLayer._fields_][:len(L.StackGradLayer._fields_)] == [n for n, _ in L.StackGradLayer._fields_]
    assert [n for n, _ in L.GatStackGradDesc._fields_] == [n for n, _ in L.StackGradDesc._fields_]


def _empty_plan(L, kind, width=64, dtype=0):
    h = ctypes.c_void_p()
    assert L.lib.sgx_batch_plan_create_ex(dtype, 0, 0, None, None, None, width, kind, ctypes.byref(h), None) == 0 and h.value
    return h


def _gdesc(L, n_layers=2, gat=(1, 1, 1, 1), dtype=0, width=8):
    d = L.GatStackGradDesc()
    d.dtype, d.n_layers = dtype, n_layers
    for l in range(4):
        d.layer[l].gemm_mode, d.layer[l].M_fea, d.layer[l].P_w = 1, width, width
        d.layer[l].W, d.layer[l].grad_W = 256, 512
        d.layer[l].gat_mode, d.layer[l].attention, d.layer[l].grad_attention, d.layer[l].alpha = gat[l], 768, 1024, 0.2
    return d


def test_backward_argument_errors_need_no_gpu(L):
    lib = L.lib
    bwd = lambda d: lib.sgx_gat_stack_backward(ctypes.byref(d), None)
    ws = lambda d: lib.sgx_gat_stack_backward_workspace_bytes(ctypes.byref(d))
    assert lib.sgx_gat_stack_backward(None, None) == -1                      # SGX_ERR_NULL
    assert lib.sgx_gat_stack_backward_workspace_bytes(None) == 0
    assert lib.sgx_gat_stack_backward_lds_bytes(None) == 0
    for n in (0, 5):
        assert bwd(_gdesc(L, n)) == -2                                        # SGX_ERR_SHAPE
    d = _gdesc(L)
    assert bwd(d) == -1                                                      # no plan
    d.dtype = 7
    assert bwd(d) == -3
    b, f = _empty_plan(L, 1), _empty_plan(L, 0)
    try:
        # those of sgx_stack_backward
        d = _gdesc(L)
        d.plan = b
        assert ws(d) > 0 and ws(d) % 256 == 0
        assert ws(d) == 256 * -(-4 * (2 * 64 + 2 * 16) // 256)               # one slice: two 8 x 8 blocks, two of 2 x 8
        g = _gdesc(L, gat=(0, 1, 0, 0))
        g.plan = b
        assert ws(g) == 256 * -(-4 * (2 * 64 + 16) // 256)
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
        # the GAT layers' own
        d.layer[1].attention = None
        assert bwd(d) == -1 and ws(d) == 0                                   # attention missing on a GAT layer
        d.layer[1].attention = 768
        d.layer[0].grad_attention = None
        assert bwd(d) == -1 and ws(d) == 0                                   # grad_attention missing
        d.layer[0].gat_mode = 0                                              # ... which a GCN layer does not need
        assert ws(d) > 0
        d.layer[0].gat_mode, d.layer[0].grad_attention = 1, 1024
        for mode in (2, -1):
            d.layer[1].gat_mode = mode
            assert bwd(d) == -3 and ws(d) == 0                               # no such gat_mode
        d.layer[1].gat_mode = 1
        d.layer[3].gat_mode = 5                                              # (a layer past n_layers is not read)
        assert ws(d) > 0
        d.plan = f                                                           # a forward-kind plan
        assert bwd(d) == -3 and ws(d) == 0 and lib.sgx_gat_stack_backward_lds_bytes(ctypes.byref(d)) == 0
        d.plan = b
        d.layer[1].P_w, d.layer[2].M_fea = 65, 65                            # wider than the plan
        assert bwd(d) == -3 and ws(d) == 0
        d.layer[1].P_w = 8
        d.dtype = 1                                                          # the plan's dtype is fp16
        assert bwd(d) == -3
    finally:
        for p in (b, f):
            assert lib.sgx_batch_plan_destroy(p) == 0


def _pitch(es, width):
    per16 = 16 // es
    return (width + per16 - 1) // per16 * per16 + per16


def lds_bytes(es, width):
    """The launch's dynamic LDS as include/sgx.h states it: R x (grad_row_bytes + 4 lds_pitch(fp32, width) + 24), R the
    backward plan's row budget."""
    grad_row = _pitch(es, width) * es + 2 * _pitch(4, width) * 4
    rows = min(65536 // grad_row // 16 * 16, 128)
    return rows, rows * (grad_row + 4 * _pitch(4, width) + 24)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("width", [1, 7, 64, 65, 252, 256])
def test_lds_size_is_computed_on_the_host(L, dtype, width):
    lib = L.lib
    p = _empty_plan(L, 1, width, dtype)
    try:
        d = _gdesc(L, dtype=dtype, width=width)
        d.plan = p
        rows, want = lds_bytes(2 if dtype == 0 else 4, width)
        assert lib.sgx_batch_plan_rows(p) == rows
        got = lib.sgx_gat_stack_backward_lds_bytes(ctypes.byref(d))
        assert got == want, (got, want)
        assert got <= 160 * 1024
        assert got < 100 * 1024                                              # (what include/sgx.h says of every width)
    finally:
        lib.sgx_batch_plan_destroy(p)
    assert lds_bytes(2, 64) == (80, 78720) and lds_bytes(4, 256) == (16, 66944)


# ---- the float64 restatement ---------------------------------------------------------------------------------------------
def _mutag12():
    from sgracex1_amd import pyg_lite as G
    raw = np.load(os.path.join(GOLD, "mutag_raw.npz"))
    graphs = G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])
    return G.collate(graphs[:12])


@pytest.mark.parametrize("gat", [1, 0])
def test_restatement_is_autograd_through_the_dense_emulation(gat):
    """GAT_POOL_PYNQ with config.acc = 0 on a 12-graph MUTAG batch: torch.autograd through FPYNQ_GAT's dense emulation
    (its custom backward: P and not P^T) and RPYNQ.  The twin's forward casts its input to fp32, so the comparison runs
    at fp32 rounding: the restatement's own tolerance with unit = 2^-24, on the twin's own layer outputs."""
    from _gat_stack_grad_ref import gat_stack_grad_f64, within
    from sgracex1_amd import config, sgrace
    saved = (config.acc, config.compute_attention, config.fake_quantization, config.hardware_quantize)
    config.acc, config.compute_attention, config.fake_quantization, config.hardware_quantize = 0, gat, 0, 0
    try:
        b = _mutag12()
        torch.manual_seed(3)
        model = sgrace.GAT_POOL_PYNQ(7, 16, 2)
        model.eval()                                                        # (dropout off; gradients on)
        kept = {}
        model.reluh.register_forward_hook(lambda m, i, o: kept.__setitem__("D0", o.detach()))
        model.att2.register_forward_hook(lambda m, i, o: kept.__setitem__("D1", o.detach()))
        out = model(b.x, b.edge_index, b.batch)
        out.sum().backward()
        n_graphs = int(b.batch.max()) + 1
        gp = np.ones((n_graphs, 2)) @ model.lin.weight.detach().double().numpy()      # d sum(lin(pooled)) / d pooled
        ei, norm = sgrace.sym_norm2(b.edge_index, b.x.size(0))
        N = b.x.size(0)
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(ei[0].numpy(), minlength=N))])
        adj = (rowptr, ei[1].numpy(), norm.double().numpy())
        ptr = np.concatenate([[0], np.cumsum(np.bincount(b.batch.numpy()))])
        layers = (model.att1, model.att2)
        ws = [c.weight.detach().double().numpy() for c in layers]
        atts = [c.attention.detach().double().numpy().reshape(-1) if gat else None for c in layers]
        r = gat_stack_grad_f64(adj, b.x.double().numpy(), ws, atts, [True, False], ptr, gp,
                               [kept["D0"].double().numpy(), kept["D1"].double().numpy()], alpha=model.att1.alpha)
        for l, c in enumerate(layers):
            ok, ratio = within(c.weight.grad.double().numpy(), r["dW"][l], r["mW"][l], r["tW"][l])
            assert ok, (l, "dW", ratio)
            if gat:
                ok, ratio = within(c.attention.grad.double().numpy().reshape(-1), r["dA"][l], r["mA"][l], r["tA"][l])
                assert ok, (l, "dA", ratio)
                # (the bound separates: no gradient at all lies outside it on layer 0; layer 1's attention gradient
                # is a sum that nearly cancels, its g being constant within a graph)
                assert l > 0 or (np.abs(r["dA"][l]) > r["tA"][l] * r["mA"][l] + 1e-30).any()
                assert np.abs(r["dA"][l]).max() > 0
            else:
                assert not c.attention.grad.any()
    finally:
        config.acc, config.compute_attention, config.fake_quantization, config.hardware_quantize = saved


@pytest.mark.parametrize("seed", range(3))
def test_all_gcn_restatement_is_stack_grad_f64(seed):
    from _gat_stack_grad_ref import gat_stack_grad_f64
    from _stack_grad_ref import stack_grad_f64
    rng = np.random.default_rng(seed)
    sizes = [int(s) for s in rng.integers(0, 9, 10)] + [0, 3]
    N = sum(sizes)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows, cols = [], []
    for a, b in zip(ptr[:-1], ptr[1:]):
        m = rng.random((b - a, b - a)) < 0.4
        r, c = np.nonzero(m)
        rows.append(r + a)
        cols.append(c + a)
    r, c = np.concatenate(rows), np.concatenate(cols)
    adj = (np.concatenate([[0], np.cumsum(np.bincount(r, minlength=N))]), c, rng.uniform(-1, 1, len(r)))
    widths = [[5, 9], [7, 16, 3], [4, 6, 6, 8]][seed]
    relus = [bool(v) for v in rng.integers(0, 2, len(widths) - 1)]
    x = rng.standard_normal((N, widths[0]))
    ws = [rng.standard_normal((m, p)) for m, p in zip(widths[:-1], widths[1:])]
    gp = rng.standard_normal((len(sizes), widths[-1]))
    outs = []
    X = x
    from _stack_ref import csr_matmul
    for W, relu in zip(ws, relus):
        X = csr_matmul(*adj, X @ W)
        X = np.maximum(X, 0) if relu else X
        outs.append(X)
    want_W, want_G = stack_grad_f64(adj, x, ws, relus, ptr, gp, outs=outs)
    got = gat_stack_grad_f64(adj, x, ws, [None] * len(ws), relus, ptr, gp, outs)
    for l in range(len(ws)):
        assert np.array_equal(got["dW"][l], want_W[l]) and np.array_equal(got["G"][l], want_G[l])
        assert got["dA"][l] is None


def test_rows_without_a_live_entry_contribute_nothing():
    """The zero rule of the restatement: a batch whose every stored value is masked gives S = 0, G = 0 and no gradient."""
    from _gat_stack_grad_ref import gat_stack_grad_f64
    rng = np.random.default_rng(0)
    adj = (np.array([0, 2, 3, 3, 5]), np.array([0, 1, 1, 2, 3]), np.array([-1.0, 0.0, -0.0, -0.5, -2.0]))
    x = rng.standard_normal((4, 3))
    r = gat_stack_grad_f64(adj, x, [rng.standard_normal((3, 5))], [rng.standard_normal(10)], [False], np.array([0, 4]),
                           rng.standard_normal((1, 5)), [None])
    assert r["dead"][0].all() and not r["S"][0].any() and not r["G"][0].any()
    assert not r["dW"][0].any() and not r["dA"][0].any()

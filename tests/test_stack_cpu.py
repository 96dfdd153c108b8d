"""sgx_stack_forward without a GPU: symbols, struct layout, argument errors, and the float64 restatement the GPU tests
compare against (tests/_stack_ref.py) checked against the model it restates."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sgx.h")
GOLD = os.path.join(ROOT, "tests", "golden")

NEW = ["sgx_batch_plan_create", "sgx_batch_plan_destroy", "sgx_batch_plan_rows", "sgx_batch_plan_groups",
       "sgx_batch_plan_max_graph", "sgx_batch_plan_fits", "sgx_stack_workspace_bytes", "sgx_stack_forward"]


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def test_new_symbols_are_exported(L):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    for name in NEW:
        assert name in L.SYMBOLS
        assert f" T {name}\n" in out, name
    assert L.lib.sgx_version() == 110


def test_stack_structs_match_the_header(L, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "sgx.h"\nint main(void){\n'
        ' printf("sizeof_layer %zu\\n", sizeof(sgx_stack_layer));\n'
        ' printf("sizeof_desc %zu\\n", sizeof(sgx_stack_desc));\n'
        + "".join(f' printf("l.{n} %zu\\n", offsetof(sgx_stack_layer, {n}));\n' for n, _ in L.StackLayer._fields_)
        + "".join(f' printf("d.{n} %zu\\n", offsetof(sgx_stack_desc, {n}));\n' for n, _ in L.StackDesc._fields_)
        + " return SGX_ERR_BLOCKS == -9 ? 0 : 1;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if not ln:
            continue
        name, val = ln.split()
        if name == "sizeof_layer":
            assert ctypes.sizeof(L.StackLayer) == int(val)
        elif name == "sizeof_desc":
            assert ctypes.sizeof(L.StackDesc) == int(val)
        elif name.startswith("l."):
            assert getattr(L.StackLayer, name[2:]).offset == int(val), name
        else:
            assert getattr(L.StackDesc, name[2:]).offset == int(val), name


def test_status_string_blocks(L):
    assert L.SGX_ERR_BLOCKS == -9
    assert L.status_string(-9) != "unknown status"
    assert "block" in L.status_string(-9)


def _desc(L, n_layers=2):
    d = L.StackDesc()
    d.dtype, d.n_layers = 0, n_layers
    for l in range(4):
        d.layer[l].gemm_mode, d.layer[l].M_fea, d.layer[l].P_w = 1, 8, 8
    return d


def test_argument_errors_need_no_gpu(L):
    lib = L.lib
    fwd = lambda d: lib.sgx_stack_forward(ctypes.byref(d), None)
    assert lib.sgx_stack_forward(None, None) == -1                          # SGX_ERR_NULL
    assert lib.sgx_stack_workspace_bytes(None) == 0
    for n in (0, 5):
        assert fwd(_desc(L, n)) == -2                                         # SGX_ERR_SHAPE
    d = _desc(L)
    assert fwd(d) == -1                                                      # no plan
    d.dtype = 7
    assert fwd(d) == -3
    # plan arguments
    h = ctypes.c_void_p()
    assert lib.sgx_batch_plan_create(0, 4, 1, None, None, None, 64, None, None) == -1
    assert lib.sgx_batch_plan_create(0, -1, 1, None, None, None, 64, ctypes.byref(h), None) == -2
    assert lib.sgx_batch_plan_create(0, 4, 1, None, None, None, 0, ctypes.byref(h), None) == -2
    assert lib.sgx_batch_plan_create(0, 4, 1, None, None, None, 64, ctypes.byref(h), None) == -1   # graph_ptr NULL
    assert lib.sgx_batch_plan_create(5, 0, 0, None, None, None, 64, ctypes.byref(h), None) == -3
    for getter in ("sgx_batch_plan_rows", "sgx_batch_plan_groups", "sgx_batch_plan_max_graph", "sgx_batch_plan_fits"):
        assert getattr(lib, getter)(None) == -1
    # the plan of an empty batch is made without touching the device
    assert lib.sgx_batch_plan_create(0, 0, 0, None, None, None, 64, ctypes.byref(h), None) == 0 and h.value
    try:
        assert lib.sgx_batch_plan_rows(h) == 128 and lib.sgx_batch_plan_fits(h) == 1
        d = _desc(L)
        d.plan = h
        d.n_graphs = 1                                                       # graph_ptr count not the plan's
        assert fwd(d) == -2
        d.n_graphs, d.n_rows = 0, 5                                          # row count not the plan's
        assert fwd(d) == -2
        d.n_rows = 0
        assert fwd(d) == -1                                                  # B missing
        for l in range(2):
            d.layer[l].B = 256
        assert fwd(d) == 0 and lib.sgx_stack_workspace_bytes(ctypes.byref(d)) == 0   # nothing to do
        d.layer[1].M_fea = 9                                                 # widths do not chain
        assert fwd(d) == -2
        d.layer[1].M_fea, d.layer[1].gemm_mode = 8, 0                        # CSR input past layer 0
        assert fwd(d) == -3
        d.layer[1].gemm_mode, d.C = 1, 2                                     # head without weights
        assert fwd(d) == -1
    finally:
        assert lib.sgx_batch_plan_destroy(h) == 0


def _mutag_cpu():
    from sgracex1_amd import pyg_lite as G
    raw = np.load(os.path.join(GOLD, "mutag_raw.npz"))
    graphs = G.load_tu_raw(raw["A"], raw["graph_indicator"], raw["graph_labels"], raw["node_labels"])
    return G.collate(graphs)


def test_f64_restatement_is_the_model_on_mutag():
    """stack_f64 equals GraphConvolution -> relu -> GraphConvolution -> global_mean_pool -> Linear (MOL cells 15, 18)
    run in float64 torch on all 188 MUTAG graphs."""
    from _stack_ref import stack_f64
    from sgracex1_amd import molecule_gcn as M
    from sgracex1_amd.pyg_lite import global_mean_pool, to_dense_adj
    b = _mutag_cpu()
    torch.manual_seed(3)
    c1, c2 = M.GraphConvolution(7, 64).double(), M.GraphConvolution(64, 64).double()
    lin = torch.nn.Linear(64, 2).double()
    adj = to_dense_adj(b.edge_index, b.num_nodes)[0].double()
    x = b.x.double()
    with torch.no_grad():
        want = lin(global_mean_pool(c2(torch.relu(c1(x, adj)), adj), b.batch))
    sp = adj.to_sparse_csr()
    ptr = np.concatenate([[0], np.cumsum(np.bincount(b.batch.numpy()))])
    outs, pooled, logits = stack_f64((sp.crow_indices().numpy(), sp.col_indices().numpy(), sp.values().numpy()), x.numpy(),
                                     [c1.weight.detach().numpy(), c2.weight.detach().numpy()], [True, False], ptr,
                                     lin.weight.detach().numpy(), lin.bias.detach().numpy())
    assert logits.shape == (188, 2) and len(outs) == 2
    np.testing.assert_allclose(logits, want.numpy(), rtol=1e-12, atol=1e-12)

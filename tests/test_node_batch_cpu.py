"""Layer-ready node batches without a GPU: the numpy restatement of the two rules (tests/_node_batch_ref.py) against
sgrace.sym_norm2 + CSR packing in torch and against dense-to-CSR of gathered rows, its values against float64; the new
symbols, the struct layout and the argument errors of sgx_node_batch_sample."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _node_batch_ref as NB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 1 / sqrt(deg) carries at most 2^-23 (two roundings of 2^-24), twice; the two products add 2^-24 each: under 2^-21.
# deg itself is exact in every case below: unit weights or multiples of 1/8, an integer fill.
REL = 2.0 ** -21


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def _case(seed=0, n=40, long_row=True):
    """A CSR over n local nodes with stored loops, repeated edges, empty rows and (long_row) a row of over 64 entries."""
    rng = np.random.default_rng(seed)
    rows = [list(rng.integers(0, n, rng.integers(0, 12))) for _ in range(n)]
    rows[0] = [0, 3, 3, 0, 5]                 # stored loops (twice), a repeated edge
    rows[1] = []                              # empty rows
    rows[2] = []
    rows[3] = [7, 7, 7, 2]                    # repeated edges, no loop; column 2 is a row that fill = 0 leaves dead
    rows[4] = [4]                             # nothing but its loop
    if long_row:
        rows[5] = list(rng.integers(0, n, 150))             # more than 64 entries, many repeats
        rows[6] = [c for c in rng.integers(0, n, 90) if c != 6]   # more than 64 entries, loop missing
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.asarray([c for r in rows for c in r], np.int64)
    return rowptr, col


def _torch_path(rowptr, col, weights, fill):
    """Today's host path on the CPU: sgrace.sym_norm2 on the edge list (row 0 = aggregating node), then CSR packing."""
    from sgracex1_amd import sgrace
    n = len(rowptr) - 1
    target = np.repeat(np.arange(n), np.diff(rowptr))
    ei = torch.as_tensor(np.stack([target, col]))
    w = None if weights is None else torch.as_tensor(weights)
    ei, norm = sgrace.sym_norm2(ei, n, edge_weight=w, fill=fill, dtype=torch.float32)
    out_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(ei[0].numpy(), minlength=n), out=out_ptr[1:])
    assert bool((ei[0][1:] >= ei[0][:-1]).all())
    return out_ptr, ei[1].numpy(), norm.numpy()


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("fill", [0, 1, 3])
def test_restated_sym_norm2_against_torch_and_float64(L, fill, weighted):
    rowptr, col = _case(seed=fill)
    rng = np.random.default_rng(7)
    weights = (rng.integers(1, 17, len(col)) / 8).astype(np.float32) if weighted else None
    out_ptr, out_col, val, dead, has_dead, max_row = NB.sym_norm2_csr(rowptr, col, weights, fill)
    t_ptr, t_col, t_val = _torch_path(rowptr, col, weights, fill)
    assert np.array_equal(out_ptr, t_ptr) and np.array_equal(out_col, t_col)          # structure: exact
    exact = NB.sym_norm2_f64(rowptr, col, weights, fill)
    assert val.dtype == np.float32 and len(val) == len(exact)
    err = np.abs(val.astype(np.float64) - exact)
    assert (err <= REL * np.abs(exact)).all(), float((err / np.maximum(np.abs(exact), 1e-300)).max())
    assert (np.abs(t_val.astype(np.float64) - exact) <= 2 * REL * np.abs(exact)).all()
    # facts: the loop count, dead rows, the longest row
    n = len(rowptr) - 1
    missing = sum(1 for r in range(n) if r not in col[rowptr[r]:rowptr[r + 1]])
    assert out_ptr[-1] == len(col) + missing
    assert max_row == np.diff(out_ptr).max() and max_row > 64
    live = np.zeros(n, bool)
    live[np.repeat(np.arange(n), np.diff(out_ptr))[val > 0]] = True
    assert np.array_equal(dead, ~live) and has_dead == bool(dead.any())
    if fill == 0:
        assert dead[1] and dead[2]                           # empty rows: a loop of weight 0, deg 0
    else:
        assert not has_dead


def test_restated_order_is_stable_and_the_loop_comes_last():
    rowptr = np.asarray([0, 4, 4])
    col = np.asarray([1, 0, 1, 1])
    w = np.asarray([0.5, 2.0, 0.25, 0.125], np.float32)      # row 0 holds its loop; row 1 is empty
    out_ptr, out_col, val, dead, has_dead, max_row = NB.sym_norm2_csr(rowptr, col, w, fill=3)
    assert out_ptr.tolist() == [0, 4, 5] and out_col.tolist() == [0, 1, 1, 1, 1]
    deg0, deg1 = np.float32(2.875), np.float32(3)
    d0, d1 = np.float32(1) / np.sqrt(deg0), np.float32(1) / np.sqrt(deg1)
    want = [(d0 * np.float32(2)) * d0, (d0 * np.float32(0.5)) * d1, (d0 * np.float32(0.25)) * d1,
            (d0 * np.float32(0.125)) * d1, (d1 * np.float32(3)) * d1]
    assert val.tolist() == [float(np.float32(v)) for v in want]
    assert not has_dead and max_row == 4


def test_restated_gather_against_dense_to_csr():
    rng = np.random.default_rng(3)
    x = (rng.random((50, 30)) < 0.2) * rng.random((50, 30))
    x[7] = 0                                                  # an all-zero feature row
    x = x.astype(np.float32)
    rowptr, col, val = NB.dense_to_csr(x)
    index = np.asarray([7, 3, 49, 0, 7 + 1, 20])
    g_ptr, g_col, g_val = NB.gather_csr(rowptr, col, val, index)
    sp = torch.as_tensor(x[index]).to_sparse_csr()
    assert np.array_equal(g_ptr, sp.crow_indices().numpy()) and np.array_equal(g_col, sp.col_indices().numpy())
    assert np.array_equal(g_val.view(np.int32), sp.values().numpy().view(np.int32))
    assert g_ptr[1] == 0                                      # the zero row is an empty row
    h_ptr, h_col, h_val = NB.gather_csr(rowptr, col, val, index, store=np.float16)
    assert np.array_equal(h_val.view(np.int16), sp.values().to(torch.float16).numpy().view(np.int16))


def test_new_symbols_struct_layout_and_argument_errors(L, tmp_path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    for name in ("sgx_node_batch_workspace_bytes", "sgx_node_batch_sample"):
        assert name in L.SYMBOLS and f" T {name}\n" in out, name
    assert L.lib.sgx_version() == 110
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sgx.h"\nint main(void){\n'
                   ' printf("sizeof %zu\\n", sizeof(sgx_node_batch));\n'
                   + "".join(f' printf("{n} %zu\\n", offsetof(sgx_node_batch, {n}));\n' for n, _ in L.NodeBatch._fields_)
                   + " return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = 0
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if ln:
            name, v = ln.split()
            seen += 1
            if name == "sizeof":
                assert ctypes.sizeof(L.NodeBatch) == int(v)
            else:
                assert getattr(L.NodeBatch, name).offset == int(v), name
    assert seen == 1 + len(L.NodeBatch._fields_)
    # the workspace query: the sampler's bounds, more bytes; bad arguments give 0
    fan = (ctypes.c_int32 * 2)(10, 10)
    mn, me, mn2, me2 = (ctypes.c_int64(0) for _ in range(4))
    a = L.lib.sgx_sample_workspace_bytes(3000, 50000, 128, 2, fan, ctypes.byref(mn), ctypes.byref(me))
    b = L.lib.sgx_node_batch_workspace_bytes(3000, 50000, 128, 2, fan, ctypes.byref(mn2), ctypes.byref(me2))
    assert b > a > 0 and (mn.value, me.value) == (mn2.value, me2.value) and b % 256 == 0
    assert L.lib.sgx_node_batch_workspace_bytes(3000, 50000, 4000, 2, fan, None, None) == 0
    # argument errors come back before anything reaches a device
    assert L.lib.sgx_node_batch_sample(None, None) == -1
    d = L.NodeBatch()
    assert L.lib.sgx_node_batch_sample(ctypes.byref(d), None) == -1            # no fan-outs
    hn, he = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 3)()
    d.fanouts, d.hop_nodes, d.hop_edges = fan, hn, he
    d.n_nodes, d.nnz, d.batch, d.n_hops, d.dtype = 3000, 50000, 128, 2, 1
    assert L.lib.sgx_node_batch_sample(ctypes.byref(d), None) == -2            # capacities below the bounds
    d.max_nodes, d.max_edges = mn.value, me.value
    assert L.lib.sgx_node_batch_sample(ctypes.byref(d), None) == -1            # buffers missing
    d.dtype = 5
    assert L.lib.sgx_node_batch_sample(ctypes.byref(d), None) == -3            # SGX_ERR_UNSUPPORTED
    d.dtype = 1
    for name, _ in L.NodeBatch._fields_:
        if name in ("rowPtr", "columnIndex", "seeds", "node_map", "n_id", "out_rowPtr", "out_col", "edge_pos", "rowPtr_norm",
                    "columnIndex_norm", "values_norm", "dead_row"):
            setattr(d, name, 256)
    assert L.lib.sgx_node_batch_sample(ctypes.byref(d), None) == -4            # SGX_ERR_WORKSPACE
    d.rowPtr_x = 256
    assert L.lib.sgx_node_batch_sample(ctypes.byref(d), None) == -1            # a feature source without its outputs

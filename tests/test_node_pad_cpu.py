"""Padded node batches without a GPU: the capacity arithmetic of sgx_node_batch_pad_capacity against the numpy restatement
(tests/_node_pad_ref.py), the "every batch fits" inequalities at their extremes, the dealing rule of the spare entries,
the new symbols' struct layout and argument errors, and the ValueErrors of NeighborLoader(pad=True) that need no device."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

import _node_pad_ref as NP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NULL, SHAPE, UNSUPPORTED = 0, -1, -2, -3


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def _capacity(L, n_nodes, nnz, batch, fanouts, rows):
    fan = (ctypes.c_int32 * len(fanouts))(*fanouts)
    p = L.NodeBatchPad()
    r = None if rows is None else np.ascontiguousarray(rows, np.int32)
    st = L.lib.sgx_node_batch_pad_capacity(n_nodes, nnz, batch, len(fanouts), fan,
                                           None if r is None else r.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(p))
    return st, p


SWEEP = [(n, b, f, k) for n, b, f, k in itertools.product((1, 7, 40, 300, 5000), (1, 8, 32), ([3, 2], [5, 5], [0, 4], [63], [1, 1, 1]),
                                                          ("none", "const", "skew"))
         if b <= n]


def test_capacity_against_the_restatement_over_a_sweep(L):
    rng = np.random.default_rng(0)
    for n, batch, fan, kind in SWEEP:
        nnz = int(min(n * 6, n * n))
        rows = None if kind == "none" else np.full(n, 5) if kind == "const" else rng.integers(0, 65, n) * (rng.random(n) < 0.3)
        st, p = _capacity(L, n, nnz, batch, fan, rows)
        want = NP.capacity(n, nnz, batch, fan, rows)
        assert st == OK, (n, batch, fan, kind)
        assert (p.n_rows, p.nnz_norm, p.nnz_fea, p.n_edges) == (want["N"], want["Ca"], want["Cf"], want["E"]), (n, batch, fan, kind)
        # the sampler's own bounds are the restated ones
        mn, me = ctypes.c_int64(0), ctypes.c_int64(0)
        fan_c = (ctypes.c_int32 * len(fan))(*fan)
        assert L.lib.sgx_node_batch_workspace_bytes(n, nnz, batch, len(fan), fan_c, ctypes.byref(mn), ctypes.byref(me)) > 0
        assert (mn.value, me.value) == (want["mn"], want["me"])


def test_every_batch_fits_at_the_extremes():
    """The inequalities of the header's proof over every (n, edges, a, f) a batch can have, extremes included: seeds
    without in-edges (a = n, edges = 0), every row storing its loop (a = edges), a graph so small that mn = n_nodes."""
    rng = np.random.default_rng(1)
    for n_nodes, batch, fan in ((6, 6, [3, 2]), (40, 8, [5, 5]), (300, 32, [3, 2]), (300, 8, [63]), (9, 1, [0, 4])):
        nnz = n_nodes * 5
        rows = rng.integers(0, 65, n_nodes)
        cap = NP.capacity(n_nodes, nnz, batch, fan, rows)
        if n_nodes == 6:
            assert cap["mn"] == n_nodes
        top = np.sort(rows)[::-1]
        for n in {batch, (batch + cap["mn"]) // 2, cap["mn"]}:
            for edges in {0, cap["me"] // 2, cap["me"]}:
                for a in {n, max(n, edges), edges + n}:                  # a row gets one loop unless it stores one
                    for f in {0, int(top[:n].sum())}:
                        P = cap["N"] - n
                        Sa, Sf = cap["Ca"] - a - P, cap["Cf"] - f
                        assert P >= cap["F"] and 0 <= Sa <= cap["me"] <= 63 * P and 0 <= Sf <= cap["Cf"] <= 64 * P
                        ptr_a, ptr_f = NP.deal(a, P, Sa, 63, 1), NP.deal(f, P, Sf, 64, 0)
                        assert ptr_a[-1] == cap["Ca"] and ptr_f[-1] == cap["Cf"]
                        la, lf = np.diff(ptr_a), np.diff(ptr_f)
                        assert la.min() >= 1 and la.max() <= 64 and lf.min() >= 0 and lf.max() <= 64
                        # dealt from filler row 0 on: full rows first, one partial row, then bare rows
                        assert (np.diff(la) <= 0).all() and (np.diff(lf) <= 0).all()
                        assert (la[:Sa // 63] == 64).all() and (lf[:Sf // 64] == 64).all()


def test_restated_padding_of_a_tiny_batch():
    cap = dict(N=5, Ca=70, Cf=66, E=4, mn=3, me=4, F=2)
    i32 = lambda *v: np.asarray(v, np.int32)
    out = NP.pad_batch(cap, 2, 1, i32(9, 4), i32(0, 1, 1), i32(1), i32(17), i32(0, 2, 3), i32(0, 1, 1), np.asarray([.5, .5, 1], np.float32),
                       np.zeros(2, bool), np.asarray([[1], [0]]), np.asarray([[0], [1]]), i32(0, 1, 1), i32(3), np.ones(1, np.float32),
                       np.asarray([2, 1]), [np.ones(2, bool)])
    assert out["n_id"].tolist() == [9, 4, -1, -1, -1] and out["out_rowptr"].tolist() == [0, 1, 1, 1, 1, 1]
    assert out["rowptr_norm"].tolist() == [0, 2, 3, 67, 69, 70]          # 64 spare entries: 63 to filler row 0, 1 to row 1
    assert out["col_norm"][3:67].tolist() == [2] * 64 and out["col_norm"][67:].tolist() == [3, 3, 4]
    assert out["val_norm"][3:].tolist() == [1] + [0] * 63 + [1, 0, 1]
    assert out["rowptr_fea"].tolist() == [0, 1, 1, 65, 66, 66] and not out["val_fea"][1:].any()
    assert out["edge_index"].tolist() == [[1, -1, -1, -1], [0, -1, -1, -1]] and out["out_col"].tolist() == [1, -1, -1, -1]
    assert out["y"].tolist() == [2, 1, 0, 0, 0] and out["masks"][0].tolist() == [True, True, False, False, False]


def test_new_symbols_struct_layout_and_argument_errors(L, tmp_path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    for name in ("sgx_node_batch_pad_capacity", "sgx_node_batch_sample_padded"):
        assert name in L.SYMBOLS and f" T {name}\n" in out, name
    assert L.lib.sgx_version() == 110
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sgx.h"\nint main(void){\n'
                   ' printf("sizeof %zu\\n", sizeof(sgx_node_batch_pad));\n'
                   + "".join(f' printf("{n} %zu\\n", offsetof(sgx_node_batch_pad, {n}));\n' for n, _ in L.NodeBatchPad._fields_)
                   + " return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = [ln.split() for ln in subprocess.check_output([str(exe)], text=True).split("\n") if ln]
    assert len(lines) == 1 + len(L.NodeBatchPad._fields_)
    for name, v in lines:
        assert (ctypes.sizeof(L.NodeBatchPad) if name == "sizeof" else getattr(L.NodeBatchPad, name).offset) == int(v), name
    # the capacity call
    fan = (ctypes.c_int32 * 2)(10, 10)
    p = L.NodeBatchPad()
    cap = L.lib.sgx_node_batch_pad_capacity
    assert cap(3000, 50000, 128, 2, fan, None, None) == NULL and cap(3000, 50000, 128, 2, None, None, ctypes.byref(p)) == NULL
    assert cap(3000, 50000, 4000, 2, fan, None, ctypes.byref(p)) == SHAPE           # batch > n_nodes
    assert cap(3000, 50000, 0, 2, fan, None, ctypes.byref(p)) == SHAPE
    assert cap(3000, 50000, 128, 2, (ctypes.c_int32 * 2)(10, -1), None, ctypes.byref(p)) == UNSUPPORTED
    assert cap(4, 8, 2, 2, fan, (ctypes.c_int32 * 4)(1, -1, 0, 0), ctypes.byref(p)) == SHAPE
    assert cap(3000, 50000, 128, 2, fan, None, ctypes.byref(p)) == OK
    # the padded call: argument errors come back before anything reaches a device
    call = L.lib.sgx_node_batch_sample_padded
    d = L.NodeBatch()
    assert call(None, ctypes.byref(p), None) == NULL and call(ctypes.byref(d), None, None) == NULL
    assert call(ctypes.byref(d), ctypes.byref(p), None) == NULL                     # no fan-outs
    d.fanouts = fan
    d.n_nodes, d.nnz, d.batch, d.n_hops, d.dtype = 3000, 50000, 0, 2, 1
    assert call(ctypes.byref(d), ctypes.byref(p), None) == SHAPE                    # batch == 0
    d.batch = 128
    assert call(ctypes.byref(d), ctypes.byref(p), None) == SHAPE                    # max_nodes / max_edges below the bounds
    mn, me = ctypes.c_int64(0), ctypes.c_int64(0)
    nbytes = L.lib.sgx_node_batch_workspace_bytes(3000, 50000, 128, 2, fan, ctypes.byref(mn), ctypes.byref(me))
    d.max_nodes, d.max_edges = mn.value, me.value
    assert call(ctypes.byref(d), ctypes.byref(p), None) == NULL                     # buffers missing
    for name in ("rowPtr", "columnIndex", "seeds", "node_map", "n_id", "out_rowPtr", "out_col", "edge_pos", "rowPtr_norm",
                 "columnIndex_norm", "values_norm", "dead_row"):
        setattr(d, name, 256)
    d.workspace, d.workspace_bytes = 256, nbytes - 1
    assert call(ctypes.byref(d), ctypes.byref(p), None) == -4                       # SGX_ERR_WORKSPACE
    d.workspace_bytes = nbytes
    assert call(ctypes.byref(d), ctypes.byref(p), None) == NULL                     # pad's device pointers missing
    p.step = p.status = p.counts = 256
    for field, value in (("n_rows", mn.value - 1), ("n_edges", me.value - 1), ("nnz_norm", me.value + p.n_rows - 1),
                         ("nnz_norm", p.n_rows + 63 * (p.n_rows - mn.value) + 1), ("nnz_norm", 1 << 31)):
        q = L.NodeBatchPad.from_buffer_copy(p)
        setattr(q, field, value)
        assert call(ctypes.byref(d), ctypes.byref(q), None) == SHAPE, field         # capacities below the rule's, or too large
    d.rowPtr_x = d.columnIndex_x = d.values_x = d.rowPtr_fea = d.columnIndex_fea = d.values_fea = 256
    q = L.NodeBatchPad.from_buffer_copy(p)
    q.nnz_fea = 64 * (p.n_rows - mn.value) + 1
    assert call(ctypes.byref(d), ctypes.byref(q), None) == SHAPE                    # more feature entries than the fillers take
    d.fanouts = (ctypes.c_int32 * 2)(10, -1)
    assert call(ctypes.byref(d), ctypes.byref(p), None) == UNSUPPORTED              # an unbounded row
    d.fanouts, d.dtype = fan, 5
    assert call(ctypes.byref(d), ctypes.byref(p), None) == UNSUPPORTED


def test_neighbor_loader_pad_value_errors_before_any_device_work():
    from sgracex1_amd import pyg_lite
    from sgracex1_amd.quant import QuantConstants
    data = pyg_lite.NodeData(torch.zeros((4, 3)), torch.zeros((2, 0), dtype=torch.int64))
    with pytest.raises(ValueError, match="prepare"):
        pyg_lite.NeighborLoader(data, [3, 2], batch_size=2, pad=True)
    with pytest.raises(ValueError, match="-1"):
        pyg_lite.NeighborLoader(data, [3, -1], batch_size=2, prepare="sym_norm2", pad=True)
    with pytest.raises(ValueError, match="64"):
        pyg_lite.NeighborLoader(data, [3, 64], batch_size=2, prepare="sym_norm2", pad=True)
    with pytest.raises(ValueError, match="quant"):
        pyg_lite.NeighborLoader(data, [3, 2], batch_size=2, prepare="sym_norm2", pad=True, quant=object.__new__(QuantConstants))
    assert pyg_lite.NodeBatch(x=1).num_real_nodes is None

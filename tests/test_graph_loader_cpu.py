"""The device graph collator and the trusted batch plans without a GPU: symbols, struct layouts, argument errors, the
host-side batch offsets, and sgx_batch_plan_group_count against a Python restatement of the plan rule of
include/sgx.h."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["sgx_collate_graphs", "sgx_batch_plan_group_count", "sgx_batch_plan_create_known", "sgx_batch_plan_export_groups"]
SHAPE, NULL, UNSUPPORTED = -2, -1, -3


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


def test_collate_structs_match_the_header(L, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "sgx.h"\nint main(void){\n'
        ' printf("sizeof_set %zu\\n", sizeof(sgx_graph_set));\n'
        ' printf("sizeof_batch %zu\\n", sizeof(sgx_graph_batch));\n'
        + "".join(f' printf("s.{n} %zu\\n", offsetof(sgx_graph_set, {n}));\n' for n, _ in L.GraphSet._fields_)
        + "".join(f' printf("b.{n} %zu\\n", offsetof(sgx_graph_batch, {n}));\n' for n, _ in L.GraphBatch._fields_)
        + " return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = 0
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if not ln:
            continue
        name, val = ln.split()
        seen += 1
        if name == "sizeof_set":
            assert ctypes.sizeof(L.GraphSet) == int(val)
        elif name == "sizeof_batch":
            assert ctypes.sizeof(L.GraphBatch) == int(val)
        elif name.startswith("s."):
            assert getattr(L.GraphSet, name[2:]).offset == int(val), name
        else:
            assert getattr(L.GraphBatch, name[2:]).offset == int(val), name
    assert seen == 2 + len(L.GraphSet._fields_) + len(L.GraphBatch._fields_)


def _full_set(L):
    s = L.GraphSet()
    s.n_graphs, s.n_feat, s.n_edges = 4, 7, 10
    for name, _ in L.GraphSet._fields_[3:]:
        setattr(s, name, 256)
    return s


def _full_batch(L):
    b = L.GraphBatch()
    b.n_graphs, b.n_rows, b.n_edges, b.nnz_adj, b.nnz_fea = 2, 9, 10, 8, 9
    for name, _ in L.GraphBatch._fields_[5:]:
        if name.startswith("values"):
            continue
        setattr(b, name, 256)
    return b


def test_collate_argument_errors_need_no_gpu(L):
    lib = L.lib
    run = lambda s, b: lib.sgx_collate_graphs(ctypes.byref(s) if s is not None else None,
                                               ctypes.byref(b) if b is not None else None, None)
    assert run(None, _full_batch(L)) == NULL
    assert run(_full_set(L), None) == NULL
    for field, value in (("n_graphs", 0), ("n_feat", 0), ("n_edges", -1)):
        s = _full_set(L)
        setattr(s, field, value)
        assert run(s, _full_batch(L)) == SHAPE, field
    for field, value in (("n_graphs", 0), ("n_rows", -1), ("n_edges", -1), ("nnz_adj", -1), ("nnz_fea", -1)):
        b = _full_batch(L)
        setattr(b, field, value)
        assert run(_full_set(L), b) == SHAPE, field
    for field in ("node_ptr", "edge_ptr", "edge_index", "x", "y", "rowPtr_adj", "columnIndex_adj", "values_adj",
                  "rowPtr_fea", "columnIndex_fea", "values_fea"):
        s = _full_set(L)
        setattr(s, field, None)
        assert run(s, _full_batch(L)) == NULL, field
    for field in ("index", "node_off", "edge_off", "adj_off", "fea_off", "x", "edge_index", "batch", "y", "graph_ptr",
                  "rowPtr_adj", "columnIndex_adj", "rowPtr_fea", "columnIndex_fea"):
        b = _full_batch(L)
        setattr(b, field, None)
        assert run(_full_set(L), b) == NULL, field


def _rows(L, dtype, width, kind):
    h = ctypes.c_void_p()
    assert L.lib.sgx_batch_plan_create_ex(dtype, 0, 0, None, None, None, width, kind, ctypes.byref(h), None) == 0
    try:
        return L.lib.sgx_batch_plan_rows(h)
    finally:
        L.lib.sgx_batch_plan_destroy(h)


def _groups_rule(n_rows, R, max_graph):
    """include/sgx.h: graph g joins group floor(graph_ptr[g] / S), S = min(ceil(n_rows / 256), R - largest graph + 1)
    (at least 1); no group when a graph is over R."""
    if R <= 0 or max_graph > R:
        return 0, None
    S = max(1, min(-(-n_rows // 256), R - max_graph + 1))
    return (-(-n_rows // S) if n_rows > 0 else 1), S


def _group_graph_rule(sizes, S, n_groups):
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    first = [0] + [int(np.searchsorted(ptr[:-1], k * S, side="left")) for k in range(1, n_groups)]
    return first + [len(sizes)]


def test_group_count_matches_the_rule(L):
    lib = L.lib
    rng = np.random.default_rng(20261016)
    seen_over = seen_fit = 0
    for trial in range(300):
        dtype, kind = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        width = int(rng.choice([7, 16, 64, 128, 256, 300]))
        B = int(rng.integers(1, 400))
        top = int(rng.choice([4, 30, 130]))
        sizes = rng.integers(1, top + 1, size=B)
        n_rows, max_graph = int(sizes.sum()), int(sizes.max())
        R = _rows(L, dtype, width, kind)
        want, S = _groups_rule(n_rows, R, max_graph)
        assert lib.sgx_batch_plan_group_count(dtype, n_rows, max_graph, width, kind) == want, (dtype, kind, width, sizes)
        if want:
            seen_fit += 1
            g = _group_graph_rule(sizes, S, want)
            assert len(g) == want + 1 and g[0] == 0 and g[-1] == B and all(a <= b for a, b in zip(g, g[1:]))
            rows_of = [int(sizes[g[k]:g[k + 1]].sum()) for k in range(want)]
            assert max(rows_of) <= R                # every group fits the budget (the rule's point)
        else:
            seen_over += 1
    assert seen_over > 10 and seen_fit > 100


def test_group_count_and_known_plan_argument_errors_need_no_gpu(L):
    lib = L.lib
    gc = lib.sgx_batch_plan_group_count
    assert gc(0, 10, 11, 64, 0) == SHAPE            # max_graph over n_rows
    assert gc(0, -1, 0, 64, 0) == SHAPE
    assert gc(0, 10, 3, 0, 0) == SHAPE
    assert gc(7, 10, 3, 64, 0) == UNSUPPORTED
    assert gc(0, 10, 3, 64, 2) == UNSUPPORTED
    assert gc(0, 10, 3, 300, 0) == 0                # wider than the fused kernel: no group
    h = ctypes.c_void_p()
    ck = lib.sgx_batch_plan_create_known
    assert ck(0, 0, 0, None, 0, 64, 0, None, None, None) == NULL
    assert ck(0, 10, 2, None, 5, 64, 0, None, ctypes.byref(h), None) == NULL        # graph_ptr
    assert ck(0, 10, 2, 256, 5, 64, 0, None, ctypes.byref(h), None) == NULL         # group_graph where it is written
    assert ck(0, 10, 2, 256, 4, 64, 0, 256, ctypes.byref(h), None) == SHAPE         # 2 graphs of <= 4 rows cannot hold 10
    assert ck(0, 10, 0, 256, 10, 64, 0, 256, ctypes.byref(h), None) == SHAPE        # rows without graphs
    assert ck(0, 10, 2, 256, 11, 64, 0, 256, ctypes.byref(h), None) == SHAPE
    assert ck(0, 10, 2, 256, 5, 0, 0, 256, ctypes.byref(h), None) == SHAPE
    assert ck(9, 10, 2, 256, 5, 64, 0, 256, ctypes.byref(h), None) == UNSUPPORTED
    assert ck(0, 10, 2, 256, 5, 64, 5, 256, ctypes.byref(h), None) == UNSUPPORTED
    assert not h.value
    assert lib.sgx_batch_plan_export_groups(None, None, 0, None) == NULL


def test_known_plans_without_a_launch_match_create_ex(L):
    """The cases that launch nothing: an empty batch, and a graph over the budget (fits 0, no group table)."""
    lib = L.lib
    for dtype, width, kind in ((0, 64, 0), (1, 64, 1), (0, 256, 1), (0, 300, 0)):
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        assert lib.sgx_batch_plan_create_ex(dtype, 0, 0, None, None, None, width, kind, ctypes.byref(a), None) == 0
        assert lib.sgx_batch_plan_create_known(dtype, 0, 0, None, 0, width, kind, None, ctypes.byref(b), None) == 0
        try:
            for f in ("rows", "groups", "max_graph", "fits"):
                assert getattr(lib, "sgx_batch_plan_" + f)(a) == getattr(lib, "sgx_batch_plan_" + f)(b), f
            assert lib.sgx_batch_plan_export_groups(b, None, 0, None) == 0
        finally:
            lib.sgx_batch_plan_destroy(a)
            assert lib.sgx_batch_plan_destroy(b) == 0
    # one graph of 200 rows, budget 128 (fp16, 64 wide, forward): recorded as not fitting, nothing written
    p = ctypes.c_void_p()
    assert lib.sgx_batch_plan_create_known(0, 200, 1, 256, 200, 64, 0, None, ctypes.byref(p), None) == 0
    try:
        assert (lib.sgx_batch_plan_rows(p), lib.sgx_batch_plan_groups(p), lib.sgx_batch_plan_max_graph(p),
                lib.sgx_batch_plan_fits(p)) == (128, 0, 200, 0)
    finally:
        assert lib.sgx_batch_plan_destroy(p) == 0       # the caller's buffer (none here) is never freed


def test_batch_offsets_match_a_restatement(L):
    from sgracex1_amd import ops
    rng = np.random.default_rng(7)
    for trial in range(50):
        G = int(rng.integers(1, 300))
        counts = [rng.integers(1, 40, G), rng.integers(0, 90, G), rng.integers(0, 90, G), rng.integers(0, 40, G)]
        B = int(rng.integers(1, G + 1))
        idx = rng.permutation(G)[:B]
        host, totals = ops.batch_offsets(counts, idx)
        assert host.dtype == np.int32 and host.size == B + 4 * (B + 1)
        assert list(host[:B]) == list(idx)
        for k in range(4):
            off, run = [0], 0
            for g in idx:
                run += int(counts[k][g])
                off.append(run)
            assert list(host[B + k * (B + 1): B + (k + 1) * (B + 1)]) == off
            assert totals[k] == off[-1]


def test_graphset_refuses_bad_graphs(L):
    from sgracex1_amd import ops, pyg_lite as G
    ok = G.Graph(torch.eye(3, 7), torch.tensor([[0, 1], [1, 2]]), torch.tensor([1]))
    empty = G.Graph(torch.zeros(0, 7), torch.zeros(2, 0, dtype=torch.int64), torch.tensor([0]))
    with pytest.raises(ValueError, match="no node"):
        ops.GraphSet([ok, empty])
    with pytest.raises(ValueError, match="leaves its graph"):
        ops.GraphSet([ok, G.Graph(torch.eye(2, 7), torch.tensor([[0], [2]]), torch.tensor([0]))])
    with pytest.raises(ValueError, match="same F"):
        ops.GraphSet([ok, G.Graph(torch.eye(2, 5), torch.zeros(2, 0, dtype=torch.int64), torch.tensor([0]))])
    with pytest.raises(ValueError, match="at least one"):
        ops.GraphSet([])
    with pytest.raises(ValueError, match="GPU"):
        ops.GraphSet([ok], device="cpu")

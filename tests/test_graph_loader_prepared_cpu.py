"""The prepared graph loader without a GPU: the numpy restatement of its rule (tests/_graph_prep_ref.py: normalise every
graph on its own, gather with shifted columns, quantise, dead rows) against sym_norm2 and a COO -> CSR in torch on the
concatenated batch, bit for bit in fp32 and after the fp16 cast, for every batch of the fixture; the fixture's dead-row
properties the GPU tests lean on; and the new entry point's symbol, struct layout and argument errors, which return before
anything reaches a device."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _graph_prep_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, NULL = -2, -1


@pytest.fixture(scope="module")
def L():
    from sgracex1_amd import build
    build.build()
    from sgracex1_amd import _lib
    return _lib


def _torch_norm_csr(ids):
    """What GAT_POOL_PYNQ.forward's normalise() builds for the collated batch, in torch on the CPU."""
    from sgracex1_amd import pyg_lite as G, sgrace
    graphs = P.torch_graphs()
    b = G.collate([graphs[i] for i in ids])
    n = b.num_nodes
    ei, norm = sgrace.sym_norm2(b.edge_index, n)
    assert norm.dtype == torch.float32
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(ei[0], minlength=n), 0)
    assert bool((ei[0][1:] >= ei[0][:-1]).all())                       # row-sorted: the COO is the CSR's entry order
    return rowptr.to(torch.int32).numpy(), ei[1].to(torch.int32).numpy(), norm


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.int16, 4: np.int32}[a.itemsize])


@pytest.mark.parametrize("ids", P.BATCHES, ids=lambda ids: "-".join(map(str, ids)))
def test_the_rule_is_sym_norm2_on_the_concatenated_batch(ids, L):
    from sgracex1_amd import quant
    qcs = [quant.constants(b) for b in (8, 4, 2, 1)]
    qcs += [c.second_layer() for c in qcs]
    got = P.prepared_batch(P.fixture(), ids, qcs)
    rowptr, col, norm = _torch_norm_csr(ids)
    assert np.array_equal(got["rowptr"], rowptr) and np.array_equal(got["col"], col)
    assert np.array_equal(_bits(got["val"]), _bits(norm.numpy()))
    assert np.array_equal(_bits(got["val16"]), _bits(norm.to(torch.float16).numpy()))
    # the quantiser and the dead-row test on the batch's values, in torch: elementwise and row-local
    for c, q, qd in zip(qcs, got["q"], got["q_dead"]):
        t = torch.clip(torch.round(1 / c.a_s * norm + c.a_z), min=0, max=2 ** c.w_qbits - 1)
        t = (t / 2 if c.w_qbits == 1 else t / (2 ** (c.w_qbits - 1))).numpy()
        assert np.array_equal(_bits(q), _bits(t))
        assert np.array_equal(qd, P.dead_rows(rowptr, t))
    assert np.array_equal(got["dead"], P.dead_rows(rowptr, norm.numpy()))


def test_fixture_shapes():
    g = P.fixture()
    assert [x["x"].shape[0] for x in g] == [1, 2, 5, 9, 6, 3, 4, 150] and all(x["x"].shape[1] == 7 for x in g)
    assert g[0]["edge_index"].shape[1] == 0
    e = g[4]["edge_index"]
    assert ((e[0] == 4) & (e[1] == 5)).sum() == 21                          # a repeated edge
    e = g[5]["edge_index"]
    assert ((e[0] == e[1])).sum() == 1                                     # a stored self loop
    assert not (g[6]["edge_index"] == 3).any()                            # an isolated node among connected ones
    assert sorted(sum(P.BATCHES[:3], [])) == list(range(8)) and len(P.BATCHES[2]) == 2     # a partial last batch
    assert sorted(P.PERMUTATION) == list(range(8))
    assert any(len(set(b)) < len(b) for b in P.BATCHES) and [7] in P.BATCHES


def test_fixture_dead_rows_are_where_the_gpu_tests_expect_them(L):
    from sgracex1_amd import quant
    g = P.fixture()
    c8, c1 = quant.constants(8), quant.constants(1)
    sub = P.prepared_batch(g, P.CONNECTED, [c8, c8.second_layer()])
    assert not sub["dead"].any() and not sub["q_dead"][0].any() and not sub["q_dead"][1].any()
    full = P.prepared_batch(g, list(range(8)), [c1, c1.second_layer()])
    rows = np.cumsum([0] + [x["x"].shape[0] for x in g])
    assert full["dead"][rows[0]] and full["dead"][rows[6] + 3] and full["dead"].sum() == 2     # fill = 0
    one = P.prepared_batch(g, P.CONNECTED, [c1, c1.second_layer()])
    for qd in one["q_dead"]:
        assert (qd & ~one["dead"]).any()                                   # live unquantised, dead at one bit
    # the repeated edge keeps its 21 equal entries
    r = rows[4] + 5
    v = full["val"][full["rowptr"][r]:full["rowptr"][r + 1]]
    assert len(v) == 22 and (v[:21] == v[0]).all() and v[0] > 0 and v[21] == 0


def test_symbol_and_struct_layout(L, tmp_path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    assert "sgx_collate_graphs_extras" in L.SYMBOLS and " T sgx_collate_graphs_extras\n" in out
    assert L.lib.sgx_version() == 110
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "sgx.h"\nint main(void){\n'
        ' printf("sizeof %zu\\n", sizeof(sgx_collate_extra));\n printf("max %d\\n", SGX_COLLATE_MAX_EXTRAS);\n'
        + "".join(f' printf("{n} %zu\\n", offsetof(sgx_collate_extra, {n}));\n' for n, _ in L.CollateExtra._fields_)
        + " return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = 0
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if not ln:
            continue
        name, val = ln.split()
        seen += 1
        if name == "sizeof":
            assert ctypes.sizeof(L.CollateExtra) == int(val)
        elif name == "max":
            assert L.SGX_COLLATE_MAX_EXTRAS == int(val) == 3
        else:
            assert getattr(L.CollateExtra, name).offset == int(val), name
    assert seen == 2 + len(L.CollateExtra._fields_)


def _valid(L):
    """A descriptor triple that passes every check (fake non-NULL addresses: nothing is dereferenced on the host)."""
    s, b = L.GraphSet(), L.GraphBatch()
    s.n_graphs, s.n_feat, s.n_edges = 4, 7, 10
    for n, t in L.GraphSet._fields_:
        if t is ctypes.c_void_p:
            setattr(s, n, 0x1000)
    b.n_graphs, b.n_rows, b.n_edges, b.nnz_adj, b.nnz_fea = 2, 5, 6, 6, 5
    for n, t in L.GraphBatch._fields_:
        if t is ctypes.c_void_p:
            setattr(b, n, 0x1000)
    xs = (L.CollateExtra * 3)()
    for x in xs:
        for n, t in L.CollateExtra._fields_:
            if t is ctypes.c_void_p:
                setattr(x, n, 0x1000)
        x.nnz = 11
    return s, b, xs


def test_argument_errors_return_before_the_device(L):
    """(Every call here is refused: one that passed would launch on these made-up addresses.)"""
    f = L.lib.sgx_collate_graphs_extras
    s, b, xs = _valid(L)
    S, B = ctypes.byref(s), ctypes.byref(b)
    assert f(S, B, xs, 4, None) == SHAPE and f(S, B, xs, -1, None) == SHAPE
    assert f(None, None, None, 7, None) == SHAPE                            # K is judged first
    # the old call's statuses
    assert f(None, B, xs, 1, None) == NULL and f(S, None, xs, 1, None) == NULL
    assert f(None, B, None, 0, None) == NULL
    b.n_graphs = 0
    assert f(S, B, xs, 1, None) == SHAPE == L.lib.sgx_collate_graphs(S, B, None)
    b.n_graphs, b.graph_ptr = 2, None
    assert f(S, B, xs, 0, None) == NULL == L.lib.sgx_collate_graphs(S, B, None)
    b.graph_ptr = 0x1000
    # the extras' own
    assert f(S, B, None, 1, None) == NULL
    for k in range(3):
        for field in ("rowPtr", "values", "entry_off"):
            keep = getattr(xs[k], field)
            setattr(xs[k], field, None)
            assert f(S, B, xs, 3, None) == NULL, (k, field)
            setattr(xs[k], field, keep)
    xs[2].rowPtr = None
    xs[2].nnz = -5
    b.n_graphs = 0                                                          # -> the old call's error, not the extras'
    assert f(S, B, xs, 2, None) == SHAPE
    b.n_graphs = 2
    xs[1].nnz = -1
    assert f(S, B, xs, 2, None) == SHAPE
    xs[1].nnz = 11
    xs[0].rowPtr_out = None                                                 # columnIndex_out without rowPtr_out
    assert f(S, B, xs, 1, None) == NULL
    xs[0].rowPtr_out, xs[0].columnIndex_out = 0x1000, None                  # a written pattern needs its columns
    assert f(S, B, xs, 1, None) == NULL
    xs[0].columnIndex_out, xs[0].columnIndex = 0x1000, None
    assert f(S, B, xs, 1, None) == NULL
    xs[0].columnIndex = 0x1000
    xs[0].dead_row = None                                                   # exactly one of the two row-byte arrays
    assert f(S, B, xs, 1, None) == NULL
    xs[0].dead_row, xs[0].dead_row_out = 0x1000, None
    assert f(S, B, xs, 1, None) == NULL


def test_batch_offsets_carry_a_fifth_count_array(L):
    from sgracex1_amd import ops
    rng = np.random.default_rng(0)
    counts = tuple(rng.integers(0, 9, 12) for _ in range(5))
    idx = np.array([3, 3, 11, 0])
    host5, tot5 = ops.batch_offsets(counts, idx)
    host4, tot4 = ops.batch_offsets(counts[:4], idx)
    B = len(idx)
    assert np.array_equal(host5[:len(host4)], host4) and tot5[:4] == tot4
    assert np.array_equal(host5[len(host4):], np.concatenate([[0], np.cumsum(counts[4][idx])])) and tot5[4] == host5[-1]
    bi = ops.BatchIndex(torch.from_numpy(host5), B, tot5, 9)
    assert bi.fea_off.numel() == B + 1 and bi.norm_off.numel() == B + 1 and bi.nnz_norm == tot5[4]
    assert ops.BatchIndex(torch.from_numpy(host4), B, tot4, 9).norm_off is None


def test_loader_argument_errors_need_no_gpu(L):
    """GraphLoader judges prepare / quant before it touches the dataset."""
    from sgracex1_amd import pyg_lite as G, quant
    qc = quant.constants(8)
    with pytest.raises(ValueError, match="quant needs prepare"):
        G.GraphLoader([], quant=qc)
    with pytest.raises(ValueError, match="float32"):
        G.GraphLoader([], prepare="sym_norm2", quant=qc, dtypes=(torch.float16,))
    with pytest.raises(ValueError, match="prepare must be None or 'sym_norm2'"):
        G.GraphLoader([], prepare="gcn_norm")
